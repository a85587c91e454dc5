"""
The two sums on the stored entries of sparse frames (`-m gpu`), through libertem_amd.hip:
`csr_sum_sig` (one value per frame) and `csr_sum_frames` (one value per pixel) on a CSR triple in HBM, against
int64 / float64 NumPy sums of the same triple.  Shapes: 16 frames x 1024 pixels (an empty frame, a one-event
frame, a frame with every pixel set, events at pixel 0 and n_px - 1), 35 x 117 (a multiple of nothing), and
150 x 9001 -- three pixel blocks of `k_csr_sum_frames`, the last one partial, and three frame splits -- with events
on both sides of every block border.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import raw_csr_recipes as recipes

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CASES = {c['name']: c for c in recipes.CASES}
DTYPES = ('u1', 'u2', 'i2', 'u4', 'i4', 'f4')
INT_DTYPES = DTYPES[:5]
OUT_DTYPES = ('f4', 'f8')
NAMES = {'u1': 'u8', 'u2': 'u16', 'i2': 'i16', 'u4': 'u32', 'i4': 'i32', 'f4': 'f32', 'f8': 'f64'}
GUARD = 64


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


def _dev(arr):
    arr = np.ascontiguousarray(arr)
    twin = {np.dtype('uint16'): np.int16, np.dtype('uint32'): np.int32, np.dtype('uint64'): np.int64}
    if arr.dtype in twin:
        arr = arr.view(twin[arr.dtype])
    return torch.from_numpy(arr).cuda()


def edge_matrix(dtype, seed=0):
    """16 frames of 1024 pixels, canonical: frame 3 empty, frame 5 one event, frame 7 every pixel (several trips
    per lane), events at pixel 0 and at pixel n_px - 1; negative values in frame 1 of signed dtypes"""
    rng = np.random.default_rng(seed)
    n, n_px = 16, 1024
    dt = np.dtype(dtype)
    dense = np.zeros((n, n_px), dtype=np.float64)
    for f in range(n):
        k = int(rng.integers(5, 120))
        dense[f, rng.choice(n_px, k, replace=False)] = rng.integers(1, 100, k)
    dense[3] = 0
    dense[5] = 0
    dense[5, 517] = 9
    dense[7] = rng.integers(1, 100, n_px)
    dense[0, 0] = 11
    dense[15, n_px - 1] = 13
    if dt.kind == 'i':
        dense[1] = -dense[1]
    if dt.kind == 'f':
        dense = dense * 0.37
    m = sp.csr_matrix(dense.astype(dt))
    m.sort_indices()
    assert m[3].nnz == 0 and m[5].nnz == 1 and m[7].nnz == n_px
    return m


def small_matrix(dtype):
    """35 frames of 117 pixels from the golden recipe of that dtype (frame 3 empty, frame 34 full)"""
    inp = recipes.make_case(CASES[f'dtype_{dtype}'])
    m = sp.csr_matrix((inp['data'], inp['indices'], inp['indptr']), shape=(35, 117))
    m.sort_indices()
    return m


def wide_matrix(dtype, seed=3):
    """150 frames of 9001 pixels: pixel blocks [0, 4096), [4096, 8192), [8192, 9001) of k_csr_sum_frames and three
    splits of 50 frames; frame 2 empty, frame 77 full, events at 4095 | 4096 and 8191 | 8192 and at both ends"""
    rng = np.random.default_rng(seed)
    n, n_px = 150, 9001
    dt = np.dtype(dtype)
    dense = np.zeros((n, n_px), dtype=np.float64)
    for f in range(n):
        k = int(rng.integers(20, 200))
        dense[f, rng.choice(n_px, k, replace=False)] = rng.integers(1, 100, k)
    dense[2] = 0
    dense[77] = rng.integers(1, 100, n_px)
    for f, px in ((0, 0), (1, 4095), (1, 4096), (4, 4096), (60, 8191), (60, 8192), (61, 8191), (149, 9000)):
        dense[f, px] = 7 + f
    if dt.kind == 'i':
        dense[5] = -dense[5]
    m = sp.csr_matrix(dense.astype(dt))
    m.sort_indices()
    return m


MAKERS = {'16x1024': edge_matrix, '35x117': small_matrix, '150x9001': wide_matrix}


def upload(m):
    return dict(indptr=_dev(m.indptr.astype(np.int64)), indices=_dev(m.indices.astype(np.int32)),
                data=_dev(m.data), dtype=m.data.dtype, n=m.shape[0], n_px=m.shape[1])


def wide(m):
    """the dense frames in the accumulator's type: int64 for integers, float64 for float32"""
    return m.toarray().astype(np.float64 if m.dtype.kind == 'f' else np.int64)


def call_sig(hip, d, odt, start=None, rows=None, row0=0, n=None, accumulate=False, size=None, at=0):
    """one ltmi_csr_sum_sig into element `at` of a buffer of `size` elements that starts as `start` (default NaN)
    -> the whole buffer on the host"""
    n = (d['n'] - row0 if rows is None else len(rows)) if n is None else n
    size = n if size is None else size
    odt = np.dtype(odt)
    buf = _dev(np.full(size, np.nan, dtype=odt) if start is None else np.asarray(start, dtype=odt))
    rows_dev = None if rows is None else _dev(np.asarray(rows, dtype=np.int32))
    hip.csr_sum_sig(0, d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), d['dtype'],
                    0 if rows_dev is None else rows_dev.data_ptr(), row0, n, d['n_px'],
                    buf.data_ptr() + at * odt.itemsize, odt, accumulate)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def call_frames(hip, d, odt, start=None, rows=None, row0=0, n=None, accumulate=False, lead=0, ws=None):
    """one ltmi_csr_sum_frames into element `lead` of a buffer of lead + n_px + lead elements (default NaN)
    -> the whole buffer on the host"""
    n = (d['n'] - row0 if rows is None else len(rows)) if n is None else n
    odt = np.dtype(odt)
    n_px = d['n_px']
    buf = _dev(np.full(n_px + 2 * lead, np.nan, dtype=odt) if start is None else np.asarray(start, dtype=odt))
    if ws is None:
        ws = torch.empty(max(1, hip.csr_sum_frames_workspace(n_px) // 8), dtype=torch.int64, device='cuda:0')
    rows_dev = None if rows is None else _dev(np.asarray(rows, dtype=np.int32))
    hip.csr_sum_frames(0, d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), d['dtype'],
                       0 if rows_dev is None else rows_dev.data_ptr(), row0, n, n_px,
                       buf.data_ptr() + lead * odt.itemsize, odt, accumulate, ws.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def sig_bound(m, odt):
    """f4 data: one final rounding plus double accumulation"""
    x = wide(m)
    return 2.0 ** -24 * np.abs(x.sum(axis=1)) + 1e-12 * np.abs(x).sum(axis=1)


def check_sig(got, m, odt, frames=None):
    x = wide(m) if frames is None else wide(m)[frames]
    if m.dtype.kind == 'f':
        b = sig_bound(m, odt) if frames is None else sig_bound(m, odt)[frames]
        assert np.all(np.abs(got.astype(np.float64) - x.sum(axis=1)) <= b)
    else:
        assert np.array_equal(got, x.sum(axis=1).astype(odt))


# ---- ltmi_csr_sum_sig ----------------------------------------------------------------------------------
@pytest.mark.parametrize('odt', OUT_DTYPES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', ('16x1024', '35x117'))
def test_sum_sig_every_dtype(hip, shape, dtype, odt):
    m = MAKERS[shape](dtype)
    d = upload(m)
    runs = [call_sig(hip, d, odt) for _ in range(3)]              # onto NaN: every frame is overwritten
    assert hip.csr_last_kernel() == f'k_csr_sum_sig<{NAMES[dtype]},{NAMES[odt]}>'
    got = runs[0]
    assert got.dtype == np.dtype(odt) and not np.isnan(got).any()
    check_sig(got, m, odt)
    assert got[3] == 0                                            # the empty frame of either shape
    assert runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()


@pytest.mark.parametrize('odt', OUT_DTYPES)
@pytest.mark.parametrize('dtype', ('u2', 'i4', 'f4'))
def test_sum_sig_accumulate_range_rows(hip, dtype, odt):
    m = edge_matrix(dtype)
    d = upload(m)
    x = wide(m)
    rng = np.random.default_rng(1)
    preset = (rng.integers(-1000, 1000, 16)).astype(odt)
    got = call_sig(hip, d, odt, start=preset, accumulate=True)
    want = preset + x.sum(axis=1).astype(odt)
    if m.dtype.kind == 'f':
        assert np.all(np.abs(got - (preset + x.sum(axis=1))) <= sig_bound(m, odt) + np.spacing(np.abs(want)))
    else:
        assert np.array_equal(got, want)
    # frames [2, 13) into elements [3, 14) of a NaN buffer: the rest stays NaN
    got = call_sig(hip, d, odt, row0=2, n=11, size=16, at=3)
    assert np.all(np.isnan(got[:3])) and np.all(np.isnan(got[14:]))
    check_sig(got[3:14], m, odt, frames=np.arange(2, 13))
    assert hip.csr_last_kernel() == f'k_csr_sum_sig<{NAMES[dtype]},{NAMES[odt]}>'
    # an ascending row list with the empty and the full frame
    sel = [0, 3, 5, 7, 15]
    got = call_sig(hip, d, odt, rows=sel, size=7, at=1)
    assert np.isnan(got[0]) and np.isnan(got[6])
    check_sig(got[1:6], m, odt, frames=sel)
    assert hip.csr_last_kernel() == f'k_csr_sum_sig<{NAMES[dtype]},{NAMES[odt]}> rows'


@pytest.mark.parametrize('odt', OUT_DTYPES)
def test_sum_sig_stored_nan(hip, odt):
    m = edge_matrix('f4')
    clean = m.copy()
    m.data[int(m.indptr[7]) + 100] = np.nan                       # one entry of the full frame
    got = call_sig(hip, upload(m), odt)
    assert np.isnan(got[7]) and not np.isnan(np.delete(got, 7)).any()
    keep = np.delete(np.arange(16), 7)
    check_sig(got[keep], clean, odt, frames=keep)


# ---- ltmi_csr_sum_frames -------------------------------------------------------------------------------
@pytest.mark.parametrize('odt', OUT_DTYPES)
@pytest.mark.parametrize('dtype', INT_DTYPES)
@pytest.mark.parametrize('shape', ('16x1024', '35x117', '150x9001'))
def test_sum_frames_every_dtype(hip, shape, dtype, odt):
    m = MAKERS[shape](dtype)
    d = upload(m)
    runs = [call_frames(hip, d, odt) for _ in range(3)]           # onto NaN
    assert hip.csr_last_kernel() == f'k_csr_sum_frames<{NAMES[dtype]},{NAMES[odt]}>'
    assert runs[0].dtype == np.dtype(odt)
    assert np.array_equal(runs[0], wide(m).sum(axis=0).astype(odt))
    assert runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()
    if np.dtype(dtype).kind == 'i':
        assert wide(m).min() < 0                                  # (negative values are part of the case)


def test_sum_frames_hot_pixel_beyond_2_24(hip):
    """300 frames (five splits) that all store 65535 at pixel 5: a float32 running sum would stall at 2^24"""
    n, n_px = 300, 16
    dense = np.zeros((n, n_px), dtype=np.uint16)
    dense[:, 5] = 65535
    dense[::7, 9] = 3
    dense[11, 0] = 1
    m = sp.csr_matrix(dense)
    m.sort_indices()
    got = call_frames(hip, upload(m), 'f4')
    want = dense.astype(np.int64).sum(axis=0)
    assert want[5] == 300 * 65535 > 2 ** 24
    assert got[5] == np.float32(np.int64(300 * 65535))
    assert np.array_equal(got, want.astype(np.float32))


def test_sum_frames_u4_maximum_f8(hip):
    dense = np.zeros((9, 40), dtype=np.uint32)
    dense[:, 17] = 2 ** 32 - 1
    dense[4, 0] = 2 ** 32 - 1
    dense[::2, 39] = 5
    m = sp.csr_matrix(dense)
    m.sort_indices()
    got = call_frames(hip, upload(m), 'f8')
    assert np.array_equal(got, dense.astype(np.int64).sum(axis=0).astype(np.float64))
    assert got[17] == 9.0 * (2 ** 32 - 1)


@pytest.mark.parametrize('odt', OUT_DTYPES)
def test_sum_frames_accumulate_and_unaligned_out(hip, odt):
    """n_px = 117 into a buffer that starts one element after a 16-byte boundary; accumulate onto preset values"""
    m = small_matrix('i2')
    d = upload(m)
    want = wide(m).sum(axis=0).astype(odt)
    got = call_frames(hip, d, odt, lead=1)
    assert np.isnan(got[0]) and np.isnan(got[-1])
    assert np.array_equal(got[1:-1], want)
    rng = np.random.default_rng(2)
    preset = rng.integers(-500, 500, 119).astype(odt)
    got = call_frames(hip, d, odt, start=preset, accumulate=True, lead=1)
    assert got[0] == preset[0] and got[-1] == preset[-1]
    assert np.array_equal(got[1:-1], preset[1:-1] + want)


def test_sum_frames_workspace_is_reusable(hip):
    """two different inputs through one workspace (the larger first): both right, whatever the first left behind"""
    a, b = wide_matrix('u2'), edge_matrix('i4')
    ws = torch.full((hip.csr_sum_frames_workspace(9001) // 8,), -12345, dtype=torch.int64, device='cuda:0')
    assert hip.csr_sum_frames_workspace(1024) <= hip.csr_sum_frames_workspace(9001)
    got_a = call_frames(hip, upload(a), 'f4', ws=ws)
    got_b = call_frames(hip, upload(b), 'f4', ws=ws)
    got_a2 = call_frames(hip, upload(a), 'f4', ws=ws)
    assert np.array_equal(got_a, wide(a).sum(axis=0).astype(np.float32))
    assert np.array_equal(got_b, wide(b).sum(axis=0).astype(np.float32))
    assert got_a2.tobytes() == got_a.tobytes()


@pytest.mark.parametrize('shape', ('16x1024', '150x9001'))
def test_sum_frames_range_and_rows(hip, shape):
    m = MAKERS[shape]('u2')
    d = upload(m)
    x = wide(m)
    n = m.shape[0]
    got = call_frames(hip, d, 'f4', row0=2, n=n - 5)
    assert np.array_equal(got, x[2:n - 3].sum(axis=0).astype(np.float32))
    assert hip.csr_last_kernel() == 'k_csr_sum_frames<u16,f32>'
    sel = [0, 3, 5, 7, 15] if shape == '16x1024' else [1, 2, 60, 61, 77, 100, 149]      # empty and full among them
    got = call_frames(hip, d, 'f8', rows=sel)
    assert np.array_equal(got, x[sel].sum(axis=0).astype(np.float64))
    assert hip.csr_last_kernel() == 'k_csr_sum_frames<u16,f64> rows'


# ---- both ----------------------------------------------------------------------------------------------
def test_no_frames_touch_nothing(hip):
    d = upload(edge_matrix('u2'))
    poison = np.full(16, 7.5, dtype=np.float32)
    before = hip.csr_last_kernel()
    assert np.array_equal(call_sig(hip, d, 'f4', start=poison, n=0, size=16), poison)
    ws = torch.full((hip.csr_sum_frames_workspace(1024) // 8,), 99, dtype=torch.int64, device='cuda:0')
    poison = np.full(1024, 7.5, dtype=np.float32)
    assert np.array_equal(call_frames(hip, d, 'f4', start=poison, n=0, ws=ws), poison)
    assert bool((ws == 99).all().cpu())
    assert hip.csr_last_kernel() == before                        # (nothing was launched)


@pytest.mark.parametrize('shape', ('16x1024', '150x9001'))
def test_unchecked_triple_stays_inside(hip, shape):
    """a stored index of -1 (first entry of a row) and one of n_px (last entry of a row), as a triple that was
    never checked could hold: both are skipped, nothing outside `out` and the workspace is written"""
    m = MAKERS[shape]('u2')
    n, n_px = m.shape
    lo_row, hi_row = 1, 9
    k_lo, k_hi = int(m.indptr[lo_row]), int(m.indptr[hi_row + 1]) - 1
    indices = m.indices.astype(np.int32).copy()
    x = wide(m)
    x[lo_row, indices[k_lo]] = 0
    x[hi_row, indices[k_hi]] = 0
    indices[k_lo], indices[k_hi] = -1, n_px
    d = upload(m)
    d['indices'] = _dev(indices)
    # per frame
    got = call_sig(hip, d, 'f4', size=n + 2 * GUARD, at=GUARD)
    assert np.all(np.isnan(got[:GUARD])) and np.all(np.isnan(got[-GUARD:]))
    assert np.array_equal(got[GUARD:-GUARD], x.sum(axis=1).astype(np.float32))
    # per pixel: `out` and the workspace from the middle of larger allocations
    n_ws = hip.csr_sum_frames_workspace(n_px) // 8
    big = torch.zeros(n_ws + 2 * GUARD, dtype=torch.int64, device='cuda:0')
    got = call_frames(hip, d, 'f4', lead=GUARD, ws=big[GUARD:GUARD + n_ws])
    assert np.all(np.isnan(got[:GUARD])) and np.all(np.isnan(got[-GUARD:]))
    assert np.array_equal(got[GUARD:-GUARD], x.sum(axis=0).astype(np.float32))
    edges = torch.cat([big[:GUARD], big[-GUARD:]]).cpu().numpy()
    assert np.all(edges == 0)


def test_argument_errors(hip):
    mf, mi = edge_matrix('f4'), edge_matrix('u2')
    df, di = upload(mf), upload(mi)
    ws = torch.empty(hip.csr_sum_frames_workspace(1024) // 8, dtype=torch.int64, device='cuda:0')
    out = torch.zeros(1024, dtype=torch.complex64, device='cuda:0')

    def frames(d, odt, indptr=None):
        hip.csr_sum_frames(0, d['indptr'].data_ptr() if indptr is None else indptr, d['indices'].data_ptr(),
                           d['data'].data_ptr(), d['dtype'], 0, 0, 16, 1024, out.data_ptr(), odt, False,
                           ws.data_ptr())

    def sig(d, odt, indptr=None):
        hip.csr_sum_sig(0, d['indptr'].data_ptr() if indptr is None else indptr, d['indices'].data_ptr(),
                        d['data'].data_ptr(), d['dtype'], 0, 0, 16, 1024, out.data_ptr(), odt, False)

    with pytest.raises(ValueError, match='float32'):
        frames(df, np.float32)                                    # float data: the dense route's business
    for fn, d in ((frames, di), (sig, di), (sig, df)):
        with pytest.raises(ValueError, match='complex64'):
            fn(d, np.complex64)
        with pytest.raises(ValueError):
            fn(d, np.float32, indptr=0)
    with pytest.raises(ValueError):
        hip.csr_sum_frames(0, di['indptr'].data_ptr(), di['indices'].data_ptr(), di['data'].data_ptr(), np.uint16,
                           0, 0, 16, 0, out.data_ptr(), np.float32, False, ws.data_ptr())
    with pytest.raises(ValueError):
        hip.csr_sum_sig(0, di['indptr'].data_ptr(), di['indices'].data_ptr(), di['data'].data_ptr(), np.uint16,
                        0, 0, -1, 1024, out.data_ptr(), np.float32, False)
    torch.cuda.synchronize()
    assert bool((out == 0).all().cpu())
