"""
k_labels (csrc/ltmi_labels.hip) at the kernel level: partition stacks -- no pixel stored by two masks -- through the
C ABI (`libertem_amd.hip`), tiles and results in guarded buffers (tests/guarded.py): NaN (float) or the dtype's maximum
(integers) around the tile, byte poison around the result, which is compared afterwards.

Shapes are the smallest at which this kernel can go wrong: 67 x 45 = 3015 pixels is 5 chunks of 512 and a ragged sixth,
rows of odd length; bins of 4 and 8 detector rows span several chunks (sums added chunk by chunk); 1, 37 and 130 frames
are less than one workgroup's 64, a ragged one, and two and a bit.  The reference of every case is the sum over the
STORED entries in float64: what the reference's CSR loop computes (common/numba/__init__.py:153-184), also for
non-finite pixels.  The label image is built with LTMI_SPARSE_LABELS=1 only (it is not the default route, DESIGN.md
4.3c): every test here runs with it set, test_route also without.  Integer frames with weights 1 must come out EQUAL (all sums < 2^24); float frames within
1e-5 * sum |x| |w| per entry, the bound of test_run_udf_elementwise_error_bound.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIG = (67, 45)
N_PX = SIG[0] * SIG[1]
SWITCHES = ('LTMI_SPARSE_LABELS', 'LTMI_SPARSE_BELL', 'LTMI_SPARSE_SCATTER', 'LTMI_SPARSE_BAND')


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


@pytest.fixture(autouse=True)
def labels_on(monkeypatch):
    """the library reads the switches when a handle is made"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('LTMI_SPARSE_LABELS', '1')


def bins(sig, factor):
    """(n_px, n_masks) CSR, the layout MaskHandle.csr takes"""
    from libertem_amd.masks import bin_masks
    return bin_masks(sig, factor).T.tocsr()


def rings(sig=(96, 96), n=12, r0=6.0, width=3.5):
    """n hard rings with non-integer weights: a hole in the middle, unlabelled corners, every ring over many chunks"""
    import scipy.sparse as sp
    yy, xx = np.mgrid[0:sig[0], 0:sig[1]]
    r = np.hypot(yy - sig[0] / 2 + 0.5, xx - sig[1] / 2 + 0.5).ravel()
    k = np.floor((r - r0) / width).astype(np.int64)
    sel = (r >= r0) & (k < n)
    px = np.flatnonzero(sel)
    w = (0.37 + 0.013 * k[sel] + 1e-3 * (px % 7)).astype(np.float32)
    m = sp.csr_matrix((w, (px, k[sel])), shape=(r.size, n))
    assert 0 < (~sel).sum() and not sel.reshape(sig)[0, 0] and not sel.reshape(sig)[sig[0] // 2, sig[1] // 2]
    return m


def stored_sum(csr, x):
    """float64 sum over the stored entries of a partition stack: (frames, n_masks)"""
    csr = csr.tocsr()
    counts = np.diff(csr.indptr)
    assert counts.max() <= 1
    px = np.flatnonzero(counts)
    with np.errstate(invalid='ignore', over='ignore'):
        terms = x[:, px].astype(np.float64) * csr.data.astype(np.float64)[None, :]
        ref = np.zeros((csr.shape[1], x.shape[0]))
        np.add.at(ref, csr.indices, terms.T)
    return ref.T


def scale_of(csr, x):
    return np.abs(x).astype(np.float64) @ np.abs(csr).astype(np.float64).toarray()


def frames(rng, dtype, n, n_px):
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return (rng.standard_normal((n, n_px)) * 100).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, (n, n_px), endpoint=True).astype(dt)


def product(h, x, n_masks, ld_tile=None, base=None, rows=None, expect='k_labels<', shift=1):
    """one guarded call; -> (result, kernel name).  Nothing outside the result's rectangle may change, the tile not at
    all."""
    dt = x.dtype
    tile = G.Region(x.shape[0], x.shape[1], ld_tile or x.shape[1], dt, shift=shift, init=x,
                    fill='nan' if dt.kind == 'f' else 'max')
    n = x.shape[0] if rows is None else len(rows)
    out = G.Region(n, n_masks, n_masks + 3, np.float32, shift=1, init=base)
    if rows is None:
        h.apply(tile.ptr, dt, n, tile.ld, out.ptr, out.ld, base is not None)
    else:
        dev_rows = torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda()
        assert h.apply_rows(tile.ptr, dt, dev_rows.data_ptr(), n, tile.ld, out.ptr, out.ld, base is not None), \
            "row list not handled"
    torch.cuda.synchronize()
    kern = h.last_kernel()
    assert expect in kern and ((',rows' in kern) == (rows is not None)), kern
    G.unchanged_outside(out, kern)
    G.unchanged(tile, kern)
    return out.result(), kern


# ---- route ----------------------------------------------------------------------------------------------------------
def test_route(hip, monkeypatch):
    import scipy.sparse as sp
    from libertem_amd.masks import is_label_stack
    csr = bins(SIG, 4)
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    x = frames(np.random.default_rng(1), np.uint16, 3, N_PX)
    product(h, x, csr.shape[1])
    assert h.nonfinite_frames() == 0
    h.close()
    twice = csr.tolil()
    twice[100, 7] = 1.0                                   # pixel 100 = (2, 10) belongs to bin 2
    twice = twice.tocsr()
    assert twice.nnz == csr.nnz + 1
    h = hip.MaskHandle.csr(0, twice, np.float32)
    assert h.kind() == 2
    product(h, x, csr.shape[1], expect='k_sell_apply<')
    h.close()
    for rd in (np.float64, np.complex64):                 # float32 results only
        h = hip.MaskHandle.csr(0, csr.astype(rd), rd)
        assert h.kind() == 2
        h.close()
    # the library's rule and its host-side twin agree
    pts = sp.csr_matrix((np.ones(3, dtype=np.float32), ([5, 700, 2999], [0, 1, 2])), shape=(N_PX, 3))
    empty = sp.csr_matrix((N_PX, 204), dtype=np.float32)
    for stack in (csr, twice, pts, empty, rings()):
        h = hip.MaskHandle.csr(0, stack, np.float32)
        assert (h.kind() == 4) == is_label_stack(stack), stack.shape
        h.close()
    # without the switch (and with 0) the image is not built: the gather kernel, as before
    for value in (None, '0'):
        monkeypatch.delenv('LTMI_SPARSE_LABELS')
        if value is not None:
            monkeypatch.setenv('LTMI_SPARSE_LABELS', value)
        h = hip.MaskHandle.csr(0, csr, np.float32)
        assert h.kind() == 2
        product(h, x, csr.shape[1], expect='k_sell_apply<')
        h.close()
        monkeypatch.setenv('LTMI_SPARSE_LABELS', '1')


def test_route_switched_off_in_a_fresh_process(hip):
    """LTMI_SPARSE_LABELS is read when the handle is made: 0 (and unset) never builds the label image"""
    code = ("import numpy as np\n"
            "from libertem_amd import hip\n"
            "from libertem_amd.masks import bin_masks\n"
            "h = hip.MaskHandle.csr(0, bin_masks((67, 45), 4).T.tocsr(), np.float32)\n"
            "print('KIND', h.kind())\n"
            "h.close()\n")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env['PYTHONPATH'] = root + os.pathsep + env.get('PYTHONPATH', '')
    for value, kind in (('0', 2), ('1', 4), (None, 2)):
        r = subprocess.run([sys.executable, '-c', code], cwd=root,
                           env=env if value is None else dict(env, LTMI_SPARSE_LABELS=value),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f'KIND {kind}' in r.stdout, (value, r.stdout)


def test_few_labelled_pixels_read_few_chunks(hip):
    """point masks: only the chunks that hold a labelled pixel are read"""
    import scipy.sparse as sp
    px = np.array([5, 700, 701, 2999])
    pts = sp.csr_matrix((np.array([1.5, -2.0, 0.25, 3.0], dtype=np.float32), (px, [0, 1, 1, 2])), shape=(N_PX, 3))
    h = hip.MaskHandle.csr(0, pts, np.float32)
    assert h.kind() == 4
    x = frames(np.random.default_rng(2), np.float32, 70, N_PX)
    x[:, 1500] = np.nan                                   # in a chunk without a label
    res, kern = product(h, x, 3)
    assert 'chunks=3 ' in kern, kern                      # pixels 5 | 700, 701 | 2999: chunks 0, 1, 5
    assert np.all(np.abs(res - stored_sum(pts, x)) <= 1e-5 * scale_of(pts, np.nan_to_num(x)))
    h.close()


# ---- integer frames: equal ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('factor', [1, 4, 8])
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'int8', 'int16'])
def test_integer_frames_exact(hip, dtype, factor):
    csr = bins(SIG, factor)
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    rng = np.random.default_rng(G.seed(dtype, factor))
    for n in (1, 37, 130):
        x = frames(rng, dtype, n, N_PX)
        want = (csr.T.astype(np.int64) @ x.astype(np.int64).T).T
        assert np.abs(want).max() < 2**24
        res, kern = product(h, x, csr.shape[1])
        assert np.array_equal(res, want.astype(np.float32)), (kern, n)
        if factor == 1:
            assert np.array_equal(res, x.astype(np.float32))      # the frames themselves
    h.close()


# ---- float frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('factor', [1, 4, 8])
def test_float_frames(hip, factor):
    csr = bins(SIG, factor)
    h = hip.MaskHandle.csr(0, csr, np.float32)
    x = frames(np.random.default_rng(G.seed('f32', factor)), np.float32, 37, N_PX)
    res, kern = product(h, x, csr.shape[1])
    assert np.all(np.abs(res - stored_sum(csr, x)) <= 1e-5 * scale_of(csr, x)), kern
    again, _ = product(h, x, csr.shape[1])
    assert np.array_equal(res.view(np.uint32), again.view(np.uint32))     # the same bits
    h.close()


@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
def test_labels_across_chunks(hip, dtype):
    csr = rings()
    n_px = csr.shape[0]
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    x = frames(np.random.default_rng(G.seed('rings', dtype)), dtype, 70, n_px)
    ref, scale = stored_sum(csr, x), scale_of(csr, x)
    res, kern = product(h, x, 12)
    assert np.all(np.abs(res - ref) <= 1e-5 * scale), kern
    wide, _ = product(h, x, 12, ld_tile=n_px + 37)                       # ld_tile > n_px, rows at odd addresses
    assert np.array_equal(res.view(np.uint32), wide.view(np.uint32))
    h.close()


def test_many_labels(hip):
    csr = bins((128, 128), 1)                                            # 16 384 labels
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    x = frames(np.random.default_rng(7), np.uint16, 5, 128 * 128)
    res, kern = product(h, x, 128 * 128)
    assert np.array_equal(res, x.astype(np.float32)), kern
    h.close()


def test_accumulate_and_empty_columns(hip):
    """columns 3 and the last store nothing: 0 on a plain product, left alone when accumulating"""
    import scipy.sparse as sp
    b = bins(SIG, 4).tocoo()
    n_masks = b.shape[1] + 2
    csr = sp.csr_matrix((b.data, (b.row, np.where(b.col >= 3, b.col + 1, b.col))), shape=(N_PX, n_masks))
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    rng = np.random.default_rng(11)
    x = frames(rng, np.uint8, 70, N_PX)
    want = (csr.T.astype(np.int64) @ x.astype(np.int64).T).T.astype(np.float32)
    res, _ = product(h, x, n_masks)
    assert np.array_equal(res, want) and np.all(res[:, [3, n_masks - 1]] == 0)
    base = rng.integers(-100, 100, (70, n_masks)).astype(np.float32)
    res, _ = product(h, x, n_masks, base=base)
    assert np.array_equal(res, want + base) and np.array_equal(res[:, [3, n_masks - 1]], base[:, [3, n_masks - 1]])
    h.close()


def test_row_lists(hip):
    csr = bins(SIG, 4)
    h = hip.MaskHandle.csr(0, csr, np.float32)
    rng = np.random.default_rng(13)
    rows = np.array([69, 3, 3, 41, 0, 68, 41] + list(rng.integers(0, 70, 70)), dtype=np.int32)    # unsorted, repeated
    for dtype in (np.uint16, np.float32):
        x = frames(rng, dtype, 70, N_PX)
        plain, _ = product(h, np.ascontiguousarray(x[rows]), csr.shape[1])
        listed, _ = product(h, x, csr.shape[1], rows=rows)
        assert np.array_equal(plain.view(np.uint32), listed.view(np.uint32))
    h.close()


# ---- non-finite pixels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_pixels(hip, bad):
    import scipy.sparse as sp
    lab = rings()
    n_px = lab.shape[0]
    stored = np.flatnonzero(np.diff(lab.indptr))
    zero_px = int(stored[len(stored) // 2])
    zero_col = int(lab.indices[lab.indptr[zero_px]])
    data = lab.data.copy()
    data[lab.indptr[zero_px]] = 0                                        # a STORED zero
    csr = sp.csr_matrix((data, lab.indices, lab.indptr), shape=lab.shape)
    assert csr.nnz == lab.nnz
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    n = 70
    clean = frames(np.random.default_rng(17), np.float32, n, n_px)
    unlabelled = np.flatnonzero(np.diff(csr.indptr) == 0)
    last = n_px - 1                                                       # a corner: unlabelled
    assert last in unlabelled and 0 in unlabelled
    labelled_px = int(stored[7])
    labelled_col = int(csr.indices[csr.indptr[labelled_px]])
    last_stored = int(stored[-1])
    scale = scale_of(csr, clean)

    def run(x):
        res, kern = product(h, x, 12)
        assert h.nonfinite_frames() == 0, kern                           # nothing to check or redo on this kernel
        ref = stored_sum(csr, x)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(res), np.isnan(ref)) and np.array_equal(res[~fin & ~np.isnan(ref)],
                                                                               ref[~fin & ~np.isnan(ref)].astype(np.float32))
        assert np.all(np.abs(res[fin] - ref[fin]) <= 1e-5 * scale[fin]), kern
        return res

    # (a) unlabelled pixels, also the frame's last pixel and the last frame: every result is finite
    x = clean.copy()
    x[3, unlabelled[5]] = bad
    x[3, last] = bad
    x[n - 1, last] = bad
    x[n - 1, 0] = bad
    assert np.all(np.isfinite(run(x)))
    # (b) a labelled pixel: exactly one column of that frame; the last stored pixel in the last frame
    x = clean.copy()
    x[5, labelled_px] = bad
    x[n - 1, last_stored] = bad
    res = run(x)
    hit = np.argwhere(~np.isfinite(res))
    assert sorted(map(tuple, hit)) == sorted({(5, labelled_col), (n - 1, int(csr.indices[csr.indptr[last_stored]]))})
    # (c) a pixel stored with weight 0: 0 * NaN = NaN, 0 * Inf = NaN -- in frame 9 and in the last frame
    x = clean.copy()
    x[9, zero_px] = bad
    x[n - 1, zero_px] = bad
    res = run(x)
    assert np.isnan(res[9, zero_col]) and np.isnan(res[n - 1, zero_col]) and np.isnan(res).sum() == 2
    h.close()


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('weight', [0.75, 0.0])
def test_non_finite_last_pixel(hip, weight, bad):
    """the frame's LAST pixel stored -- pixel 3014 of 67 x 45, in the ragged sixth chunk whose loads take the guarded
    scalar path -- with a weight (case b) or with a stored zero (case c), non-finite in a middle frame and in the last
    frame: exactly the last bin of those frames is non-finite, NaN for the stored zero"""
    import scipy.sparse as sp
    lab = bins(SIG, 4)
    data = (0.5 + 0.01 * (np.arange(lab.nnz) % 13)).astype(np.float32)
    assert lab.indptr[N_PX] - lab.indptr[N_PX - 1] == 1
    data[lab.indptr[N_PX - 1]] = weight                                  # (0.0: a STORED zero)
    csr = sp.csr_matrix((data, lab.indices, lab.indptr), shape=lab.shape)
    assert csr.nnz == N_PX
    col = int(csr.indices[csr.indptr[N_PX - 1]])
    assert col == csr.shape[1] - 1
    h = hip.MaskHandle.csr(0, csr, np.float32)
    assert h.kind() == 4
    n = 70
    x = frames(np.random.default_rng(19), np.float32, n, N_PX)
    scale = scale_of(csr, x)
    x[33, N_PX - 1] = bad
    x[n - 1, N_PX - 1] = bad
    res, kern = product(h, x, csr.shape[1])
    assert h.nonfinite_frames() == 0, kern
    ref = stored_sum(csr, x)
    fin = np.isfinite(ref)
    assert sorted(map(tuple, np.argwhere(~fin))) == [(33, col), (n - 1, col)]
    assert np.array_equal(np.isnan(res), np.isnan(ref)) and np.array_equal(res[~fin & ~np.isnan(ref)],
                                                                           ref[~fin & ~np.isnan(ref)].astype(np.float32))
    if weight == 0:
        assert np.isnan(res[33, col]) and np.isnan(res[n - 1, col])
    assert np.all(np.abs(res[fin] - ref[fin]) <= 1e-5 * scale[fin]), kern
    h.close()


# ---- the gather kernel on the same inputs ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'float32'])
def test_against_the_gather_kernel(hip, dtype):
    for csr in (bins(SIG, 4), rings()):
        n_px, n_masks = csr.shape
        x = frames(np.random.default_rng(G.seed('gather', dtype, n_px)), dtype, 37, n_px)
        h = hip.MaskHandle.csr(0, csr, np.float32)
        new, _ = product(h, x, n_masks)
        h.close()
        g = hip.MaskHandle.csr(0, csr, np.float32, gather_only=True)
        assert g.kind() == 2
        old, _ = product(g, x, n_masks, expect='k_sell_apply<')
        g.close()
        if np.dtype(dtype).kind in 'iu' and n_px == N_PX:
            assert np.array_equal(new, old)
        else:
            assert np.all(np.abs(new - old) <= 1e-5 * scale_of(csr, x))
