"""
raw_csr datasets on the GPU (`-m gpu`): the sparse-frame kernels through the C ABI against scipy / float64
NumPy, and `run_udf` over a RawCSRDataSet against the reference's results (tests/golden/raw_csr.npz) and
against a MemoryDataSet of the densified frames.  Expected values come from the golden file, scipy and
NumPy only.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import raw_csr_recipes as recipes

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, 'golden', 'raw_csr.npz'))
CASES = {c['name']: c for c in recipes.CASES}
DTYPES = ('u1', 'u2', 'i2', 'u4', 'i4', 'f4')


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


def _dev(arr):
    arr = np.ascontiguousarray(arr)
    twin = {np.dtype('uint16'): np.int16, np.dtype('uint32'): np.int32, np.dtype('uint64'): np.int64}
    if arr.dtype in twin:
        arr = arr.view(twin[arr.dtype])
    return torch.from_numpy(arr).cuda()


def _host(t, dtype):
    a = t.cpu().numpy()
    return a if a.dtype == np.dtype(dtype) else a.view(dtype)


def edge_matrix(dtype, seed=0):
    """nav 4x4, sig 32x32 as a canonical CSR matrix (16, 1024): frame 0 and 15 (first / last of a tile)
    non-empty, an empty frame, a single-event frame, a frame with every pixel set (1024 events: several loop
    trips per lane), events at pixel 0 and at pixel n_px - 1"""
    rng = np.random.default_rng(seed)
    n, n_px = 16, 1024
    dt = np.dtype(dtype)
    dense = np.zeros((n, n_px), dtype=np.float64)
    for f in range(n):
        k = int(rng.integers(5, 120))
        px = rng.choice(n_px, k, replace=False)
        dense[f, px] = rng.integers(1, 100, k)
    dense[3] = 0                                            # empty
    dense[5] = 0
    dense[5, 517] = 9                                       # one event
    dense[7] = rng.integers(1, 100, n_px)                   # every pixel
    dense[0, 0] = 11                                        # pixel 0
    dense[15, n_px - 1] = 13                                # pixel n_px - 1
    if dt.kind == 'i':
        dense[1] = -dense[1]
    if dt.kind == 'f':
        dense = dense * 0.37
    m = sp.csr_matrix(dense.astype(dt))
    m.sort_indices()
    assert m[3].nnz == 0 and m[5].nnz == 1 and m[7].nnz == n_px
    return m


def small_matrix(dtype, seed=1):
    """35 frames of 117 pixels (a multiple of nothing) from the golden recipe of that dtype"""
    case = CASES[f'dtype_{dtype}']
    inp = recipes.make_case(case)
    m = sp.csr_matrix((inp['data'], inp['indices'], inp['indptr']), shape=(35, 117))
    m.sort_indices()
    return m


def upload(m):
    return dict(indptr=_dev(m.indptr.astype(np.int64)), indices=_dev(m.indices.astype(np.int32)),
                data=_dev(m.data), dtype=m.data.dtype, n=m.shape[0], n_px=m.shape[1])


# ---- ltmi_csr_check ------------------------------------------------------------------------------------
def test_check_flags(hip):
    m = edge_matrix('u2')
    d = upload(m)
    assert hip.csr_check(0, d['indptr'].data_ptr(), d['indices'].data_ptr(), 16, 1024, m.nnz) == 0
    swapped = m.indices.astype(np.int32).copy()
    a = int(m.indptr[7])
    swapped[a], swapped[a + 1] = swapped[a + 1], swapped[a]
    assert hip.csr_check(0, d['indptr'].data_ptr(), _dev(swapped).data_ptr(), 16, 1024, m.nnz) == 2
    dup = m.indices.astype(np.int32).copy()
    dup[a + 1] = dup[a]
    assert hip.csr_check(0, d['indptr'].data_ptr(), _dev(dup).data_ptr(), 16, 1024, m.nnz) == 2
    high = m.indices.astype(np.int32).copy()
    high[-1] = 1024
    assert hip.csr_check(0, d['indptr'].data_ptr(), _dev(high).data_ptr(), 16, 1024, m.nnz) & 1
    neg = m.indices.astype(np.int32).copy()
    neg[0] = -1
    assert hip.csr_check(0, d['indptr'].data_ptr(), _dev(neg).data_ptr(), 16, 1024, m.nnz) & 1
    ptr = m.indptr.astype(np.int64).copy()
    ptr[4] = ptr[3] - 1                                     # decreasing
    assert hip.csr_check(0, _dev(ptr).data_ptr(), d['indices'].data_ptr(), 16, 1024, m.nnz) & 1
    short = m.indptr.astype(np.int64).copy()
    short[-1] -= 1                                          # does not end at nnz
    assert hip.csr_check(0, _dev(short).data_ptr(), d['indices'].data_ptr(), 16, 1024, m.nnz) & 1


# ---- ltmi_csr_densify ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('make', (edge_matrix, small_matrix), ids=('32x32', '9x13'))
def test_densify_bit_exact(hip, dtype, make):
    m = make(dtype)
    d = upload(m)
    n, n_px = m.shape
    dense = m.toarray()
    # contiguous, all frames
    out = _dev(np.full((n, n_px), 7, dtype=m.dtype))
    hip.csr_densify(0, d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), m.dtype, 0, 0, n,
                    n_px, out.data_ptr(), n_px)
    assert np.array_equal(_host(out, m.dtype), dense)
    # frames [2, n - 1) into rows of ld > n_px at an odd element offset: the padding keeps its poison
    ld = n_px + 5
    buf = _dev(np.full(1 + n * ld, 7, dtype=m.dtype))
    hip.csr_densify(0, d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), m.dtype, 0, 2,
                    n - 3, n_px, buf.data_ptr() + m.dtype.itemsize, ld)
    got = _host(buf, m.dtype)
    rows = got[1:].reshape(n, ld)
    assert got[0] == 7
    assert np.array_equal(rows[:n - 3, :n_px], dense[2:n - 1])
    assert np.all(rows[:n - 3, n_px:] == 7) and np.all(rows[n - 3:] == 7)
    # a row list (unordered, one frame twice)
    sel = np.array([n - 1, 0, 7, 3, 7, 5], dtype=np.int32)
    out = _dev(np.full((len(sel), n_px), 7, dtype=m.dtype))
    hip.csr_densify(0, d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), m.dtype,
                    _dev(sel).data_ptr(), 0, len(sel), n_px, out.data_ptr(), n_px)
    assert np.array_equal(_host(out, m.dtype), dense[sel])


# ---- ltmi_apply_masks_csr ------------------------------------------------------------------------------
def _apply_csr(hip, m, masks2d, result_dtype, rows=None, row0=0, n=None, accumulate_into=None):
    d = upload(m)
    h = hip.MaskHandle.dense(0, masks2d, result_dtype)
    n = (m.shape[0] - row0 if rows is None else len(rows)) if n is None else n
    rd = np.dtype(result_dtype)
    ld = masks2d.shape[0] + 3
    out_np = np.full((n, ld), 7, dtype=rd) if accumulate_into is None else accumulate_into.astype(rd).copy()
    outs = []
    for _ in range(2):                                      # two launches: identical bits
        out = _dev(out_np)
        rows_dev = None if rows is None else _dev(np.asarray(rows, dtype=np.int32))
        ok = h.apply_csr(d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), m.dtype,
                         0 if rows_dev is None else rows_dev.data_ptr(), row0, n, out.data_ptr(), ld,
                         accumulate_into is not None)
        torch.cuda.synchronize()
        assert ok
        outs.append(_host(out, rd))
    kern = h.last_kernel()
    h.close()
    assert kern.startswith('k_apply_csr<')
    assert outs[0].tobytes() == outs[1].tobytes()
    assert np.all(outs[0][:, masks2d.shape[0]:] == out_np[:, masks2d.shape[0]:])      # padding of the rows
    return outs[0][:, :masks2d.shape[0]]


def _check_bound(got, m, masks2d, base=None):
    """every entry within the project's per-entry bound 1e-5 * sum |x| |w| of the float64 product"""
    x = m.toarray().astype(np.float64)
    w = masks2d.astype(np.float64)
    ref = x @ w.T + (0 if base is None else base.astype(np.float64))
    bound = 1e-5 * (np.abs(x) @ np.abs(w).T + (0 if base is None else np.abs(base)))
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bound), (float(err.max()), float(bound.min()))


@pytest.mark.parametrize('n_masks', (1, 3, 16, 17, 64))
@pytest.mark.parametrize('make', (edge_matrix, small_matrix), ids=('32x32', '9x13'))
def test_apply_csr_f32(hip, n_masks, make):
    m = make('u2')
    rng = np.random.default_rng(n_masks)
    masks = (rng.random((n_masks, m.shape[1])) - 0.3).astype(np.float32)
    got = _apply_csr(hip, m, masks, np.float32)
    assert got.dtype == np.float32
    _check_bound(got, m, masks)
    assert np.all(got[3] == 0) if make is edge_matrix else True        # the empty frame


@pytest.mark.parametrize('dtype', DTYPES)
def test_apply_csr_dtypes_exact(hip, dtype):
    """integer data with small integer-valued weights: every product and sum is exact in float32"""
    m = edge_matrix(dtype)
    rng = np.random.default_rng(5)
    masks = rng.integers(-3, 4, (3, m.shape[1])).astype(np.float32)
    rd = np.result_type(m.dtype, np.float32)
    got = _apply_csr(hip, m, masks, rd)
    assert got.dtype == rd
    if m.dtype.kind == 'f':
        _check_bound(got, m, masks)
    else:
        assert np.array_equal(got.astype(np.float64), m.toarray().astype(np.float64) @ masks.astype(np.float64).T)


@pytest.mark.parametrize('n_masks', (1, 3, 17, 64))
def test_apply_csr_f64(hip, n_masks):
    m = edge_matrix('i4')
    rng = np.random.default_rng(n_masks)
    masks = rng.random((n_masks, m.shape[1])) - 0.3
    got = _apply_csr(hip, m, masks, np.float64)
    assert got.dtype == np.float64
    x = m.toarray().astype(np.float64)
    # float64 accumulation: 1e-13 of the sum of magnitudes covers 1024 terms of 2^-53 relative error each
    assert np.all(np.abs(got - x @ masks.T) <= 1e-13 * (np.abs(x) @ np.abs(masks).T))


def test_apply_csr_accumulate_rows_and_range(hip):
    m = edge_matrix('u2')
    rng = np.random.default_rng(9)
    masks = (rng.random((16, m.shape[1])) - 0.3).astype(np.float32)
    base = rng.random((16, 19)).astype(np.float32) * 100
    got = _apply_csr(hip, m, masks, np.float32, accumulate_into=base)
    _check_bound(got, m, masks, base=base[:, :16])
    sel = [15, 0, 7, 3, 7, 5]
    got = _apply_csr(hip, m, masks, np.float32, rows=sel)
    _check_bound(got, m[sel], masks)
    got = _apply_csr(hip, m, masks, np.float32, row0=2, n=13)
    _check_bound(got, m[2:15], masks)


def test_apply_csr_not_handled(hip):
    """more masks than the cap, complex and integer stacks: nothing is done, the caller densifies"""
    m = edge_matrix('u2')
    d = upload(m)
    from libertem_amd.udf.masks import CSR_DIRECT_MAX_MASKS
    assert hip.csr_max_masks() == CSR_DIRECT_MAX_MASKS == 64      # (the kernel's cap and the UDF's are one number)
    for masks, rd in ((np.ones((65, 1024), np.float32), np.float32), (np.ones((2, 1024), np.complex64), np.complex64),
                      (np.ones((2, 1024), np.int32), np.int32)):
        h = hip.MaskHandle.dense(0, masks, rd)
        out = _dev(np.full((16, masks.shape[0]), 7, dtype=rd))
        assert not h.apply_csr(d['indptr'].data_ptr(), d['indices'].data_ptr(), d['data'].data_ptr(), m.dtype, 0, 0,
                               16, out.data_ptr(), masks.shape[0], False)
        torch.cuda.synchronize()
        assert np.all(_host(out, rd) == 7)
        h.close()


# ---- run_udf -------------------------------------------------------------------------------------------
def _load(ctx, tmp_path, case, inp, **kw):
    path = recipes.write_files(case, inp, str(tmp_path), **kw)
    return ctx.load('raw_csr', path=path, sync_offset=case['sync_offset'], num_partitions=case['num_partitions'])


def _positioned(case, inp):
    frames = recipes.dense_frames(inp)
    n, so = frames.shape[0], case['sync_offset']
    out = np.zeros_like(frames)
    for p in range(n):
        if 0 <= p + so < n:
            out[p] = frames[p + so]
    return out.reshape(recipes.NAV + recipes.SIG)


def _last_kernels(udf):
    return [h.last_kernel() for h in udf.masks._handle_cache.values()]


@pytest.mark.parametrize('name', sorted(CASES))
def test_golden_apply_masks_direct(ctx, tmp_path, name):
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    case = CASES[name]
    inp = recipes.make_case(case)
    masks = inp['masks']
    ds = _load(ctx, tmp_path, case, inp)
    udf = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                        mask_dtype=masks.dtype)
    res = ctx.run_udf(dataset=ds, udf=[udf, SumUDF(), SumSigUDF()], roi=inp['roi'])
    kernels = _last_kernels(udf)
    assert kernels and all(k.startswith('k_apply_csr<') for k in kernels), kernels
    got = res[0]['intensity'].data
    gold = GOLDEN[f'{name}__masks']
    assert got.shape == gold.shape and got.dtype == gold.dtype
    dense = _positioned(case, inp).astype(np.float64)
    w = masks.reshape(len(masks), -1).astype(np.float64)
    x = dense.reshape(35, -1)
    ref = (x @ w.T).reshape(recipes.NAV + (len(masks),))
    bound = (1e-5 * (np.abs(np.nan_to_num(x)) @ np.abs(w).T)).reshape(ref.shape)
    roi = inp['roi'] if inp['roi'] is not None else np.ones(recipes.NAV, dtype=bool)
    assert np.all(np.isnan(got[~roi]))
    ok = np.isfinite(ref) & roi[..., None]
    assert np.array_equal(np.isnan(got[roi]), np.isnan(ref[roi]))
    assert np.all(np.abs(got - ref)[ok] <= bound[ok])
    if name == 'sync_m4_roi':
        # (the reference puts the per-frame rows of the first partition early: tests/test_raw_csr_cpu.py)
        assert np.all(np.abs(np.sort(got[roi], axis=0) - np.sort(gold[roi], axis=0)) <= bound[roi].max())
    else:
        assert np.array_equal(np.isnan(got), np.isnan(gold))
        assert np.all(np.abs(got - gold)[ok] <= bound[ok])
    gs = GOLDEN[f'{name}__sum']
    fin = np.isfinite(gs)
    assert np.array_equal(np.isnan(res[1]['intensity'].data), np.isnan(gs))
    assert np.all(np.abs(res[1]['intensity'].data - gs)[fin] <= 1e-5 * np.abs(dense[roi]).sum(axis=0)[fin] + 1e-30)


def _route_udfs():
    from libertem_amd.udf.masks import ApplyMasksUDF, CSR_DIRECT_MAX_MASKS
    rng = np.random.default_rng(77)
    sig = recipes.SIG
    many = (rng.random((CSR_DIRECT_MAX_MASKS + 1,) + sig) - 0.3).astype(np.float32)
    three = (rng.random((3,) + sig) - 0.3).astype(np.float32)
    cplx = (three + 1j * three[::-1]).astype(np.complex64)
    ints = rng.integers(-3, 4, (3,) + sig).astype(np.int32)
    return {
        'cap_plus_1': (ApplyMasksUDF(mask_factories=lambda: many, use_sparse=False), many, None),
        'shifts': (ApplyMasksUDF(mask_factories=lambda: three, use_sparse=False, shifts=(1, -2)), three, (1, -2)),
        'complex': (ApplyMasksUDF(mask_factories=lambda: cplx, use_sparse=False), cplx, None),
        'integer': (ApplyMasksUDF(mask_factories=lambda: ints, use_sparse=False), ints, None),
        'use_sparse': (ApplyMasksUDF(mask_factories=lambda: three, use_sparse=True), three, None),
    }


@pytest.mark.parametrize('route', ('cap_plus_1', 'shifts', 'complex', 'integer', 'use_sparse'))
def test_materialise_routes(ctx, tmp_path, route):
    case = CASES['dtype_u2']
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    udf, masks, shift = _route_udfs()[route]
    got = ctx.run_udf(dataset=ds, udf=udf)['intensity'].data
    kernels = _last_kernels(udf)
    assert kernels and not any('k_apply_csr' in k for k in kernels), kernels
    dense = recipes.dense_frames(inp)
    if shift is not None:
        moved = np.zeros_like(masks)
        dy, dx = shift
        h, w = recipes.SIG
        moved[:, max(0, dy):min(h, h + dy), max(0, dx):min(w, w + dx)] = \
            masks[:, max(0, -dy):min(h, h - dy), max(0, -dx):min(w, w - dx)]
        masks = moved
    wide = np.complex128 if np.iscomplexobj(masks) else np.float64
    x, w2 = dense.reshape(35, -1).astype(wide), masks.reshape(len(masks), -1).astype(wide)
    ref = (x @ w2.T).reshape(recipes.NAV + (len(masks),))
    # (the frames reach the UDF as result_type(float32, u2) = float32, the preferred input dtype)
    assert got.dtype == np.result_type(np.result_type(np.float32, dense.dtype), masks.dtype)
    if got.dtype.kind in 'iu':
        assert np.array_equal(got, ref.astype(got.dtype))
    else:
        bound = (1e-5 * (np.abs(x) @ np.abs(w2).T)).reshape(ref.shape)
        assert np.all(np.abs(got - ref) <= bound)


def test_stored_nan_on_the_materialise_route(ctx, tmp_path, monkeypatch):
    """the f4 case with a NaN in a stored entry through densify + the dense kernels (no stack is eligible for the
    direct kernel with a cap of 0): the golden's result, as on the direct route"""
    from libertem_amd.udf import masks as masks_mod
    monkeypatch.setattr(masks_mod, 'CSR_DIRECT_MAX_MASKS', 0)
    case = CASES['nan_f4']
    inp = recipes.make_case(case)
    masks = inp['masks']
    ds = _load(ctx, tmp_path, case, inp)
    udf = masks_mod.ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                                  mask_dtype=masks.dtype)
    got = ctx.run_udf(dataset=ds, udf=udf, roi=inp['roi'])['intensity'].data
    kernels = _last_kernels(udf)
    assert kernels and not any('k_apply_csr' in k for k in kernels), kernels
    gold = GOLDEN['nan_f4__masks']
    assert got.shape == gold.shape and got.dtype == gold.dtype
    assert np.isnan(gold).any() and not np.isnan(gold).all()
    assert np.array_equal(np.isnan(got), np.isnan(gold))
    x = np.abs(np.nan_to_num(_positioned(case, inp).astype(np.float64))).reshape(35, -1)
    bound = (1e-5 * (x @ np.abs(masks.reshape(len(masks), -1).astype(np.float64)).T)).reshape(gold.shape)
    fin = np.isfinite(gold)
    assert np.all(np.abs(got - gold)[fin] <= bound[fin])


@pytest.mark.parametrize('name', ('dtype_u2', 'sync_m4'))
def test_com_and_pick_equal_memory_dataset(ctx, tmp_path, name):
    """CoMUDF takes the sparse view (direct kernel, accumulating into its private buffer), PickUDF the densified
    frames: both as on a MemoryDataSet of the same frames"""
    from libertem_amd.udf.com import CoMUDF
    from libertem_amd.udf.raw import PickUDF
    case = CASES[name]
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    dense = recipes.dense_frames(inp).reshape(recipes.NAV + recipes.SIG)
    mem = ctx.load('memory', data=dense, sig_dims=2, num_partitions=case['num_partitions'],
                   sync_offset=case['sync_offset'])
    a = ctx.run_udf(dataset=ds, udf=CoMUDF.with_params(cy=4., cx=6., r=5.))
    b = ctx.run_udf(dataset=mem, udf=CoMUDF.with_params(cy=4., cx=6., r=5.))
    # raw_com = sum(x w) / sum(x) with x >= 0 and coordinates |w| <= 13: the numerator is within 1e-5 * 13 * sum(x)
    # of the exact one (the project's per-entry bound), the denominator within 1e-5 * sum(x), so a quotient is within
    # 2 * 1e-5 * 13 of the exact one on either dataset and the two agree to 4 * 1e-5 * 13
    for key in ('raw_com', 'field'):
        assert a[key].data.shape == b[key].data.shape
        assert np.array_equal(np.isnan(a[key].data), np.isnan(b[key].data))
        assert np.allclose(a[key].data, b[key].data, rtol=0, atol=4e-5 * 13, equal_nan=True), key
    roi = np.zeros(recipes.NAV, dtype=bool)
    roi[1, 2] = roi[3, 0] = roi[4, 6] = True
    pa = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=roi)['intensity'].data
    pb = ctx.run_udf(dataset=mem, udf=PickUDF(), roi=roi)['intensity'].data
    assert pa.dtype == pb.dtype and np.array_equal(pa, pb)


@pytest.mark.parametrize('name', ('dtype_u2', 'sync_p3_roi', 'sync_m4', 'parts3', 'dtype_f4'))
def test_dense_udfs_equal_memory_dataset(ctx, tmp_path, name):
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.stddev import StdDevUDF
    from libertem_amd.udf.logsum import LogsumUDF
    case = CASES[name]
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    mem = ctx.load('memory', data=recipes.dense_frames(inp).reshape(recipes.NAV + recipes.SIG), sig_dims=2,
                   num_partitions=case['num_partitions'], sync_offset=case['sync_offset'])
    for make, keys in ((SumUDF, ('intensity',)), (StdDevUDF, ('varsum', 'num_frames', 'sum')),
                       (LogsumUDF, ('logsum',))):
        a = ctx.run_udf(dataset=ds, udf=make(), roi=inp['roi'])
        b = ctx.run_udf(dataset=mem, udf=make(), roi=inp['roi'])
        for key in keys:
            # the same kernels on the same dense frames, partitions and tiles: the same bits (NaN where no frame is)
            assert a[key].data.shape == b[key].data.shape and a[key].data.dtype == b[key].data.dtype
            assert np.array_equal(a[key].data, b[key].data, equal_nan=True), (make.__name__, key)


def test_same_udf_twice(ctx, tmp_path):
    """a cached plan over tiles that are not stable between runs"""
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.udf.sum import SumUDF
    case = CASES['parts3']
    inp = recipes.make_case(case)
    masks = inp['masks']
    ds = _load(ctx, tmp_path, case, inp)
    assert ds.stable_device_tiles is False
    for udf, key in ((ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False), 'intensity'),
                     (SumUDF(), 'intensity')):
        first = ctx.run_udf(dataset=ds, udf=udf)[key].data.copy()
        second = ctx.run_udf(dataset=ds, udf=udf)[key].data.copy()
        third = ctx.run_udf(dataset=ds, udf=udf)[key].data.copy()
        assert first.tobytes() == second.tobytes() == third.tobytes()
        assert np.any(first != 0)


def test_unsorted_and_duplicates_are_canonicalised(ctx, tmp_path):
    from libertem_amd.udf.masks import ApplyMasksUDF
    case = CASES['dtype_u2']
    inp = recipes.make_case(case)
    masks = inp['masks']
    udf = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False)
    ds = _load(ctx, tmp_path, case, inp)
    assert ds.canonicalised is False
    want = ctx.run_udf(dataset=ds, udf=udf)['intensity'].data
    # every row reversed; the last entry of frame 0 split into two entries for the same pixel
    indptr, indices, data = inp['indptr'], inp['indices'].copy(), inp['data'].copy()
    for a, b in zip(indptr[:-1], indptr[1:]):
        indices[a:b], data[a:b] = indices[a:b][::-1].copy(), data[a:b][::-1].copy()
    k = int(indptr[1]) - 1
    extra = data[k] - data[k] // 2
    data[k] //= 2
    indices2 = np.insert(indices, k, indices[k])
    data2 = np.insert(data, k, extra)
    indptr2 = indptr.copy()
    indptr2[1:] += 1
    ds2 = _load(ctx, tmp_path, case, inp, name='messy', indptr=indptr2, indices=indices2, data=data2)
    assert ds2.canonicalised is True
    got = ctx.run_udf(dataset=ds2, udf=udf)['intensity'].data
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize('idx', ('<i4', '<i8'))
def test_out_of_range_index_raises(ctx, tmp_path, idx):
    from libertem_amd.io.dataset.base import DataSetException
    case = dict(CASES['dtype_u2'], indices_dtype=idx)
    inp = recipes.make_case(case)
    bad = inp['indices'].copy()
    bad[len(bad) // 2] = 117
    with pytest.raises(DataSetException):
        _load(ctx, tmp_path, case, inp, indices=bad)
