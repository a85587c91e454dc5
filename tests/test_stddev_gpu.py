"""
StdDevUDF on the MI355X: `ltmi_moments_frames` against an exact restatement (Python integers for
integer frames, np.longdouble two-pass for float frames) over every tile dtype x result dtype, a
long-run stability case, bitwise repeatability, and the UDF on device-resident and host-streamed
data against the reference's results (tests/golden/stddev.npz).
"""
import os

import numpy as np
import pytest

import stddev_recipes

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

TILE_DTYPES = ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32', 'float64',
               'complex64', 'complex128']
KEYS = ('sum', 'varsum', 'num_frames', 'var', 'std', 'mean')
CONST_PX = (0, 5, 77)             # pixels with the same value in every frame


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'stddev.npz'))


def _frames(dt, n, n_px, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind == 'u':
        hi = min(np.iinfo(dt).max, 2 ** 31)
        x = rng.integers(0, hi, (n, n_px), endpoint=True).astype(dt)
    elif dt.kind == 'i':
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, (n, n_px), endpoint=True).astype(dt)
    elif dt.kind == 'c':
        x = (rng.normal(3., 2., (n, n_px)) + 1j * rng.normal(-1., 1., (n, n_px))).astype(dt)
    else:
        x = rng.normal(2., 1.5, (n, n_px)).astype(dt)
    for p in (c for c in CONST_PX if c < n_px):
        x[:, p] = 7 if dt.kind in 'iu' else 2.5
    return x


def _exact(x):
    """-> (sum, varsum, mean) of the frames x (n, n_px) as float64 from exact / extended arithmetic"""
    n = x.shape[0]
    if x.dtype.kind in 'iu':
        xo = x.astype(object)
        s = xo.sum(axis=0)
        q = (xo * xo).sum(axis=0)
        from fractions import Fraction
        var = np.array([float(Fraction(int(qq) * n - int(ss) * int(ss), n)) for ss, qq in zip(s, q)])
        return s.astype(np.float64), var, (s.astype(np.float64) / n)
    if x.dtype.kind == 'c':
        re, im = (np.ascontiguousarray(x.real.T).astype(np.longdouble),
                  np.ascontiguousarray(x.imag.T).astype(np.longdouble))
        mr, mi = re.sum(axis=1) / n, im.sum(axis=1) / n
        var = (((re - mr[:, None]) ** 2).sum(axis=1) + ((im - mi[:, None]) ** 2).sum(axis=1))
        return ((mr * n).astype(np.float64) + 1j * (mi * n).astype(np.float64), var.astype(np.float64),
                mr.astype(np.float64) + 1j * mi.astype(np.float64))
    xl = np.ascontiguousarray(x.T).astype(np.longdouble)
    m = xl.sum(axis=1) / n
    var = ((xl - m[:, None]) ** 2).sum(axis=1)
    return (m * n).astype(np.float64), var.astype(np.float64), m.astype(np.float64)


def _run_kernel(x, sum_dt, var_dt, split, pad=5, offset=1, repeat=1):
    """fold x (n, n_px) in two calls (frames [0, split), [split, n)) into fresh buffers; tile rows
    of ld = n_px + pad, starting `offset` elements into the allocation (unaligned rows)"""
    from libertem_amd import hip
    n, n_px = x.shape
    ld = n_px + pad
    host = np.zeros((n * ld + offset,), dtype=x.dtype)
    host[offset:].reshape((n, ld))[:, :n_px] = x
    storage = host.view(np.int16) if x.dtype == np.uint16 else host.view(np.int32) \
        if x.dtype == np.uint32 else host
    tile = torch.from_numpy(storage).cuda()
    isz = x.dtype.itemsize
    outs = []
    for _ in range(repeat):
        sm = torch.zeros((n_px * np.dtype(sum_dt).itemsize,), dtype=torch.uint8, device='cuda')
        vs = torch.zeros((n_px * np.dtype(var_dt).itemsize,), dtype=torch.uint8, device='cuda')
        n_prev = 0
        for a, b in ((0, split), (split, n)):
            if b <= a:
                continue
            ws = torch.empty((max(16, hip.moments_workspace(b - a, n_px, x.dtype)),), dtype=torch.uint8,
                             device='cuda')
            hip.moments_frames(0, tile.data_ptr() + (offset + a * ld) * isz, x.dtype, b - a, n_px, ld,
                               n_prev, sm.data_ptr(), sum_dt, vs.data_ptr(), var_dt, ws.data_ptr())
            n_prev += b - a
        torch.cuda.synchronize()
        outs.append((sm.cpu().numpy().view(sum_dt), vs.cpu().numpy().view(var_dt)))
    return outs if repeat > 1 else outs[0]


def _result_dtypes(tile_dt):
    if np.dtype(tile_dt).kind == 'c':
        return [('complex128', 'float64'), ('complex64', 'float32'), ('complex128', 'float32')] \
            if tile_dt == 'complex64' else [('complex128', 'float64'), ('complex64', 'float32')]
    return [('float64', 'float64'), ('float32', 'float32'), ('float64', 'float32'), ('float32', 'float64')]


CASES = [(t, s, v) for t in TILE_DTYPES for s, v in _result_dtypes(t)]


@pytest.mark.parametrize('tile_dt,sum_dt,var_dt', CASES, ids=['-'.join(c) for c in CASES])
@pytest.mark.parametrize('split', [0, 29], ids=['n_prev0', 'n_prev29'])
def test_moments_kernel_exact(tile_dt, sum_dt, var_dt, split):
    n, n_px = 83, 1003                # n_px not a multiple of any vector width
    x = _frames(tile_dt, n, n_px, seed=100 + 2 * TILE_DTYPES.index(tile_dt) + (split > 0))
    got_sum, got_var = _run_kernel(x, sum_dt, var_dt, split)
    s, var, mean = _exact(x)
    const = list(CONST_PX)
    assert np.all(got_var[const] == 0), got_var[const]
    mean2 = np.abs(mean) ** 2
    if var_dt == 'float64' and sum_dt in ('float64', 'complex128'):
        assert np.all(np.abs(got_var - var) <= 1e-12 * var + 1e-15 * n * mean2), \
            np.max(np.abs(got_var - var) / np.maximum(var, 1e-300))
    else:
        assert np.allclose(got_var, var, rtol=1e-6, atol=1e-6 * var.max())
    stol = 1e-6 if np.dtype(sum_dt) in (np.float32, np.complex64) else 1e-13
    assert np.allclose(got_sum, s, rtol=stol, atol=stol * np.abs(s).max())


def test_moments_kernel_strided_output():
    """partial-width sig slice: tile pixels land in a strided sub-rectangle (rows of `cols` at ld_out)"""
    from libertem_amd import hip
    x = _frames('uint16', 40, 6 * 7, seed=5)
    H, W, r0, c0 = 10, 20, 3, 4
    tile = torch.from_numpy(x.view(np.int16)).cuda()
    sm = torch.full((H, W), -1., dtype=torch.float64, device='cuda')
    vs = torch.full((H, W), -1., dtype=torch.float64, device='cuda')
    ws = torch.empty((max(16, hip.moments_workspace(40, 42, np.uint16)),), dtype=torch.uint8, device='cuda')
    off = r0 * W + c0
    hip.moments_frames(0, tile.data_ptr(), np.uint16, 40, 42, 42, 0, sm.data_ptr() + off * 8, np.float64,
                       vs.data_ptr() + off * 8, np.float64, ws.data_ptr(), cols=7, ld_out=W)
    s, var, _ = _exact(x)
    got_s, got_v = sm.cpu().numpy(), vs.cpu().numpy()
    assert np.allclose(got_s[r0:r0 + 6, c0:c0 + 7].reshape(-1), s, rtol=1e-15)
    assert np.allclose(got_v[r0:r0 + 6, c0:c0 + 7].reshape(-1), var, rtol=1e-12)
    mask = np.ones((H, W), dtype=bool)
    mask[r0:r0 + 6, c0:c0 + 7] = False
    assert np.all(got_s[mask] == -1) and np.all(got_v[mask] == -1)


def test_moments_stability_long_run():
    """float32 frames of 1e4 + N(0, 1) over 10^6 frames, float64 results: 1e-10 relative"""
    from libertem_amd import hip
    n, n_px = 1_000_000, 64
    g = torch.Generator(device='cuda').manual_seed(1234)
    x = (torch.randn((n, n_px), generator=g, device='cuda', dtype=torch.float64) + 1e4).to(torch.float32)
    sm = torch.empty((n_px,), dtype=torch.float64, device='cuda')
    vs = torch.empty((n_px,), dtype=torch.float64, device='cuda')
    ws = torch.empty((max(16, hip.moments_workspace(n, n_px, np.float32)),), dtype=torch.uint8, device='cuda')
    hip.moments_frames(0, x.data_ptr(), np.float32, n, n_px, n_px, 0, sm.data_ptr(), np.float64,
                       vs.data_ptr(), np.float64, ws.data_ptr())
    torch.cuda.synchronize()
    # reference: two passes in float64 with pairwise sums along contiguous rows
    xt = np.ascontiguousarray(x.cpu().numpy().T).astype(np.float64)
    mean = xt.sum(axis=1) / n
    var = ((xt - mean[:, None]) ** 2).sum(axis=1)
    got = vs.cpu().numpy()
    assert np.all(np.abs(got - var) <= 1e-10 * var), np.max(np.abs(got - var) / var)
    assert np.allclose(sm.cpu().numpy() / n, mean, rtol=1e-12)


@pytest.mark.parametrize('tile_dt', ['uint16', 'float32', 'complex64'])
def test_moments_bitwise_repeatable(tile_dt):
    x = _frames(tile_dt, 4096, 3001, seed=9)
    sum_dt = 'complex128' if tile_dt == 'complex64' else 'float64'
    (s1, v1), (s2, v2) = _run_kernel(x, sum_dt, 'float64', 1000, repeat=2)
    assert s1.tobytes() == s2.tobytes() and v1.tobytes() == v2.tobytes()


def test_moments_non_finite_pixels_propagate():
    """a NaN / inf pixel gives a NaN variance, in one slab and over several, as NumPy's two passes do"""
    for n, split in ((10, 0), (200, 0), (200, 70)):
        x = _frames('float32', n, 300, seed=21)
        x[3, 11] = np.nan
        x[n - 1, 12] = np.inf
        got_sum, got_var = _run_kernel(x, 'float64', 'float64', split)
        assert np.isnan(got_var[11]) and np.isnan(got_var[12]), (n, split, got_var[11:13])
        assert np.isnan(got_sum[11]) and not np.isfinite(got_sum[12])
        ok = np.ones(300, dtype=bool)
        ok[[11, 12]] = False
        assert np.all(np.isfinite(got_var[ok]))


def test_moments_rejects_bad_arguments():
    from libertem_amd import hip
    x = torch.zeros((4, 16), dtype=torch.float32, device='cuda')
    out = torch.zeros((16,), dtype=torch.float64, device='cuda')
    ws = torch.empty((4096,), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match=r'unsupported dtypes.*\(code -2\)'):     # LTMI_E_DTYPE: complex sum of real frames
        hip.moments_frames(0, x.data_ptr(), np.float32, 4, 16, 16, 0, out.data_ptr(), np.complex128,
                           out.data_ptr(), np.float64, ws.data_ptr())
    with pytest.raises(ValueError, match=r'do not fit.*\(code -3\)'):     # LTMI_E_SHAPE: 16 pixels are not rows of 5
        hip.moments_frames(0, x.data_ptr(), np.float32, 4, 16, 16, 0, out.data_ptr(), np.float64,
                           out.data_ptr(), np.float64, ws.data_ptr(), cols=5, ld_out=5)


# --- the UDF ---------------------------------------------------------------------------------------
def _check(res, golden, name, corrected=False):
    tol = 1e-5 if golden[f'{name}__varsum'].dtype == np.float32 else 1e-12
    if corrected:
        # corrected float32 tiles: ltmi_correct rounds (x - dark) * gain once, the reference's
        # float32 arithmetic twice -- tiles one ulp apart
        tol = 1e-6
    for k in KEYS:
        got, exp = np.asarray(res[k].data), golden[f'{name}__{k}']
        assert got.dtype == exp.dtype and got.shape == exp.shape, (k, got.dtype, exp.dtype)
        if k == 'num_frames':
            assert np.array_equal(got, exp), (got, exp)
        else:
            assert np.allclose(got, exp, rtol=tol, atol=tol * np.abs(exp).max()), \
                (k, np.abs(got - exp).max(), np.abs(exp).max())


def _udf_inputs(case, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.io.corrections import CorrectionSet
    data, roi, corr = stddev_recipes.make_stddev_case(case)
    kw = dict(num_partitions=case['num_partitions'], sig_dims=2, tileshape=case.get('tileshape'))
    if case.get('sync_offset'):
        kw['sync_offset'] = case['sync_offset']
    src = HipArray.from_numpy(data, 0) if resident else data
    corrections = None if corr is None else CorrectionSet(dark=corr[0], gain=corr[1])
    return src, kw, roi, corrections


# (a sync_offset of a MemoryDataSet needs host data: those cases run host-streamed only)
UDF_CASES = [(c, r) for c in stddev_recipes.STDDEV_CASES for r in (True, False)
             if not (r and c.get('sync_offset'))]


@pytest.mark.parametrize('case,resident', UDF_CASES,
                         ids=[c['name'] + ('-resident' if r else '-streamed') for c, r in UDF_CASES])
def test_stddev_udf_vs_golden(ctx, golden, case, resident):
    from libertem_amd.udf.stddev import StdDevUDF
    src, kw, roi, corrections = _udf_inputs(case, resident)
    ds = ctx.load('memory', data=src, **kw)
    res = ctx.run_udf(dataset=ds, udf=StdDevUDF(**case.get('udf_kwargs', {})), roi=roi,
                      corrections=corrections)
    _check(res, golden, case['name'], corrected=corrections is not None)


@pytest.mark.parametrize('case', [c for c in stddev_recipes.STDDEV_CASES if c.get('sync_offset')],
                         ids=lambda c: c['name'])
def test_stddev_raw_file_sync_offset_and_roi(ctx, golden, case, tmp_path):
    from libertem_amd.udf.stddev import StdDevUDF
    data, _, _ = stddev_recipes.make_stddev_case(case)
    path = str(tmp_path / 'scan.raw')
    data.tofile(path)
    ds = ctx.load('raw', path=path, dtype=data.dtype, nav_shape=tuple(case['nav']),
                  sig_shape=tuple(case['sig']), sync_offset=case['sync_offset'],
                  num_partitions=case['num_partitions'])
    _check(ctx.run_udf(dataset=ds, udf=StdDevUDF()), golden, case['name'])
    # ROI over the blank positions and frames that exist
    n_nav = int(np.prod(case['nav']))
    roi = np.zeros(n_nav, dtype=bool)
    roi[[0, 1, 2, 4, 9, n_nav - 4, n_nav - 2, n_nav - 1]] = True
    roi = roi.reshape(case['nav'])
    res = ctx.run_udf(dataset=ds, udf=StdDevUDF(), roi=roi)
    so = case['sync_offset']
    flat = data.reshape((n_nav, -1)).astype(np.float64)
    pos = np.flatnonzero(roi.reshape(-1))
    src = pos + so
    sel = flat[src[(src >= 0) & (src < n_nav)]]
    assert res['num_frames'].data[0] == len(sel)
    assert np.allclose(res['var'].data.reshape(-1), sel.var(axis=0), rtol=1e-12)
    assert np.allclose(res['mean'].data.reshape(-1), sel.mean(axis=0), rtol=1e-12)


def test_stddev_memory_sync_offset_roi(ctx):
    from libertem_amd.udf.stddev import StdDevUDF
    data = np.random.default_rng(4).integers(0, 900, (6, 6, 16, 16)).astype(np.uint16)
    flat = data.reshape((36, -1)).astype(np.float64)
    roi = np.zeros(36, dtype=bool)
    roi[[0, 1, 5, 20, 33, 34, 35]] = True
    for so in (3, -3):
        ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2, sync_offset=so)
        res = ctx.run_udf(dataset=ds, udf=StdDevUDF(), roi=roi.reshape((6, 6)))
        src = np.flatnonzero(roi) + so
        sel = flat[src[(src >= 0) & (src < 36)]]
        assert res['num_frames'].data[0] == len(sel)
        assert np.allclose(res['var'].data.reshape(-1), sel.var(axis=0), rtol=1e-12)


@pytest.mark.parametrize('resident', [True, False], ids=['resident', 'streamed'])
def test_stddev_run_udf_iter_last_equals_run_udf(ctx, resident):
    from libertem_amd.udf.stddev import StdDevUDF
    from libertem_amd.common.hiparray import HipArray
    data = np.random.default_rng(8).normal(10., 2., (6, 8, 24, 24)).astype(np.float32)
    src = HipArray.from_numpy(data, 0) if resident else data
    ds = ctx.load('memory', data=src, num_partitions=4, sig_dims=2)
    parts = [{k: np.array(p.buffers[0][k].data) for k in ('sum', 'varsum', 'num_frames')}
             for p in ctx.run_udf_iter(dataset=ds, udf=StdDevUDF())]
    assert len(parts) == 4
    assert [int(p['num_frames'][0]) for p in parts] == [12, 24, 36, 48]
    full = ctx.run_udf(dataset=ds, udf=StdDevUDF())
    for k in ('sum', 'varsum', 'num_frames'):
        assert np.array_equal(parts[-1][k], np.asarray(full[k].data)), k
    flat = data.reshape((48, -1)).astype(np.float64)
    assert np.allclose(full['var'].data.reshape(-1), flat.var(axis=0), rtol=1e-12)


def test_stddev_reused_udf_on_device(ctx):
    """kept task instances (REUSE_TASK_INSTANCES): the frame counters restart with every run"""
    from libertem_amd.udf.stddev import StdDevUDF
    from libertem_amd.common.hiparray import HipArray
    data = np.random.default_rng(12).integers(0, 4000, (8, 8, 32, 32)).astype(np.uint16)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=4, sig_dims=2)
    udf = StdDevUDF()
    r = [ctx.run_udf(dataset=ds, udf=udf) for _ in range(3)]
    for x in r:
        assert x['num_frames'].data[0] == 64
        assert np.array_equal(x['varsum'].data, r[0]['varsum'].data)
    s, var, _ = _exact(data.reshape((64, -1)))
    assert np.allclose(r[0]['varsum'].data.reshape(-1), var, rtol=1e-12)


MIB_CASE = dict(name='sd_u16', kind='u', bits=16, sig=(32, 64), frames=(7, 5), nav=(3, 4), seed=1401)


@pytest.mark.parametrize('streamed', [False, True], ids=['resident', 'streamed'])
@pytest.mark.parametrize('sync_offset', [3, -3])
def test_stddev_mib_sync_offset(ctx, tmp_path, monkeypatch, sync_offset, streamed):
    """.mib series: positions a sync_offset leaves without a frame are not counted (resident and
    windowed-decode datasets), with and without an ROI"""
    import recipes
    from libertem_amd.io.dataset.mib import MIBDataSet
    from libertem_amd.udf.stddev import StdDevUDF
    frames, files, hdr = recipes.make_mib_case(MIB_CASE)
    for fn, blob in files.items():
        (tmp_path / fn).write_bytes(blob)
    hdr_path = tmp_path / (MIB_CASE['name'] + '.hdr')
    hdr_path.write_text(hdr)
    if streamed:
        monkeypatch.setattr(MIBDataSet, 'MAX_RESIDENT_BYTES', 2 * 32 * 64 * 2)
    ds = ctx.load('mib', path=str(hdr_path), sync_offset=sync_offset)
    monkeypatch.setattr(MIBDataSet, 'MAX_RESIDENT_BYTES', None)
    assert ds.is_streamed == streamed
    n_nav = 12
    flat = frames.reshape((len(frames), -1)).astype(np.float64)
    for roi in (None, np.isin(np.arange(n_nav), [0, 1, 2, 5, 9, 10, 11]).reshape((3, 4))):
        pos = np.arange(n_nav) if roi is None else np.flatnonzero(roi.reshape(-1))
        src = pos + sync_offset
        sel = flat[src[(src >= 0) & (src < len(frames))]]
        res = ctx.run_udf(dataset=ds, udf=StdDevUDF(), roi=roi)
        assert res['num_frames'].data[0] == len(sel) < len(pos)
        assert np.allclose(res['var'].data.reshape(-1), sel.var(axis=0), rtol=1e-12)
        assert np.allclose(res['mean'].data.reshape(-1), sel.mean(axis=0), rtol=1e-12)
        assert np.allclose(res['sum'].data.reshape(-1), sel.sum(axis=0), rtol=1e-15)
