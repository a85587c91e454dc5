"""
FEMUDF and LogsumUDF on the MI355X: `ltmi_ring_moments` and `ltmi_logsum_frames` through ctypes against a
float64 restatement for every stored dtype, bitwise repeatability, NaN / empty-ring cases, strided output,
and the UDFs on device-resident, host-streamed, raw and .mib data against the reference's results
(tests/golden/framestats.npz).
"""
import os

import numpy as np
import pytest

import framestats_recipes

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

FEM_DTYPES = ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32', 'float64',
              'complex64', 'complex128']
LOG_DTYPES = FEM_DTYPES[:8]


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'framestats.npz'))


def _frames(dt, shape, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        return rng.integers(int(info.min), int(info.max), shape, endpoint=True).astype(dt)
    if dt.kind == 'c':
        return (rng.normal(3., 2., shape) + 1j * rng.normal(-1., 1., shape)).astype(dt)
    return rng.normal(-5., 40., shape).astype(dt)


def _device(x, offset=0, pad=0):
    """x (n, H, W) on the device with a frame stride of H * W + pad elements, `offset` elements into the
    allocation; -> (tensor keeping it alive, pointer, ld)"""
    n = x.shape[0]
    n_px = int(np.prod(x.shape[1:]))
    ld = n_px + pad
    host = np.zeros((n * ld + offset,), dtype=x.dtype)
    host[offset:].reshape((n, ld))[:, :n_px] = x.reshape((n, n_px))
    view = {np.dtype('uint16'): np.int16, np.dtype('uint32'): np.int32}.get(x.dtype)
    t = torch.from_numpy(host.view(view) if view is not None else host.view(np.uint8)).cuda()
    return t, t.data_ptr() + offset * x.dtype.itemsize, ld


# --- FEM kernel ------------------------------------------------------------------------------------
def _ring_kernel(x, center, rad_in, rad_out, offset=0, pad=0):
    from libertem_amd import hip
    from libertem_amd.udf.FEM import ring_mask, ring_spans
    n, H, W = x.shape
    mask = ring_mask(center, rad_in, rad_out, (H, W))
    spans = ring_spans(mask)
    sp = torch.from_numpy(spans.reshape(-1).copy() if spans.size else np.zeros(3, np.int32)).cuda()
    t, ptr, ld = _device(x, offset, pad)
    out = torch.full((n,), -1., dtype=torch.float32, device='cuda')
    hip.ring_moments(0, ptr, x.dtype, n, W, ld, sp.data_ptr(), len(spans), int(mask.sum()), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), mask


def _ring_exact(x, mask):
    v = x.reshape((x.shape[0], -1))[:, mask.reshape(-1)]
    if v.dtype.kind == 'c':
        v = v.astype(np.clongdouble)
        return np.sqrt(np.mean(np.abs(v - v.mean(axis=1, keepdims=True)) ** 2, axis=1)).astype(np.float64)
    v = v.astype(np.longdouble)
    return np.sqrt(np.mean((v - v.mean(axis=1, keepdims=True)) ** 2, axis=1)).astype(np.float64)


@pytest.mark.parametrize('dt', FEM_DTYPES)
def test_ring_kernel_every_dtype(dt):
    x = _frames(dt, (37, 40, 52), seed=300 + FEM_DTYPES.index(dt))
    got, mask = _ring_kernel(x, (17.3, 30.6), 5.5, 19., offset=1, pad=3)
    exp = _ring_exact(x, mask)
    assert np.allclose(got, exp, rtol=1e-6, atol=0), np.max(np.abs(got - exp) / exp)


def test_ring_kernel_bitwise_repeatable():
    x = _frames('uint16', (300, 64, 64), seed=8)
    a, _ = _ring_kernel(x, (30, 33), 6, 28)
    b, _ = _ring_kernel(x, (30, 33), 6, 28)
    assert a.tobytes() == b.tobytes()


def test_ring_kernel_nan_and_empty():
    x = _frames('float32', (6, 20, 20), seed=9)
    x[1, 0, 0] = np.nan          # outside the ring: no effect
    x[2, 10, 13] = np.nan        # inside
    x[3, 10, 13] = np.inf
    x[4, 10, 13] = -np.inf
    got, mask = _ring_kernel(x, (10, 10), 2, 6)
    assert mask[10, 13] and not mask[0, 0]
    assert np.all(np.isnan(got[2:5]))
    exp = _ring_exact(x, mask)
    ok = [0, 1, 5]
    assert np.allclose(got[ok], exp[ok], rtol=1e-6)
    empty, _ = _ring_kernel(x, (10, 10), 6, 4)
    assert np.all(np.isnan(empty))
    outside, m = _ring_kernel(x, (100, 100), 0, 5)
    assert not m.any() and np.all(np.isnan(outside))


def test_ring_kernel_partly_outside_and_constant():
    x = _frames('int16', (5, 24, 30), seed=10)
    got, mask = _ring_kernel(x, (-3.5, 27.2), 4, 15)
    assert 0 < mask.sum() < 0.5 * np.pi * 15 ** 2
    assert np.allclose(got, _ring_exact(x, mask), rtol=1e-6)
    c = np.full((3, 16, 16), 1234, dtype=np.uint16)
    zero, _ = _ring_kernel(c, (8, 8), 2, 6)
    assert np.all(zero == 0)


# --- logsum kernel ---------------------------------------------------------------------------------
def _logsum_exact(x):
    """float64 restatement: the reference's terms (rounded in result_type(float32, dtype)), summed in float64"""
    ct = np.result_type(np.float32, x.dtype)
    f = x.reshape((x.shape[0], -1)).astype(ct)
    with np.errstate(all='ignore'):
        terms = np.log(f - f.min(axis=1, keepdims=True) + ct.type(1))
    return terms.astype(np.float64).sum(axis=0)


def _logsum_kernel(x, offset=0, pad=0, splits=(), out=None, cols=None, ld_out=None, out_off=0):
    from libertem_amd import hip
    n = x.shape[0]
    n_px = int(np.prod(x.shape[1:]))
    t, ptr, ld = _device(x, offset, pad)
    if out is None:
        out = torch.zeros((n_px,), dtype=torch.float32, device='cuda')
    bounds = [0, *splits, n]
    for a, b in zip(bounds[:-1], bounds[1:]):
        ws = torch.empty((max(16, hip.logsum_workspace(b - a, n_px, x.dtype)),), dtype=torch.uint8, device='cuda')
        hip.logsum_frames(0, ptr + a * ld * x.dtype.itemsize, x.dtype, b - a, n_px, ld,
                          out.data_ptr() + out_off * 4, ws.data_ptr(), cols=cols, ld_out=ld_out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('dt', LOG_DTYPES)
def test_logsum_kernel_every_dtype(dt):
    x = _frames(dt, (57, 33, 35), seed=400 + LOG_DTYPES.index(dt))
    got = _logsum_kernel(x, offset=1, pad=5)
    exp = _logsum_exact(x)
    assert np.all(np.isfinite(got))
    assert np.allclose(got, exp, rtol=1e-6, atol=0), np.max(np.abs(got - exp) / np.abs(exp))


def test_logsum_kernel_many_chunks():
    # 1.1 GiB of uint16 frames of 256 x 256: several chunks of frames, slabs merged in order
    n = 8800
    g = torch.Generator(device='cuda').manual_seed(5)
    dev = torch.randint(0, 65536, (n, 256 * 256), generator=g, device='cuda', dtype=torch.int32)
    dev[:, 0] = 0
    dev[:, 1] = 65535
    t = torch.where(dev > 32767, dev - 65536, dev).to(torch.int16)      # the uint16 bit patterns
    from libertem_amd import hip
    out = torch.zeros((256 * 256,), dtype=torch.float32, device='cuda')
    ws = torch.empty((hip.logsum_workspace(n, 256 * 256, np.uint16),), dtype=torch.uint8, device='cuda')
    hip.logsum_frames(0, t.data_ptr(), np.uint16, n, 256 * 256, 256 * 256, out.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    vals = dev.to(torch.float32)
    exp = torch.log(vals - vals.min(dim=1, keepdim=True).values + 1).to(torch.float64).sum(dim=0).cpu().numpy()
    assert np.allclose(got, exp, rtol=1e-6), np.max(np.abs(got - exp) / exp)
    assert got[1] == pytest.approx(n * np.log(np.float32(65536.)), rel=1e-6)


def test_logsum_kernel_accumulates_and_repeats():
    x = _frames('float32', (200, 20, 30), seed=11)
    a = _logsum_kernel(x, splits=(70, 71))
    b = _logsum_kernel(x, splits=(70, 71))
    assert a.tobytes() == b.tobytes()
    assert np.allclose(a, _logsum_exact(x), rtol=1e-6)


def test_logsum_kernel_nan_frame():
    x = _frames('float32', (9, 16, 16), seed=12)
    x[4, 3, 3] = np.nan
    got = _logsum_kernel(x)
    assert np.all(np.isnan(got))
    y = _frames('float32', (9, 16, 16), seed=12)
    y[4, 3, 3] = np.inf
    got = _logsum_kernel(y)
    assert np.isinf(got[3 * 16 + 3]) and np.isfinite(np.delete(got, 3 * 16 + 3)).all()


def test_logsum_kernel_strided_output():
    """partial-width output: tile pixels land in a strided sub-rectangle (rows of `cols` at ld_out)"""
    x = _frames('uint16', (40, 6, 7), seed=13)
    H, W, r0, c0 = 10, 20, 3, 4
    out = torch.full((H, W), -1., dtype=torch.float32, device='cuda')
    got = _logsum_kernel(x, out=out, cols=7, ld_out=W, out_off=r0 * W + c0)
    exp = _logsum_exact(x)
    assert np.allclose(got[r0:r0 + 6, c0:c0 + 7].reshape(-1) + 1, exp, rtol=1e-6)
    mask = np.ones((H, W), dtype=bool)
    mask[r0:r0 + 6, c0:c0 + 7] = False
    assert np.all(got[mask] == -1)


def test_logsum_kernel_rejects_complex():
    from libertem_amd import hip
    x = torch.zeros((4, 32), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError, match=r'\(code -2\)'):
        hip.logsum_frames(0, x.data_ptr(), np.complex64, 2, 16, 16, x.data_ptr(), x.data_ptr())


# --- the UDFs --------------------------------------------------------------------------------------
def _check(got, exp, rtol=1e-5):
    got = np.asarray(got)
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    if ok.any():
        assert np.allclose(got[ok], exp[ok], rtol=rtol, atol=rtol * np.abs(exp[ok]).max()), \
            np.abs(got[ok] - exp[ok]).max()


def _make_udf(case):
    from libertem_amd.udf.FEM import FEMUDF
    from libertem_amd.udf.logsum import LogsumUDF
    if 'center' in case:
        return FEMUDF(center=case['center'], rad_in=case['rad_in'], rad_out=case['rad_out']), 'intensity'
    return LogsumUDF(), 'logsum'


ALL_CASES = framestats_recipes.FEM_CASES + framestats_recipes.LOGSUM_CASES
UDF_CASES = [(c, r) for c in ALL_CASES for r in (True, False) if not (r and c.get('sync_offset'))]


@pytest.mark.parametrize('case,resident', UDF_CASES,
                         ids=[c['name'] + ('-resident' if r else '-streamed') for c, r in UDF_CASES])
def test_udf_vs_golden(ctx, golden, case, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.io.corrections import CorrectionSet
    data, roi, corr = framestats_recipes.make_case(case)
    kw = dict(num_partitions=case['num_partitions'], sig_dims=2)
    if case.get('sync_offset'):
        kw['sync_offset'] = case['sync_offset']
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, **kw)
    corrections = None if corr is None else CorrectionSet(dark=corr[0], gain=corr[1])
    udf, key = _make_udf(case)
    res = ctx.run_udf(dataset=ds, udf=udf, roi=roi, corrections=corrections)
    _check(res[key].data, golden[case['name'] + '__' + key])


@pytest.mark.parametrize('case', [c for c in ALL_CASES if c.get('sync_offset')], ids=lambda c: c['name'])
def test_udf_raw_file(ctx, golden, case, tmp_path):
    data, _, _ = framestats_recipes.make_case(case)
    path = str(tmp_path / 'scan.raw')
    data.tofile(path)
    ds = ctx.load('raw', path=path, dtype=data.dtype, nav_shape=tuple(case['nav']),
                  sig_shape=tuple(case['sig']), sync_offset=case['sync_offset'],
                  num_partitions=case['num_partitions'])
    udf, key = _make_udf(case)
    _check(ctx.run_udf(dataset=ds, udf=udf)[key].data, golden[case['name'] + '__' + key])


def test_udf_results_on_device(ctx, golden):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf.FEM import FEMUDF
    from libertem_amd.udf.logsum import LogsumUDF
    fem_case, log_case = framestats_recipes.FEM_CASES[0], framestats_recipes.LOGSUM_CASES[2]
    data, _, _ = framestats_recipes.make_case(fem_case)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=3, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=FEMUDF(center=fem_case['center'], rad_in=fem_case['rad_in'],
                                             rad_out=fem_case['rad_out']), result_where='device')
    assert isinstance(res['intensity'].device_data, HipArray)
    _check(res['intensity'].data, golden['fem_u16__intensity'])
    data, _, _ = framestats_recipes.make_case(log_case)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=3, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=LogsumUDF(), result_where='device')
    assert isinstance(res['logsum'].device_data, HipArray)
    _check(res['logsum'].data, golden['log_u16_full__logsum'])


def test_udf_errors_on_device(ctx):
    from libertem_amd.udf.FEM import FEMUDF
    from libertem_amd.udf.logsum import LogsumUDF
    ds = ctx.load('memory', data=np.ones((2, 3, 8, 8), np.complex64), num_partitions=2, sig_dims=2)
    with pytest.raises(TypeError):
        ctx.run_udf(dataset=ds, udf=LogsumUDF())
    ds = ctx.load('memory', data=np.ones((2, 3, 16, 16), np.float32), num_partitions=2, sig_dims=2,
                  tileshape=(2, 8, 16))
    for udf in (LogsumUDF(), FEMUDF(center=(8, 8), rad_in=2, rad_out=6)):
        with pytest.raises(ValueError, match=r'tileshape \(2, 8, 16\)'):
            ctx.run_udf(dataset=ds, udf=udf)


MIB_CASE = dict(name='fs_u16', kind='u', bits=16, sig=(32, 64), frames=(7, 5), nav=(3, 4), seed=1402)


@pytest.mark.parametrize('streamed', [False, True], ids=['resident', 'streamed'])
def test_udf_mib(ctx, tmp_path, monkeypatch, streamed):
    import recipes
    from libertem_amd.io.dataset.mib import MIBDataSet
    from libertem_amd.udf.FEM import FEMUDF, ring_mask
    from libertem_amd.udf.logsum import LogsumUDF
    frames, files, hdr = recipes.make_mib_case(MIB_CASE)
    for fn, blob in files.items():
        (tmp_path / fn).write_bytes(blob)
    hdr_path = tmp_path / (MIB_CASE['name'] + '.hdr')
    hdr_path.write_text(hdr)
    if streamed:
        monkeypatch.setattr(MIBDataSet, 'MAX_RESIDENT_BYTES', 2 * 32 * 64 * 2)
    ds = ctx.load('mib', path=str(hdr_path))
    monkeypatch.setattr(MIBDataSet, 'MAX_RESIDENT_BYTES', None)
    assert ds.is_streamed == streamed
    x = frames[:12].reshape((12, 32, 64))
    fem = ctx.run_udf(dataset=ds, udf=FEMUDF(center=(14.5, 40.), rad_in=3, rad_out=12))
    mask = ring_mask((14.5, 40.), 3, 12, (32, 64))
    exp = _ring_exact(x.astype(np.float32), mask)
    assert np.allclose(fem['intensity'].data.reshape(-1), exp, rtol=1e-5)
    logsum = ctx.run_udf(dataset=ds, udf=LogsumUDF())
    assert np.allclose(logsum['logsum'].data, _logsum_exact(x).reshape((32, 64)), rtol=1e-5)
