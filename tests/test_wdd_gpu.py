"""
WDDUDF on the MI355X (Context.make_with('hip')) against the index-by-index float64 restatement (tests/wdd_ref.py): the
generic fixture (12 x 10 scan of 24 x 28 Poisson frames, rotated geometry, epsilon 1e-2) with the windows (16, 16),
(16, 18) and (20, 16) through `run_wdd`, a plain `run_udf` (the window pixels come to the host, NumPy reconstructs) and
`result_where='device'` (the native plan); uint16, uint8 and float32 datasets, host and device-resident; the window
pixels kept on the device; a second run on the cached plan; and the simulated phase object (16 x 16 scan of 32 x 32
frames, window 24, epsilon 1e-4) through every route.  The tolerance is SSB's unless the float32 restatement reaches a
quarter of its atol on the fixture (`wdd_ref.atol_rule`).
"""
import numpy as np
import pytest

import ssb_ref as sr
import wdd_ref as wr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

IMAGES = ('complex', 'phase', 'amplitude')
NAV, SIG = sr.GENERIC_NAV, sr.GENERIC_SIG


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def generic():
    """the frames and, per window, the restatement's results and the atol of the rule"""
    frames = sr.generic_frames()
    refs = {}
    for w in wr.WINDOWS:
        ref = wr.reference(frames, w, wr.GENERIC_EPSILON, **wr.GENERIC)
        single = wr.reference(frames, w, wr.GENERIC_EPSILON, single=True, **wr.GENERIC)
        refs[w] = (ref, wr.atol_rule(ref['fourier'], single['fourier'])[0])
    return frames, refs


@pytest.fixture(scope='module')
def physical():
    """amplitude -> (phi, whole counts (16, 16, 32, 32), the restatement's results, the atol, single-sideband's)"""
    from libertem_amd.utils.generate import weak_phase_scan
    out = {}
    for amplitude in (0.1, 1.0):
        phi = sr.physical_phase(amplitude)
        counts = np.rint(weak_phase_scan(phi, sr.PHYS_STEP, sr.PHYS_SEMICONV_PIX, counts=1e6)).astype(np.uint32)
        ref = wr.reference(counts, wr.PHYS_WINDOW, wr.PHYS_EPSILON, **wr.physical_params())
        single = wr.reference(counts, wr.PHYS_WINDOW, wr.PHYS_EPSILON, single=True, **wr.physical_params())
        atol, base, single_err = wr.atol_rule(ref['fourier'], single['fourier'])
        print(f"amplitude {amplitude}: float32 restatement error {single_err:.3e}, SSB atol {base:.3e}, atol {atol:.3e}")
        out[amplitude] = (phi, counts, ref, atol, sr.reference(counts, **sr.physical_params()))
    return out


def check(res, ref, atol, what):
    """a dict of result arrays (or buffers) against the restatement"""
    arrays = {k: np.asarray(res[k].data if hasattr(res[k], 'data') and not isinstance(res[k], np.ndarray) else res[k])
              for k in ('fourier',) + IMAGES}
    assert arrays['fourier'].dtype == np.complex64 and arrays['complex'].dtype == np.complex64
    assert arrays['phase'].dtype == np.float32 and arrays['amplitude'].dtype == np.float32
    wr.assert_fourier(arrays['fourier'], ref['fourier'], what, atol=atol)
    assert np.array_equal(arrays['fourier'] == 0, ref['fourier'] == 0), what
    wr.assert_images(arrays, ref, what, atol=atol)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
@pytest.mark.parametrize('dtype', ['uint16', 'uint8', 'float32'])
def test_run_wdd_generic(ctx, generic, dtype, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_wdd
    frames, refs = generic
    window = (16, 18)
    ref, atol = refs[window]
    data = frames.astype(dtype)
    assert np.array_equal(data.astype(np.uint16), frames)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=3, sig_dims=2)
    out = run_wdd(ctx, ds, window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)
    assert set(out) == {'fourier'} | set(IMAGES)
    assert out['fourier'].shape == NAV
    check(out, ref, atol, f"run_wdd {dtype}")


@pytest.mark.parametrize('window', wr.WINDOWS, ids=str)
def test_every_route(ctx, generic, window):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import WDDUDF, run_wdd
    from libertem_amd.udf import wdd
    from libertem_amd.udf.wdd import window_pixels
    frames, refs = generic
    ref, atol = refs[window]
    n_k = window[0] * window[1]
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)
    udf = WDDUDF(window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)
    host = ctx.run_udf(dataset=ds, udf=udf)                    # bf comes to the host, NumPy reconstructs
    check(host, ref, atol, f'run_udf {window}')
    idx = window_pixels(SIG, window, 11.6, 14.2)
    assert np.array_equal(host['bf'].data.reshape(120, n_k), frames.reshape(120, -1)[:, idx].astype(np.float32))
    dev = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert isinstance(dev['bf'].device_data, HipArray)
    check(dev, ref, atol, f"result_where='device' {window}")
    out = run_wdd(ctx, ds, window=window, epsilon=wr.GENERIC_EPSILON, keep_bf=True, **wr.GENERIC)
    assert isinstance(out['bf'], HipArray) and out['bf'].dtype == np.float32
    assert np.array_equal(out['bf'].cpu().reshape(120, n_k), host['bf'].data.reshape(120, n_k))
    check(out, ref, atol, f'run_wdd keep_bf {window}')
    # the same UDF again: the cached plan, the same bytes
    n_plans = len(wdd._PLANS)
    assert out['fourier'].tobytes() == dev['fourier'].data.tobytes() and n_plans >= 1
    again = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert len(wdd._PLANS) == n_plans
    assert again['fourier'].data.tobytes() == dev['fourier'].data.tobytes()
    plans = list(wdd._PLANS.values())
    assert any(p.last_kernel() == f'k_transpose<4> + hipfft_r2c + k_transpose<8> + k_wdd_dot + k_wdd_finish batch={n_k}'
               for p in plans)
    # the plans go with their executor (HipJobExecutor.close calls this); the next run makes a new one
    wdd.release_plans(0)
    assert not wdd._PLANS and all(p._ptr is None for p in plans)
    fresh = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert fresh['fourier'].data.tobytes() == dev['fourier'].data.tobytes() and len(wdd._PLANS) == 1


def test_physical_fixture(ctx, physical):
    from libertem_amd.udf import WDDUDF, run_wdd
    for amplitude, (phi, counts, ref, atol, ssb) in physical.items():
        corr_ref, scale_ref = sr.phase_agreement(ref['phase'], phi)
        scale_ssb = sr.phase_agreement(ssb['phase'], phi)[1]
        params = dict(wr.physical_params(), window=wr.PHYS_WINDOW, epsilon=wr.PHYS_EPSILON)
        ds = ctx.load('memory', data=counts, num_partitions=2, sig_dims=2)
        outs = {'run_wdd': run_wdd(ctx, ds, **params), 'run_udf': ctx.run_udf(dataset=ds, udf=WDDUDF(**params)),
                'device': ctx.run_udf(dataset=ds, udf=WDDUDF(**params), result_where='device')}
        for what, out in outs.items():
            check(out, ref, atol, f"physical {amplitude} {what}")
            phase = np.asarray(out['phase'].data if what != 'run_wdd' else out['phase'], dtype=np.float64)
            corr, scale = sr.phase_agreement(phase, phi)
            print(f"amplitude {amplitude} {what}: correlation {corr:.7f}, scale {scale:.4f}")
            assert abs(corr - corr_ref) < 1e-3 and abs(scale - scale_ref) < 1e-3
            if amplitude == 0.1:
                assert corr > 0.99
            else:
                assert abs(1 - scale) < abs(1 - scale_ssb)


def test_errors_on_device(ctx, generic):
    from libertem_amd.udf import WDDUDF, run_wdd
    frames, _ = generic
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)
    roi = np.zeros(NAV, bool)
    roi[1] = True
    with pytest.raises(ValueError, match='roi'):
        ctx.run_udf(dataset=ds, udf=WDDUDF(window=16, **wr.GENERIC), roi=roi)
    with pytest.raises(ValueError, match='does not hold the disk pixel'):
        run_wdd(ctx, ds, window=12, **wr.GENERIC)
    with pytest.raises(ValueError, match='leave the frame'):
        run_wdd(ctx, ds, window=26, **wr.GENERIC)
    with pytest.raises(ValueError, match='epsilon 0'):
        run_wdd(ctx, ds, window=16, epsilon=0, **wr.GENERIC)
    sliced = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, tileshape=(7, 4, 28))
    with pytest.raises(ValueError, match='whole frames'):
        run_wdd(ctx, sliced, window=16, **wr.GENERIC)
