"""
SSBUDF on the MI355X (Context.make_with('hip')) against the index-by-index float64 restatement (tests/ssb_ref.py), at
the tolerance of the holography tests: the generic fixture (12 x 10 scan of 24 x 28 Poisson frames, rotated geometry,
cutoff 4) and the simulated weak phase object (16 x 16 scan of 32 x 32 frames) through `run_ssb`, a plain `run_udf`
(the bright-field pixels come to the host, NumPy reconstructs) and `result_where='device'` (the native plan); uint16,
uint8 and float32 datasets, host and device-resident; the bright-field pixels kept on the device; a sync offset; a
second run on the cached plan; the parameter errors on the device.
"""
import numpy as np
import pytest

import ssb_ref as sr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

IMAGES = ('complex', 'phase', 'amplitude')


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def cpu():
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def generic():
    frames = sr.generic_frames()
    return frames, sr.reference(frames, **sr.GENERIC)


@pytest.fixture(scope='module')
def physical():
    from libertem_amd.utils.generate import weak_phase_scan
    phi = sr.physical_phase()
    counts = np.rint(weak_phase_scan(phi, sr.PHYS_STEP, sr.PHYS_SEMICONV_PIX, counts=1e6)).astype(np.uint32)
    return phi, counts, sr.reference(counts, **sr.physical_params())


def check(res, ref, what):
    """a dict of result arrays (or buffers) against the restatement"""
    arrays = {k: np.asarray(res[k].data if hasattr(res[k], 'data') and not isinstance(res[k], np.ndarray) else res[k])
              for k in ('fourier',) + IMAGES}
    assert arrays['fourier'].dtype == np.complex64 and arrays['complex'].dtype == np.complex64
    assert arrays['phase'].dtype == np.float32 and arrays['amplitude'].dtype == np.float32
    sr.assert_fourier(arrays['fourier'], ref['fourier'], what)
    assert np.array_equal(arrays['fourier'] == 0, ref['fourier'] == 0), what
    sr.assert_images(arrays, ref, what)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
@pytest.mark.parametrize('dtype', ['uint16', 'uint8', 'float32'])
def test_run_ssb_generic(ctx, generic, dtype, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_ssb
    frames, ref = generic
    data = frames.astype(dtype)
    assert np.array_equal(data.astype(np.uint16), frames)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=3, sig_dims=2)
    out = run_ssb(ctx, ds, **sr.GENERIC)
    assert set(out) == {'fourier'} | set(IMAGES)
    assert out['fourier'].shape == sr.GENERIC_NAV
    check(out, ref, f"run_ssb {dtype}")


def test_keep_bf_is_the_fancy_index(ctx, generic):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_ssb
    from libertem_amd.udf.ssb import bf_pixels
    frames, ref = generic
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)
    out = run_ssb(ctx, ds, keep_bf=True, **sr.GENERIC)
    assert isinstance(out['bf'], HipArray) and out['bf'].dtype == np.float32
    idx = bf_pixels(sr.GENERIC_SIG, 7.3, 11.6, 14.2)
    assert np.array_equal(out['bf'].cpu().reshape(120, 167), frames.reshape(120, -1)[:, idx].astype(np.float32))
    check(out, ref, 'run_ssb keep_bf')


@pytest.mark.parametrize('num_partitions', [1, 3])
def test_plain_run_udf_and_result_on_device(ctx, cpu, generic, num_partitions):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import SSBUDF
    from libertem_amd.udf import ssb
    frames, ref = generic
    ds = ctx.load('memory', data=frames, num_partitions=num_partitions, sig_dims=2)
    udf = SSBUDF(**sr.GENERIC)
    host = ctx.run_udf(dataset=ds, udf=udf)                    # bf comes to the host, NumPy reconstructs
    check(host, ref, 'run_udf')
    inline = cpu.run_udf(dataset=cpu.load('memory', data=frames, num_partitions=num_partitions, sig_dims=2), udf=udf)
    assert np.array_equal(host['bf'].data, inline['bf'].data)
    assert host['fourier'].data.tobytes() == inline['fourier'].data.tobytes()
    dev = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert isinstance(dev['bf'].device_data, HipArray)
    check(dev, ref, "result_where='device'")
    # the same UDF again: the cached plan, the same bytes
    n_plans = len(ssb._PLANS)
    again = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert len(ssb._PLANS) == n_plans
    assert again['fourier'].data.tobytes() == dev['fourier'].data.tobytes()
    plans = [p for key, p in ssb._PLANS.items() if key[1:3] == sr.GENERIC_NAV]
    assert plans and all(p.last_kernel() == 'k_transpose<4> + hipfft_r2c + k_transpose<8> + k_ssb_trotter batch=167'
                         for p in plans)
    # the plans go with their executor (HipJobExecutor.close calls this); the next run makes a new one
    ssb.release_plans(0)
    assert not ssb._PLANS and all(p._ptr is None for p in plans)
    fresh = ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    assert fresh['fourier'].data.tobytes() == dev['fourier'].data.tobytes() and len(ssb._PLANS) == 1


def test_physical_fixture(ctx, physical):
    from libertem_amd.udf import SSBUDF, run_ssb
    phi, counts, ref = physical
    ds = ctx.load('memory', data=counts, num_partitions=2, sig_dims=2)
    outs = {'run_ssb': run_ssb(ctx, ds, **sr.physical_params()),
            'run_udf': ctx.run_udf(dataset=ds, udf=SSBUDF(**sr.physical_params())),
            'device': ctx.run_udf(dataset=ds, udf=SSBUDF(**sr.physical_params()), result_where='device')}
    for what, out in outs.items():
        check(out, ref, f"physical {what}")
        phase = np.asarray(out['phase'].data if what != 'run_ssb' else out['phase'], dtype=np.float64)
        corr, scale = sr.phase_agreement(phase, phi)
        print(f"{what}: correlation {corr:.7f}, scale {scale:.4f}")
        assert corr > 0.999
        assert abs(scale - 1) < 0.02


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset_leaves_zero_rows(ctx, cpu, generic, sync_offset):
    from libertem_amd.udf import SSBUDF, run_ssb
    frames, _ = generic
    flat = frames.reshape((120,) + sr.GENERIC_SIG)
    src = np.arange(120) + sync_offset
    valid = (src >= 0) & (src < 120)
    shifted = np.zeros_like(flat)
    shifted[valid] = flat[src[valid]]
    ref = sr.reference(shifted.reshape(frames.shape), **sr.GENERIC)
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    ds_cpu = cpu.load('memory', data=frames, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    out = run_ssb(ctx, ds, keep_bf=True, **sr.GENERIC)
    host = cpu.run_udf(dataset=ds_cpu, udf=SSBUDF(**sr.GENERIC))
    bf = out['bf'].cpu().reshape(120, 167)
    assert np.array_equal(bf, host['bf'].data.reshape(120, 167))
    assert np.all(bf[~valid] == 0) and np.all(bf[valid].sum(axis=1) > 0)      # no frame, no pixels
    check(out, ref, f"sync_offset {sync_offset}")
    check(host, ref, f"sync_offset {sync_offset} inline")


def test_errors_on_device(ctx, generic):
    from libertem_amd.udf import SSBUDF, run_ssb
    frames, _ = generic
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)
    roi = np.zeros(sr.GENERIC_NAV, bool)
    roi[1] = True
    with pytest.raises(ValueError, match='roi'):
        ctx.run_udf(dataset=ds, udf=SSBUDF(**sr.GENERIC), roi=roi)
    with pytest.raises(ValueError, match='P = 0'):
        run_ssb(ctx, ds, **dict(sr.GENERIC, cx=-30.))
    with pytest.raises(ValueError, match='cutoff'):
        run_ssb(ctx, ds, **dict(sr.GENERIC, cutoff=0))
    sliced = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, tileshape=(7, 4, 28))
    with pytest.raises(ValueError, match='whole frames'):
        run_ssb(ctx, sliced, **sr.GENERIC)
