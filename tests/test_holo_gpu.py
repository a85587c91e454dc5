"""
HoloReconstructUDF on the MI355X (Context.make_with('hip')) against its own NumPy-branch run on the inline executor,
within the bound of tests/holo_ref.py: nav (3, 4) of 32 x 20 uint16 holograms reconstructed to (6, 9); host and
device-resident data, a region of interest, sync offsets, three partitions, a run next to SumSigUDF, a cached second
run, results left on the device, a reference wave, detector corrections, the kernels the plan reports.
"""
import numpy as np
import pytest

import holo_ref as hr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG = (32, 20)
NAV = (3, 4)
OUT = (6, 9)
K = (8, 5)
SB = ((-K[0]) % SIG[0], (-K[1]) % SIG[1])


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
def scan():
    """12 uint16 holograms, the aperture, the float64 restatement"""
    from libertem_amd.udf.holography import disk_aperture
    frames = hr.hologram_frames(SIG, 12, K, dtype='uint16')
    aperture = disk_aperture(OUT, 2.5, 0.5)
    return frames, aperture, hr.reference(frames, OUT, SB, aperture)


def udf(aperture, reference_wave=None):
    from libertem_amd.udf import HoloReconstructUDF
    return HoloReconstructUDF(out_shape=OUT, sb_position=SB, aperture=aperture, reference_wave=reference_wave)


def waves(res, raw=False):
    return np.asarray(res['wave'].raw_data if raw else res['wave'].data).reshape((-1,) + OUT)


def check(dev, host, scan, pos=None, src=None, reference_wave=None):
    """rows `pos` of the device run against the same rows of the NumPy-branch run; they hold the frames `src`"""
    frames, aperture, ref64 = scan
    pos = np.arange(len(dev)) if pos is None else pos
    src = pos if src is None else src
    ref = ref64[src]
    # the reference values are the NumPy branch's; both restate one definition
    assert np.allclose(host[pos], ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    return hr.compare(dev[pos], host[pos].astype(np.complex128), frames[src], aperture, reference_wave, what='udf')


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
@pytest.mark.parametrize('num_partitions', [2, 3])
def test_udf_vs_numpy_branch(ctx, cpu, scan, resident, num_partitions):
    from libertem_amd.common.hiparray import HipArray
    data = scan[0].reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data,
                  num_partitions=num_partitions, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=num_partitions, sig_dims=2)
    dev = ctx.run_udf(dataset=ds, udf=udf(scan[1]))
    assert dev['wave'].data.shape == NAV + OUT and dev['wave'].data.dtype == np.complex64
    check(waves(dev), waves(cpu.run_udf(dataset=ds_cpu, udf=udf(scan[1]))), scan)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_roi(ctx, cpu, scan, resident):
    from libertem_amd.common.hiparray import HipArray
    data = scan[0].reshape(NAV + SIG)
    roi = np.zeros(NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[1, 3] = roi[2, 2] = roi[2, 3] = True
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=2, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2)
    dev = waves(ctx.run_udf(dataset=ds, udf=udf(scan[1]), roi=roi), raw=True)
    host = waves(cpu.run_udf(dataset=ds_cpu, udf=udf(scan[1]), roi=roi), raw=True)
    assert len(dev) == 5
    check(dev, host, scan, pos=np.arange(5), src=np.flatnonzero(roi.reshape(-1)))


@pytest.mark.parametrize('sync_offset', [2, -2])
def test_sync_offset(ctx, cpu, scan, sync_offset):
    data = scan[0].reshape(NAV + SIG)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    dev = waves(ctx.run_udf(dataset=ds, udf=udf(scan[1])))
    host = waves(cpu.run_udf(dataset=ds_cpu, udf=udf(scan[1])))
    src = np.arange(12) + sync_offset
    valid = (src >= 0) & (src < 12)
    check(dev, host, scan, pos=np.flatnonzero(valid), src=src[valid])
    assert np.all(dev[~valid] == 0)                              # no frame, no result


def test_next_to_sumsig_cached_and_on_device(ctx, cpu, scan):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf.sumsigudf import SumSigUDF
    from libertem_amd.udf import holography
    frames, aperture, _ = scan
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=2, sig_dims=2)
    host = waves(cpu.run_udf(dataset=cpu.load('memory', data=data, num_partitions=2, sig_dims=2), udf=udf(aperture)))
    both = ctx.run_udf(dataset=ds, udf=[udf(aperture), SumSigUDF()])
    check(waves(both[0]), host, scan)
    sums = frames.reshape((12, -1)).astype(np.float64).sum(axis=1)
    assert np.allclose(np.asarray(both[1]['intensity'].data).reshape(-1), sums, rtol=1e-6)
    # the same UDF object again: kept task instances, the cached plan -- and the same bytes
    u = udf(aperture)
    first = waves(ctx.run_udf(dataset=ds, udf=u))
    n_plans = len(holography._PLANS)
    second = waves(ctx.run_udf(dataset=ds, udf=u))
    assert len(holography._PLANS) == n_plans
    assert first.tobytes() == second.tobytes() == waves(both[0]).tobytes()
    on_dev = ctx.run_udf(dataset=ds, udf=u, result_where='device')
    assert isinstance(on_dev['wave'].device_data, HipArray)
    check(waves(on_dev), host, scan)
    plans = [p for key, p in holography._PLANS.items() if key[1:5] == SIG + OUT]
    assert plans
    for name in ('k_corr_load<uint16>', 'hipfft_r2c', 'k_holo_crop', 'hipfft_c2c', 'k_holo_store'):
        assert any(name in p.last_kernel() for p in plans), [p.last_kernel() for p in plans]


def test_reference_wave(ctx, cpu, scan):
    frames, aperture, _ = scan
    case = (SIG, OUT, SB)
    ref_wave = hr.reference_wave_for(case)
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=3, sig_dims=2)
    dev = waves(ctx.run_udf(dataset=ds, udf=udf(aperture, ref_wave)))
    host = waves(cpu.run_udf(dataset=ds_cpu, udf=udf(aperture, ref_wave)))
    check(dev, host, (frames, aperture, hr.reference(frames, OUT, SB, aperture, ref_wave)), reference_wave=ref_wave)


def test_corrections(ctx, cpu, scan):
    from libertem_amd.io.corrections import CorrectionSet
    frames, aperture, _ = scan
    rng = np.random.default_rng(21)
    dark = rng.uniform(0., 500., SIG)
    gain = rng.uniform(0.9, 1.1, SIG)
    corrected = ((frames.astype(np.float64) - dark) * gain).astype(np.float32)     # (one rounding, as on the device)
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    dev = waves(ctx.run_udf(dataset=ds, udf=udf(aperture), corrections=CorrectionSet(dark=dark, gain=gain)))
    ds_cpu = cpu.load('memory', data=corrected.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    host = waves(cpu.run_udf(dataset=ds_cpu, udf=udf(aperture)))
    ref = hr.reference(corrected, OUT, SB, aperture)
    check(dev, host, (corrected, aperture, ref))
    # ... and the device run on the host-corrected frames
    ds2 = ctx.load('memory', data=corrected.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    check(waves(ctx.run_udf(dataset=ds2, udf=udf(aperture))), host, (corrected, aperture, ref))


def test_errors_on_device(ctx, scan):
    from libertem_amd.udf import HoloReconstructUDF
    ds = ctx.load('memory', data=scan[0].reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='sb_position'):
        ctx.run_udf(dataset=ds, udf=HoloReconstructUDF(OUT, (32, 0), scan[1]))
    with pytest.raises(ValueError, match='out_shape'):
        ctx.run_udf(dataset=ds, udf=HoloReconstructUDF((33, 9), SB, np.ones((33, 9), np.float32)))
