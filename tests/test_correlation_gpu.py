"""
CorrelationUDF on the MI355X (Context.make_with('hip')) against its own NumPy-branch run on the inline executor, with
the tolerances of tests/correlation_ref.py: host and device-resident data, a region of interest, sync offsets, three
partitions, a run next to SumSigUDF, a cached second run, results left on the device, detector corrections, and the
kernels the plan reports.
"""
import numpy as np
import pytest

import correlation_ref as cr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG = (48, 48)
NAV = (4, 5)
PEAKS = np.array([(14, 14), (14, 34), (34, 24), (2, 45)], dtype=np.int32)     # (the last window is clipped)
R, Q = 4, 1
NAMES = ('centers', 'refineds', 'peak_values', 'peak_elevations')


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
    """20 uint16 frames, the last 5 blurred; template; the float64 reference (gaps and weights of the tolerances)"""
    frames, _, _ = cr.make_frames(SIG, PEAKS, R, 20, seed=4, dtype='uint16', n_blurred=5)
    template = cr.disk_template(SIG)
    return frames, template, cr.reference(frames, template, PEAKS, R, Q)


def udf():
    from libertem_amd.udf import CorrelationUDF
    return CorrelationUDF(peaks=PEAKS, template=cr.disk_template(SIG), crop_radius=R, refine_radius=Q)


def flat(res, raw=False):
    out = {}
    for name in NAMES:
        a = np.asarray(res[name].raw_data if raw else res[name].data)
        tail = (len(PEAKS), 2) if name in ('centers', 'refineds') else (len(PEAKS),)
        out[name] = a.reshape((-1,) + tail)
    return out


def check(dev, host, scan, pos=None, src=None, frames=None):
    """rows `pos` of the device run against the same rows of the NumPy-branch run; they hold the frames `src`"""
    all_frames, template, ref64 = scan
    n = len(dev['peak_values'])
    pos = np.arange(n) if pos is None else pos
    src = pos if src is None else src
    got = {k: dev[k][pos] for k in NAMES}
    ref = {k: v[src] for k, v in ref64.items()}
    for k in NAMES:
        # the reference values are the NumPy branch's; both restate one definition
        assert np.allclose(host[k][pos], ref[k], rtol=1e-5, atol=1e-6), k
        ref[k] = host[k][pos].astype(np.int64 if k == 'centers' else np.float64)
    return cr.compare(got, ref, (all_frames if frames is None else frames)[src], template, Q)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
@pytest.mark.parametrize('num_partitions', [2, 3])
def test_udf_vs_numpy_branch(ctx, cpu, scan, resident, num_partitions):
    from libertem_amd.common.hiparray import HipArray
    frames = scan[0]
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data,
                  num_partitions=num_partitions, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=num_partitions, sig_dims=2)
    dev = ctx.run_udf(dataset=ds, udf=udf())
    assert dev['centers'].data.shape == NAV + (4, 2) and dev['centers'].data.dtype == np.int32
    assert dev['peak_elevations'].data.shape == NAV + (4,) and dev['refineds'].data.dtype == np.float32
    check(flat(dev), flat(cpu.run_udf(dataset=ds_cpu, udf=udf())), scan)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_roi(ctx, cpu, scan, resident):
    from libertem_amd.common.hiparray import HipArray
    data = scan[0].reshape(NAV + SIG)
    roi = np.zeros(NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[2, 3] = roi[3, 4] = roi[3, 0] = True
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=2, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(), roi=roi), raw=True)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(), roi=roi), raw=True)
    assert len(dev['centers']) == 5
    check(dev, host, scan, pos=np.arange(5), src=np.flatnonzero(roi.reshape(-1)))


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset(ctx, cpu, scan, sync_offset):
    data = scan[0].reshape(NAV + SIG)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf()))
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf()))
    src = np.arange(20) + sync_offset
    valid = (src >= 0) & (src < 20)
    check(dev, host, scan, pos=np.flatnonzero(valid), src=src[valid])
    for k in NAMES:
        assert np.all(dev[k][~valid] == 0), k              # no frame, no result


def test_next_to_sumsig_cached_and_on_device(ctx, cpu, scan):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf.sumsigudf import SumSigUDF
    frames = scan[0]
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=2, sig_dims=2)
    host = flat(cpu.run_udf(dataset=cpu.load('memory', data=data, num_partitions=2, sig_dims=2), udf=udf()))
    both = ctx.run_udf(dataset=ds, udf=[udf(), SumSigUDF()])
    check(flat(both[0]), host, scan)
    sums = frames.reshape((20, -1)).astype(np.float64).sum(axis=1)
    assert np.allclose(np.asarray(both[1]['intensity'].data).reshape(-1), sums, rtol=1e-6)
    # the same UDF object again: kept task instances, the cached plan -- and the same bytes
    u = udf()
    first = flat(ctx.run_udf(dataset=ds, udf=u))
    second = flat(ctx.run_udf(dataset=ds, udf=u))
    for k in NAMES:
        assert first[k].tobytes() == second[k].tobytes() == flat(both[0])[k].tobytes(), k
    on_dev = ctx.run_udf(dataset=ds, udf=u, result_where='device')
    for k in NAMES:
        assert isinstance(on_dev[k].device_data, HipArray), k
    check(flat(on_dev), host, scan)


def test_corrections(ctx, cpu, scan):
    from libertem_amd.io.corrections import CorrectionSet
    frames = scan[0]
    rng = np.random.default_rng(21)
    dark = rng.uniform(0., 500., SIG)
    gain = rng.uniform(0.9, 1.1, SIG)
    corrected = ((frames.astype(np.float64) - dark) * gain).astype(np.float32)     # (one rounding, as on the device)
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(), corrections=CorrectionSet(dark=dark, gain=gain)))
    ds_cpu = cpu.load('memory', data=corrected.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf()))
    template = scan[1]
    ref = cr.reference(corrected, template, PEAKS, R, Q)
    check(dev, host, (corrected, template, ref))
    # ... and the device run on the host-corrected frames
    ds2 = ctx.load('memory', data=corrected.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    check(flat(ctx.run_udf(dataset=ds2, udf=udf())), host, (corrected, template, ref))


def test_plan_names_its_kernels(ctx, scan):
    from libertem_amd.udf import correlation
    ds = ctx.load('memory', data=scan[0].reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    ctx.run_udf(dataset=ds, udf=udf())
    plans = [p for key, p in correlation._PLANS.items() if key[1:3] == SIG]
    assert plans
    for name in ('k_corr_load<uint16>', 'k_corr_mul', 'k_corr_peaks'):
        assert any(name in p.last_kernel() for p in plans), [p.last_kernel() for p in plans]


def test_errors_on_device(ctx, scan):
    from libertem_amd.udf import CorrelationUDF
    ds = ctx.load('memory', data=scan[0].reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='outside'):
        ctx.run_udf(dataset=ds, udf=CorrelationUDF(np.array([(48, 0)]), scan[1], R))
    with pytest.raises(ValueError, match='template'):
        ctx.run_udf(dataset=ds, udf=CorrelationUDF(PEAKS, scan[1][:40], R))
