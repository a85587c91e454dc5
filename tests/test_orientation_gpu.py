"""
OrientationMatchUDF on the MI355X (Context.make_with('hip')) against its own NumPy-branch run on the inline executor:
the 90 recovery frames of tests/orientation_ref.py as a 9 x 10 scan of 64 x 64 uint16 frames, host-streamed and
device-resident, a region of interest, sync offsets, results left on the device, detector corrections.  template,
rotation and correlation are EQUAL, polar_norm lies within one float32 ulp, and the recovered (template, rotation)
are the ones the frames were rendered with.
"""
import numpy as np
import pytest

import orientation_ref as oref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG, NAV = oref.REC_SIG, oref.REC_NAV
NAMES = ('template', 'rotation', 'correlation', 'polar_norm')
N_BEST = 2


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
    from libertem_amd.udf import polar_library
    spot_lists, frames, truth = oref.recovery()
    return frames, polar_library(spot_lists, oref.REC_N_R, oref.REC_N_PHI), truth


def udf(lib, n_best=N_BEST):
    from libertem_amd.udf import OrientationMatchUDF
    return OrientationMatchUDF(lib, oref.REC_CENTER, oref.REC_N_R, oref.REC_N_PHI, n_best=n_best)


def flat(res, n_best=N_BEST, raw=False):
    out = {}
    for name in NAMES:
        a = np.asarray(res[name].raw_data if raw else res[name].data)
        out[name] = a.reshape((-1,) + (() if name == 'polar_norm' else (n_best,)))
    return out


def check(dev, host, pos=None):
    pos = np.arange(len(host['polar_norm'])) if pos is None else pos
    for name in NAMES[:3]:
        assert oref.same(dev[name][pos], host[name][pos]), name
    assert oref.within_one_ulp(dev['polar_norm'][pos], host['polar_norm'][pos])


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_udf_vs_numpy_branch(ctx, cpu, scan, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_orientation_match
    frames, lib, truth = scan
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=3, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=3, sig_dims=2)
    kw = dict(library=lib, center=oref.REC_CENTER, n_r=oref.REC_N_R, n_phi=oref.REC_N_PHI, n_best=N_BEST)
    res = run_orientation_match(ctx, ds, **kw)
    assert res['template'].data.shape == NAV + (N_BEST,) and res['template'].data.dtype == np.int32
    assert res['correlation'].data.dtype == np.float32 and res['polar_norm'].data.shape == NAV
    dev = flat(res)
    check(dev, flat(run_orientation_match(cpu, ds_cpu, **kw)))
    assert np.array_equal(dev['template'][:, 0], truth[:, 0]) and np.array_equal(dev['rotation'][:, 0], truth[:, 1])


def test_roi(ctx, cpu, scan):
    frames, lib, truth = scan
    data = frames.reshape(NAV + SIG)
    roi = np.zeros(NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[2, 3] = roi[8, 9] = roi[4, 0] = True
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(lib), roi=roi), raw=True)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(lib), roi=roi), raw=True)
    assert len(dev['polar_norm']) == 5
    check(dev, host)
    src = np.flatnonzero(roi.reshape(-1))
    assert np.array_equal(dev['template'][:, 0], truth[src, 0]) and np.array_equal(dev['rotation'][:, 0], truth[src, 1])


@pytest.mark.parametrize('sync_offset', [7, -7])
def test_sync_offset(ctx, cpu, scan, sync_offset):
    frames, lib, truth = scan
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(lib)))
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(lib)))
    src = np.arange(90) + sync_offset
    valid = (src >= 0) & (src < 90)
    check(dev, host, pos=np.flatnonzero(valid))
    assert np.array_equal(dev['template'][valid, 0], truth[src[valid], 0])
    assert np.array_equal(dev['rotation'][valid, 0], truth[src[valid], 1])
    for name in NAMES:
        assert np.all(dev[name][~valid] == 0), name          # no frame, no result


def test_on_device_and_cached_plan(ctx, cpu, scan):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import orientation
    frames, lib, truth = scan
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=2, sig_dims=2)
    host = flat(cpu.run_udf(dataset=cpu.load('memory', data=data, num_partitions=2, sig_dims=2), udf=udf(lib)))
    u = udf(lib)
    first = flat(ctx.run_udf(dataset=ds, udf=u))
    n_plans = len(orientation._PLANS)
    second = flat(ctx.run_udf(dataset=ds, udf=u))            # kept task instances, the cached plan: the same bytes
    assert len(orientation._PLANS) == n_plans
    for name in NAMES:
        assert first[name].tobytes() == second[name].tobytes(), name
    on_dev = ctx.run_udf(dataset=ds, udf=u, result_where='device')
    for name in NAMES:
        assert isinstance(on_dev[name].device_data, HipArray), name
    check(flat(on_dev), host)
    plans = [pl for key, pl in orientation._PLANS.items() if key[1:3] == SIG]
    assert plans and any(pl.last_kernel().startswith('k_orient_match<uint16,2> ') for pl in plans), \
        [pl.last_kernel() for pl in plans]


def test_corrections(ctx, cpu, scan):
    from libertem_amd.io.corrections import CorrectionSet
    frames, lib, truth = scan
    rng = np.random.default_rng(21)
    dark = rng.uniform(0., 1., SIG)
    gain = rng.uniform(0.95, 1.05, SIG)
    corrected = ((frames.astype(np.float64) - dark) * gain).astype(np.float32)
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(lib), corrections=CorrectionSet(dark=dark, gain=gain)))
    ds_cpu = cpu.load('memory', data=corrected.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(lib)))
    check(dev, host)
    assert np.array_equal(dev['template'][:, 0], truth[:, 0]) and np.array_equal(dev['rotation'][:, 0], truth[:, 1])


def test_errors_on_device(ctx, scan):
    frames, lib, _ = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='n_best 17'):
        ctx.run_udf(dataset=ds, udf=udf(lib, n_best=17))
    ds64 = ctx.load('memory', data=frames[:4].astype(np.float64).reshape((2, 2) + SIG), num_partitions=1, sig_dims=2)
    with pytest.raises(ValueError, match='float64'):
        ctx.run_udf(dataset=ds64, udf=udf(lib))
