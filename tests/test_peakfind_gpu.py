"""
PeakFindUDF on the MI355X (Context.make_with('hip')) against its own NumPy-branch run on the inline executor: a 4 x 5
scan of 48 x 40 uint16 frames, host and device-resident, a region of interest, sync offsets, results left on the
device, detector corrections, next to CorrelationUDF on the plan they share.  The seeded frames are decided
(tests/test_peakfind_cpu.py), so n_found and centers must be equal; peak_values lie within correlation_ref's bound,
refineds within 0.02 px and peak_elevations within 1e-3 relative.  One noisy frame whose float64 map is NOT decided is
held to properties only.
"""
import numpy as np
import pytest

import correlation_ref as cr
import peakfind_ref as pr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG, NAV = pr.SCAN_SIG, pr.SCAN_NAV
NAMES = pr.NAMES


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
    frames, tmpl, p, _ = pr.scan_case()
    return frames, tmpl, p


def udf(tmpl, p):
    from libertem_amd.udf import PeakFindUDF
    return PeakFindUDF(template=tmpl, **p)


def flat(res, n_peaks, raw=False):
    out = {}
    for name in NAMES:
        a = np.asarray(res[name].raw_data if raw else res[name].data)
        tail = {'n_found': (), 'centers': (n_peaks, 2), 'refineds': (n_peaks, 2)}.get(name, (n_peaks,))
        out[name] = a.reshape((-1,) + tail)
    return out


def check(dev, host, frames, tmpl, pos=None, src=None):
    """rows `pos` of the device run against the same rows of the NumPy-branch run; they hold the frames `src`"""
    n, k = dev['peak_values'].shape
    pos = np.arange(n) if pos is None else pos
    src = pos if src is None else src
    assert np.array_equal(dev['n_found'][pos], host['n_found'][pos])
    assert np.all(host['n_found'][pos] == 9)                 # the nine seeded disks
    assert np.array_equal(dev['centers'][pos], host['centers'][pos])
    found = np.arange(k)[None] < host['n_found'][pos][:, None]
    bound = cr.value_bound(frames[src], tmpl)[:, None] * np.ones((1, k))
    err = np.abs(dev['peak_values'][pos].astype(np.float64) - host['peak_values'][pos])
    assert (err[found] / bound[found]).max() <= 1.0
    e_ref = np.abs(dev['refineds'][pos].astype(np.float64) - host['refineds'][pos])
    assert e_ref[found].max() <= pr.REFINED_TOL
    e_el = np.abs(dev['peak_elevations'][pos].astype(np.float64) - host['peak_elevations'][pos])
    assert np.all(e_el[found] <= pr.ELEVATION_RTOL * np.abs(host['peak_elevations'][pos][found]))
    for name in ('refineds', 'peak_values', 'peak_elevations'):
        assert np.all(np.isnan(dev[name][pos][~found])), name
    assert np.all(dev['centers'][pos][~found] == -1)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_udf_vs_numpy_branch(ctx, cpu, scan, resident):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import run_peakfind
    frames, tmpl, p = scan
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=3, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=3, sig_dims=2)
    dev = run_peakfind(ctx, ds, tmpl, **p)
    n = p['num_peaks']
    assert dev['n_found'].data.shape == NAV and dev['n_found'].data.dtype == np.int32
    assert dev['centers'].data.shape == NAV + (n, 2) and dev['centers'].data.dtype == np.int32
    assert dev['peak_elevations'].data.shape == NAV + (n,) and dev['refineds'].data.dtype == np.float32
    check(flat(dev, n), flat(run_peakfind(cpu, ds_cpu, tmpl, **p), n), frames, tmpl)


def test_roi(ctx, cpu, scan):
    frames, tmpl, p = scan
    data = frames.reshape(NAV + SIG)
    roi = np.zeros(NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[2, 3] = roi[3, 4] = roi[3, 0] = True
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2)
    n = p['num_peaks']
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(tmpl, p), roi=roi), n, raw=True)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(tmpl, p), roi=roi), n, raw=True)
    assert len(dev['n_found']) == 5
    check(dev, host, frames, tmpl, pos=np.arange(5), src=np.flatnonzero(roi.reshape(-1)))


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset(ctx, cpu, scan, sync_offset):
    frames, tmpl, p = scan
    data = frames.reshape(NAV + SIG)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    ds_cpu = cpu.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    n = p['num_peaks']
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(tmpl, p)), n)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(tmpl, p)), n)
    src = np.arange(20) + sync_offset
    valid = (src >= 0) & (src < 20)
    check(dev, host, frames, tmpl, pos=np.flatnonzero(valid), src=src[valid])
    for name in NAMES:
        assert np.all(dev[name][~valid] == 0), name          # no frame, no result


def test_on_device_cached_and_next_to_correlation(ctx, cpu, scan):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import CorrelationUDF, correlation
    frames, tmpl, p = scan
    data = frames.reshape(NAV + SIG)
    n = p['num_peaks']
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=2, sig_dims=2)
    host = flat(cpu.run_udf(dataset=cpu.load('memory', data=data, num_partitions=2, sig_dims=2), udf=udf(tmpl, p)), n)
    u = udf(tmpl, p)
    first = flat(ctx.run_udf(dataset=ds, udf=u), n)
    second = flat(ctx.run_udf(dataset=ds, udf=u), n)         # kept task instances, the cached plan: the same bytes
    for name in NAMES:
        assert first[name].tobytes() == second[name].tobytes(), name
    on_dev = ctx.run_udf(dataset=ds, udf=u, result_where='device')
    for name in NAMES:
        assert isinstance(on_dev[name].device_data, HipArray), name
    check(flat(on_dev, n), host, frames, tmpl)
    plans = [pl for key, pl in correlation._PLANS.items() if key[1:3] == SIG]
    assert plans and any('k_pf_select' in pl.last_kernel() for pl in plans), [pl.last_kernel() for pl in plans]
    # frame 0's peaks as the list of a CorrelationUDF in the same run: the plan is shared, the rows agree
    peaks = first['centers'][0, :9]
    both = ctx.run_udf(dataset=ds, udf=[udf(tmpl, p), CorrelationUDF(peaks, tmpl, p['min_distance'])])
    check(flat(both[0], n), host, frames, tmpl)
    at = np.asarray(both[1]['peak_values'].data).reshape((20, 9))
    assert at[0].tobytes() == flat(both[0], n)['peak_values'][0, :9].tobytes()


def test_corrections(ctx, cpu, scan):
    from libertem_amd.io.corrections import CorrectionSet
    frames, tmpl, p = scan
    corrected, dark, gain = pr.corrected_scan()
    n = p['num_peaks']
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(tmpl, p), corrections=CorrectionSet(dark=dark, gain=gain)), n)
    ds_cpu = cpu.load('memory', data=corrected.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    host = flat(cpu.run_udf(dataset=ds_cpu, udf=udf(tmpl, p)), n)
    check(dev, host, corrected, tmpl)


def test_undecided_frame_keeps_the_properties(ctx):
    frames, tmpl, p = pr.undecided_frame()
    n, d = p['num_peaks'], p['min_distance']
    ds = ctx.load('memory', data=frames.reshape((1, 1) + SIG), num_partitions=1, sig_dims=2)
    got = flat(ctx.run_udf(dataset=ds, udf=udf(tmpl, p)), n)
    k = int(got['n_found'][0])
    assert 9 < k <= n
    c = got['centers'][0, :k].astype(np.int64)
    v = got['peak_values'][0, :k].astype(np.float64)
    apart = np.abs(c[:, None] - c[None]).max(axis=2) + (d + 1) * np.eye(k, dtype=np.int64)
    assert apart.min() > d                                   # spacing
    assert np.all(np.diff(v) <= 0)                           # order
    corr = cr.correlation(frames[0], tmpl)
    bound = cr.value_bound(frames, tmpl)[0]
    assert np.abs(v - corr[c[:, 0], c[:, 1]]).max() <= bound
    h, w = SIG
    for y, x in c:
        win = corr[max(y - d, 0):min(y + d, h - 1) + 1, max(x - d, 0):min(x + d, w - 1) + 1]
        assert corr[y, x] >= win.max() - 2 * bound           # a maximum of its neighbourhood to within the error


def test_errors_on_device(ctx, scan):
    frames, tmpl, p = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='num_peaks 2000'):
        ctx.run_udf(dataset=ds, udf=udf(tmpl, dict(p, num_peaks=2000)))
    with pytest.raises(ValueError, match='template'):
        ctx.run_udf(dataset=ds, udf=udf(tmpl[:40], p))
