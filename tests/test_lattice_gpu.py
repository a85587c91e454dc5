"""
LatticeRefineUDF on the MI355X (Context.make_with('hip')) against its own NumPy-branch run on the inline executor:
host and device-resident data, two and three partitions, a region of interest, sync offsets, a run next to SumSigUDF,
a cached second run, results left on the device, weighted and unweighted fits, and the kernels the run reports.

Tolerance of zero, a, b (and, as an absolute bound, of error): the device's refineds may differ from the host's by the
per-pair tolerance tol_ref of correlation_ref.compare and its weights by tol_el |elevation|; to first order
|dX| <= |G|_inf max tol_ref + |(M^T W M)^-1 M^T|_inf max|dw| max|res|, G = (M^T W M)^-1 M^T W.  Both terms come from
lattice_ref.reference on the host run's values; twice their sum is allowed, for the second order.  With
weighted=False only the first term applies.  selector is equal: tests/test_lattice_cpu.py establishes that no pair of
this scan lies below the correlation gap or within 0.05 px of the tolerance.
"""
import numpy as np
import pytest

import correlation_ref as cr
import lattice_ref as lr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CORR_NAMES = ('centers', 'refineds', 'peak_values', 'peak_elevations')
ALL_NAMES = CORR_NAMES + lr.NAMES
N_PEAKS = len(lr.INDICES)
TAILS = {'centers': (N_PEAKS, 2), 'refineds': (N_PEAKS, 2), 'peak_values': (N_PEAKS,), 'peak_elevations': (N_PEAKS,),
         'zero': (2,), 'a': (2,), 'b': (2,), 'selector': (N_PEAKS,), 'error': ()}
START = np.concatenate([lr.ZERO, lr.A, lr.B])


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
    """20 uint16 frames, the template, the expected peaks and the float64 correlation reference (computed once)"""
    frames, _ = lr.make_scan()
    template = cr.disk_template(lr.SIG)
    peaks = np.rint(lr.lattice_positions(lr.ZERO, lr.A, lr.B)).astype(np.int32)
    return frames, template, cr.reference(frames, template, peaks, lr.R, lr.Q)


@pytest.fixture(scope='module')
def host_runs(cpu, scan):
    """the NumPy-branch runs on the whole scan, weighted and not"""
    data = scan[0].reshape(lr.NAV + lr.SIG)
    ds = cpu.load('memory', data=data, num_partitions=2, sig_dims=2)
    return {w: flat(cpu.run_udf(dataset=ds, udf=udf(w))) for w in (True, False)}


def udf(weighted=True):
    from libertem_amd.udf import LatticeRefineUDF
    return LatticeRefineUDF(indices=lr.INDICES, zero=lr.ZERO, a=lr.A, b=lr.B, template=cr.disk_template(lr.SIG),
                            crop_radius=lr.R, refine_radius=lr.Q, tolerance=lr.UDF_TOL, weighted=weighted)


def flat(res, raw=False):
    return {name: np.asarray(res[name].raw_data if raw else res[name].data).reshape((-1,) + TAILS[name])
            for name in ALL_NAMES}


def check(dev, host, scan, weighted=True, pos=None, src=None):
    """rows `pos` of the device run against the rows `src` of the whole-scan NumPy-branch run (the frames `src`)"""
    frames, template, ref64 = scan
    n = len(dev['error'])
    pos = np.arange(n) if pos is None else pos
    src = pos if src is None else src
    # the parent's four buffers still satisfy the correlation's comparison
    got = {k: dev[k][pos] for k in CORR_NAMES}
    ref = {k: v[src] for k, v in ref64.items()}
    for k in CORR_NAMES:
        assert np.allclose(host[k][src], ref[k], rtol=1e-5, atol=1e-6), k
        ref[k] = host[k][src].astype(np.int64 if k == 'centers' else np.float64)
    cr.compare(got, ref, frames[src], template, lr.Q)
    # the tolerances of that comparison, per pair
    bound = cr.value_bound(frames[src], template)[:, None]
    with np.errstate(all='ignore'):
        d_ref = (2 * lr.Q + 1) ** 2 * 4 * lr.Q * bound / ref['wsum']
        d_el = 2 * bound * (1 / ref['rise'] + 1 / ref['std'])
    tol_ref = np.maximum(cr.REFINED_TOL, np.where(np.isfinite(d_ref), d_ref, cr.REFINED_TOL))
    tol_el = np.maximum(cr.ELEVATION_RTOL, np.where(np.isfinite(d_el), d_el, cr.ELEVATION_RTOL))
    fit = lr.reference(host['refineds'][src], host['peak_elevations'][src] if weighted else None,
                       None if weighted else host['peak_values'][src], lr.INDICES, START, lr.UDF_TOL)
    assert np.array_equal(host['selector'][src], fit['selector'])
    assert dev['selector'].dtype == np.bool_ and np.array_equal(dev['selector'][pos], fit['selector'])
    sel = fit['selector']
    first = np.abs(fit['G']).sum(axis=2).max(axis=1) * np.where(sel, tol_ref, 0).max(axis=1)
    second = 0.
    if weighted:
        dw = np.where(sel, tol_el * np.abs(host['peak_elevations'][src].astype(np.float64)), 0).max(axis=1)
        second = np.abs(fit['H']).sum(axis=2).max(axis=1) * dw * fit['res']
    lim = 2 * (first + second)
    exists = ~np.isnan(fit['error'])
    assert exists.sum() >= min(3, len(pos))
    worst = 0.
    for name in ('zero', 'a', 'b', 'error'):
        d = dev[name][pos].astype(np.float64).reshape((len(pos), -1))
        h = host[name][src].astype(np.float64).reshape((len(pos), -1))
        assert np.array_equal(np.isnan(d), np.isnan(h)) and np.array_equal(np.isnan(h[:, 0]), ~exists), name
        ratio = (np.abs(d - h)[exists] / lim[exists, None]).max()
        print(f"lattice udf: largest {name} difference / bound = {ratio:.3g} (bound up to {lim[exists].max():.3g} px)")
        assert ratio <= 1, (name, float(ratio))
        worst = max(worst, float(ratio))
    return worst


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
@pytest.mark.parametrize('num_partitions', [2, 3])
def test_udf_vs_numpy_branch(ctx, scan, host_runs, resident, num_partitions):
    from libertem_amd import hip
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import correlation
    data = scan[0].reshape(lr.NAV + lr.SIG)
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data,
                  num_partitions=num_partitions, sig_dims=2)
    weighted = num_partitions == 2
    dev = ctx.run_udf(dataset=ds, udf=udf(weighted))
    assert dev['zero'].data.shape == lr.NAV + (2,) and dev['zero'].data.dtype == np.float32
    assert dev['selector'].data.shape == lr.NAV + (N_PEAKS,) and dev['selector'].data.dtype == np.bool_
    assert dev['error'].data.shape == lr.NAV
    check(flat(dev), host_runs[weighted], scan, weighted)
    plans = [p for key, p in correlation._PLANS.items() if key[1:3] == lr.SIG]
    assert any('k_corr_peaks' in p.last_kernel() for p in plans), [p.last_kernel() for p in plans]
    assert hip.lattice_last_kernel() == 'k_lattice_fit'


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_roi(ctx, scan, host_runs, resident):
    from libertem_amd.common.hiparray import HipArray
    data = scan[0].reshape(lr.NAV + lr.SIG)
    roi = np.zeros(lr.NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[2, 3] = roi[3, 4] = roi[3, 0] = True
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0) if resident else data, num_partitions=2, sig_dims=2)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf(), roi=roi), raw=True)
    assert len(dev['zero']) == 5
    check(dev, host_runs[True], scan, pos=np.arange(5), src=np.flatnonzero(roi.reshape(-1)))


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset(ctx, scan, host_runs, sync_offset):
    data = scan[0].reshape(lr.NAV + lr.SIG)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    dev = flat(ctx.run_udf(dataset=ds, udf=udf()))
    src = np.arange(20) + sync_offset
    valid = (src >= 0) & (src < 20)
    check(dev, host_runs[True], scan, pos=np.flatnonzero(valid), src=src[valid])
    for k in ALL_NAMES:
        assert np.all(dev[k][~valid] == 0), k               # no frame: zeros in all nine buffers


def test_next_to_sumsig_cached_and_on_device(ctx, scan, host_runs):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf.sumsigudf import SumSigUDF
    frames = scan[0]
    ds = ctx.load('memory', data=HipArray.from_numpy(frames.reshape(lr.NAV + lr.SIG), 0), num_partitions=2,
                  sig_dims=2)
    both = ctx.run_udf(dataset=ds, udf=[udf(), SumSigUDF()])
    check(flat(both[0]), host_runs[True], scan)
    sums = frames.reshape((20, -1)).astype(np.float64).sum(axis=1)
    assert np.allclose(np.asarray(both[1]['intensity'].data).reshape(-1), sums, rtol=1e-6)
    # the same UDF object again: kept task instances, the cached plan and index list -- and the same bytes
    u = udf()
    first = flat(ctx.run_udf(dataset=ds, udf=u))
    second = flat(ctx.run_udf(dataset=ds, udf=u))
    for k in ALL_NAMES:
        assert first[k].tobytes() == second[k].tobytes() == flat(both[0])[k].tobytes(), k
    on_dev = ctx.run_udf(dataset=ds, udf=u, result_where='device')
    for k in ALL_NAMES:
        assert isinstance(on_dev[k].device_data, HipArray), k
    check(flat(on_dev), host_runs[True], scan)
