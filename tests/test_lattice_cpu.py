"""
LatticeRefineUDF without a GPU: `fit_lattice` (the NumPy branch) against the frame-by-frame float64 restatement of the
definition (tests/lattice_ref.py) on every kernel case, the conditions the GPU tests rely on -- checked here in
float64 so that a GPU failure cannot hide behind them --, an exact lattice, `lattice_peaks`, `lattice_strain`, the
argument errors, whole runs on the inline executor with a region of interest and sync offsets, and the declaration of
the two library entries.

Tolerance of zero, a, b, error: eps32 |ref| (the final cast) + 16 kappa P eps64 max|refineds| (the float64 solve;
kappa the condition number of the weighted normal matrix, 16 the allowance for the constants of the elimination).
"""
import os
import re

import numpy as np
import pytest

import correlation_ref as cr
import lattice_ref as lr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import (CorrelationUDF, LatticeRefineUDF, fit_lattice, lattice_peaks, lattice_strain,
                              run_refine)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR_NAMES = ('centers', 'refineds', 'peak_values', 'peak_elevations')


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def scan():
    """the scan of the UDF tests, its correlation reference and the lattice reference on top of it"""
    frames, true = lr.make_scan()
    template = cr.disk_template(lr.SIG)
    peaks = np.rint(lr.lattice_positions(lr.ZERO, lr.A, lr.B)).astype(np.int32)
    corr = cr.reference(frames, template, peaks, lr.R, lr.Q)
    start = np.concatenate([lr.ZERO, lr.A, lr.B])
    fits = {w: lr.reference(corr['refineds'], corr['peak_elevations'] if w else None,
                            None if w else corr['peak_values'], lr.INDICES, start, lr.UDF_TOL) for w in (True, False)}
    return frames, true, template, peaks, corr, fits


def got_of(res):
    return dict(zip(lr.NAMES, res))


@pytest.mark.parametrize('case', lr.KERNEL_CASES, ids=lambda c: c[0])
def test_fit_lattice_vs_definition(case):
    c = lr.kernel_case(case)
    ref = lr.case_reference(c)
    res = fit_lattice(c['refineds'], c['weights'], c['peak_values'], c['indices'], c['start'][0:2], c['start'][2:4],
                      c['start'][4:6], c['tol'])
    assert [r.dtype for r in res] == [np.float32] * 3 + [np.bool_, np.float32]
    assert res[0].shape == (case[2], 2) and res[3].shape == (case[2], len(c['indices'])) and res[4].shape == (case[2],)
    lr.compare(got_of(res), ref, c['refineds'])
    # what the case is there for
    fit = ~np.isnan(ref['error'])
    n_peaks = len(c['indices'])
    if n_peaks < 3 or case[1] == 'p3-line':
        assert not fit.any()
    for f, what in case[5].items():
        if what == 'reject_all':
            assert not ref['selector'][f].any() and not fit[f]
        elif what == 'three':
            assert ref['selector'][f].sum() == 3 and fit[f]
        else:
            assert ref['selector'][f].sum() >= 3 and not fit[f]
    if n_peaks >= 7:
        assert fit.any() and not ref['selector'].all()
    if case[1] == 'p3-span':
        assert fit.any() and not fit.all()


@pytest.mark.parametrize('case', lr.KERNEL_CASES, ids=lambda c: c[0])
def test_kernel_cases_keep_their_margins(case):
    c = lr.kernel_case(case)
    ref = lr.case_reference(c)
    dist = ref['dist'][np.isfinite(ref['dist'])]
    assert dist.size and np.abs(dist - c['tol']).min() >= 1e-3, float(np.abs(dist - c['tol']).min())
    fit = ~np.isnan(ref['kappa'])
    if fit.any():
        solve = ref['kappa'][fit] * len(c['indices']) * lr.EPS64 * lr.largest(c['refineds'])
        assert solve.max() < lr.EPS32 / 16, float(solve.max())


def test_scan_keeps_its_margins(scan):
    frames, _, template, peaks, corr, fits = scan
    bound = cr.value_bound(frames, template)[:, None]
    assert np.all(corr['gap'] > 2 * bound), float((corr['gap'] / (2 * bound)).min())
    for weighted, fit in fits.items():
        assert np.abs(fit['dist'] - lr.UDF_TOL).min() >= 0.05, float(np.abs(fit['dist'] - lr.UDF_TOL).min())
        exists = ~np.isnan(fit['error'])
        assert exists.sum() >= 15 and not fit['selector'].all() and fit['selector'].any(axis=1).all()


def test_exact_lattice_is_recovered():
    idx = lr.INDEX_SETS['p64']
    zero, a, b = np.array([30.25, 28.5]), np.array([0.5, 9.75]), np.array([10.25, -0.75])
    r = (zero[None] + idx[:, :1] * a[None] + idx[:, 1:] * b[None])[None].astype(np.float32)     # (exact in float32)
    assert np.array_equal(r.astype(np.float64)[0], zero[None] + idx[:, :1] * a[None] + idx[:, 1:] * b[None])
    start = np.concatenate([zero + 0.3, a * 1.01, b * 0.99])
    ref = lr.reference(r, None, None, idx, start, 2.0)
    assert ref['selector'].all()
    res = got_of(fit_lattice(r, None, None, idx, start[0:2], start[2:4], start[4:6], 2.0))
    lr.compare(res, ref, r)
    solve = float(lr.value_tolerance(ref, r)[0, 0])
    for name, exact in (('zero', zero), ('a', a), ('b', b)):
        assert np.all(np.abs(res[name][0].astype(np.float64) - exact) <= lr.EPS32 * np.abs(exact) + solve), name
    assert res['error'][0] <= solve


def test_lattice_peaks_order_and_margin():
    idx, peaks = lattice_peaks((48, 48), (24, 24), (0, 10), (10, 0), 2)
    assert idx.dtype == np.int32 and peaks.dtype == np.int32
    assert len(idx) == 25 and [tuple(v) for v in idx[:6]] == [(-2, -2), (-2, -1), (-2, 0), (-2, 1), (-2, 2), (-1, -2)]
    assert np.array_equal(peaks, 24 + 10 * idx[:, ::-1])
    idx5, peaks5 = lattice_peaks((48, 48), (24, 24), (0, 10), (10, 0), 2, margin=5)
    assert len(idx5) == 9 and np.abs(idx5).max() == 1 and peaks5.min() == 14 and peaks5.max() == 34
    assert [tuple(v) for v in idx5] == [(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)]
    idx4, peaks4 = lattice_peaks((48, 48), (24, 24), (0, 10), (10, 0), 2, margin=4)
    assert len(idx4) == 16 and peaks4.max() == 34            # 44 lies 3 pixels inside a 48-pixel edge, 4 inside 49
    idx4, peaks4 = lattice_peaks((49, 49), (24, 24), (0, 10), (10, 0), 2, margin=4)
    assert len(idx4) == 25 and peaks4.min() == 4 and peaks4.max() == 44


def test_lattice_strain():
    ref_a, ref_b = np.array([0., 10.]), np.array([10., 0.])
    theta = 1e-3
    rot = np.array([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])       # rows and columns (y, x)
    s = lattice_strain(rot @ ref_a, rot @ ref_b, ref_a, ref_b)
    assert abs(s['rotation'] - np.sin(theta)) < 1e-14
    for name in ('e_yy', 'e_xx'):
        assert abs(s[name] - (np.cos(theta) - 1)) < 1e-14 and abs(s[name]) < theta ** 2          # zero to first order
    assert abs(s['e_yx']) < 1e-14
    stretch = np.diag([1.01, 1.0])                          # 1 % along y
    a = np.stack([stretch @ ref_a, ref_a, np.full(2, np.nan)]).reshape((3, 1, 2))
    b = np.stack([stretch @ ref_b, ref_b, ref_b]).reshape((3, 1, 2))
    s = lattice_strain(a, b, ref_a, ref_b)
    assert s['e_yy'].shape == (3, 1) and s['e_yy'].dtype == np.float64
    assert abs(s['e_yy'][0, 0] - 0.01) < 1e-14 and abs(s['e_xx'][0, 0]) < 1e-14
    assert all(abs(s[k][1, 0]) < 1e-14 for k in s)
    assert np.isnan(s['e_xx'][2, 0]) and np.isnan(s['rotation'][2, 0])
    shear = np.array([[1., 0.02], [0., 1.]])                # y' = y + 0.02 x
    s = lattice_strain(shear @ ref_a, shear @ ref_b, ref_a, ref_b)
    assert abs(s['e_yx'] - 0.01) < 1e-14 and abs(s['rotation'] - 0.01) < 1e-14


def flat(res, names, n_peaks, raw=False):
    out = {}
    for name in names:
        a = np.asarray(res[name].raw_data if raw else res[name].data)
        tail = {'centers': (n_peaks, 2), 'refineds': (n_peaks, 2), 'peak_values': (n_peaks,),
                'peak_elevations': (n_peaks,), 'zero': (2,), 'a': (2,), 'b': (2,), 'selector': (n_peaks,),
                'error': ()}[name]
        out[name] = a.reshape((-1,) + tail)
    return out


def check_run(res, scan, weighted, pos=None, src=None, raw=False):
    """rows `pos` of a run hold the frames `src`: the parent's four buffers as the correlation reference has them,
    the five new ones as the lattice reference has them"""
    _, _, _, peaks, corr, fits = scan
    got = flat(res, CORR_NAMES + lr.NAMES, len(peaks), raw=raw)
    n = len(got['error'])
    pos = np.arange(n) if pos is None else pos
    src = pos if src is None else src
    for name in CORR_NAMES:
        assert np.allclose(got[name][pos], corr[name][src], rtol=1e-5, atol=1e-6), name
    # the fit of the NumPy branch starts from ITS float32 refineds and elevations: the reference on the same inputs
    ref = lr.reference(got['refineds'][pos], got['peak_elevations'][pos] if weighted else None,
                       None if weighted else got['peak_values'][pos], lr.INDICES,
                       np.concatenate([lr.ZERO, lr.A, lr.B]), lr.UDF_TOL)
    assert np.array_equal(ref['selector'], fits[weighted]['selector'][src])
    lr.compare({k: got[k][pos] for k in lr.NAMES}, ref, got['refineds'][pos])
    assert got['selector'].dtype == np.bool_ and got['zero'].dtype == np.float32
    return got


@pytest.mark.parametrize('weighted', [True, False])
def test_run_refine(ctx, scan, weighted):
    frames, true = scan[0], scan[1]
    ds = ctx.load('memory', data=frames.reshape(lr.NAV + lr.SIG), num_partitions=2, sig_dims=2)
    res = run_refine(ctx, ds, lr.ZERO, lr.A, lr.B, lr.INDICES, scan[2], lr.R, refine_radius=lr.Q,
                     tolerance=lr.UDF_TOL, weighted=weighted)
    assert res['zero'].data.shape == lr.NAV + (2,) and res['selector'].data.shape == lr.NAV + (10,)
    assert res['error'].data.shape == lr.NAV
    got = check_run(res, scan, weighted)
    # the fitted lattice explains the disks' true positions to about the rounding of their integer centres
    fit = ~np.isnan(got['error'])
    model = (got['zero'][:, None] + lr.INDICES[None, :, :1] * got['a'][:, None] + lr.INDICES[None, :, 1:]
             * got['b'][:, None])
    off = np.abs(model - true)[fit][got['selector'][fit]]
    assert off.max() < 1.0 and got['error'][fit].max() < 1.0


def test_roi(ctx, scan):
    ds = ctx.load('memory', data=scan[0].reshape(lr.NAV + lr.SIG), num_partitions=2, sig_dims=2)
    roi = np.zeros(lr.NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[2, 3] = roi[3, 4] = roi[3, 0] = True
    res = run_refine(ctx, ds, lr.ZERO, lr.A, lr.B, lr.INDICES, scan[2], lr.R, tolerance=lr.UDF_TOL, roi=roi)
    check_run(res, scan, True, pos=np.arange(5), src=np.flatnonzero(roi.reshape(-1)), raw=True)


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset(ctx, scan, sync_offset):
    ds = ctx.load('memory', data=scan[0].reshape(lr.NAV + lr.SIG), num_partitions=2, sig_dims=2,
                  sync_offset=sync_offset)
    res = run_refine(ctx, ds, lr.ZERO, lr.A, lr.B, lr.INDICES, scan[2], lr.R, tolerance=lr.UDF_TOL)
    src = np.arange(20) + sync_offset
    valid = (src >= 0) & (src < 20)
    got = check_run(res, scan, True, pos=np.flatnonzero(valid), src=src[valid])
    for name in CORR_NAMES + lr.NAMES:
        assert np.all(got[name][~valid] == 0), name         # no frame: zeros in all nine buffers


def test_value_errors(ctx, scan):
    template = scan[2]
    ds = ctx.load('memory', data=scan[0].reshape(lr.NAV + lr.SIG), num_partitions=2, sig_dims=2)

    def run(**kw):
        args = dict(zero=lr.ZERO, a=lr.A, b=lr.B, indices=lr.INDICES, template=template, crop_radius=lr.R,
                    tolerance=lr.UDF_TOL)
        args.update(kw)
        return run_refine(ctx, ds, **args)

    for bad in (lr.INDICES.astype(np.float32), lr.INDICES[:, :1], np.zeros((0, 2), np.int32), lr.INDICES.reshape(-1)):
        with pytest.raises(ValueError, match='indices'):
            run(indices=bad)
    with pytest.raises(ValueError, match='indices'):
        run(indices=np.array([(0, 0), (2**20 + 1, 0)]))
    with pytest.raises(ValueError, match='outside'):
        run(indices=np.array([(0, 0), (3, 0)]))             # (24, 54)
    with pytest.raises(ValueError, match='outside'):
        run(indices=np.array([(0, -3)]))                    # (-6, 24)
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(ValueError, match='tolerance'):
            run(tolerance=bad)
    with pytest.raises(ValueError, match='zero'):
        run(zero=(np.nan, 24.))
    with pytest.raises(ValueError, match='a must'):
        run(a=(0., 10., 0.))
    with pytest.raises(ValueError, match='crop_radius'):
        run(crop_radius=0)
    with pytest.raises(ValueError, match='template'):
        run(template=template[:, :40])


def test_udf_declarations():
    udf = LatticeRefineUDF(lr.INDICES, lr.ZERO, lr.A, lr.B, cr.disk_template(lr.SIG), lr.R, tolerance=1.5)
    assert isinstance(udf, CorrelationUDF)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_dist_merge() == {k: 'disjoint' for k in CORR_NAMES + lr.NAMES}
    bufs = udf.get_result_buffers()
    assert {k: (b.kind, np.dtype(b.dtype), b.extra_shape) for k, b in bufs.items()} == {
        'centers': ('nav', np.dtype('int32'), (10, 2)), 'refineds': ('nav', np.dtype('float32'), (10, 2)),
        'peak_values': ('nav', np.dtype('float32'), (10,)), 'peak_elevations': ('nav', np.dtype('float32'), (10,)),
        'zero': ('nav', np.dtype('float32'), (2,)), 'a': ('nav', np.dtype('float32'), (2,)),
        'b': ('nav', np.dtype('float32'), (2,)), 'selector': ('nav', np.dtype('bool'), (10,)),
        'error': ('nav', np.dtype('float32'), ())}
    assert udf.params.refine_radius == 1 and udf.params.weighted is True
    assert np.array_equal(udf._peaks(), np.rint(lr.lattice_positions(lr.ZERO, lr.A, lr.B)).astype(np.int32))
    assert tuple(udf._peaks()[-1]) == (4, 44)
    again = udf.copy()
    assert np.array_equal(again._peaks(), udf._peaks())


def _declared_arguments(name):
    """number of parameters of `name` in the header text"""
    hdr = open(os.path.join(ROOT, 'include', 'ltmi.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, hdr)
    assert m, f"{name} is not declared in include/ltmi.h"
    args = m.group(1).strip()
    return 0 if args in ('', 'void') else len(args.split(','))


@pytest.mark.parametrize('name, n_args', [('ltmi_lattice_fit', 15), ('ltmi_lattice_last_kernel', 0)])
def test_header_and_binding_agree(name, n_args):
    from libertem_amd import hip
    assert _declared_arguments(name) == n_args
    assert name in hip.EXPORTS
    fn = getattr(hip.lib(), name)
    assert len(fn.argtypes) == n_args
    assert callable(hip.lattice_fit) and callable(hip.lattice_last_kernel)
