"""
PeakFindUDF without a GPU: `find_in_maps` against the brute-force restatement (tests/peakfind_ref.py) on quantised
maps full of ties, the constant map, spacing and order of the kept peaks, the NumPy branch against
`correlate_frames` at the found centres, `run_udf` on the inline executor with a region of interest and sync offsets,
`find_peaks` of a summed frame feeding CorrelationUDF, the argument errors, the signatures of the bindings -- and that
every seeded case of the GPU tests is decided: an error within the transforms' bound cannot change what a frame keeps.
"""
import inspect

import numpy as np
import pytest

import correlation_ref as cr
import peakfind_ref as pr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import PeakFindUDF, find_in_maps, find_peaks, run_correlation, run_peakfind
from libertem_amd.udf.correlation import correlate_frames

NAMES = pr.NAMES


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def scan():
    """the scan of the GPU test: frames, template, parameters, seeded positions; its float64 reference, computed once"""
    frames, tmpl, p, pos = pr.scan_case()
    maps = np.stack([cr.correlation(f, tmpl) for f in frames])
    return frames, tmpl, p, pos, pr.reference(maps, **p)


def equal_to_reference(got, ref, rtol=1e-6):
    """the five arrays of find_in_maps against the restatement's: decisions and values exact, statistics to the
    rounding of their float32 cast"""
    n_found, centers, refineds, values, elevations = got
    assert n_found.dtype == np.int32 and centers.dtype == np.int32
    assert refineds.dtype == values.dtype == elevations.dtype == np.float32
    assert np.array_equal(n_found, ref['n_found'])
    assert np.array_equal(centers, ref['centers'])
    assert np.array_equal(values, ref['peak_values'].astype(np.float32), equal_nan=True)
    assert np.allclose(refineds, ref['refineds'], rtol=rtol, atol=0, equal_nan=True)
    assert np.allclose(elevations, ref['peak_elevations'], rtol=rtol, atol=1e-7, equal_nan=True)


@pytest.mark.parametrize('d', [1, 2, 5])
@pytest.mark.parametrize('sig', pr.MAP_SIGS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_find_in_maps_equals_the_restatement(sig, d):
    for dtype in ('float32', 'float64'):
        maps = pr.quantised_maps(sig, 2, seed=sig[1] + d, dtype=dtype)
        # (thresholds inside the value range, so that both cut; N = 1, 7 and more than there are candidates)
        for b, n, t_abs, t_rel in ((0, 1, 0.0, 0.0), (3, 7, -3.0, 0.0), (0, 1000, -3.0, 0.0), (3, 1000, 1.0, 0.5)):
            p = pr.params(n, d, border=b, threshold_abs=t_abs, threshold_rel=t_rel, refine_radius=2)
            ref = pr.reference(maps, **p)
            if n == 1000:
                assert np.all(ref['n_found'] < n)
            equal_to_reference(find_in_maps(maps, **p), ref)


@pytest.mark.parametrize('d', [1, 5, 40])
def test_special_maps(d):
    # constant, corners and edges, ties across cell boundaries, a threshold on a value, NaN and Inf
    maps = pr.special_maps((33, 35), d)
    for kw in (dict(threshold_abs=-1.0), dict(threshold_rel=0.5), dict(border=3)):
        p = pr.params(20, d, **kw)
        got = find_in_maps(maps, **p)
        equal_to_reference(got, pr.reference(maps, **p))
        assert got[0][4] == 0 and got[0][6] == 0 and got[0][5] == got[0][1]      # NaN, Inf, and the frame between
    rel = find_in_maps(maps[3:4], 20, d, threshold_rel=0.5)
    kept = rel[3][0, :rel[0][0]]
    if d == 40:                                              # (the whole frame is one neighbourhood)
        assert list(kept) == [8.0]
        return
    assert 4.0 in kept and 2.0 not in kept and 3.0 not in kept                  # not below 0.5 * 8: 4 stays


def test_constant_map():
    ones = np.ones((1, 9, 11), np.float32)
    assert pr.candidates(ones[0], 2) == [(0, 0)]
    n_found, centers, refineds, values, elevations = find_in_maps(ones, 3, 2)
    assert n_found[0] == 1 and tuple(centers[0, 0]) == (0, 0) and np.all(centers[0, 1:] == -1)
    assert values[0, 0] == 1 and elevations[0, 0] == 0 and tuple(refineds[0, 0]) == (0, 0)
    assert np.all(np.isnan(values[0, 1:])) and np.all(np.isnan(refineds[0, 1:]))
    # the default threshold_abs is 0 and strict: a zero map keeps nothing
    zero = find_in_maps(np.zeros((1, 9, 11)), 3, 2)
    assert zero[0][0] == 0 and np.all(zero[1] == -1) and np.all(np.isnan(zero[3]))
    assert find_in_maps(np.zeros((1, 9, 11)), 3, 2, threshold_abs=-1.0)[0][0] == 1


@pytest.mark.parametrize('d', [1, 2, 5])
def test_spacing_and_order(d):
    maps = pr.quantised_maps((48, 40), 3, seed=d)
    n_found, centers, _, values, _ = find_in_maps(maps, 40, d, threshold_abs=-5.0)
    for f in range(3):
        n = n_found[f]
        assert n > 5
        c = centers[f, :n].astype(np.int64)
        apart = np.abs(c[:, None] - c[None]).max(axis=2) + (d + 1) * np.eye(n, dtype=np.int64)
        assert apart.min() > d
        assert np.all(np.diff(values[f, :n]) <= 0)
        assert np.array_equal(values[f, :n], maps[f][c[:, 0], c[:, 1]])


def flat(res, n_peaks, raw=False):
    out = {}
    for name in NAMES:
        a = np.asarray(res[name].raw_data if raw else res[name].data)
        tail = {'n_found': (), 'centers': (n_peaks, 2), 'refineds': (n_peaks, 2)}.get(name, (n_peaks,))
        out[name] = a.reshape((-1,) + tail)
    return out


def check_rows(got, ref, rows, src):
    """rows `rows` of a run hold the frames `src` of the reference"""
    assert np.array_equal(got['n_found'][rows], ref['n_found'][src])
    assert np.array_equal(got['centers'][rows], ref['centers'][src])
    for name in ('refineds', 'peak_values', 'peak_elevations'):
        assert np.allclose(got[name][rows], ref[name][src], rtol=1e-5, atol=1e-6, equal_nan=True), name


def test_numpy_branch_equals_the_definition_and_correlate_frames(ctx, scan):
    frames, tmpl, p, pos, ref = scan
    ds = ctx.load('memory', data=frames.reshape(pr.SCAN_NAV + pr.SCAN_SIG), num_partitions=2, sig_dims=2)
    res = run_peakfind(ctx, ds, tmpl, **p)
    n = p['num_peaks']
    assert res['n_found'].data.shape == pr.SCAN_NAV and res['n_found'].data.dtype == np.int32
    assert res['centers'].data.shape == pr.SCAN_NAV + (n, 2) and res['peak_elevations'].data.shape == pr.SCAN_NAV + (n,)
    got = flat(res, n)
    check_rows(got, ref, np.arange(20), np.arange(20))
    # the nine seeded disks, strongest first, and empty slots behind them
    assert np.all(got['n_found'] == 9)
    for f in range(20):
        assert sorted(map(tuple, got['centers'][f, :9])) == sorted(map(tuple, pos[f]))
    assert np.all(got['centers'][:, 9:] == -1) and np.all(np.isnan(got['peak_values'][:, 9:]))
    # what CorrelationUDF's definition gives at the found centres, window radius d
    for f in (0, 7, 19):
        c, r, v, e = correlate_frames(frames[f:f + 1], tmpl, got['centers'][f, :9], p['min_distance'],
                                      p['refine_radius'])
        assert np.array_equal(c[0], got['centers'][f, :9])
        assert np.allclose(r[0], got['refineds'][f, :9], rtol=1e-6, atol=0)
        assert np.allclose(v[0], got['peak_values'][f, :9], rtol=1e-6, atol=0)
        assert np.allclose(e[0], got['peak_elevations'][f, :9], rtol=1e-5, atol=0)


def test_roi(ctx, scan):
    frames, tmpl, p, _, ref = scan
    ds = ctx.load('memory', data=frames.reshape(pr.SCAN_NAV + pr.SCAN_SIG), num_partitions=2, sig_dims=2)
    roi = np.zeros(pr.SCAN_NAV, bool)
    roi[0, 1] = roi[2, 3] = roi[3, 4] = roi[1, 0] = True
    got = flat(run_peakfind(ctx, ds, tmpl, roi=roi, **p), p['num_peaks'], raw=True)
    assert len(got['n_found']) == 4
    check_rows(got, ref, np.arange(4), np.flatnonzero(roi.reshape(-1)))


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset(ctx, scan, sync_offset):
    frames, tmpl, p, _, ref = scan
    ds = ctx.load('memory', data=frames.reshape(pr.SCAN_NAV + pr.SCAN_SIG), num_partitions=3, sig_dims=2,
                  sync_offset=sync_offset)
    got = flat(run_peakfind(ctx, ds, tmpl, **p), p['num_peaks'])
    src = np.arange(20) + sync_offset                        # position i holds frame i + sync_offset
    valid = (src >= 0) & (src < 20)
    check_rows(got, ref, np.flatnonzero(valid), src[valid])
    for name in NAMES:
        assert np.all(got[name][~valid] == 0), name          # no frame, no result


def test_nonfinite_frame(ctx, scan):
    frames, tmpl, p, _, ref = scan
    data = frames.astype(np.float32)
    data[7, 3, 3] = np.inf
    data[11, 30, 5] = np.nan
    ds = ctx.load('memory', data=data.reshape(pr.SCAN_NAV + pr.SCAN_SIG), num_partitions=2, sig_dims=2)
    got = flat(run_peakfind(ctx, ds, tmpl, **p), p['num_peaks'])
    ok = ~np.isin(np.arange(20), (7, 11))
    check_rows(got, ref, np.flatnonzero(ok), np.flatnonzero(ok))
    for f in (7, 11):
        assert got['n_found'][f] == 0 and np.all(got['centers'][f] == -1) and np.all(np.isnan(got['refineds'][f]))


def test_find_peaks_of_a_summed_frame_feeds_correlation(ctx):
    from libertem_amd.udf.sum import SumUDF
    one, pos, _ = pr.make_frames(pr.SCAN_SIG, 1, seed=31, dtype='uint16')
    rng = np.random.default_rng(5)
    frames = (one.astype(np.int64) + rng.integers(0, 200, (6,) + pr.SCAN_SIG)).astype(np.uint16)
    tmpl = pr.template(pr.SCAN_SIG)
    ds = ctx.load('memory', data=frames.reshape((2, 3) + pr.SCAN_SIG), num_partitions=2, sig_dims=2)
    total = np.asarray(ctx.run_udf(dataset=ds, udf=SumUDF())['intensity'].data)
    peaks = find_peaks(total, tmpl, num_peaks=16, min_distance=5, threshold_abs=6 * pr.threshold_for(frames, tmpl))
    assert peaks.dtype.kind == 'i' and peaks.shape == (9, 2)
    assert sorted(map(tuple, peaks)) == sorted(map(tuple, pos[0]))
    res = run_correlation(ctx, ds, peaks, tmpl, crop_radius=3)
    assert np.array_equal(res['centers'].data.reshape((6, 9, 2)), np.broadcast_to(peaks, (6, 9, 2)))


def test_value_errors(ctx, scan):
    frames, tmpl, p, _, _ = scan
    ds = ctx.load('memory', data=frames.reshape(pr.SCAN_NAV + pr.SCAN_SIG), num_partitions=2, sig_dims=2)
    for kw, match in ((dict(num_peaks=0), 'num_peaks 0'), (dict(num_peaks=1025), 'num_peaks 1025'),
                      (dict(min_distance=0), 'min_distance 0'), (dict(border=-1), 'border -1'),
                      (dict(border=20), 'border 20'), (dict(threshold_rel=1.5), 'threshold_rel 1.5'),
                      (dict(threshold_rel=-0.1), 'threshold_rel -0.1'), (dict(threshold_abs=np.nan), 'threshold_abs'),
                      (dict(refine_radius=0), 'refine_radius 0')):
        with pytest.raises(ValueError, match=match):
            run_peakfind(ctx, ds, tmpl, **dict(p, **kw))
        if 'num_peaks' not in kw or kw['num_peaks'] == 0:
            with pytest.raises(ValueError, match=match):
                find_in_maps(np.zeros((1,) + pr.SCAN_SIG), **dict(p, **kw))
    with pytest.raises(ValueError, match='template'):
        run_peakfind(ctx, ds, tmpl[:, :30], **p)
    with pytest.raises(ValueError, match='template'):
        find_peaks(np.zeros((8, 8)), np.zeros((8, 9)), 3, 1)
    with pytest.raises(ValueError, match='maps'):
        find_in_maps(np.zeros((4, 4), np.float32), 3, 1)
    with pytest.raises(ValueError, match='maps'):
        find_in_maps(np.zeros((1, 4, 4), np.int32), 3, 1)
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D'):
        run_peakfind(ctx, ds3, np.zeros((4, 8, 8), np.float32), 3, 1)


def test_udf_declarations():
    udf = PeakFindUDF(pr.template((32, 32)), 7, 3)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {k: 'disjoint' for k in NAMES}
    bufs = udf.get_result_buffers()
    assert {k: (b.kind, np.dtype(b.dtype), b.extra_shape) for k, b in bufs.items()} == {
        'n_found': ('nav', np.dtype('int32'), ()),
        'centers': ('nav', np.dtype('int32'), (7, 2)), 'refineds': ('nav', np.dtype('float32'), (7, 2)),
        'peak_values': ('nav', np.dtype('float32'), (7,)), 'peak_elevations': ('nav', np.dtype('float32'), (7,))}
    assert (udf.params.border, udf.params.threshold_abs, udf.params.threshold_rel, udf.params.refine_radius) == \
        (0, 0.0, 0.0, 1)


def test_binding_signatures():
    from libertem_amd import hip
    from libertem_amd.udf import correlation, peakfind
    search = ['num_peaks', 'min_distance', 'border', 'threshold_abs', 'threshold_rel', 'refine_radius']
    outputs = ['n_found_ptr', 'centers_ptr', 'refineds_ptr', 'peak_values_ptr', 'peak_elevations_ptr', 'stream']
    assert list(inspect.signature(hip.CorrPlan.find_peaks).parameters) == [
        'self', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile'] + search + outputs
    assert list(inspect.signature(hip.find_peaks_maps).parameters) == [
        'device', 'maps_ptr', 'n_frames', 'h', 'w', 'ld_map'] + search + outputs
    for name in ('ltmi_find_peaks_maps', 'ltmi_correlate_find', 'ltmi_find_peaks_last_kernel'):
        assert name in hip.EXPORTS
    assert peakfind.plan_for is correlation.plan_for          # one plan cache
    assert not hasattr(peakfind, '_PLANS')


@pytest.mark.parametrize('case', pr.PLAN_CASES, ids=lambda c: c[0])
def test_plan_cases_are_decided(case):
    # the GPU tests demand equal n_found and centers: no seeded frame may hang on an error within the bound
    frames, tmpl, p = pr.plan_case(case)
    undecided = int((~pr.all_decided(frames, tmpl, p)).sum())
    assert undecided == 0, undecided


def test_scans_are_decided_and_the_noisy_frame_is_not():
    frames, tmpl, p, _ = pr.scan_case()
    assert int((~pr.all_decided(frames, tmpl, p)).sum()) == 0
    assert int((~pr.all_decided(pr.corrected_scan()[0], tmpl, p)).sum()) == 0
    noisy, tmpl, p = pr.undecided_frame()
    assert not pr.all_decided(noisy, tmpl, p)[0]              # (held to properties only on the GPU)


def test_pool_is_decided():
    # the many-frame tests: every member of the 8 x 8 pool keeps the same peaks under any error within the bound, some
    # members keep one peak and some two; the map pools hold distinct members, a constant one and one with a NaN
    frames, tmpl, p = pr.pool_case()
    assert int((~pr.all_decided(frames, tmpl, p)).sum()) == 0
    maps = np.stack([cr.correlation(f, tmpl) for f in frames])
    n_found = pr.reference(maps, **p)['n_found']
    assert set(n_found) == {1, 2}
    for sig, seed in pr.POOL_MAPS:
        pool = pr.pool_maps(sig, seed)
        assert pool.shape == (cr.POOL,) + sig and pool.dtype == np.float32
        assert len({m.tobytes() for m in pool}) == cr.POOL
        assert np.all(pool[7] == 1.5) and np.isnan(pool[23]).sum() == 1 and np.isfinite(np.delete(pool, 23, 0)).all()
