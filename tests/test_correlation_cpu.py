"""
CorrelationUDF without a GPU: the NumPy branch on the inline executor against the float64 restatement of the
definition (tests/correlation_ref.py) -- exact centres on integer-shifted disks, sub-pixel refinement on blurred ones,
regions of interest, sync offsets, partitions, stored dtypes, windows clipped at every border --, the argument errors,
the signature of hip.CorrPlan, and that the seeded inputs of the kernel tests hold no near-tie.
"""
import inspect

import numpy as np
import pytest

import correlation_ref as cr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import CorrelationUDF, run_correlation

SIG = (48, 48)
PEAKS = np.array([(14, 14), (14, 34), (34, 24)], dtype=np.int32)       # 20 px apart: no disk in another's window
R = 4
NAMES = ('centers', 'refineds', 'peak_values', 'peak_elevations')


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def scan():
    """(4, 5) positions of 48 x 48 float32, the last 5 frames blurred; its reference, computed once"""
    frames, shifts, frac = cr.make_frames(SIG, PEAKS, R, 20, seed=11, n_blurred=5)
    template = cr.disk_template(SIG)
    return frames, shifts, frac, template, cr.reference(frames, template, PEAKS, R)


def check(res, ref):
    """the run's buffers against the reference (flat nav order)"""
    for name in NAMES:
        exp = ref[name]
        got = np.asarray(res[name].data).reshape(exp.shape)
        if name == 'centers':
            assert got.dtype == np.int32 and np.array_equal(got, exp)
        else:
            assert got.dtype == np.float32
            assert np.allclose(got, exp, rtol=1e-5, atol=1e-6), (name, np.abs(got - exp).max())


def test_numpy_branch_equals_definition(ctx, scan):
    frames, shifts, frac, template, ref = scan
    ds = ctx.load('memory', data=frames.reshape((4, 5) + SIG), num_partitions=2, sig_dims=2)
    res = run_correlation(ctx, ds, PEAKS, template, R)
    assert res['centers'].data.shape == (4, 5, 3, 2) and res['peak_values'].data.shape == (4, 5, 3)
    check(res, ref)
    sharp = np.all(frac == 0, axis=1)
    assert sharp.sum() == 15
    centers = res['centers'].data.reshape((20, 3, 2))
    assert np.array_equal(centers[sharp], (PEAKS[None] + shifts)[sharp])
    true = PEAKS[None] + shifts + frac[:, None, :]
    refined = res['refineds'].data.reshape((20, 3, 2))
    assert np.abs(refined - true).max() < 0.5
    assert np.abs(refined - true)[~sharp].max() > 0           # (the blurred frames are there)
    # a disk that equals the template rises well above its window
    assert res['peak_elevations'].data.min() > 2


def test_roi(ctx, scan):
    frames, _, _, template, ref = scan
    ds = ctx.load('memory', data=frames.reshape((4, 5) + SIG), num_partitions=2, sig_dims=2)
    roi = np.zeros((4, 5), bool)
    roi[0, 1] = roi[2, 3] = roi[3, 4] = roi[1, 0] = True
    res = run_correlation(ctx, ds, PEAKS, template, R, roi=roi)
    rows = np.flatnonzero(roi.reshape(-1))
    for name in NAMES:
        got = np.asarray(res[name].raw_data)
        assert np.allclose(got, ref[name][rows], rtol=1e-5, atol=1e-6), name


@pytest.mark.parametrize('sync_offset', [3, -3])
def test_sync_offset(ctx, scan, sync_offset):
    frames, _, _, template, ref = scan
    ds = ctx.load('memory', data=frames.reshape((4, 5) + SIG), num_partitions=2, sig_dims=2,
                  sync_offset=sync_offset)
    res = run_correlation(ctx, ds, PEAKS, template, R)
    pos = np.arange(20)
    src = pos + sync_offset                              # position i holds frame i + sync_offset
    valid = (src >= 0) & (src < 20)
    for name in NAMES:
        got = np.asarray(res[name].data).reshape((20,) + ref[name].shape[1:])
        assert np.allclose(got[valid], ref[name][src[valid]], rtol=1e-5, atol=1e-6), name
        assert np.all(got[~valid] == 0)                  # no frame, no result


def test_three_partitions_and_refine_radius(ctx, scan):
    frames, _, _, template, _ = scan
    ds = ctx.load('memory', data=frames.reshape((4, 5) + SIG), num_partitions=3, sig_dims=2)
    res = run_correlation(ctx, ds, PEAKS, template, R, refine_radius=2)
    check(res, cr.reference(frames, template, PEAKS, R, 2))


@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
def test_stored_dtypes_and_clipped_windows(ctx, dtype):
    sig = (36, 51)
    peaks = cr.border_peaks(sig)                         # clipped at each of the four borders and at a corner
    frames, _, _ = cr.make_frames(sig, peaks, 6, 6, seed=5, dtype=dtype, n_blurred=2)
    template = cr.disk_template(sig)
    ds = ctx.load('memory', data=frames.reshape((2, 3) + sig), num_partitions=2, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=CorrelationUDF(peaks, template, 6))
    ref = cr.reference(frames, template, peaks, 6)
    check(res, ref)
    c = res['centers'].data.reshape((-1, len(peaks), 2))
    assert np.all(c >= 0) and np.all(c[..., 0] < sig[0]) and np.all(c[..., 1] < sig[1])
    assert np.all(c[:, 4] <= 6)                          # the corner's window is [0, 6] x [0, 6]


def test_nonfinite_frame(ctx, scan):
    frames, _, _, template, ref = scan
    frames = frames.copy()
    frames[7, 3, 3] = np.nan
    ds = ctx.load('memory', data=frames.reshape((4, 5) + SIG), num_partitions=2, sig_dims=2)
    res = run_correlation(ctx, ds, PEAKS, template, R)
    v = res['peak_values'].data.reshape((20, 3))
    assert np.all(np.isnan(v[7]))
    ok = np.arange(20) != 7
    assert np.allclose(v[ok], ref['peak_values'][ok], rtol=1e-5)


def test_value_errors(ctx, scan):
    frames, _, _, template, _ = scan
    ds = ctx.load('memory', data=frames.reshape((4, 5) + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='outside'):
        run_correlation(ctx, ds, np.array([(14, 14), (48, 3)]), template, R)
    with pytest.raises(ValueError, match='outside'):
        run_correlation(ctx, ds, np.array([(-1, 3)]), template, R)
    with pytest.raises(ValueError, match='template'):
        run_correlation(ctx, ds, PEAKS, template[:, :40], R)
    with pytest.raises(ValueError, match='crop_radius'):
        run_correlation(ctx, ds, PEAKS, template, 0)
    with pytest.raises(ValueError, match='refine_radius'):
        run_correlation(ctx, ds, PEAKS, template, R, refine_radius=0)
    with pytest.raises(ValueError, match='peaks'):
        run_correlation(ctx, ds, PEAKS.astype(np.float32), template, R)
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D'):
        run_correlation(ctx, ds3, np.array([(1, 1)]), np.zeros((4, 8, 8), np.float32), 1)


def test_udf_declarations():
    udf = CorrelationUDF(PEAKS, cr.disk_template(SIG), R)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {k: 'disjoint' for k in NAMES}
    bufs = udf.get_result_buffers()
    assert {k: (b.kind, np.dtype(b.dtype), b.extra_shape) for k, b in bufs.items()} == {
        'centers': ('nav', np.dtype('int32'), (3, 2)), 'refineds': ('nav', np.dtype('float32'), (3, 2)),
        'peak_values': ('nav', np.dtype('float32'), (3,)), 'peak_elevations': ('nav', np.dtype('float32'), (3,))}
    assert udf.params.refine_radius == 1


def test_corr_plan_signature():
    from libertem_amd import hip
    assert list(inspect.signature(hip.CorrPlan.__init__).parameters) == [
        'self', 'device', 'sig_h', 'sig_w', 'max_batch', 'template']
    assert list(inspect.signature(hip.CorrPlan.correlate_peaks).parameters) == [
        'self', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'peaks_ptr', 'n_peaks', 'crop_radius',
        'refine_radius', 'centers_ptr', 'refineds_ptr', 'peak_values_ptr', 'peak_elevations_ptr', 'stream']
    for name in ('ltmi_corr_plan_create', 'ltmi_corr_plan_destroy', 'ltmi_correlate_peaks',
                 'ltmi_corr_plan_last_kernel'):
        assert name in hip.EXPORTS
    assert callable(hip.CorrPlan.last_kernel) and callable(hip.CorrPlan.close)


@pytest.mark.parametrize('case', cr.KERNEL_CASES, ids=lambda c: c[0])
def test_kernel_inputs_hold_no_near_tie(case):
    # the kernel tests skip (frame, peak) pairs whose top-two gap is below twice the error bound: none is, here
    frames, template, peaks, r, q = cr.kernel_case(case)
    ref = cr.reference(frames, template, peaks, r, q)
    bound = cr.value_bound(frames, template)[:, None]
    assert np.all(ref['gap'] > 2 * bound), float((ref['gap'] / (2 * bound)).min())


def test_pool_is_decided_by_the_reference_alone():
    # the many-frame kernel tests leave out no (frame, peak) pair: every window of every pool member has a top-two
    # gap above twice the bound, and the members differ, so that a frame taken from another slot shows
    pool, template = cr.pool_frames(), cr.pool_template()
    assert pool.shape == (cr.POOL,) + cr.POOL_SIG and pool.dtype == np.uint8
    assert len({m.tobytes() for m in pool}) == cr.POOL
    ref = cr.reference(pool, template, cr.POOL_PEAKS, cr.POOL_R, cr.POOL_Q)
    bound = cr.value_bound(pool, template)[:, None]
    assert np.all(ref['gap'] > 2 * bound), float((ref['gap'] / (2 * bound)).min())
    values = ref['peak_values']
    assert len({v.tobytes() for v in values}) == cr.POOL      # (no two members give the same results)


@pytest.mark.parametrize('n,extra', [(70000, ()), (524300, (524279, 524280, 524281)), (16400, (16383, 16384))])
def test_pool_index_marks_the_frames_at_the_limits(n, extra):
    idx = cr.pool_index(n, extra)
    assert idx.shape == (n,) and idx.min() == 0 and idx.max() == cr.POOL - 1
    assert np.array_equal(idx, cr.pool_index(n, extra))
    for f in {0, cr.GRID_ROWS - 1, cr.GRID_ROWS, cr.GRID_ROWS + 1, n - 1, *extra}:
        if f < n:
            assert all(idx[f] != idx[g] for g in (f - 1, f + 1) if 0 <= g < n), f
    assert np.all(np.bincount(idx, minlength=cr.POOL) > 0)
