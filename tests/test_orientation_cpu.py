"""
libertem_amd.udf.orientation without a GPU: `polar_table`, `polar_library`, `polar_frames` and `match_polar` are EQUAL
to the loops of tests/orientation_ref.py on its case table (polar_norm within one float32 ulp); the properties of the
sampling table and of the library builder; the recovery of known templates at known rotations, first by the loops --
which checks the definition itself -- then by `match_polar`; OrientationMatchUDF on the inline executor with several
partitions, a region of interest, sync offsets and more slots than templates; every parameter error.
"""
import inspect

import numpy as np
import pytest

import orientation_ref as oref
from libertem_amd.udf import orientation
from libertem_amd.udf.orientation import (
    OrientationMatchUDF, match_polar, polar_frames, polar_library, polar_table, rotation_angles, run_orientation_match,
)

NAMES = orientation.NAMES


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    return Context(InlineJobExecutor())


def flat(res, n_best, raw=False):
    out = {}
    for name in NAMES:
        a = np.asarray(res[name].raw_data if raw else res[name].data)
        out[name] = a.reshape((-1,) + (() if name == 'polar_norm' else (n_best,)))
    return out


def numpy_match(case):
    tap_idx, tap_w = polar_table(case.sig, case.center, case.n_r, case.n_phi, case.r_min, case.delta_r)
    P = polar_frames(case.frames, tap_idx, tap_w)
    return (P,) + match_polar(P, case.lib, case.n_best)


@pytest.mark.parametrize('name', sorted(oref.CASES))
def test_numpy_equals_the_loops(name):
    case = oref.case(name)
    ref_idx, ref_w = case.table()
    tap_idx, tap_w = polar_table(case.sig, case.center, case.n_r, case.n_phi, case.r_min, case.delta_r)
    assert oref.same(tap_idx, ref_idx) and oref.same(tap_w, ref_w)
    got, ref = numpy_match(case), oref.reference(name)
    for g, r, what in zip(got[:4], ref[:4], ('P',) + NAMES[:3]):
        assert oref.same(g, r), what
    assert got[4].dtype == np.float32 and oref.within_one_ulp(got[4], ref[4])


def test_many_frames_equal_the_loops():
    case, ref = oref.many_frames()
    got = numpy_match(case)
    for g, r in zip(got[:4], ref[:4]):
        assert oref.same(g, r)
    assert oref.within_one_ulp(got[4], ref[4])


def test_cases_hold_what_they_are_for():
    # the identical templates tie, and template 0 wins; the symmetric template ties between two rotations
    ref = oref.reference('33x31-u16-phi64-identical')
    assert np.all(ref[1][:, 0] != 2)
    case = oref.case('33x31-u16-phi64-identical')
    c, rot = oref.scores(ref[0][0], case.lib)
    assert c[0] == c[2] and rot[0] == rot[2]
    case = oref.case('32x32-u32-phi100-symmetric')
    ref = oref.reference('32x32-u32-phi100-symmetric')
    assert case.lib[0][1] == 2 and case.lib[1][:2].tolist() == [5, 5] and case.lib[2][:2].tolist() == [10, 60]
    w = case.lib[3][:2]
    twice = np.concatenate([ref[0][0], ref[0][0]], axis=1)
    acc = w[0] * twice[5, 10:110] + w[1] * twice[5, 60:160]
    assert acc.max() > 0 and np.flatnonzero(acc == acc.max()).tolist() == [6, 56]
    assert ref[1][0, 0] == 0 and ref[2][0, 0] == 6           # the lower of the two rotations
    # special frames: NaN or infinity at a sampled tap is flagged, NaN at pixel 0 -- named by every tap outside the
    # frame, read by none -- is not, and the all-zero frame ties everywhere
    case = oref.case('32x32-f32-phi36-special')
    ref = oref.reference('32x32-f32-phi36-special')
    tap_idx, tap_w = case.table()
    assert np.any((tap_idx == 0) & (tap_w == 0)) and not np.any((tap_idx == 0) & (tap_w != 0))
    assert np.array_equal(np.isnan(ref[4]), [False, True, False, False, True, False])
    assert np.all(ref[1][[1, 4]] == -1) and np.all(ref[2][[1, 4]] == -1) and np.all(np.isnan(ref[3][[1, 4]]))
    assert np.all(ref[1][2] >= 0) and np.all(np.isfinite(ref[3][2]))
    assert np.array_equal(ref[1][3], [0, 1, 2]) and np.all(ref[2][3] == 0) and np.all(ref[3][3] == 0)
    # more slots than templates
    ref = oref.reference('32x32-i16-phi65-negative-best16')
    assert np.all(ref[1][:, :5] >= 0) and np.all(ref[1][:, 5:] == -1) and np.all(ref[2][:, 5:] == -1)
    assert np.all(np.isnan(ref[3][:, 5:]))
    # the block edge: the copy behind the block ties with template 3 and comes second
    ref = oref.reference('32x32-u8-phi36-block-edge')
    assert ref[1][0, :2].tolist() == [3, oref.SCORE_BLOCK] and ref[3][0, 0] == ref[3][0, 1]


# ---- the sampling table -------------------------------------------------------------------------------------------
def test_table_weights():
    tap_idx, tap_w = polar_table((40, 48), (19.3, 24.6), 25, 90)
    assert tap_idx.dtype == np.int32 and tap_w.dtype == np.float32 and tap_idx.shape == tap_w.shape == (25, 90, 4)
    r = 1.0 + np.arange(25)[:, None]
    phi = 2 * np.pi * np.arange(90)[None, :] / 90
    y, x = 19.3 + r * np.sin(phi), 24.6 + r * np.cos(phi)
    inside = (np.floor(y) >= 0) & (np.floor(y) + 1 < 40) & (np.floor(x) >= 0) & (np.floor(x) + 1 < 48)
    assert inside.any() and not inside.all()
    total = tap_w.astype(np.float64).sum(axis=2)
    assert np.all(np.abs(total[inside] - 1) <= 2 * np.spacing(np.float32(1)))
    assert np.all(tap_w >= 0) and np.all(total <= 1 + 2 * np.spacing(np.float32(1)))
    # a tap outside the frame: index 0, weight 0; inside: the pixel it names
    ty = np.stack([np.floor(y), np.floor(y), np.floor(y) + 1, np.floor(y) + 1], axis=-1)
    tx = np.stack([np.floor(x), np.floor(x) + 1, np.floor(x), np.floor(x) + 1], axis=-1)
    out = (ty < 0) | (ty >= 40) | (tx < 0) | (tx >= 48)
    assert np.all(tap_idx[out] == 0) and np.all(tap_w[out] == 0)
    assert np.array_equal(tap_idx[~out], (ty * 48 + tx)[~out].astype(np.int32))
    # the image of a linear ramp is the ramp at the sampling point, where all four taps lie inside
    yy, xx = np.mgrid[:40, :48]
    ramp = (3 * yy + 2 * xx).astype(np.float32)
    P = polar_frames(ramp[None], tap_idx, tap_w)[0]
    assert np.allclose(P[inside], (3 * y + 2 * x)[inside], rtol=1e-5)


def test_centre_outside_the_frame():
    tap_idx, tap_w = polar_table((8, 8), (-40.0, 100.0), 6, 12)
    assert np.all(tap_w == 0) and np.all(tap_idx == 0)
    frames = np.random.default_rng(0).integers(1, 200, (2, 8, 8)).astype(np.uint8)
    P = polar_frames(frames, tap_idx, tap_w)
    assert P.dtype == np.float32 and np.all(P == 0)
    lib = oref.random_library(np.random.default_rng(1), 4, 6, 12, 3)
    t, r, c, n = match_polar(P, lib, 3)
    assert np.array_equal(t, [[0, 1, 2]] * 2) and np.all(r == 0) and np.all(c == 0) and np.all(n == 0)


# ---- the library --------------------------------------------------------------------------------------------------
def test_library_properties():
    n_r, n_phi = 10, 36
    ang = 2 * np.pi / 36
    spots = [
        # (1) two spots of one bin are added, (2) a spot beyond the last radius and one inside r_min go
        (np.array([0.0, 0.02, 5 * np.sin(7 * ang), 40.0, 0.1]), np.array([3.0, 3.05, 5 * np.cos(7 * ang), 0.0, 0.0]),
         np.array([1.0, 2.0, 4.0, 9.0, 9.0])),
        (np.array([50.0]), np.array([50.0]), np.array([1.0])),                 # every spot out of range: empty
        (np.array([-2.0, 2.0, 0.0]), np.array([0.0, 0.0, -6.0]), np.array([0.5, 0.25, 1.0])),
    ]
    indptr, spot_r, spot_phi, spot_w = polar_library(spots, n_r, n_phi)
    assert (indptr.dtype, spot_r.dtype, spot_phi.dtype, spot_w.dtype) == (np.int64, np.int32, np.int32, np.float32)
    assert indptr.tolist() == [0, 2, 2, 5]
    assert spot_r[:2].tolist() == [2, 4] and spot_phi[:2].tolist() == [0, 7]
    assert np.array_equal(spot_w[:2], (np.array([3.0, 4.0]) / 5.0).astype(np.float32))
    # -90 degrees is bin 27, 90 degrees bin 9, 180 degrees bin 18: sorted by (r, phi)
    assert spot_r[2:].tolist() == [1, 1, 5] and spot_phi[2:].tolist() == [9, 27, 18]
    for t in (0, 2):
        w = spot_w[indptr[t]:indptr[t + 1]].astype(np.float64)
        assert abs(np.sqrt((w * w).sum()) - 1) <= len(w) * np.spacing(np.float32(1))
    key = spot_r.astype(np.int64) * n_phi + spot_phi
    for t in range(3):
        assert np.all(np.diff(key[indptr[t]:indptr[t + 1]]) > 0)
    ref = oref.library(spots, n_r, n_phi)
    for a, b in zip((indptr, spot_r, spot_phi, spot_w), ref):
        assert oref.same(a, b)
    # r_min and delta_r
    lib = polar_library([(np.array([0.0]), np.array([7.0]), np.array([2.0]))], 5, 8, r_min=3.0, delta_r=2.0)
    assert lib[1].tolist() == [2] and lib[2].tolist() == [0] and lib[3].tolist() == [1.0]
    assert oref.same(lib[3], oref.library([(np.array([0.0]), np.array([7.0]), np.array([2.0]))], 5, 8, 3.0, 2.0)[3])


def test_rotation_angles():
    got = rotation_angles(np.array([[0, 18, -1]]), 72)
    assert got.shape == (1, 3) and got[0, 0] == 0 and got[0, 1] == np.pi / 2 and np.isnan(got[0, 2])


# ---- recovery -------------------------------------------------------------------------------------------------------
def test_recovery_of_known_templates_and_rotations():
    spot_lists, frames, truth = oref.recovery()
    assert frames.shape == (90, 64, 64) and frames.dtype == np.uint16 and len(truth) == 90
    # first the definition itself, as loops
    _, t_ref, r_ref, c_ref, _ = oref.recovery_reference()
    assert np.array_equal(t_ref[:, 0], truth[:, 0]) and np.array_equal(r_ref[:, 0], truth[:, 1])
    assert np.all(c_ref[:, 1] < c_ref[:, 0])
    # then the package
    lib = polar_library(spot_lists, oref.REC_N_R, oref.REC_N_PHI)
    tap_idx, tap_w = polar_table(oref.REC_SIG, oref.REC_CENTER, oref.REC_N_R, oref.REC_N_PHI)
    t, r, c, n = match_polar(polar_frames(frames, tap_idx, tap_w), lib, 2)
    assert np.array_equal(t[:, 0], truth[:, 0]) and np.array_equal(r[:, 0], truth[:, 1])
    assert oref.same(t, t_ref) and oref.same(r, r_ref) and oref.same(c, c_ref)
    assert np.allclose(rotation_angles(r[:, 0], oref.REC_N_PHI), 2 * np.pi * truth[:, 1] / oref.REC_N_PHI)


def test_spot_pattern_frames():
    from libertem_amd.utils.generate import spot_pattern_frames
    spots = [(np.array([10.0]), np.array([0.0]), np.array([1.0]))]
    a = spot_pattern_frames(spots, [(0, 0.0), (0, np.pi / 2)], (48, 48), (24.0, 24.0), seed=3)
    assert a.dtype == np.uint16 and a.shape == (2, 48, 48)
    assert np.array_equal(a, spot_pattern_frames(spots, [(0, 0.0), (0, np.pi / 2)], (48, 48), (24.0, 24.0), seed=3))
    # the spot at (qy, qx) = (10, 0) lies below the centre; a quarter turn takes it to qx = -10
    assert a[0, 34, 24] > 500 and a[1, 24, 14] > 500 and a[0, 24, 14] < 50 and a[1, 34, 24] < 50
    assert a[0, 24, 24] > 100                                # the beam
    with pytest.raises(ValueError, match='sigma 0'):
        spot_pattern_frames(spots, [(0, 0.0)], (8, 8), (4, 4), sigma=0)


# ---- the UDF on the inline executor ---------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scan():
    spot_lists, frames, truth = oref.recovery()
    lib = polar_library(spot_lists, oref.REC_N_R, oref.REC_N_PHI)
    tap_idx, tap_w = polar_table(oref.REC_SIG, oref.REC_CENTER, oref.REC_N_R, oref.REC_N_PHI)
    return frames, lib, truth, tap_idx, tap_w


def params(lib, n_best=2):
    return dict(library=lib, center=oref.REC_CENTER, n_r=oref.REC_N_R, n_phi=oref.REC_N_PHI, n_best=n_best)


def direct(scan, n_best, rows):
    frames, lib, _, tap_idx, tap_w = scan
    return dict(zip(NAMES, match_polar(polar_frames(frames[rows], tap_idx, tap_w), lib, n_best)))


def test_udf_several_partitions(ctx, scan):
    frames, lib, truth, _, _ = scan
    ds = ctx.load('memory', data=frames.reshape(oref.REC_NAV + oref.REC_SIG), num_partitions=4, sig_dims=2)
    res = run_orientation_match(ctx, ds, **params(lib))
    assert res['template'].data.shape == oref.REC_NAV + (2,) and res['template'].data.dtype == np.int32
    assert res['correlation'].data.dtype == np.float32 and res['polar_norm'].data.shape == oref.REC_NAV
    got, ref = flat(res, 2), direct(scan, 2, np.arange(90))
    for name in NAMES:
        assert oref.same(got[name], ref[name]), name
    assert np.array_equal(got['template'][:, 0], truth[:, 0]) and np.array_equal(got['rotation'][:, 0], truth[:, 1])


def test_udf_roi(ctx, scan):
    frames, lib, _, _, _ = scan
    ds = ctx.load('memory', data=frames.reshape(oref.REC_NAV + oref.REC_SIG), num_partitions=3, sig_dims=2)
    roi = np.zeros(oref.REC_NAV, bool)
    roi[0, 1] = roi[2, 3] = roi[8, 9] = roi[4, 0] = roi[4, 1] = True
    got = flat(run_orientation_match(ctx, ds, roi=roi, **params(lib)), 2, raw=True)
    ref = direct(scan, 2, np.flatnonzero(roi.reshape(-1)))
    for name in NAMES:
        assert oref.same(got[name], ref[name]), name


@pytest.mark.parametrize('sync_offset', [7, -7])
def test_udf_sync_offset(ctx, scan, sync_offset):
    frames, lib, _, _, _ = scan
    ds = ctx.load('memory', data=frames.reshape(oref.REC_NAV + oref.REC_SIG), num_partitions=3, sig_dims=2,
                  sync_offset=sync_offset)
    got = flat(run_orientation_match(ctx, ds, **params(lib)), 2)
    src = np.arange(90) + sync_offset                        # position i holds frame i + sync_offset
    valid = (src >= 0) & (src < 90)
    ref = direct(scan, 2, src[valid])
    for name in NAMES:
        assert oref.same(got[name][valid], ref[name]), name
        assert np.all(got[name][~valid] == 0), name          # no frame, no result


def test_udf_more_slots_than_templates(ctx, scan):
    frames, lib, _, _, _ = scan
    ds = ctx.load('memory', data=frames[:12].reshape((3, 4) + oref.REC_SIG), num_partitions=2, sig_dims=2)
    got = flat(run_orientation_match(ctx, ds, **params(lib, n_best=9)), 9)
    ref = direct(scan, 9, np.arange(12))
    for name in NAMES:
        assert oref.same(got[name], ref[name]), name
    assert np.all(got['template'][:, 6:] == -1) and np.all(got['rotation'][:, 6:] == -1)
    assert np.all(np.isnan(got['correlation'][:, 6:]))
    assert np.all(np.sort(got['template'][:, :6], axis=1) == np.arange(6))


def test_udf_declarations(scan):
    udf = OrientationMatchUDF(scan[1], (3.0, 4.0), 5, 36, n_best=4)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {k: 'disjoint' for k in NAMES}
    bufs = udf.get_result_buffers()
    assert {k: (b.kind, np.dtype(b.dtype), b.extra_shape) for k, b in bufs.items()} == {
        'template': ('nav', np.dtype('int32'), (4,)), 'rotation': ('nav', np.dtype('int32'), (4,)),
        'correlation': ('nav', np.dtype('float32'), (4,)), 'polar_norm': ('nav', np.dtype('float32'), ())}
    assert (udf.params.r_min, udf.params.delta_r) == (1.0, 1.0)
    assert OrientationMatchUDF(scan[1], (3.0, 4.0), 5, 36).params.n_best == 1


def test_binding_signatures():
    from libertem_amd import hip
    assert list(inspect.signature(hip.OrientPlan.__init__).parameters) == [
        'self', 'device', 'sig_h', 'sig_w', 'tap_idx', 'tap_w', 'library', 'n_best']
    assert list(inspect.signature(hip.OrientPlan.match).parameters) == [
        'self', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'template_ptr', 'rotation_ptr', 'correlation_ptr',
        'norm_ptr', 'stream']
    assert list(inspect.signature(hip.OrientPlan.polar).parameters) == [
        'self', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'polar_ptr', 'ld_polar', 'stream']
    for name in ('ltmi_orient_plan_create', 'ltmi_orient_plan_destroy', 'ltmi_orient_match', 'ltmi_orient_polar',
                 'ltmi_orient_plan_last_kernel', 'ltmi_orient_max_polar_words', 'ltmi_orient_score_block'):
        assert name in hip.EXPORTS
    from libertem_amd.build import header_exports
    assert set(n for n in hip.EXPORTS if n.startswith('ltmi_orient')) == \
        set(n for n in header_exports() if n.startswith('ltmi_orient'))


def test_value_errors(ctx, scan):
    frames, lib, _, _, _ = scan
    ds = ctx.load('memory', data=frames[:4].reshape((2, 2) + oref.REC_SIG), num_partitions=2, sig_dims=2)
    indptr, spot_r, spot_phi, spot_w = lib
    words = orientation.MAX_POLAR_WORDS
    too_many = words // 1024 + 1
    for kw, match in ((dict(n_best=0), 'n_best 0'), (dict(n_best=17), 'n_best 17'), (dict(n_phi=0), 'n_phi 0'),
                      (dict(n_phi=1025), 'n_phi 1025'), (dict(n_r=0), 'n_r 0'),
                      (dict(n_r=too_many, n_phi=1024), f'n_r {too_many} x n_phi 1024 = {too_many * 1024}'),
                      (dict(library=(indptr[:1], spot_r[:0], spot_phi[:0], spot_w[:0])), '0 templates'),
                      (dict(n_r=20), 'spot_r 2[0-9] lies outside'), (dict(n_phi=60), 'spot_phi [67][0-9] lies outside'),
                      (dict(library=(indptr, spot_r, spot_phi, np.where(np.arange(len(spot_w)) == 5, np.nan, spot_w))),
                       'spot_w nan'),
                      (dict(library=(indptr, spot_r[:-1], spot_phi, spot_w)), 'indptr ends at 48'),
                      (dict(library=(indptr[::-1], spot_r, spot_phi, spot_w)), 'indptr must start at 0'),
                      (dict(library=lib[:3]), 'quadruple')):
        with pytest.raises(ValueError, match=match):
            run_orientation_match(ctx, ds, **dict(params(lib), **kw))
    for kw, match in ((dict(n_best=0), 'n_best 0'), (dict(n_best=17), 'n_best 17')):
        with pytest.raises(ValueError, match=match):
            match_polar(np.zeros((1, oref.REC_N_R, oref.REC_N_PHI), np.float32), lib, **kw)
    with pytest.raises(ValueError, match='n_phi 1025'):
        polar_table((8, 8), (4, 4), 2, 1025)
    with pytest.raises(ValueError, match='n_r 0'):
        polar_library([], 0, 8)
    with pytest.raises(ValueError, match='0 templates'):
        polar_library([], 4, 8)
    with pytest.raises(ValueError, match='2D'):
        polar_table((4, 8, 8), (4, 4), 2, 8)
    with pytest.raises(ValueError, match='float32'):
        match_polar(np.zeros((1, 28, 72)), lib)
    with pytest.raises(ValueError, match=r'\(n, h, w\)'):
        polar_frames(np.zeros((8, 8)), *scan[3:5])
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D'):
        run_orientation_match(ctx, ds3, **params(lib))
