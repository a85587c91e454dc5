"""
ltmi_orient_polar / ltmi_orient_match (csrc/ltmi_orient.hip) on the MI355X, through `hip.OrientPlan` on guarded
regions (tests/guarded.py), against the loops of tests/orientation_ref.py.

Every case of orientation_ref's table -- frames of 1 x 1, 5 x 7, 33 x 31 and 32 x 32 in all seven dtypes, n_phi of 1,
36, 64, 65, 100 and 130 (below, at and above a wave of rotations, a partial last chunk), n_r of 1 and 12, fractional
centres and one whose taps leave the frame, libraries of one template, of five with an empty and a single-spot one, of
identical templates, of a symmetric one, with negative weights, of 70, 1100 and one more than the kernel's score block,
n_best of 1, 3 and 16 and more slots than templates, frames with NaN or infinity at a sampled tap, with NaN where no
tap reads, all zero -- with contiguous frames and with padded frames (NaN or the dtype's maximum in the padding) behind
an element-aligned base.  The polar images, templates, rotations and correlations are EQUAL to the reference,
polar_norm lies within one float32 ulp, a second run gives the same bytes, no byte around an input or an output
changes.  3000 frames check the grid stride.  Wrong arguments come back as error codes and launch nothing.
"""
import numpy as np
import pytest

import orientation_ref as oref
from guarded import Region, unchanged, unchanged_outside

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F32, I32 = np.dtype('float32'), np.dtype('int32')


def hip():
    from libertem_amd import hip as h
    return h


class Setup:
    """the frames of a case on the device and a plan for them"""

    def __init__(self, case, padded):
        self.case = case
        frames = case.frames
        n, h, w = frames.shape
        self.n, self.npx = n, h * w
        self.ld, shift = (self.npx + 5, 1) if padded else (self.npx, 0)
        self.padded = padded
        fill = 'nan' if frames.dtype.kind == 'f' else 'max'
        self.tile = Region(n, self.npx, self.ld, frames.dtype, shift=shift, init=frames.reshape((n, -1)), fill=fill)
        tap_idx, tap_w = case.table()
        self.plan = hip().OrientPlan(0, h, w, tap_idx, tap_w, case.lib, case.n_best)
        self.n_points = case.n_r * case.n_phi

    def polar(self):
        ld = self.n_points + (3 if self.padded else 0)
        out = Region(self.n, self.n_points, ld, F32, shift=1 if self.padded else 0)
        self.plan.polar(self.tile.ptr, self.case.frames.dtype, self.n, self.ld, out.ptr, ld)
        got = out.result()
        unchanged_outside(out, 'polar')
        return got.reshape((self.n, self.case.n_r, self.case.n_phi))

    def match(self):
        k = self.case.n_best
        outs = [Region(self.n, k, k, I32), Region(self.n, k, k, I32), Region(self.n, k, k, F32),
                Region(1, self.n, self.n, F32)]
        self.plan.match(self.tile.ptr, self.case.frames.dtype, self.n, self.ld, *(r.ptr for r in outs))
        got = [r.result() for r in outs]
        for r, what in zip(outs, ('template', 'rotation', 'correlation', 'polar_norm')):
            unchanged_outside(r, what)
        got[3] = got[3][0]
        return got


def check(setup, ref):
    P, template, rotation, correlation, norm = ref
    got_p = setup.polar()
    assert oref.same(got_p, P)
    assert setup.plan.last_kernel().startswith('k_orient_polar<')
    got = setup.match()
    assert oref.same(got[0], template) and oref.same(got[1], rotation)
    assert oref.same(got[2], correlation)
    assert oref.within_one_ulp(got[3], norm)
    again = setup.match()
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    unchanged(setup.tile, 'tile')
    nch = (setup.case.n_phi + 63) // 64
    assert setup.plan.last_kernel().startswith(f'k_orient_match<{setup.case.frames.dtype.name},{nch}> ')


@pytest.mark.parametrize('padded', (False, True), ids=('contiguous', 'padded'))
@pytest.mark.parametrize('name', sorted(oref.CASES))
def test_kernels_equal_the_definition(name, padded):
    check(Setup(oref.case(name), padded), oref.reference(name))


def test_limits_are_the_exported_ones():
    from libertem_amd.udf import orientation
    assert hip().orient_score_block() == oref.SCORE_BLOCK
    assert hip().orient_max_polar_words() == orientation.MAX_POLAR_WORDS
    assert len(oref.case('32x32-u8-phi36-block-edge').lib[0]) - 1 == oref.SCORE_BLOCK + 1


def test_special_frames_are_what_the_case_says():
    ref = oref.reference('32x32-f32-phi36-special')
    assert np.array_equal(np.isnan(ref[4]), [False, True, False, False, True, False])
    assert np.all(ref[1][[1, 4]] == -1) and np.all(ref[1][2] >= 0)
    assert np.array_equal(ref[1][3], [0, 1, 2]) and np.all(ref[2][3] == 0) and np.all(ref[3][3] == 0)


def test_one_frame_of_many():
    """a single frame: the one workgroup of the launch"""
    name = '32x32-i32-phi130-edge-70'
    c = oref.case(name)
    one = oref.Case(c.frames[1:2], c.center, c.n_r, c.n_phi, c.lib, c.n_best)
    check(Setup(one, padded=True), tuple(a[1:2] for a in oref.reference(name)))


def test_more_frames_than_workgroups():
    case, ref = oref.many_frames()
    assert len(case.frames) == 3000
    setup = Setup(case, padded=False)
    check(setup, ref)
    grid = int(setup.plan.last_kernel().split('grid=')[1].split()[0])
    assert grid < 3000


def test_the_largest_polar_image_launches():
    """n_r x n_phi at the exported bound: all of the 160 KiB of LDS"""
    words = hip().orient_max_polar_words()
    n_phi = 1024
    n_r = words // n_phi
    rng = np.random.default_rng(3)
    frames = oref.random_frames(rng, 2, (80, 80), 'uint16')
    from libertem_amd.udf import orientation
    tap_idx, tap_w = orientation.polar_table((80, 80), (40.2, 39.7), n_r, n_phi)
    lib = oref.random_library(rng, 20, n_r, n_phi, 4)
    case = oref.Case(frames, (40.2, 39.7), n_r, n_phi, lib, 2)
    case.table = lambda: (tap_idx, tap_w)
    _, ref_t, ref_r, ref_c, ref_n = oref.match(frames, tap_idx, tap_w, lib, 2)
    setup = Setup(case, padded=True)
    got = setup.match()
    assert oref.same(got[0], ref_t) and oref.same(got[1], ref_r) and oref.same(got[2], ref_c)
    assert oref.within_one_ulp(got[3], ref_n)
    assert f',{n_phi // 64}> ' in setup.plan.last_kernel()


def test_no_frames_launches_nothing():
    setup = Setup(oref.case('5x7-i8-phi36-empty-and-single'), padded=False)
    out = Region(1, 16, 16, I32)
    setup.plan.match(setup.tile.ptr, np.int8, 0, setup.ld, out.ptr, out.ptr, out.ptr, out.ptr)
    setup.plan.match(None, np.int8, 0, setup.ld, None, None, None, None)
    setup.plan.polar(setup.tile.ptr, np.int8, 0, setup.ld, out.ptr, setup.n_points)
    torch.cuda.synchronize()
    assert np.array_equal(out.download(), out.host)
    assert setup.plan.last_kernel() == ''


def test_error_codes():
    c = oref.case('5x7-i8-phi36-empty-and-single')
    tap_idx, tap_w = c.table()
    indptr, spot_r, spot_phi, spot_w = c.lib

    def plan(sig=(5, 7), tap_idx=tap_idx, tap_w=tap_w, lib=c.lib, n_best=3):
        return hip().OrientPlan(0, sig[0], sig[1], tap_idx, tap_w, lib, n_best)

    def changed(a, at, value):
        a = a.copy()
        a.reshape(-1)[at] = value
        return a

    with pytest.raises(ValueError, match=r'spot_r\[2\] = 12 .*code -3'):
        plan(lib=(indptr, changed(spot_r, 2, 12), spot_phi, spot_w))
    with pytest.raises(ValueError, match=r'spot_r\[0\] = -1 .*code -3'):
        plan(lib=(indptr, changed(spot_r, 0, -1), spot_phi, spot_w))
    with pytest.raises(ValueError, match=r'spot_phi\[1\] = 36 .*code -3'):
        plan(lib=(indptr, spot_r, changed(spot_phi, 1, 36), spot_w))
    with pytest.raises(ValueError, match=r'spot_w\[3\] = (nan|-nan|inf).*code -3'):
        plan(lib=(indptr, spot_r, spot_phi, changed(spot_w, 3, np.inf)))
    with pytest.raises(ValueError, match=r'tap_idx\[5\] = 35 .*code -3'):
        plan(tap_idx=changed(tap_idx, 5, 35))
    with pytest.raises(ValueError, match=r'tap_w\[4\] .*code -3'):
        plan(tap_w=changed(tap_w, 4, np.nan))
    with pytest.raises(ValueError, match=r'indptr\[2\] .*code -3'):
        plan(lib=(changed(indptr, 1, indptr[2] + 1), spot_r, spot_phi, spot_w))
    for n_best in (0, 17):
        with pytest.raises(ValueError, match=rf'n_best {n_best} .*code -3'):
            plan(n_best=n_best)
    with pytest.raises(ValueError, match=r'n_phi 1025 .*code -3'):
        plan(tap_idx=np.zeros((1, 1025, 4), np.int32), tap_w=np.zeros((1, 1025, 4), np.float32))
    words = hip().orient_max_polar_words()
    n_r = words // 1024 + 1
    with pytest.raises(ValueError, match=rf'n_r {n_r} x n_phi 1024 = {n_r * 1024} .*code -3'):
        plan(tap_idx=np.zeros((n_r, 1024, 4), np.int32), tap_w=np.zeros((n_r, 1024, 4), np.float32))
    with pytest.raises(ValueError, match=r'n_templates 0 .*code -3'):
        plan(lib=(indptr[:1], spot_r[:0], spot_phi[:0], spot_w[:0]))
    with pytest.raises(ValueError, match=r'frames of 0 x 7.*code -3'):
        plan(sig=(0, 7))

    setup = Setup(c, padded=False)
    out = Region(1, 64, 64, I32)

    def match(dtype=np.int8, n=3, ld=35, tile=setup.tile.ptr):
        setup.plan.match(tile, dtype, n, ld, out.ptr, out.ptr, out.ptr, out.ptr)

    def polar(dtype=np.int8, n=3, ld=35, tile=setup.tile.ptr, ld_polar=setup.n_points):
        setup.plan.polar(tile, dtype, n, ld, out.ptr, ld_polar)

    for call in (match, polar):
        for dtype in (np.float64, np.uint64, np.int64, np.bool_, np.complex64):
            with pytest.raises(ValueError, match=r'code -2'):
                call(dtype=dtype)
        for over in (dict(n=-1), dict(ld=34)):
            with pytest.raises(ValueError, match=r'code -3'):
                call(**over)
        with pytest.raises(ValueError, match=r'code -1'):
            call(tile=None)
    with pytest.raises(ValueError, match=r'ld_polar 431 .*code -3'):
        polar(ld_polar=setup.n_points - 1)
    torch.cuda.synchronize()
    assert np.array_equal(out.download(), out.host)          # none of them launched
    assert setup.plan.last_kernel() == ''
