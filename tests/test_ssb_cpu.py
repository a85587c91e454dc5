"""
Single-sideband ptychography without a GPU: `SSBUDF` on the inline executor and `reconstruct_bf` against the
index-by-index float64 restatement (tests/ssb_ref.py) on the generic fixture -- a 12 x 10 scan of 24 x 28 uint16
Poisson(40) frames, a geometry rotated by 25 degrees with unequal scan steps, cutoff 4: P = 167, 112 of the 120
spatial frequencies non-zero, every pixel at least 2.9e-3 (in distance squared) from every rim -- at the tolerance of
the holography tests (Q != 0: rtol 1e-5, atol 1e-5 max|ref|; DC: rtol 1e-6); the physics on a simulated weak phase
object (`weak_phase_scan`: correlation of the mean-free phase with the truth above 0.999, scale within 2 %);
`trotter_masks` against the restatement's masks; the parameter errors; `wavelength`; the declarations.
"""
import inspect

import numpy as np
import pytest

import ssb_ref as sr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import SSBUDF
from libertem_amd.udf.ssb import bf_pixels, check_params, reconstruct_bf, trotter_masks, wavelength
from libertem_amd.utils.generate import weak_phase_scan

IMAGES = ('complex', 'phase', 'amplitude')


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def generic():
    """the frames (12, 10, 24, 28) and the restatement's results"""
    frames = sr.generic_frames()
    return frames, sr.reference(frames, **sr.GENERIC)


@pytest.fixture(scope='module')
def physical():
    """the phase, the simulated scan (16, 16, 32, 32) and the restatement's results"""
    phi = sr.physical_phase()
    frames = weak_phase_scan(phi, sr.PHYS_STEP, sr.PHYS_SEMICONV_PIX, counts=1e4)
    return phi, frames, sr.reference(frames, **sr.physical_params())


def test_generic_fixture_is_what_the_tests_need(generic):
    frames, ref = generic
    p = sr.full_params(sr.GENERIC_SIG, **sr.GENERIC)
    assert frames.shape == sr.GENERIC_NAV + sr.GENERIC_SIG and frames.dtype == np.uint16
    assert sr.disk(sr.GENERIC_SIG, p).sum() == 167
    # no pixel sits on a rim: the masks do not depend on the last bits of the predicate arithmetic
    margin = sr.rim_margin(sr.GENERIC_SIG, sr.GENERIC_NAV, p)
    assert margin >= 1e-6
    assert 2.8e-3 < margin < 3.0e-3
    # both branches of the cutoff rule occur
    enough = (ref['n_pos'] >= 4) & (ref['n_neg'] >= 4)
    enough[0, 0] = True
    assert enough.sum() == 113 and (~enough).sum() == 7
    assert np.all((ref['fourier'] != 0) == enough)
    # ... and not only for empty trotters: some hold pixels, but fewer than the cutoff
    assert np.any(~enough & ((ref['n_pos'] > 0) | (ref['n_neg'] > 0)))
    # fourier is not antisymmetric at the Nyquist indices of the even axes: Q and -Q are the same index there
    assert ref['fourier'][6, 0] != 0 and ref['fourier'][0, 5] != 0


@pytest.mark.parametrize('num_partitions', [1, 3])
def test_udf_equals_restatement(ctx, generic, num_partitions):
    frames, ref = generic
    ds = ctx.load('memory', data=frames, num_partitions=num_partitions, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=SSBUDF(**sr.GENERIC))
    assert res['fourier'].data.shape == sr.GENERIC_NAV and res['fourier'].data.dtype == np.complex64
    assert res['complex'].data.dtype == np.complex64
    assert res['phase'].data.dtype == np.float32 and res['amplitude'].data.dtype == np.float32
    sr.assert_fourier(res['fourier'].data, ref['fourier'], 'SSBUDF inline')
    sr.assert_images({k: res[k].data for k in IMAGES}, ref, 'SSBUDF inline')
    idx = bf_pixels(sr.GENERIC_SIG, 7.3, 11.6, 14.2)
    assert res['bf'].data.shape == sr.GENERIC_NAV + (167,) and res['bf'].data.dtype == np.float32
    assert np.array_equal(res['bf'].data.reshape(120, 167), frames.reshape(120, -1)[:, idx].astype(np.float32))


@pytest.mark.parametrize('dtype', ['uint16', 'float32', 'float64'])
def test_reconstruct_bf_equals_restatement(generic, dtype):
    frames, ref = generic
    idx = bf_pixels(sr.GENERIC_SIG, 7.3, 11.6, 14.2)
    assert idx.dtype == np.int32 and idx.shape == (167,)
    bf = frames.reshape(120, -1)[:, idx].astype(dtype)
    out = reconstruct_bf(bf, sr.GENERIC_NAV, sr.GENERIC_SIG, **sr.GENERIC)
    sr.assert_fourier(out['fourier'], ref['fourier'], f'reconstruct_bf {dtype}')
    sr.assert_images(out, ref, f'reconstruct_bf {dtype}')
    with pytest.raises(ValueError, match='bf of shape'):
        reconstruct_bf(bf[:, :-1], sr.GENERIC_NAV, sr.GENERIC_SIG, **sr.GENERIC)


def test_defaults_scalar_step_identity_centre():
    # dpix as one number, no transformation, the centre (h / 2, w / 2), cutoff 1; an odd scan and an odd frame
    rng = np.random.default_rng(5)
    frames = rng.poisson(30., (9, 7, 17, 20)).astype(np.float32)
    params = dict(lamb=2.5e-12, dpix=0.3e-10, semiconv=0.02, semiconv_pix=5.1)
    ref = sr.reference(frames, **params)
    assert sr.rim_margin((17, 20), (9, 7), sr.full_params((17, 20), **params)) >= 1e-6
    idx = bf_pixels((17, 20), 5.1, 8.5, 10.0)
    out = reconstruct_bf(frames.reshape(63, -1)[:, idx], (9, 7), (17, 20), **params)
    sr.assert_fourier(out['fourier'], ref['fourier'], 'defaults')


def test_physics(ctx, physical):
    phi, frames, ref = physical
    # the restatement alone
    corr, scale = sr.phase_agreement(ref['phase'], phi)
    assert corr > 0.99999 and abs(scale - 1) < 0.02
    # the package, on whole counts
    counts = np.rint(frames * 100).astype(np.uint32)
    ds = ctx.load('memory', data=counts, num_partitions=2, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=SSBUDF(**sr.physical_params()))
    corr, scale = sr.phase_agreement(res['phase'].data.astype(np.float64), phi)
    print(f"correlation {corr:.7f}, scale {scale:.4f}")
    assert corr > 0.999
    assert abs(scale - 1) < 0.02
    # the opposite shift gives the opposite phase
    flipped = sr.reference(frames, transformation=-np.eye(2), **sr.physical_params())
    assert sr.phase_agreement(flipped['phase'], phi)[0] < -0.999


def test_weak_phase_scan():
    phi = sr.physical_phase()
    frames = weak_phase_scan(phi, 4, 6.5, counts=500.)
    assert frames.shape == (8, 8, 32, 32) and frames.dtype == np.float64
    assert np.allclose(frames.sum(axis=(2, 3)), 500.)
    # the bright-field disk holds nearly all of the beam, around (16, 16)
    inside = sr.distance2((32, 32), 16., 16.) < 6.5 ** 2
    assert frames[:, :, inside].sum() > 0.97 * frames.sum()
    # a flat phase: every frame is the aperture
    flat = weak_phase_scan(np.zeros((32, 32)), 16, 6.5)
    assert np.allclose(flat[0, 0], flat[1, 1]) and np.allclose(flat[0, 0][~inside], 0, atol=1e-9)
    with pytest.raises(ValueError, match='step'):
        weak_phase_scan(phi, 5, 6.5)
    with pytest.raises(ValueError, match='2D'):
        weak_phase_scan(np.zeros(8), 2, 2.0)
    with pytest.raises(ValueError, match='aperture'):
        weak_phase_scan(phi, 2, 0.0)


@pytest.mark.parametrize('q', [(1, 2), (6, 0), (11, 5), (3, 9)], ids=str)       # (6, 0), (11, 5): Nyquist indices
def test_trotter_masks(q):
    p = sr.full_params(sr.GENERIC_SIG, **sr.GENERIC)
    pos, neg = trotter_masks(sr.GENERIC_SIG, q, sr.GENERIC_NAV, **sr.GENERIC)
    ref_pos, ref_neg = sr.masks(sr.GENERIC_SIG, sr.GENERIC_NAV, q[0], q[1], p)
    assert pos.dtype == bool and pos.shape == sr.GENERIC_SIG
    assert np.array_equal(pos, ref_pos) and np.array_equal(neg, ref_neg)
    assert not np.any(pos & neg)


def test_trotter_masks_without_overlap():
    # a coarse detector: the first spatial frequency already shifts the disks by more than their diameter
    params = dict(sr.GENERIC, semiconv=0.001, transformation=None)
    p = sr.full_params(sr.GENERIC_SIG, **params)
    d = sr.shift(p, sr.GENERIC_NAV, 1, 0)
    assert np.hypot(*d) >= 2 * 7.3
    pos, neg = trotter_masks(sr.GENERIC_SIG, (1, 0), sr.GENERIC_NAV, **params)
    assert not pos.any() and not neg.any()
    with pytest.raises(ValueError, match='q_index'):
        trotter_masks(sr.GENERIC_SIG, (12, 0), sr.GENERIC_NAV, **sr.GENERIC)


def test_parameter_errors(ctx, generic):
    frames, _ = generic
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)

    def run(dataset=ds, roi=None, **kw):
        return ctx.run_udf(dataset=dataset, udf=SSBUDF(**dict(sr.GENERIC, **kw)), roi=roi)

    roi = np.zeros(sr.GENERIC_NAV, bool)
    roi[2:5] = True
    with pytest.raises(ValueError, match='roi'):
        run(roi=roi)
    with pytest.raises(ValueError, match='P = 0'):
        run(cy=-40.)
    with pytest.raises(ValueError, match='cutoff 0'):
        run(cutoff=0)
    with pytest.raises(ValueError, match='cutoff 1.5'):
        run(cutoff=1.5)
    with pytest.raises(ValueError, match=r'transformation of shape \(3, 2\)'):
        run(transformation=np.ones((3, 2)))
    with pytest.raises(ValueError, match='transformation of shape'):
        run(transformation=np.ones(4))
    with pytest.raises(ValueError, match='semiconv_pix'):
        run(semiconv_pix=0.)
    with pytest.raises(ValueError, match='lamb'):
        run(lamb=-1e-12)
    with pytest.raises(ValueError, match='dpix'):
        run(dpix=(1e-10, 1e-10, 1e-10))
    with pytest.raises(ValueError, match='dx'):
        run(dpix=(1e-10, np.nan))
    sliced = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, tileshape=(7, 4, 4))
    with pytest.raises(ValueError, match='whole frames'):
        run(dataset=sliced)
    line = ctx.load('memory', data=frames.reshape((120,) + sr.GENERIC_SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='2D scan'):
        run(dataset=line)
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 2, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D frames'):
        run(dataset=ds3)
    assert check_params((24, 28), 2e-12, 1e-10, 0.02, 7.)['cy'] == 12. and \
        check_params((24, 28), 2e-12, 1e-10, 0.02, 7.)['cx'] == 14.


def test_wavelength():
    for kilovolts, picometres in ((300, 1.9687), (200, 2.5079), (80, 4.1757)):
        assert abs(wavelength(kilovolts) * 1e12 - picometres) < 5e-5, kilovolts


def test_udf_declarations():
    udf = SSBUDF(**sr.GENERIC)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {'bf': 'disjoint'}
    assert list(inspect.signature(SSBUDF.__init__).parameters) == [
        'self', 'lamb', 'dpix', 'semiconv', 'semiconv_pix', 'cy', 'cx', 'transformation', 'cutoff']


def test_hip_signatures():
    from libertem_amd import hip
    assert list(inspect.signature(hip.ssb_gather).parameters) == [
        'device', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'n_px', 'idx_ptr', 'n_idx', 'out_ptr', 'ld_out',
        'stream']
    assert list(inspect.signature(hip.SSBPlan.__init__).parameters) == [
        'self', 'device', 'nav_y', 'nav_x', 'sig_w', 'idx', 'max_batch', 'geom', 'cutoff']
    assert list(inspect.signature(hip.SSBPlan.reconstruct).parameters) == [
        'self', 'bf_ptr', 'ld_bf', 'fourier_ptr', 'stream']
    assert list(inspect.signature(hip.ssb_trotter).parameters) == [
        'device', 'spec_ptr', 'ld_spec', 'nav_y', 'nav_x', 'idx_ptr', 'n_idx', 'sig_w', 'geom', 'cutoff',
        'fourier_ptr', 'stream']
    for name in ('ltmi_ssb_gather', 'ltmi_ssb_plan_create', 'ltmi_ssb_plan_destroy', 'ltmi_ssb_reconstruct',
                 'ltmi_ssb_plan_last_kernel', 'ltmi_ssb_trotter'):
        assert name in hip.EXPORTS
    geom = hip.ssb_geometry(2e-12, (3e-11, 4e-11), 0.02, 7.3, 11.6, 14.2, [[1, 2], [3, 4]])
    assert geom.dtype == np.float64 and geom.tolist() == [2e-12, 3e-11, 4e-11, 0.02, 7.3, 11.6, 14.2, 1, 2, 3, 4]
