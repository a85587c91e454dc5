"""
Wigner-distribution deconvolution without a GPU: `reconstruct_window` and `WDDUDF` on the inline executor against the
index-by-index float64 restatement in its rho-space form (tests/wdd_ref.py), at the tolerance of the ssb tests, on the
generic fixture of tests/ssb_ref.py -- a 12 x 10 scan of 24 x 28 uint16 Poisson(40) frames, rotated geometry, centre
11.6 / 14.2, radius 7.3 -- with windows (16, 16), (16, 18) and (20, 16) and epsilon 1e-2; the physics on the simulated
phase object (window 24, epsilon 1e-4): the sign, the correlation at 0.1 rad, the phase scale at 1.0 rad against
single-sideband's; `wdd_filter` and `window_pixels`; every parameter error; the declarations.
"""
import inspect

import numpy as np
import pytest

import ssb_ref as sr
import wdd_ref as wr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import WDDUDF
from libertem_amd.udf.wdd import check_params, reconstruct_window, wdd_filter, window_pixels
from libertem_amd.utils.generate import weak_phase_scan

IMAGES = ('complex', 'phase', 'amplitude')
NAV, SIG = sr.GENERIC_NAV, sr.GENERIC_SIG


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.fixture(scope='module')
def generic():
    """the frames (12, 10, 24, 28) and, per window, the restatement's results in float64 and in float32"""
    frames = sr.generic_frames()
    refs = {w: (wr.reference(frames, w, wr.GENERIC_EPSILON, **wr.GENERIC),
                wr.reference(frames, w, wr.GENERIC_EPSILON, single=True, **wr.GENERIC)) for w in wr.WINDOWS}
    return frames, refs


@pytest.fixture(scope='module')
def physical():
    """amplitude -> (phi, the simulated scan (16, 16, 32, 32), the restatement's results, single-sideband's)"""
    out = {}
    for amplitude in (0.1, 1.0):
        phi = sr.physical_phase(amplitude)
        frames = weak_phase_scan(phi, sr.PHYS_STEP, sr.PHYS_SEMICONV_PIX, counts=1e4)
        out[amplitude] = (phi, frames, wr.reference(frames, wr.PHYS_WINDOW, wr.PHYS_EPSILON, **wr.physical_params()),
                          sr.reference(frames, **sr.physical_params()))
    return out


def test_fixtures_are_what_the_tests_need(generic):
    frames, refs = generic
    p = sr.full_params(SIG, **wr.GENERIC)
    # no pixel sits on a rim: Gamma does not depend on the last bits of the predicate arithmetic
    assert sr.rim_margin(SIG, NAV, p) >= 1e-6
    assert sr.rim_margin((32, 32), (16, 16), sr.full_params((32, 32), **wr.physical_params())) >= 1e-6
    assert [wr.window_origin(p, w)[:2] for w in wr.WINDOWS] == [(3, 6), (3, 5), (1, 6)]
    for w, (ref, single) in refs.items():
        # some Qs have no overlap (S = 0 exactly), most have one
        assert (ref['overlap'] == 0).sum() == 7 and np.all((ref['s'] == 0) == (ref['overlap'] == 0))
        assert abs(abs(ref['fourier'][0, 0]) - 1) < 1e-12
        # the float32 restatement stays below a quarter of SSB's atol here: SSB's number is kept
        atol, base, single_err = wr.atol_rule(ref['fourier'], single['fourier'])
        print(f"window {w}: float32 restatement error {single_err:.3e}, SSB atol {base:.3e}")
        assert atol == base and single_err < base / 4


@pytest.mark.parametrize('window', wr.WINDOWS, ids=str)
@pytest.mark.parametrize('dtype', ['uint16', 'float64'])
def test_reconstruct_window_equals_restatement(generic, window, dtype):
    frames, refs = generic
    ref = refs[window][0]
    idx = window_pixels(SIG, window, 11.6, 14.2)
    assert idx.dtype == np.int32 and idx.shape == (window[0] * window[1],)
    bf = frames.reshape(120, -1)[:, idx].astype(dtype)
    out = reconstruct_window(bf, NAV, SIG, window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)
    wr.assert_fourier(out['fourier'], ref['fourier'], f'reconstruct_window {window} {dtype}')
    wr.assert_images(out, ref, f'reconstruct_window {window} {dtype}')
    assert np.array_equal(out['fourier'] == 0, ref['fourier'] == 0)
    with pytest.raises(ValueError, match='bf of shape'):
        reconstruct_window(bf[:, :-1], NAV, SIG, window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)


@pytest.mark.parametrize('window', wr.WINDOWS, ids=str)
def test_udf_equals_restatement(ctx, generic, window):
    frames, refs = generic
    ref = refs[window][0]
    ds = ctx.load('memory', data=frames, num_partitions=3, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=WDDUDF(window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC))
    assert res['fourier'].data.shape == NAV and res['fourier'].data.dtype == np.complex64
    assert res['complex'].data.dtype == np.complex64
    assert res['phase'].data.dtype == np.float32 and res['amplitude'].data.dtype == np.float32
    wr.assert_fourier(res['fourier'].data, ref['fourier'], f'WDDUDF inline {window}')
    wr.assert_images({k: res[k].data for k in IMAGES}, ref, f'WDDUDF inline {window}')
    idx = window_pixels(SIG, window, 11.6, 14.2)
    assert res['bf'].data.shape == NAV + (idx.size,) and res['bf'].data.dtype == np.float32
    assert np.array_equal(res['bf'].data.reshape(120, -1), frames.reshape(120, -1)[:, idx].astype(np.float32))


def test_scalar_window_defaults_and_odd_shapes():
    # window as one number, dpix as one number, no transformation, the centre (h / 2, w / 2); an odd scan and frame
    rng = np.random.default_rng(5)
    frames = rng.poisson(30., (9, 7, 17, 20)).astype(np.float32)
    params = dict(lamb=2.5e-12, dpix=0.3e-10, semiconv=0.02, semiconv_pix=5.1)
    assert sr.rim_margin((17, 20), (9, 7), sr.full_params((17, 20), **params)) >= 1e-6
    ref = wr.reference(frames, 13, 1e-2, **params)
    idx = window_pixels((17, 20), 13)
    assert idx[0] == 2 * 20 + 4 and idx[-1] == 14 * 20 + 16
    out = reconstruct_window(frames.reshape(63, -1)[:, idx], (9, 7), (17, 20), window=13, epsilon=1e-2, **params)
    wr.assert_fourier(out['fourier'], ref['fourier'], 'defaults')
    wr.assert_images(out, ref, 'defaults')


def test_sign_and_physics(ctx, physical):
    for amplitude, (phi, frames, ref, ssb) in physical.items():
        corr, scale = sr.phase_agreement(ref['phase'], phi)
        corr_ssb, scale_ssb = sr.phase_agreement(ssb['phase'], phi)
        print(f"amplitude {amplitude}: WDD correlation {corr:.5f} scale {scale:.4f}; SSB correlation {corr_ssb:.5f} "
              f"scale {scale_ssb:.4f}")
        # the sign: +phi, not -phi
        assert corr > 0
        if amplitude == 0.1:
            assert corr > 0.99
        else:
            assert abs(1 - scale) < abs(1 - scale_ssb)
        # the opposite shift gives the opposite phase
        flipped = wr.reference(frames, wr.PHYS_WINDOW, wr.PHYS_EPSILON, transformation=-np.eye(2),
                               **wr.physical_params())
        assert sr.phase_agreement(flipped['phase'], phi)[0] < -0.99
        # every route agrees with the restatement's correlation and scale to 1e-3
        params = dict(wr.physical_params(), window=wr.PHYS_WINDOW, epsilon=wr.PHYS_EPSILON)
        idx = window_pixels((32, 32), wr.PHYS_WINDOW)
        direct = reconstruct_window(frames.reshape(256, -1)[:, idx], (16, 16), (32, 32), **params)
        ds = ctx.load('memory', data=frames.astype(np.float32), num_partitions=2, sig_dims=2)
        udf = ctx.run_udf(dataset=ds, udf=WDDUDF(**params))
        for what, phase in (('reconstruct_window', direct['phase']), ('WDDUDF', udf['phase'].data)):
            c, s = sr.phase_agreement(np.asarray(phase, dtype=np.float64), phi)
            assert abs(c - corr) < 1e-3 and abs(s - scale) < 1e-3, (what, c, s)


@pytest.mark.parametrize('q', [(0, 0), (1, 2), (6, 0), (11, 5), (3, 9), (6, 5)], ids=str)
def test_wdd_filter(q):
    window = (16, 18)
    ref = wr.filters(SIG, NAV, window, wr.GENERIC_EPSILON, **wr.GENERIC)[q].reshape(window)
    got = wdd_filter(SIG, q, NAV, window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)
    assert got.shape == window and got.dtype == np.complex128
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    with pytest.raises(ValueError, match='q_index'):
        wdd_filter(SIG, (12, 0), NAV, window=window, epsilon=wr.GENERIC_EPSILON, **wr.GENERIC)


def test_filter_without_overlap_is_zero():
    # a coarse detector: the first spatial frequency already shifts the disk by more than its diameter
    params = dict(wr.GENERIC, semiconv=0.001, transformation=None)
    p = sr.full_params(SIG, **params)
    assert np.hypot(*sr.shift(p, NAV, 1, 0)) >= 2 * 7.3
    got = wdd_filter(SIG, (1, 0), NAV, window=16, epsilon=1e-2, **params)
    assert np.all(got == 0)
    assert np.any(wdd_filter(SIG, (0, 0), NAV, window=16, epsilon=1e-2, **params) != 0)


def test_parameter_errors(ctx, generic):
    frames, _ = generic
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2)

    def run(dataset=ds, roi=None, **kw):
        params = dict(wr.GENERIC, window=16, epsilon=1e-2)
        params.update(kw)
        return ctx.run_udf(dataset=dataset, udf=WDDUDF(**params), roi=roi)

    roi = np.zeros(NAV, bool)
    roi[2:5] = True
    with pytest.raises(ValueError, match='roi'):
        run(roi=roi)
    with pytest.raises(ValueError, match='window 0'):
        run(window=0)
    with pytest.raises(ValueError, match=r'window \(16, 1.5\)'):
        run(window=(16, 1.5))
    with pytest.raises(ValueError, match=r'window \(16, 16, 16\)'):
        run(window=(16, 16, 16))
    with pytest.raises(ValueError, match=r'window rows \[-3, 25\)'):
        run(window=(28, 16))
    with pytest.raises(ValueError, match=r'window columns \[-1, 29\)'):
        run(window=(16, 30))
    with pytest.raises(ValueError, match=r'does not hold the disk pixel \(17, 10\)'):
        run(window=(12, 16))
    with pytest.raises(ValueError, match=r'does not hold the disk pixel \(9, 21\)'):
        run(window=(16, 14))
    with pytest.raises(ValueError, match='epsilon 0'):
        run(epsilon=0)
    with pytest.raises(ValueError, match='epsilon -1'):
        run(epsilon=-1)
    with pytest.raises(ValueError, match='epsilon nan'):
        run(epsilon=np.nan)
    with pytest.raises(ValueError, match='epsilon inf'):
        run(epsilon=np.inf)
    with pytest.raises(ValueError, match='P = 0'):
        run(semiconv_pix=0.1, cy=11.5, cx=14.5)
    with pytest.raises(ValueError, match=r'transformation of shape \(3, 2\)'):
        run(transformation=np.ones((3, 2)))
    with pytest.raises(ValueError, match='semiconv_pix'):
        run(semiconv_pix=0.)
    with pytest.raises(ValueError, match='lamb'):
        run(lamb=-1e-12)
    with pytest.raises(ValueError, match='dpix'):
        run(dpix=(1e-10, 1e-10, 1e-10))
    with pytest.raises(ValueError, match='dx'):
        run(dpix=(1e-10, np.nan))
    with pytest.raises(ValueError, match='disk centre'):
        run(cy=np.inf)
    sliced = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, tileshape=(7, 4, 4))
    with pytest.raises(ValueError, match='whole frames'):
        run(dataset=sliced)
    line = ctx.load('memory', data=frames.reshape((120,) + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='2D scan'):
        run(dataset=line)
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 2, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D frames'):
        run(dataset=ds3)
    with pytest.raises(ValueError, match='leave the frame'):
        window_pixels(SIG, 30)
    p = check_params(SIG, 2e-12, 1e-10, 0.02, 7., 16)
    assert (p['cy'], p['cx'], p['window'], p['epsilon']) == (12., 14., (4, 6, 16, 16), 0.01)


def test_all_zero_frames_give_nan(ctx):
    ds = ctx.load('memory', data=np.zeros(NAV + SIG, np.uint16), num_partitions=1, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=WDDUDF(window=16, **wr.GENERIC))
    assert np.all(np.isnan(res['fourier'].data)) and np.all(np.isnan(res['phase'].data))


def test_udf_declarations():
    udf = WDDUDF(window=16, **wr.GENERIC)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {'bf': 'disjoint'}
    assert udf.params.epsilon == 0.01
    assert list(inspect.signature(WDDUDF.__init__).parameters) == [
        'self', 'lamb', 'dpix', 'semiconv', 'semiconv_pix', 'window', 'epsilon', 'cy', 'cx', 'transformation']


def test_hip_signatures():
    from libertem_amd import hip
    from libertem_amd.build import header_exports
    assert list(inspect.signature(hip.wdd_filter).parameters) == [
        'device', 'nav_y', 'nav_x', 'window', 'geom', 'epsilon', 'q0', 'n_q', 'q_batch', 'filter_ptr', 'stream']
    assert list(inspect.signature(hip.wdd_dot).parameters) == [
        'device', 'spec_ptr', 'ld_spec', 'nav_y', 'nav_x', 'filter_ptr', 'ld_filter', 'k0', 'n_k', 'acc_ptr', 'first',
        'stream']
    assert list(inspect.signature(hip.WDDPlan.__init__).parameters) == [
        'self', 'device', 'nav_y', 'nav_x', 'window', 'max_batch', 'geom', 'epsilon']
    assert list(inspect.signature(hip.WDDPlan.reconstruct).parameters) == [
        'self', 'bf_ptr', 'ld_bf', 'fourier_ptr', 'stream']
    names = ('ltmi_wdd_filter', 'ltmi_wdd_dot', 'ltmi_wdd_finish', 'ltmi_wdd_plan_create', 'ltmi_wdd_plan_destroy',
             'ltmi_wdd_reconstruct', 'ltmi_wdd_plan_last_kernel')
    for name in names:
        assert name in hip.EXPORTS and name in header_exports()
