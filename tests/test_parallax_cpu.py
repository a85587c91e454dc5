"""
`libertem_amd.udf.parallax` without a GPU: the NumPy branch (`parallax_bf`, ParallaxUDF on the inline executor) against
the index-by-index float64 restatement (tests/parallax_ref.py) on both scans of the fixture, with and without
`regularize`; the physical checks on the noise-free frames; `fit_shifts`, `parallax_aberrations`, `defocused_scan`;
every ValueError; the declarations of the UDF and of the bindings.
"""
import inspect

import numpy as np
import pytest

import parallax_ref as pr
from libertem_amd.udf import ParallaxUDF, fit_shifts, parallax_aberrations, parallax_bf
from libertem_amd.udf.ssb import bf_pixels
from libertem_amd.utils.generate import defocused_scan

NAV_IDS = ['12x10', '9x16']


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    return Context(InlineJobExecutor())


def bf_of(data):
    idx = bf_pixels(pr.SIG, pr.SEMICONV_PIX, pr.CY, pr.CX)
    assert idx.size == pr.N_BF
    return np.asarray(data).reshape(data.shape[0] * data.shape[1], -1)[:, idx]


@pytest.mark.parametrize('regularize', [False, True], ids=['free', 'regularized'])
@pytest.mark.parametrize('kind', ['frames', 'counted'])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_parallax_bf_vs_restatement(nav, kind, regularize):
    """both are float64 and differ in the order of their sums only: 1e-9 of the largest value"""
    data = pr.frames(nav) if kind == 'frames' else pr.counted(nav)
    ref = pr.reference_of(kind, nav, regularize)
    res = parallax_bf(bf_of(data), nav, pr.SIG, regularize=regularize, image_dtype=np.float64, **pr.PARAMS)
    assert res['shifts'].shape == (pr.N_BF, 2) and res['matrix'].shape == (2, 2) and res['offset'].shape == (2,)
    assert all(res[k].dtype == np.float64 for k in res)
    assert res['image'].shape == nav and res['bright_field'].shape == nav
    for name in ('shifts', 'matrix', 'offset', 'image', 'bright_field'):
        assert np.abs(res[name] - ref[name]).max() <= 1e-9 * np.abs(ref[name]).max(), name
    if not regularize:
        assert pr.same_integer_parts(res, ref)
    cast = parallax_bf(bf_of(data), nav, pr.SIG, regularize=regularize, **pr.PARAMS)
    assert cast['image'].dtype == np.float32 and cast['bright_field'].dtype == np.float32
    assert np.array_equal(cast['image'], res['image'].astype(np.float32))
    assert cast['shifts'].tobytes() == res['shifts'].tobytes()


@pytest.mark.parametrize('regularize', [False, True], ids=['free', 'regularized'])
@pytest.mark.parametrize('kind', ['frames', 'counted'])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_fixture_has_no_near_ties(nav, kind, regularize):
    """In both iterations the restatement's best candidate of every pixel beats every candidate that is no neighbour
    of it by more than 1e-3 of the peak (12 x 10: 0.20, 9 x 16: 0.27 at the committed seeds), so a float32 transform
    cannot move a shift to another part of the window.  The seeds were also chosen so that the best candidate beats
    its eight neighbours by more than 1e-3 of the peak (1.2e-3 and 2.9e-3): the integer part of a shift is stable too."""
    ref = pr.reference_of(kind, nav, regularize)
    assert ref['margins'].shape == (2, pr.N_BF)
    assert ref['margins'].min() > 1e-3
    assert ref['adjacent'].min() > 1e-3


@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_physical_checks(nav):
    """The noise-free fixture after two iterations, against the truth it was made from.  The restatement gives, on
    12 x 10 / 9 x 16: largest shift error 0.116 / 0.184 scan pixels (the bias of the three-point parabola and the
    common offset it leaves), matrix error 9.3e-4 / 3.1e-3 absolute, rotation error 0.017 / 0.105 degrees, largest
    error of `image` against the object 0.025 / 0.013 and of `bright_field` 0.30 / 0.26.  The bounds are twice the
    restatement's own figures; `image` is closer to the object than `bright_field` by a factor of 5 at least (here
    12 and 19)."""
    ref = pr.reference_of('frames', nav)
    res = parallax_bf(bf_of(pr.frames(nav)), nav, pr.SIG, **pr.PARAMS)
    true = pr.true_shifts()
    obj = pr.make_obj(nav)

    def figures(r):
        return (np.abs(r['shifts'] - true).max(), np.abs(r['matrix'] - pr.MATRIX).max(),
                abs(pr.rotation_deg(r['matrix']) - pr.ANGLE_DEG),
                np.abs(np.asarray(r['image'], dtype=np.float64) / 1000. - obj).max(),
                np.abs(np.asarray(r['bright_field'], dtype=np.float64) / 1000. - obj).max())

    ref_fig, got = figures(ref), figures(res)
    print(f"{nav}: restatement shift {ref_fig[0]:.4f} matrix {ref_fig[1]:.5f} rotation {ref_fig[2]:.4f} deg "
          f"image {ref_fig[3]:.4f} bright field {ref_fig[4]:.4f}")
    for have, bound in zip(got[:3], ref_fig[:3]):
        assert have <= 2 * bound
    assert got[3] * 5 <= got[4]
    rot = parallax_aberrations(res['matrix'], 1., 1., 1.)
    assert abs(rot['rotation_deg'] - pr.ANGLE_DEG) <= 2 * ref_fig[2]


@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_regularized_shifts_are_affine(nav):
    res = parallax_bf(bf_of(pr.frames(nav)), nav, pr.SIG, regularize=True, **pr.PARAMS)
    offsets = np.array([(y - pr.CY, x - pr.CX) for y, x in pr.pixels()])
    predicted = offsets @ res['matrix'].T + res['offset']
    assert np.abs(res['shifts'] - predicted).max() < 1e-12
    free = parallax_bf(bf_of(pr.frames(nav)), nav, pr.SIG, **pr.PARAMS)
    assert np.abs(free['shifts'] - (offsets @ free['matrix'].T + free['offset'])).max() > 1e-3


def test_fit_shifts():
    rng = np.random.default_rng(3)
    offsets = rng.normal(size=(40, 2)) * 5
    m, b = np.array([[0.4, -0.2], [0.3, 0.5]]), np.array([0.7, -1.1])
    exact = offsets @ m.T + b
    got_m, got_b, fitted = fit_shifts(exact, offsets)
    assert np.abs(got_m - m).max() < 1e-13 and np.abs(got_b - b).max() < 1e-13 and np.abs(fitted - exact).max() < 1e-12
    noisy = exact + rng.normal(size=exact.shape) * 0.05
    ref_m, ref_b, ref_fit = pr.affine_fit(noisy, offsets)
    got_m, got_b, fitted = fit_shifts(noisy, offsets)
    assert np.abs(got_m - ref_m).max() < 1e-12 and np.abs(got_b - ref_b).max() < 1e-12
    assert np.abs(fitted - ref_fit).max() < 1e-12
    with pytest.raises(ValueError, match=r'\(P, 2\)'):
        fit_shifts(exact[:, :1], offsets)
    with pytest.raises(ValueError, match=r'\(P, 2\)'):
        fit_shifts(exact, offsets[:-1])


@pytest.mark.parametrize('angle, defocus, astig, axis', [(25., 800., 120., 30.), (-140., 35., 0., 0.),
                                                         (90., 5e3, 4e3, -75.), (0., 1., 0.25, 90.)])
def test_aberrations_invert_a_known_matrix(angle, defocus, astig, axis):
    dpix, semiconv, semiconv_pix = 0.35, 0.021, 17.5
    a = np.radians(axis)
    sym = defocus * np.eye(2) + astig * np.array([[np.cos(2 * a), np.sin(2 * a)], [np.sin(2 * a), -np.cos(2 * a)]])
    matrix = pr.rot(angle) @ sym * (semiconv / semiconv_pix) / dpix
    out = parallax_aberrations(matrix, dpix, semiconv, semiconv_pix)
    assert abs(out['rotation_deg'] - angle) < 1e-12 * 180
    assert np.abs(out['transformation'] - pr.rot(angle).T).max() < 1e-12
    assert abs(out['defocus'] - defocus) < 1e-12 * defocus
    assert abs(out['astigmatism'] - astig) < 1e-12 * defocus
    if astig:
        assert abs(out['astigmatism_axis_deg'] - axis) < 1e-9
    # the defocus as the issue states it, from the matrix in pixel units
    u, s, vt = np.linalg.svd(matrix)
    assert abs(out['defocus'] - np.trace(vt.T @ np.diag(s) @ vt) / 2 * dpix / (semiconv / semiconv_pix)) < 1e-9 * defocus
    two = parallax_aberrations(matrix, (dpix, dpix), semiconv, semiconv_pix)
    assert two['defocus'] == out['defocus'] and two['rotation_deg'] == out['rotation_deg']


def test_aberrations_sign_and_errors():
    # an indefinite S (astigmatism above the defocus) keeps a proper rotation
    sym = np.array([[1., 0.], [0., -0.5]])
    out = parallax_aberrations(pr.rot(10.) @ sym, 1., 1., 1.)
    assert abs(out['rotation_deg'] - 10.) < 1e-12 and abs(out['defocus'] - 0.25) < 1e-12
    assert abs(out['astigmatism'] - 0.75) < 1e-12
    assert abs(np.linalg.det(out['transformation']) - 1) < 1e-12
    with pytest.raises(ValueError, match='2 x 2'):
        parallax_aberrations(np.eye(3), 1., 1., 1.)
    with pytest.raises(ValueError, match='2 x 2'):
        parallax_aberrations([[1., np.nan], [0., 1.]], 1., 1., 1.)
    with pytest.raises(ValueError, match='dpix'):
        parallax_aberrations(np.eye(2), (1., 1., 1.), 1., 1.)
    with pytest.raises(ValueError, match='semiconv_pix'):
        parallax_aberrations(np.eye(2), 1., 1., 0.)
    with pytest.raises(ValueError, match='dx'):
        parallax_aberrations(np.eye(2), (1., -1.), 1., 1.)


def test_defocused_scan():
    nav = (9, 16)
    obj = pr.make_obj(nav)
    flat = defocused_scan(obj, np.zeros((2, 2)), pr.SIG, pr.SEMICONV_PIX, pr.CY, pr.CX, counts=10.)
    assert flat.shape == nav + pr.SIG and flat.dtype == np.float64
    inside = np.zeros(pr.SIG, bool)
    for y, x in pr.pixels():
        inside[y, x] = True
    assert np.all(flat[:, :, ~inside] == 0)
    # the zero matrix: identical scan images, the object itself
    images = flat[:, :, inside]
    assert np.all(images == images[:, :, :1])
    assert np.abs(images[:, :, 0] - 10 * obj).max() < 1e-12
    # an integer shift is a roll: I_K(r) = O(r - s_K)
    moved = defocused_scan(obj, np.zeros((2, 2)), pr.SIG, pr.SEMICONV_PIX, pr.CY, pr.CX, offset=(2, -3))
    assert np.abs(moved[:, :, 5, 7] - 1000 * np.roll(obj, (2, -3), axis=(0, 1))).max() < 1e-9
    # the matrix acts on (y, x) of k - c
    one = defocused_scan(obj, [[0., 1.], [0., 0.]], (12, 14), 4.3, 5., 7.)
    assert np.abs(one[:, :, 5, 9] - 1000 * np.roll(obj, 2, axis=0)).max() < 1e-9
    centred = defocused_scan(obj, pr.MATRIX, (8, 8), 2.)
    assert np.abs(centred[:, :, 4, 4] - 1000 * obj).max() < 1e-9             # (the default centre (h / 2, w / 2))
    with pytest.raises(ValueError, match='2D array'):
        defocused_scan(obj[0], pr.MATRIX, pr.SIG, 4.3)
    with pytest.raises(ValueError, match='2 x 2'):
        defocused_scan(obj, np.eye(3), pr.SIG, 4.3)


@pytest.mark.parametrize('num_partitions', [1, 3])
def test_udf_on_the_inline_executor(ctx, num_partitions):
    nav = (12, 10)
    data = pr.counted(nav)
    ds = ctx.load('memory', data=np.array(data), num_partitions=num_partitions, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=ParallaxUDF(**pr.PARAMS))
    direct = parallax_bf(bf_of(data), nav, pr.SIG, **pr.PARAMS)
    for name in ('shifts', 'matrix', 'offset', 'image', 'bright_field'):
        assert res[name].data.dtype == direct[name].dtype and res[name].data.shape == direct[name].shape
        assert res[name].data.tobytes() == direct[name].tobytes(), name
    assert np.array_equal(res['bf'].data.reshape(120, pr.N_BF), bf_of(data).astype(np.float32))
    reg = ctx.run_udf(dataset=ds, udf=ParallaxUDF(regularize=True, **pr.PARAMS))
    assert reg['shifts'].data.tobytes() == parallax_bf(bf_of(data), nav, pr.SIG, regularize=True,
                                                       **pr.PARAMS)['shifts'].tobytes()


def test_value_errors(ctx):
    nav = (12, 10)
    data = np.array(pr.counted(nav))
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2)

    def run(dataset=ds, roi=None, **kw):
        return ctx.run_udf(dataset=dataset, udf=ParallaxUDF(**dict(pr.PARAMS, **kw)), roi=roi)

    roi = np.zeros(nav, bool)
    roi[1] = True
    with pytest.raises(ValueError, match='roi'):
        run(roi=roi)
    with pytest.raises(ValueError, match=r'2 \* max_shift \+ 1 = 11'):
        run(max_shift=5)                                                   # (10 columns < 11)
    with pytest.raises(ValueError, match='max_shift 0'):
        run(max_shift=0)
    with pytest.raises(ValueError, match='max_shift 1.5'):
        run(max_shift=1.5)
    with pytest.raises(ValueError, match='iterations 0'):
        run(iterations=0)
    with pytest.raises(ValueError, match='P = 0'):
        run(semiconv_pix=0.1, cy=5.5, cx=7.5)
    with pytest.raises(ValueError, match='semiconv_pix'):
        run(semiconv_pix=0.)
    with pytest.raises(ValueError, match='disk centre'):
        run(cy=np.inf)
    sliced = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, tileshape=(7, 4, 14))
    with pytest.raises(ValueError, match='whole frames'):
        run(dataset=sliced)
    line = ctx.load('memory', data=data.reshape((120,) + pr.SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='2D scan'):
        run(dataset=line)
    ds3 = ctx.load('memory', data=np.zeros((12, 10, 2, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D frames'):
        run(dataset=ds3)
    with pytest.raises(ValueError, match=r'bf of shape \(120, 57\)'):
        parallax_bf(bf_of(data)[:, :57], nav, pr.SIG, **pr.PARAMS)
    with pytest.raises(ValueError, match=r'2 \* max_shift \+ 1 = 11'):
        parallax_bf(bf_of(data), nav, pr.SIG, **dict(pr.PARAMS, max_shift=5))
    with pytest.raises(ValueError, match='P = 0'):
        parallax_bf(np.zeros((120, 0)), nav, pr.SIG, 0.1, 5.5, 7.5)
    assert run(max_shift=4)['shifts'].data.shape == (pr.N_BF, 2)              # 2 * 4 + 1 = 9 fits both axes


def test_constant_scan_images_stay_in_the_window(ctx):
    ds = ctx.load('memory', data=np.full((12, 10) + pr.SIG, 7, np.uint16), num_partitions=1, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=ParallaxUDF(**pr.PARAMS))
    assert np.all(np.abs(res['shifts'].data) <= pr.MAX_SHIFT + 0.5)
    assert np.allclose(res['image'].data, 7) and np.allclose(res['bright_field'].data, 7)


def test_udf_declarations():
    udf = ParallaxUDF(**pr.PARAMS)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {'bf': 'disjoint'}
    assert udf.params.regularize is False and udf.params.iterations == 2
    assert list(inspect.signature(ParallaxUDF.__init__).parameters) == [
        'self', 'semiconv_pix', 'cy', 'cx', 'max_shift', 'iterations', 'regularize']
    from libertem_amd.udf import run_parallax
    assert list(inspect.signature(run_parallax).parameters) == [
        'ctx', 'dataset', 'semiconv_pix', 'cy', 'cx', 'max_shift', 'iterations', 'regularize', 'keep_bf']


def test_hip_signatures():
    from libertem_amd import hip
    from libertem_amd.build import SOURCES, header_exports
    from libertem_amd.udf import parallax
    assert 'ltmi_parallax.hip' in SOURCES
    assert list(inspect.signature(hip.plx_ramps).parameters) == [
        'device', 'sh_ptr', 'n', 'nav_y', 'nav_x', 'ey_ptr', 'ex_ptr', 'stream']
    assert list(inspect.signature(hip.plx_sum).parameters) == [
        'device', 'spec_ptr', 'n', 'nav_y', 'nav_x', 'ey_ptr', 'ex_ptr', 's_ptr', 'stream']
    assert list(inspect.signature(hip.plx_mul).parameters) == [
        'device', 'spec_ptr', 'n', 'nav_y', 'nav_x', 'ref_ptr', 'x_ptr', 'stream']
    assert list(inspect.signature(hip.plx_peaks).parameters) == [
        'device', 'maps_ptr', 'n', 'nav_y', 'nav_x', 'max_shift', 'shifts_ptr', 'stream']
    assert list(inspect.signature(hip.ParallaxPlan.__init__).parameters) == [
        'self', 'device', 'nav_y', 'nav_x', 'n_idx', 'max_batch', 'max_shift', 'store_limit_bytes']
    names = ('ltmi_plx_ramps', 'ltmi_plx_sum', 'ltmi_plx_mul', 'ltmi_plx_peaks', 'ltmi_plx_plan_create',
             'ltmi_plx_plan_destroy', 'ltmi_plx_plan_load', 'ltmi_plx_plan_iterate', 'ltmi_plx_plan_sum',
             'ltmi_plx_plan_last_kernel')
    for name in names:
        assert name in hip.EXPORTS and name in header_exports()
    assert parallax.STORE_LIMIT_BYTES == 8 << 30
    assert parallax.plan_batch((12, 10), 58) == 58 and parallax.plan_batch((4096, 4096), 58) >= 1
