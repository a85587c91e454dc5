"""
Holography without a GPU: the NumPy branch (`reconstruct_frames`) against the index-free float64 restatement of the
definition (tests/holo_ref.py) on every case of the kernel table; `hologram_frame` against the reference's function
(tests/golden/holo_frames.npz, written by tests/golden/generate_holo_golden.py), its Poisson path against the formula
and its three ValueErrors; the physics -- a hologram with a known amplitude and phase ramp reconstructs to them --;
`disk_aperture` and `find_sideband`; the reference wave; the parameter errors; a MemoryDataSet run on the inline
executor; the half-spectrum gather rule of the kernel tests against the same restatement; the names
`libertem.udf.holography` and `libertem.utils.generate` through `libertem_amd.compat`.

The physics test holds the operation to 1e-9 of the object's amplitude on the float64 hologram (the restatement with
its float32 step left out).  The definition takes the frame as float32: that step alone moves the 64 x 48 result by
1.1e-8 relative (measured), so `reconstruct_frames` and the restatement proper are held to the bound derived from it in
the test, 1.8e-6 relative; the two agree with each other to 1e-10 (test_numpy_branch_equals_restatement).
It finds the sideband of a FLAT-phase hologram at +-k.  The hologram with the phase ramp of (2, 1) cycles
per frame has its strongest component at +-(k - (2, 1)): the ramp moves the sideband, and `find_sideband` reports that.
"""
import inspect
import os

import numpy as np
import pytest

import holo_ref as hr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import HoloReconstructUDF, run_holo
from libertem_amd.udf.holography import disk_aperture, find_sideband, reconstruct_frames
from libertem_amd.utils.generate import hologram_frame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'holo_frames.npz')


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.mark.parametrize('with_reference', [False, True], ids=['plain', 'reference'])
@pytest.mark.parametrize('case', hr.CASES, ids=hr.case_id)
def test_numpy_branch_equals_restatement(case, with_reference):
    sig, out_shape, sb = case
    frames = hr.noise_frames(sig, 3, 'float32')
    aperture = hr.aperture_for(case)
    ref_wave = hr.reference_wave_for(case) if with_reference else None
    ref = hr.reference(frames, out_shape, sb, aperture, ref_wave)
    got = reconstruct_frames(frames, out_shape, sb, aperture, ref_wave, dtype=np.complex128)
    assert got.dtype == np.complex128 and got.shape == (3,) + out_shape
    for f in range(3):
        assert np.linalg.norm(got[f] - ref[f]) <= 1e-10 * np.linalg.norm(ref[f]), f
    # the UDF's dtype: the same values, rounded once
    got32 = reconstruct_frames(frames, out_shape, sb, aperture, ref_wave)
    assert got32.dtype == np.complex64 and np.array_equal(got32, got.astype(np.complex64))


@pytest.mark.parametrize('case', hr.CASES, ids=hr.case_id)
def test_gather_rule_of_the_kernel_tests(case):
    # hr.gather on rfft2 spectra, then the plain inverse DFT matrices: the definition again, to float32 accuracy
    sig, out_shape, sb = case
    h, w = sig
    oh, ow = out_shape
    frames = hr.noise_frames(sig, 2, 'float32')
    aperture = hr.aperture_for(case)
    spec = (np.fft.rfft2(frames.astype(np.float64)) / (h * w)).astype(np.complex64)
    g = hr.gather(spec, sig, out_shape, sb, aperture).astype(np.complex128)
    d_y = hr._phases(hr.signed(oh), oh, +1).T
    d_x = hr._phases(hr.signed(ow), ow, +1).T
    ref = hr.reference(frames, out_shape, sb, aperture)
    for f in range(2):
        wave = d_y @ g[f] @ d_x.T
        assert np.linalg.norm(wave - ref[f]) <= 1e-5 * np.linalg.norm(ref[f])


def test_hologram_frame_equals_the_reference():
    gold = np.load(GOLDEN)
    amp, phi = gold['amp'], gold['phi']
    assert np.allclose(hologram_frame(amp, phi), gold['default'], rtol=1e-12, atol=1e-9)
    counts, sampling, visibility, f_angle = gold['params__kwargs']
    got = hologram_frame(amp, phi, counts=counts, sampling=sampling, visibility=visibility, f_angle=f_angle)
    assert np.allclose(got, gold['params'], rtol=1e-12, atol=1e-9)
    counts, sampling, sigma = gold['gauss__kwargs']
    got = hologram_frame(amp, phi, counts=counts, sampling=sampling, gaussian_noise=float(sigma))
    assert np.allclose(got, gold['gauss'], rtol=1e-12, atol=1e-9)
    assert not np.allclose(gold['gauss'], hologram_frame(amp, phi, counts=counts, sampling=sampling))
    # the defaults are those of the reference's signature
    defaults = {k: v.default for k, v in inspect.signature(hologram_frame).parameters.items()}
    assert defaults == {'amp': inspect.Parameter.empty, 'phi': inspect.Parameter.empty, 'counts': 1000.,
                        'sampling': 5., 'visibility': 1., 'f_angle': 30., 'gaussian_noise': None,
                        'poisson_noise': None}


def test_hologram_frame_poisson_path():
    gold = np.load(GOLDEN)
    amp, phi = gold['amp'], gold['phi']
    clean = hologram_frame(amp, phi, counts=400.)
    np.random.seed(7)
    got = hologram_frame(amp, phi, counts=400., poisson_noise=0.01)
    np.random.seed(7)
    scale = 0.01 * 400.
    assert np.array_equal(got, scale * np.random.poisson(clean / scale))
    assert not np.array_equal(got, clean)


def test_hologram_frame_value_errors():
    amp = np.ones((8, 8))
    with pytest.raises(ValueError):
        hologram_frame(amp, np.zeros((8, 9)))
    with pytest.raises(ValueError, match='poisson_noise'):
        hologram_frame(amp, np.zeros((8, 8)), poisson_noise='0.1')
    with pytest.raises(ValueError, match='gaussian_noise'):
        hologram_frame(amp, np.zeros((8, 8)), gaussian_noise=[1.0])


def test_physics():
    h, w = sig = (64, 48)
    oh, ow = out_shape = (16, 12)
    k = (10, 9)
    counts, amp0, vis = 1000., 0.8, 0.5
    sampling, f_angle = hr.carrier_params(sig, k)
    yy, xx = np.mgrid[:h, :w]
    phi = 2 * np.pi * (2 * yy / h + 1 * xx / w) + 0.3
    amp = np.full(sig, amp0)
    holo = hologram_frame(amp, phi, counts=counts, sampling=sampling, visibility=vis, f_angle=f_angle)
    minus_k = ((-k[0]) % h, (-k[1]) % w)
    aperture = disk_aperture(out_shape, 4)
    ii, jj = np.mgrid[:oh, :ow]
    phi_s = 2 * np.pi * (2 * ii / oh + 1 * jj / ow) + 0.3            # phi at (i h / oh, j w / ow)
    expected = counts / 2 * amp0 * vis * np.exp(1j * phi_s)
    scale = counts / 2 * amp0 * vis
    # the operation itself, on the float64 hologram
    exact = hr.reference(holo[None], out_shape, minus_k, aperture, round_input=False)[0]
    rel = np.abs(exact - expected).max() / scale
    print(f"physics: largest |wave - c/2 amp V exp(i phi)| / (c/2 amp V) = {rel:.3e} at -k")
    assert rel <= 1e-9
    conj = hr.reference(holo[None], out_shape, k, aperture, round_input=False)[0]
    assert np.abs(conj - np.conj(expected)).max() <= 1e-9 * scale
    # the definition takes the frame as float32: a residual r with |r| <= eps32 / 2 |y| per pixel reaches a wave pixel
    # through the K non-zero aperture elements, |d wave| <= sqrt(K) |r|_2 / sqrt(h w) <= sqrt(K) eps32 / 2 rms(y)
    quantised = np.sqrt(np.count_nonzero(aperture)) * hr.EPS32 / 2 * np.sqrt((holo ** 2).mean())
    for fn in (lambda sb: reconstruct_frames(holo[None], out_shape, sb, aperture, dtype=np.complex128)[0],
               lambda sb: hr.reference(holo[None], out_shape, sb, aperture)[0]):
        err = np.abs(fn(minus_k) - expected).max()
        print(f"physics: with the frame as float32 {err / scale:.3e}, bound {quantised / scale:.3e}")
        assert err <= quantised
        assert np.abs(fn(k) - np.conj(expected)).max() <= quantised
    # the sideband of the same carrier under a flat phase lies at +-k ...
    flat = hologram_frame(amp, np.full(sig, 0.3), counts=counts, sampling=sampling, visibility=vis, f_angle=f_angle)
    assert find_sideband(flat, half='upper') == k
    assert find_sideband(flat, half='lower') == minus_k
    assert find_sideband(flat) == k
    # ... and the ramp of (2, 1) cycles per frame moves it by that much
    assert find_sideband(holo, half='upper') == (k[0] - 2, k[1] - 1)
    assert find_sideband(holo, half='lower') == (h - k[0] + 2, w - k[1] + 1)


def test_find_sideband_exclusion_and_errors():
    rng = np.random.default_rng(3)
    frame = np.zeros((32, 24))
    yy, xx = np.mgrid[:32, :24]
    frame += 5 * np.cos(2 * np.pi * (1 * yy / 32))                   # strong, inside the default radius min(h, w) / 16
    frame += 1 * np.cos(2 * np.pi * (6 * yy / 32 - 4 * xx / 24))
    frame += 1e-6 * rng.random(frame.shape)
    assert find_sideband(frame) == (6, 20)                           # (6, -4): upper half by its row
    assert find_sideband(frame, half='lower') == (26, 4)
    assert find_sideband(frame, exclude_radius=0.5) == (1, 0)
    with pytest.raises(ValueError, match='half'):
        find_sideband(frame, half='left')
    with pytest.raises(ValueError, match='2D'):
        find_sideband(frame[None])


@pytest.mark.parametrize('shape', [(8, 8), (7, 5), (16, 12), (9, 1), (1, 1)])
def test_disk_aperture(shape):
    a = disk_aperture(shape, 2.5)
    assert a.dtype == np.float32 and a.shape == shape
    sy, sx = hr.signed(shape[0]), hr.signed(shape[1])
    for u in range(shape[0]):
        for v in range(shape[1]):
            assert a[u, v] == (1.0 if np.hypot(sy[u], sx[v]) <= 2.5 else 0.0)
    assert a[0, 0] == 1
    # point symmetry about the centre wherever the mirror frequency exists (not for the Nyquist line of an even axis)
    for u in range(shape[0]):
        for v in range(shape[1]):
            if -sy[u] in sy and -sx[v] in sx:
                assert a[u, v] == a[(-u) % shape[0], (-v) % shape[1]]
    assert np.array_equal(disk_aperture(shape, 0), (np.add.outer(np.abs(sy), np.abs(sx)) == 0).astype(np.float32))
    smooth = disk_aperture(shape, 2.5, 1.0)
    assert smooth.dtype == np.float32 and smooth.shape == shape
    assert np.isclose(smooth.sum(), a.sum(), rtol=1e-5)              # the blur wraps around: nothing is lost
    if min(shape) >= 7:
        assert 0 < smooth[0, 0] < 1 and smooth.max() == smooth[0, 0]


def test_reference_wave_divides():
    case = hr.CASES[4]
    sig, out_shape, sb = case
    frames = hr.noise_frames(sig, 2, 'uint16')
    aperture = hr.aperture_for(case)
    ref_wave = hr.reference_wave_for(case)
    plain = reconstruct_frames(frames, out_shape, sb, aperture, dtype=np.complex128)
    divided = reconstruct_frames(frames, out_shape, sb, aperture, ref_wave, dtype=np.complex128)
    assert np.allclose(divided, plain / ref_wave[None], rtol=1e-14, atol=0)
    # a zero in the reference: Inf / NaN at that pixel only
    ref_wave[2, 3] = 0
    holed = reconstruct_frames(frames, out_shape, sb, aperture, ref_wave)
    assert not np.isfinite(holed[:, 2, 3]).any()
    ok = np.ones(out_shape, bool)
    ok[2, 3] = False
    assert np.isfinite(holed[:, ok]).all()


def test_value_errors(ctx):
    sig = (16, 12)
    ds = ctx.load('memory', data=np.zeros((2, 2) + sig, np.float32), num_partitions=1, sig_dims=2)
    ap = np.ones((8, 6), np.float32)
    with pytest.raises(ValueError, match='sb_size'):
        HoloReconstructUDF((8, 6), (3, 3))
    with pytest.raises(ValueError, match=r'out_shape \(17, 6\)'):
        run_holo(ctx, ds, (17, 6), (3, 3), np.ones((17, 6), np.float32))
    with pytest.raises(ValueError, match=r'out_shape \(8, 13\)'):
        run_holo(ctx, ds, (8, 13), (3, 3), np.ones((8, 13), np.float32))
    with pytest.raises(ValueError, match=r'out_shape \(0, 6\)'):
        run_holo(ctx, ds, (0, 6), (3, 3), np.ones((0, 6), np.float32))
    with pytest.raises(ValueError, match=r'sb_position \(16, 3\)'):
        run_holo(ctx, ds, (8, 6), (16, 3), ap)
    with pytest.raises(ValueError, match=r'sb_position \(3, -1\)'):
        run_holo(ctx, ds, (8, 6), (3, -1), ap)
    with pytest.raises(ValueError, match='two integers'):
        run_holo(ctx, ds, (8, 6), (3.5, 1), ap)
    with pytest.raises(ValueError, match=r'aperture of shape \(8, 5\)'):
        run_holo(ctx, ds, (8, 6), (3, 3), ap[:, :5])
    with pytest.raises(ValueError, match='aperture must be real'):
        run_holo(ctx, ds, (8, 6), (3, 3), ap.astype(np.complex64))
    with pytest.raises(ValueError, match=r'reference_wave of shape \(6, 8\)'):
        run_holo(ctx, ds, (8, 6), (3, 3), ap, reference_wave=np.ones((6, 8), np.complex64))
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D'):
        run_holo(ctx, ds3, (4, 4), (1, 1), np.ones((4, 4), np.float32))


def test_udf_declarations():
    udf = HoloReconstructUDF((6, 9), (16, 10), sb_size=3, sb_smoothness=0.0)
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {'wave': 'disjoint'}
    bufs = udf.get_result_buffers()
    assert {k: (b.kind, np.dtype(b.dtype), b.extra_shape) for k, b in bufs.items()} == {
        'wave': ('nav', np.dtype('complex64'), (6, 9))}
    assert np.array_equal(udf.params.aperture, disk_aperture((6, 9), 3))


def test_hip_signatures():
    from libertem_amd import hip
    assert list(inspect.signature(hip.HoloPlan.__init__).parameters) == [
        'self', 'device', 'sig_h', 'sig_w', 'out_h', 'out_w', 'max_batch', 'sb_y', 'sb_x', 'aperture',
        'reference_wave']
    assert list(inspect.signature(hip.HoloPlan.reconstruct).parameters) == [
        'self', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'out_ptr', 'ld_out', 'stream']
    assert list(inspect.signature(hip.holo_crop).parameters) == [
        'device', 'spec_ptr', 'n_frames', 'h', 'w', 'ld_spec', 'out_h', 'out_w', 'sb_y', 'sb_x', 'aperture_ptr',
        'g_ptr', 'ld_g', 'stream']
    for name in ('ltmi_holo_plan_create', 'ltmi_holo_plan_destroy', 'ltmi_holo_reconstruct',
                 'ltmi_holo_plan_last_kernel', 'ltmi_holo_crop'):
        assert name in hip.EXPORTS
    assert callable(hip.HoloPlan.last_kernel) and callable(hip.HoloPlan.close)


def test_memory_dataset_roi_three_partitions(ctx):
    sig, out_shape, k = (32, 20), (6, 9), (8, 5)
    nav = (3, 4)
    frames = hr.hologram_frames(sig, 12, k, dtype='uint16')
    sb = ((-k[0]) % sig[0], (-k[1]) % sig[1])
    aperture = disk_aperture(out_shape, 2.5, 0.5)
    expected = reconstruct_frames(frames, out_shape, sb, aperture)
    ds = ctx.load('memory', data=frames.reshape(nav + sig), num_partitions=3, sig_dims=2)
    res = run_holo(ctx, ds, out_shape, sb, aperture)
    assert res['wave'].data.shape == nav + out_shape and res['wave'].data.dtype == np.complex64
    assert np.array_equal(np.asarray(res['wave'].data).reshape((12,) + out_shape), expected)
    roi = np.zeros(nav, bool)
    roi[0, 1] = roi[1, 0] = roi[1, 3] = roi[2, 2] = roi[2, 3] = True
    part = run_holo(ctx, ds, out_shape, sb, sb_size=2.5, sb_smoothness=0.5, roi=roi)
    rows = np.flatnonzero(roi.reshape(-1))
    got = np.asarray(part['wave'].raw_data)
    assert got.shape == (5,) + out_shape
    for i, r in enumerate(rows):
        assert np.array_equal(got[i], expected[r]), (i, r)
    # the amplitude of the object: counts / 2 * amp * visibility with amp in [0.5, 0.9]
    assert 0.4 * 1000 < np.abs(expected).mean() < 1.0 * 1000


def test_compat_names():
    import libertem_amd.compat as compat
    from libertem_amd.udf import holography
    from libertem_amd.utils import generate
    was_active = compat._finder is not None
    assert compat.install()
    try:
        import importlib
        assert importlib.import_module('libertem.udf.holography').HoloReconstructUDF is holography.HoloReconstructUDF
        assert importlib.import_module('libertem.utils.generate').hologram_frame is generate.hologram_frame
    finally:
        if not was_active:
            compat.uninstall()


def test_pools_of_the_many_frame_tests():
    # distinct members, and a sideband whose gather reads mirrored columns and the stored Nyquist column
    from correlation_ref import POOL
    (h, w), (oh, ow), (sy, sx) = hr.POOL_CASE
    frames, spec = hr.pool_frames(), hr.pool_spectra()
    assert frames.shape == (POOL, h, w) and frames.dtype == np.uint8
    assert spec.shape == (POOL, h, w // 2 + 1) and spec.dtype == np.complex64
    assert len({m.tobytes() for m in frames}) == POOL and len({m.tobytes() for m in spec}) == POOL
    kx = sorted((sx + int(s)) % w for s in hr.signed(ow))
    assert kx == [4, 5, 6, 7]
    g = hr.gather(spec, (h, w), (oh, ow), (sy, sx), hr.aperture_for(hr.POOL_CASE))
    assert len({m.tobytes() for m in g}) == POOL
    # EXTREMES reach the uint32 frames of the kernel tests
    typed = hr.typed_frames((16, 16), 5, 'uint32')
    assert typed[2].max() == 2 ** 32 - 1 and (typed[2] == 2 ** 31).sum() == 1 and (typed[2] == 2 ** 24 + 1).sum() == 1
