"""
`ltmi_holo_crop` and `ltmi_holo_reconstruct` on the MI355X through hip.holo_crop / hip.HoloPlan (csrc/ltmi_holo.hip).

The gather alone, BIT FOR BIT against the NumPy gather of tests/holo_ref.py (itself checked against the index-free
restatement in tests/test_holo_cpu.py) on random complex64 half spectra -- a conjugation and one float32 multiply per
component leave no rounding freedom.  Frame -> output, sideband, and what the row probes:

    (16,16) -> (8,8),   sb (3,12)    the mirrored half only
    (16,16) -> (8,8),   sb (0,8)     straddles the Nyquist column and row 0
    (15,17) -> (7,5),   sb (14,9)    odd everything, wraps in y
    (16,12) -> (16,12), sb (0,6)     output equal to the frame: every index, both halves
    (32,20) -> (6,9),   sb (16,10)   both Nyquist lines
    (16,16) -> (1,1),   sb (5,0)     a single output element
    (9,8)   -> (9,1),   sb (0,0)     the DC column

with 1 and 5 frames and padded ld_spec / ld_g, NaN around the spectra and poison around the results.

The whole route on the same shapes against the float64 restatement, within the bound of tests/holo_ref.py (C = 8, no
case exempt): uint8, int8, uint16, int16, uint32 (with the ends of its range), float32 and float64 tiles; 1 frame;
5 frames in three batches with a partial last one; a batch larger than the tile; padded ld_tile and ld_out; with and
without a reference wave; guard bytes; bitwise repeats; a NaN pixel; no frames; every error code; the `last_kernel`
string.
"""
import ctypes

import numpy as np
import pytest

import guarded
import holo_ref as hr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


# ---- the gather ---------------------------------------------------------------------------------------------------------
def random_spectra(case, n):
    (h, w), _, _ = case
    rng = np.random.default_rng([5, n] + [int(v) for pair in case for v in pair])
    shape = (n, h, w // 2 + 1)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


class Crop:
    """guarded half spectra, a guarded result and the aperture on the device"""

    def __init__(self, case, n, pad_spec=0, pad_g=0, spec_host=None):
        (h, w), (oh, ow), _ = self.case = case
        self.n = n
        self.spec_host = random_spectra(case, n) if spec_host is None else spec_host
        n_spec = h * (w // 2 + 1)
        self.spec = guarded.Region(n, n_spec, n_spec + pad_spec, np.complex64, init=self.spec_host.reshape((n, n_spec)),
                                   fill='nan')
        self.g = guarded.Region(n, oh * ow, oh * ow + pad_g, np.complex64)
        self.aperture_host = hr.aperture_for(case)
        self.aperture = torch.from_numpy(self.aperture_host.copy()).cuda()

    def run(self, **kw):
        from libertem_amd import hip
        (h, w), (oh, ow), (sy, sx) = self.case
        args = dict(device=0, spec_ptr=self.spec.ptr, n_frames=self.n, h=h, w=w, ld_spec=self.spec.ld, out_h=oh,
                    out_w=ow, sb_y=sy, sb_x=sx, aperture_ptr=self.aperture.data_ptr(), g_ptr=self.g.ptr,
                    ld_g=self.g.ld)
        args.update(kw)
        hip.holo_crop(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.g, 'g')
        guarded.unchanged(self.spec, 'spec')
        return self.g.result().reshape((self.n, oh, ow))


@pytest.mark.parametrize('n,pad_spec,pad_g', [(1, 0, 0), (5, 3, 2), (5, 0, 7)], ids=['1', '5-padded', '5-ld_g'])
@pytest.mark.parametrize('case', hr.CASES, ids=hr.case_id)
def test_crop_bit_for_bit(case, n, pad_spec, pad_g):
    sig, out_shape, sb = case
    call = Crop(case, n, pad_spec, pad_g)
    got = call.run()
    ref = hr.gather(call.spec_host, sig, out_shape, sb, call.aperture_host)
    assert got.dtype == np.complex64
    assert got.tobytes() == ref.tobytes(), np.argwhere(got.view(np.uint64) != ref.view(np.uint64))[:4]
    assert call.run().tobytes() == got.tobytes()


def test_crop_no_frames_and_error_codes():
    case = hr.CASES[4]
    (h, w), (oh, ow), (sy, sx) = case
    empty = Crop(case, 0)
    assert empty.run().shape == (0, oh, ow)
    call = Crop(case, 2)
    n_spec = h * (w // 2 + 1)
    for kw in (dict(out_h=h + 1), dict(out_w=w + 1), dict(out_h=0), dict(sb_y=h), dict(sb_y=-1), dict(sb_x=w),
               dict(sb_x=-1), dict(ld_spec=n_spec - 1), dict(ld_g=oh * ow - 1), dict(n_frames=-1), dict(h=0)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for name in ('spec_ptr', 'aperture_ptr', 'g_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    # nothing of that reached the result, and the call still works
    got = call.run()
    assert got.tobytes() == hr.gather(call.spec_host, (h, w), (oh, ow), (sy, sx), call.aperture_host).tobytes()


# ---- the whole route ----------------------------------------------------------------------------------------------------
class Call:
    """one plan, a guarded tile and a guarded result"""

    def __init__(self, case, frames, max_batch, pad_tile=0, pad_out=0, with_reference=False):
        from libertem_amd import hip
        (h, w), (oh, ow), (sy, sx) = self.case = case
        n = frames.shape[0]
        self.n, self.frames = n, frames
        self.aperture = hr.aperture_for(case)
        self.reference_wave = hr.reference_wave_for(case) if with_reference else None
        self.plan = hip.HoloPlan(0, h, w, oh, ow, max_batch, sy, sx, self.aperture, self.reference_wave)
        fill = 'nan' if frames.dtype.kind == 'f' else 'max'
        self.tile = guarded.Region(n, h * w, h * w + pad_tile, frames.dtype, init=frames.reshape((n, h * w)), fill=fill)
        self.out = guarded.Region(n, oh * ow, oh * ow + pad_out, np.complex64)

    def run(self, **kw):
        args = dict(tile_ptr=self.tile.ptr, tile_dtype=self.frames.dtype, n_frames=self.n, ld_tile=self.tile.ld,
                    out_ptr=self.out.ptr, ld_out=self.out.ld)
        args.update(kw)
        self.plan.reconstruct(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.out, 'wave')
        guarded.unchanged(self.tile, 'tile')
        return self.out.result().reshape((self.n,) + self.case[1])

    def compare(self, got, skip_frames=(), what=''):
        _, out_shape, sb = self.case
        ref = hr.reference(self.frames, out_shape, sb, self.aperture, self.reference_wave)
        return hr.compare(got, ref, self.frames, self.aperture, self.reference_wave, skip_frames, what)


# (tile dtype, frames, max_batch, pad of ld_tile, pad of ld_out, reference wave)
VARIANTS = [
    ('uint8', 5, 2, 3, 0, False),          # three batches, the last one partial; rows that are not 16-byte aligned
    ('uint16', 5, 2, 0, 2, True),
    ('int16', 1, 1, 0, 0, False),
    ('float32', 5, 8, 1, 5, True),         # a batch larger than the tile
    ('float64', 5, 2, 5, 0, False),
    ('float32', 1, 4, 0, 0, True),
    ('uint16', 5, 5, 0, 0, False),         # one full batch, contiguous rows: the vector loads of k_corr_load
    ('int8', 5, 2, 3, 0, False),           # signed bytes, the whole range
    ('uint32', 5, 2, 0, 2, True),          # 2^32 - 1, 2^31, 2^31 + 1 and 2^24 + 1 in frame 2 (holo_ref.typed_frames)
]


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: f"{v[0]}-n{v[1]}-b{v[2]}-ld{v[3]}.{v[4]}{'-ref' if v[5] else ''}")
@pytest.mark.parametrize('case', hr.CASES, ids=hr.case_id)
def test_reconstruct_vs_definition(case, variant):
    dtype, n, max_batch, pad_tile, pad_out, with_reference = variant
    frames = hr.typed_frames(case[0], n, dtype)
    call = Call(case, frames, max_batch, pad_tile, pad_out, with_reference)
    got = call.run()
    call.compare(got, what=f"{hr.case_id(case)} {dtype}")
    kern = call.plan.last_kernel()
    assert kern == f'k_corr_load<{np.dtype(dtype).name}> + hipfft_r2c + k_holo_crop + hipfft_c2c + k_holo_store ' \
                   f'batch={max_batch}'
    # no atomics: a second call gives the same bytes
    assert call.run().tobytes() == got.tobytes()


def test_holograms_reconstruct_to_their_objects():
    # the physics on the device: 32 x 20 uint16 holograms of constant amplitude and a phase ramp, carrier on (8, 5)
    from libertem_amd.udf.holography import disk_aperture
    from libertem_amd.utils.generate import hologram_frame
    from libertem_amd import hip
    h, w = sig = (32, 20)
    oh, ow = out_shape = (8, 10)
    k = (8, 5)
    sampling, f_angle = hr.carrier_params(sig, k)
    yy, xx = np.mgrid[:h, :w]
    ii, jj = np.mgrid[:oh, :ow]
    frames = np.empty((3,) + sig, np.uint16)
    expected = np.empty((3,) + out_shape, np.complex128)
    for f in range(3):
        phi = 2 * np.pi * ((f - 1) * yy / h + xx / w) + 0.5 * f
        frames[f] = np.rint(hologram_frame(np.full(sig, 0.8), phi, counts=40000., sampling=sampling, visibility=0.5,
                                           f_angle=f_angle))
        expected[f] = 20000. * 0.8 * 0.5 * np.exp(1j * (2 * np.pi * ((f - 1) * ii / oh + jj / ow) + 0.5 * f))
    aperture = disk_aperture(out_shape, 3)
    plan = hip.HoloPlan(0, h, w, oh, ow, 2, (-k[0]) % h, (-k[1]) % w, aperture)
    tile = guarded.Region(3, h * w, h * w, np.uint16, init=frames.reshape((3, h * w)), fill='max')
    out = guarded.Region(3, oh * ow, oh * ow, np.complex64)
    plan.reconstruct(tile.ptr, np.uint16, 3, tile.ld, out.ptr, out.ld)
    torch.cuda.synchronize()
    got = out.result().reshape((3,) + out_shape)
    ref = hr.reference(frames, out_shape, ((-k[0]) % h, (-k[1]) % w), aperture)
    hr.compare(got, ref, frames, aperture, what='holograms')
    # rounding to whole counts is white noise of variance 1 / 12 per pixel: sqrt(K / (12 h w)) per wave pixel through the
    # K = 29 aperture elements, 0.06 counts; 1 count is sixteen of those
    assert np.abs(ref - expected).max() < 1.0
    assert np.abs(got - expected).max() < 1.0 + hr.bound(frames, out_shape, aperture).max()


def test_nan_pixel_stays_in_its_frame():
    case = hr.CASES[4]
    frames = hr.noise_frames(case[0], 5, 'float32')
    frames[2, 7, 3] = np.nan
    call = Call(case, frames, 2)                               # (frame 2 shares a batch with frame 3)
    got = call.run()
    assert np.all(np.isfinite(got[[0, 1, 3, 4]]))
    call.compare(got, skip_frames=[2], what='NaN pixel')


def test_no_frames_launches_nothing():
    case = hr.CASES[0]
    call = Call(case, np.zeros((0,) + case[0], np.float32), 4)
    assert call.run().shape == (0,) + case[1]
    assert call.plan.last_kernel() == ''


def test_error_codes():
    from libertem_amd import hip
    case = hr.CASES[4]
    (h, w), (oh, ow), (sy, sx) = case
    frames = hr.noise_frames(case[0], 3, 'uint16')
    call = Call(case, frames, 2)
    for kw in (dict(ld_tile=h * w - 1), dict(ld_out=oh * ow - 1), dict(n_frames=-1)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for dt in (np.complex64, np.uint64):
        with pytest.raises(ValueError, match=r'code -2'):
            call.run(tile_dtype=dt)
    for name in ('tile_ptr', 'out_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    ap = call.aperture
    for args in ((h, w, h + 1, ow, 2, sy, sx), (h, w, oh, w + 1, 2, sy, sx), (h, w, oh, ow, 2, h, sx),
                 (h, w, oh, ow, 2, sy, w), (h, w, oh, ow, 2, -1, sx), (h, w, oh, ow, 2, sy, -1),
                 (h, w, oh, ow, 2 ** 31 // (h * w) + 1, sy, sx)):
        a = np.ones((args[2], args[3]), np.float32)
        with pytest.raises(ValueError, match=r'code -3'):
            hip.HoloPlan(0, *args, a)
    with pytest.raises(ValueError, match=r'code -1'):
        hip.HoloPlan(0, h, w, oh, ow, 0, sy, sx, ap)
    with pytest.raises(ValueError):
        hip.HoloPlan(0, h, w, oh, ow, 2, sy, sx, ap[:, :4])
    with pytest.raises(ValueError):
        hip.HoloPlan(0, h, w, oh, ow, 2, sy, sx, ap, np.ones((oh, ow + 1), np.complex64))
    out = ctypes.c_void_p()
    rc = hip.lib().ltmi_holo_plan_create(0, h, w, oh, ow, 2, sy, sx, None, None, ctypes.byref(out))
    assert rc == -1 and not out.value
    rc = hip.lib().ltmi_holo_plan_create(0, h, w, oh, ow, 2, sy, sx, ap.ctypes.data_as(ctypes.c_void_p), None, None)
    assert rc == -1
    # nothing of that reached the result, and the plan still works
    call.compare(call.run(), what='after the errors')
    # ... and the creates that failed left nothing that keeps a new plan from working
    after = Call(case, frames, 2)
    after.compare(after.run(), what='a plan made after the errors')


# ---- one plan, two streams; plans that go away --------------------------------------------------------------------------
SMALLEST = min(hr.CASES, key=lambda c: c[0][0] * c[0][1])


def test_one_plan_on_two_streams():
    """One plan called on the default stream, on a second stream and on the default stream again, different frames each
    time, one synchronisation at the end (tests/plan_checks.py); the smallest case, 5 frames in batches of 2, so the
    memset of the tail runs too.  Every result is byte for byte what a fresh plan of the same arguments gives for the
    same frames on the default stream."""
    from libertem_amd import hip
    import plan_checks
    (h, w), (oh, ow), (sy, sx) = SMALLEST
    aperture = hr.aperture_for(SMALLEST)
    sets = [hr.noise_frames((h, w), 5, 'uint16', seed=60 + i) for i in range(3)]
    tiles = [torch.from_numpy(s.view(np.int16).reshape(5, h * w)).cuda() for s in sets]

    def run(plan, tile, out, stream):
        plan.reconstruct(tile.data_ptr(), np.uint16, 5, h * w, out.data_ptr(), oh * ow, stream=stream)

    outs = [torch.full((5, oh * ow), np.nan, dtype=torch.complex64, device='cuda') for _ in range(3)]
    plan = hip.HoloPlan(0, h, w, oh, ow, 2, sy, sx, aperture)
    plan_checks.three_calls_on_two_streams(lambda i, stream: run(plan, tiles[i], outs[i], stream))
    plan.close()
    for i in range(3):
        fresh = hip.HoloPlan(0, h, w, oh, ow, 2, sy, sx, aperture)
        ref = torch.full((5, oh * ow), np.nan, dtype=torch.complex64, device='cuda')
        run(fresh, tiles[i], ref, None)
        torch.cuda.synchronize()
        fresh.close()
        assert outs[i].cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), i
        assert np.all(np.isfinite(ref.cpu().numpy()))


HOLO_PLAN_BYTES = 25165824


def test_plans_go_away_completely():
    """64 plans made and closed in a row; free memory after cycle 64 less than ONE live plan below that after cycle 8
    (tests/plan_checks.py).  HOLO_PLAN_BYTES = 25165824 bytes: torch.cuda.mem_get_info() before minus after one
    hip.HoloPlan of SMALLEST with max_batch 2 on the MI355X, measured at the commit before `ltmi::FftHandle` (the
    plans then destroyed their hipFFT handles by hand); a second and a third plan made beside live ones cost the same."""
    from libertem_amd import hip
    import plan_checks
    (h, w), (oh, ow), (sy, sx) = SMALLEST
    aperture = hr.aperture_for(SMALLEST)
    plan_checks.assert_plans_go_away(lambda: hip.HoloPlan(0, h, w, oh, ow, 2, sy, sx, aperture), HOLO_PLAN_BYTES,
                                     'HoloPlan')
