"""
Kernel-level tests of the hipFFT route of ltmi_crystallinity / ltmi_crystallinity_corrected (csrc/ltmi_fft.hip):
k_fft_prepare or k_fft_prepare_corr, k_fft_repair, hipfftExecR2C and k_abs_dot -- the route of every frame shape the
fused kernels of csrc/ltmi_cryst.hip do not take.  `-m gpu` only.

Reference: float64 `np.fft.rfft2` of the frame times the real-space mask (tests/cryst_ref.py), on frames corrected by
`oracle.corrections.correct` where corrections apply.  Tolerance: |got - ref| <= 1e-5 max|ref| (F32_TOL) unless a test
says otherwise.  Every call's output starts as 7.0, and every test asserts the label 'hipfft_r2c<' of the route.
"""
import functools
import os
import zlib

import numpy as np
import pytest

from cryst_ref import EXTREMES, F32_TOL, SAME_FRAMES_RTOL, _cryst_reference, _cryst_run, cryst_reference_many
from oracle import corrections as oc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROUTE = 'hipfft_r2c<'


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


@pytest.fixture(scope='module')
def plans(hip):
    """plan(h, w, batch): one hip.FFTPlan per shape and batch for the whole module"""
    made = {}

    def plan(h, w, batch):
        key = (h, w, batch)
        if key not in made:
            made[key] = hip.FFTPlan(0, h, w, batch)
        return made[key]
    yield plan
    torch.cuda.synchronize()
    for p in made.values():
        p.close()


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _tables(sig, dark=None, gain=None, coords=None):
    from libertem_amd.io.corrections import CorrectionSet
    kw = {}
    if dark is not None:
        kw['dark'] = np.asarray(dark, dtype=np.float64).reshape(sig)
    if gain is not None:
        kw['gain'] = np.asarray(gain, dtype=np.float64).reshape(sig)
    if coords:
        bad = np.zeros(sig, dtype=bool)
        for c in coords:
            bad[c] = True
        kw['excluded_pixels'] = bad
    return CorrectionSet(**kw).device_tables(0, sig)


def _err(got, ref, scale=None):
    """max |got - ref| / max|ref|, printed by the callers before they assert"""
    scale = np.abs(ref).max() if scale is None else scale
    return float(np.abs(got - ref).max() / scale)


def _ring(sig):
    return min(sig) / 16, min(sig) / 4


# --- 2a: single-pixel frames -- every pixel of the conversion, elementwise -----------------------------------------
SINGLE_VARIANTS = ('plain', 'gain', 'dark+gain', 'dark+gain+excl')


def _excluded(sig, rng):
    h, w = sig
    coords = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1),          # the four corners
              (0, w // 3),                                             # on an edge
              (h // 3, w // 4), (h // 3, w // 4 + 1),                  # an adjacent pair
              (h // 2, w // 2)]                                        # inside the masked disk
    while len(coords) < 12:
        c = (int(rng.integers(2, h - 2)), int(rng.integers(2, w - 2)))
        if abs(c[0] - h // 2) > min(sig) // 8 + 2 and all(max(abs(c[0] - o[0]), abs(c[1] - o[1])) > 2 for o in coords):
            coords.append(c)
    return coords


@functools.lru_cache(maxsize=None)
def _single_pixel_case(sig, variant):
    """frame p = dark + v[p] at pixel p (as int16: exact in uint8, uint16 and float32), its tables' ingredients and the
    float64 reference -- shared by the pixel types, left unchanged"""
    h, w = sig
    n_px = h * w
    rng = np.random.default_rng(_seed('single-pixel', sig, variant))
    v = rng.integers(1, 201, n_px)
    dark = rng.integers(0, 50, n_px).astype(np.float64) if 'dark' in variant else None
    gain = rng.random(n_px) * 0.6 + 0.7 if 'gain' in variant else None
    coords = _excluded(sig, rng) if 'excl' in variant else None
    frames = np.zeros((n_px, n_px), dtype=np.int16)
    frames[np.arange(n_px), np.arange(n_px)] = v
    if dark is not None:
        frames += dark.astype(np.int16)
    assert frames.max() <= 255
    frames = frames.reshape(n_px, h, w)
    real = ((h / 2, w / 2), min(sig) / 8)                              # a disk of zeros in the real-space mask
    corrected = oc.correct(frames.astype(np.float32), sig, dark=dark, gain=gain, coords=coords) \
        if variant != 'plain' else frames
    ref, real_mask, half = cryst_reference_many(corrected.reshape(n_px, h, w), *_ring(sig), real)
    # on the CPU, before any kernel runs: the tolerance hides no frame
    zero = ref == 0
    masked = real_mask.reshape(-1) == 0
    if coords:
        masked[[y * w + x for y, x in coords]] = True                  # (an excluded pixel takes its dark neighbours' 0)
    assert zero.sum() >= 1 and np.all(masked[zero]) and zero.sum() >= (real_mask == 0).sum()
    assert ref[~zero].min() >= 1e-3 * ref.max(), (ref[~zero].min(), ref.max())
    for a in (frames, ref, real_mask, half):
        a.setflags(write=False)
    return frames, dark, gain, coords, ref, real_mask, half


@pytest.mark.parametrize('variant', SINGLE_VARIANTS)
@pytest.mark.parametrize('sig,dtype', [((33, 31), 'uint16'), ((33, 31), 'float32'),
                                       ((24, 40), 'uint16'), ((24, 40), 'float32'), ((24, 40), 'uint8'),
                                       ((40, 52), 'uint16'), ((40, 52), 'float32')])
def test_single_pixel_frames_every_pixel_of_the_conversion(hip, plans, sig, dtype, variant):
    """One frame per pixel p, zero but for v[p] there (on top of an integer dark frame): |F| = |v'| in every bin, so
    out[p] depends on exactly one load, one gain[p] and one real_mask[p].  33 x 31: n_px = 1023, the scalar tail alone;
    24 x 40: the vector path; 40 x 52: n_px = 2080, a second block of k_fft_prepare_corr with 4 live threads.  With
    dead pixels a hot neighbour also lights the patched pixel: compared with the float64 reference, not the closed
    form.  Frames whose pixel is masked out or patched from dark neighbours are exactly 0."""
    frames, dark, gain, coords, ref, real_mask, half = _single_pixel_case(sig, variant)
    h, w = sig
    tables = None if variant == 'plain' else _tables(sig, dark, gain, coords)
    got, label = _cryst_run(hip, frames.astype(dtype), real_mask, half, tables=tables, plan=plans(h, w, 512))
    assert label.startswith(ROUTE + dtype), label
    print(f'single-pixel {sig} {dtype} {variant}: max err {_err(got, ref):.3g} of max|ref|')
    bad = np.flatnonzero(np.abs(got - ref) > F32_TOL * ref.max())
    assert len(bad) == 0, (bad[:10], got[bad[:10]], ref[bad[:10]])
    assert np.all(got[ref == 0] == 0)


# --- 2b: all pixel types, both prepare branches ----------------------------------------------------------------------
ALL_DTYPES = ['bool', 'uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32', 'float64']


def _typed_frames(dtype, corrected):
    sig = (40, 48)
    dt = np.dtype(dtype)
    rng = np.random.default_rng(_seed('all-types', dtype, corrected))
    n = 33
    if dt.kind == 'b':
        frames = rng.random((n,) + sig) < 0.3
    elif dt.kind == 'f':
        frames = (rng.normal(size=(n,) + sig) * 100).astype(dt)
    else:
        info = np.iinfo(dt)
        frames = rng.integers(max(info.min, -4000), min(info.max, 4000), size=(n,) + sig, endpoint=True).astype(dt)
    frames[0, 10:20, 30:40] = 1 if dt.kind == 'b' else 100              # structure on top of the noise
    extreme = None
    if dtype in EXTREMES and n > 2:
        extreme = 2
        frames[2].reshape(-1)[[0, 7, 8, 333, 959, 960, 1911, 1919]] = np.array(EXTREMES[dtype]).astype(dt)
    dark = gain = None
    if corrected:
        dark = rng.integers(0, 2 if dt.kind == 'b' else 50, sig).astype(np.float64)
        gain = rng.random(sig) * 0.6 + 0.7
        frames[1] = dark.astype(dt)                                    # corrects to exactly 0
    else:
        frames[1] = 0
    return frames, dark, gain, extreme


@pytest.mark.parametrize('corrected', [False, True], ids=['plain', 'corrected'])
@pytest.mark.parametrize('dtype', ALL_DTYPES)
def test_all_pixel_types_alignments_and_frame_counts(hip, plans, dtype, corrected):
    """40 x 48 noise frames of every pixel type, one structured, one that is (or corrects to) exactly 0, and for the
    32-bit integers and float64 one with values at the type's extremes / of more than 24 significant bits (reference:
    the float32 value of the pixel, the documented conversion).  Aligned rows take the vector branch of k_fft_prepare
    -- with dark and gain k_fft_prepare_corr --, a padded stride (ld = n_px + 1) and a tile pointer one element past
    an aligned address the scalar branch; float64 always the scalar one.  1, 15, 17 and 33 frames in batches of 16 and
    64 straddle the 16-frame blocks of k_fft_prepare_corr and end in a short batch.  The three layouts convert the same
    frames: they agree to 2e-6."""
    sig = (40, 48)
    frames, dark, gain, extreme = _typed_frames(dtype, corrected)
    real = ((17.5, 30), 6.5)
    if corrected:
        conv = oc.correct(frames, sig, dark=dark, gain=gain)
        tables = _tables(sig, dark, gain)
    else:
        conv = frames.astype(np.float32) if np.dtype(dtype).kind in 'iub' else frames
        tables = None
    ref, real_mask, half = _cryst_reference(conv, *_ring(sig), real)
    assert ref[1] == 0
    normal = np.ones(len(ref), dtype=bool)
    if extreme is not None:
        normal[extreme] = False
        assert abs(ref[extreme]) > 100 * np.abs(ref[normal]).max()       # (it would set the scale of every other frame)
    itemsize = np.dtype(dtype).itemsize
    worst = 0.0
    for batch in (16, 64):
        for n in (1, 15, 17, 33):
            res = {}
            for layout, kw in (('aligned', {}), ('padded', dict(ld_pad=1)), ('offset', dict(offset_bytes=itemsize))):
                got, label = _cryst_run(hip, frames[:n], real_mask, half, tables=tables, plan=plans(40, 48, batch), **kw)
                assert label == f'hipfft_r2c<{dtype}> batch={batch}', label
                res[layout] = got
                # each frame against the largest reference of its own kind: the extreme frame is ~10^6 times the others
                scale = np.where(normal[:n], np.abs(ref[:n][normal[:n]]).max(), np.abs(ref[:n]))
                err = np.abs(got - ref[:n]) / scale
                worst = max(worst, float(err.max()))
                assert np.all(err <= F32_TOL), (layout, batch, n, got, ref[:n])
                if n > 1:
                    assert got[1] == 0
            for layout in ('padded', 'offset'):
                assert np.allclose(res[layout], res['aligned'], rtol=SAME_FRAMES_RTOL, atol=0), (layout, batch, n)
    print(f'all-types {dtype} corrected={corrected}: max err {worst:.3g}')


# --- 2c: shapes ---------------------------------------------------------------------------------------------------------
SHAPES = [(96, 96), (128, 256), (256, 128), (255, 256), (256, 257), (130, 100), (67, 131)]


def _shape_frames(sig, dtype):
    rng = np.random.default_rng(_seed('shapes', sig, dtype))
    n = 9
    if dtype == 'uint16':
        frames = rng.integers(0, 4096, size=(n,) + sig).astype(np.uint16)
    else:
        frames = (rng.normal(size=(n,) + sig) * 100).astype(np.float32)
    frames[4, sig[0] // 3:sig[0] // 3 + 10, sig[1] // 2:sig[1] // 2 + 10] += 17
    return frames


def _yardstick(frames, real_mask, half, ref):
    """the error of a float32 CPU transform (torch.fft.rfft2) of the same masked frames against the float64 reference"""
    fr = frames.astype(np.float32)
    if real_mask is not None:
        fr = fr * real_mask.astype(np.float32)
    spec = torch.fft.rfft2(torch.from_numpy(np.ascontiguousarray(fr)))
    cpu32 = (spec.abs() * torch.from_numpy(half.astype(np.float32))).sum(dim=(1, 2)).numpy()
    return _err(cpu32, ref)


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('sig', SHAPES)
def test_frame_shapes_off_the_fused_path(hip, sig, dtype, masked):
    """Square, rectangular, odd, one-off-a-power-of-two and prime-edged frames; 9 frames in batches of 4: three
    batches, the last with one frame.  1e-5 of max|ref| holds at every shape, (67, 131) with both edges prime
    included: measured there 1.3e-7 ... 2.0e-7 of max|ref| (the other shapes 5e-8 ... 1.5e-7), where the yardstick a
    wider bound would have had to come from -- the float32 CPU transform (torch.fft.rfft2) of the same masked frames
    against the float64 reference, printed next to the measured error -- is 1.5e-7 ... 2.7e-7.  No other bound is
    needed."""
    frames = _shape_frames(sig, dtype)
    h, w = sig
    real = ((h / 2 + 1, w / 2 - 2), min(sig) / 10) if masked else None
    ref, real_mask, half = _cryst_reference(frames, *_ring(sig), real)
    got, label = _cryst_run(hip, frames, real_mask, half, batch=4)
    assert label == f'hipfft_r2c<{dtype}> batch=4', label
    print(f'shape {sig} {dtype} masked={masked}: max err {_err(got, ref):.3g} of max|ref|, '
          f'float32 CPU transform {_yardstick(frames, real_mask, half, ref):.3g}')
    assert np.all(np.abs(got - ref) <= F32_TOL * np.abs(ref).max()), (got, ref)


@pytest.mark.parametrize('sig', [(24, 40), (96, 200)])
def test_ring_that_covers_every_row(hip, sig):
    """rad_out >= h / 2: every row of the half spectrum is in the ring's bounding box, which mask_box states as
    (h, h, n_cols) -- k_abs_dot's prefix is all there is."""
    from libertem_amd.udf.crystallinity import mask_box
    h, w = sig
    for dtype in ('uint16', 'float32'):
        frames = _shape_frames(sig, dtype)
        ref, real_mask, half = _cryst_reference(frames, h / 8, h / 2 + 2, ((h / 2, w / 2), h / 6))
        assert mask_box(half)[:2] == (h, h) and mask_box(half)[2] <= w // 2 + 1, mask_box(half)
        got, label = _cryst_run(hip, frames, real_mask, half, batch=4)
        assert label == f'hipfft_r2c<{dtype}> batch=4', label
        print(f'every-row ring {sig} {dtype}: box {mask_box(half)}, max err {_err(got, ref):.3g}')
        assert np.all(np.abs(got - ref) <= F32_TOL * np.abs(ref).max()), (got, ref)


# --- 2d: every bin of the box ------------------------------------------------------------------------------------------
def test_every_bin_of_the_box(hip):
    """Frames that are single plane waves cos(2 pi (ky y / h + kx x / w)) on 48 x 80: h w / 2 in the half-spectrum bin
    (ky, kx) (h w at the self-conjugate bins; with kx = 0 also in (h - ky, 0)) -- each probes whether ONE bin is inside
    the sum.  The probes straddle the box's row_lo, row_hi and n_cols, the ring's inner edge, row 0, row h - 1 and
    column 0."""
    from libertem_amd.udf.crystallinity import crystallinity_masks, mask_box
    h, w = 48, 80
    rad_in, rad_out = 5, 14
    _, half0 = crystallinity_masks((h, w), rad_in, rad_out, None, None)
    row_lo, row_hi, n_cols = mask_box(half0)
    assert 0 < row_lo < row_hi < h and n_cols < w // 2 + 1, (row_lo, row_hi, n_cols)
    waves = [(row_lo - 1, 0), (row_lo, 0), (row_lo - 1, 1), (row_lo, 1),            # the prefix's last row and beyond
             (row_hi - 1, 1), (row_hi, 1), (row_hi, 0), (row_hi + 1, 3),            # the suffix's first row and before
             (0, n_cols - 1), (0, n_cols), (1, n_cols - 1), (h - 1, n_cols - 1),    # the last column and beyond
             (0, rad_in + 1), (0, rad_in), (rad_in + 1, 0), (rad_in, 0), (3, 4), (4, 4), (h - 3, 4), (h - 4, 4),
             (0, 0), (h - 1, 6), (h - 1, 1), (0, 9), (h - 9, 0), (9, 9), (h - 9, 9),
             (h // 2, w // 2), (h // 2, 0), (0, w // 2), (h - 11, 8), (20, 30)]
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.stack([np.cos(2 * np.pi * (ky * yy / h + kx * xx / w)) for ky, kx in waves]).astype(np.float32)
    ref, _, half = _cryst_reference(frames, rad_in, rad_out, None)
    inside = ref > h * w / 4
    assert inside.sum() >= 5 and (~inside).sum() >= 4
    # ... and on both sides of each edge
    state = dict(zip(waves, inside))
    assert state[(row_lo - 1, 0)] and not state[(row_lo, 1)] and state[(row_hi, 0)] and not state[(row_hi - 1, 1)]
    assert state[(0, n_cols - 1)] and not state[(0, n_cols)]
    assert state[(0, rad_in + 1)] and not state[(0, rad_in)] and state[(h - 4, 4)] and not state[(h - 3, 4)]
    assert state[(h - 1, 6)] and not state[(h - 1, 1)] and not state[(0, 0)]
    got, label = _cryst_run(hip, frames, None, half)
    assert label.startswith(ROUTE), label
    print(f'every bin: box {(row_lo, row_hi, n_cols)}, {inside.sum()} probes inside, max err '
          f'{np.abs(got - ref).max():.3g} of a peak of {h * w / 2}')
    assert np.allclose(got, ref, rtol=1e-5, atol=h * w * 1e-4), (got, ref)     # float32 round-off of the empty bins


# --- 2e: accumulate, non-finite pixels, two streams ---------------------------------------------------------------------
def test_accumulate_onto_a_base(hip):
    """accumulate=1 with a padded stride and a short last batch: out = base + the sum"""
    rng = np.random.default_rng(_seed('fft-accumulate'))
    frames = rng.integers(0, 4096, size=(21, 40, 48)).astype(np.uint16)
    ref, real_mask, half = _cryst_reference(frames, *_ring((40, 48)), ((20, 24), 5))
    got, label = _cryst_run(hip, frames, real_mask, half, ld_pad=8, batch=8)
    assert label == 'hipfft_r2c<uint16> batch=8', label
    assert np.all(np.abs(got - ref) <= F32_TOL * np.abs(ref).max())
    base = rng.normal(size=21).astype(np.float32) * 1e6
    got2, label2 = _cryst_run(hip, frames, real_mask, half, accumulate_into=base, ld_pad=8, batch=8)
    assert label2 == label
    assert np.allclose(got2, base + got, rtol=1e-6)


@pytest.mark.parametrize('sig', [(40, 48), (33, 31)])
def test_non_finite_pixels_stay_in_their_frame(hip, plans, sig):
    """A NaN pixel in one frame of a batch of 8 and an Inf pixel in another: those two results are non-finite (NaN for
    the NaN), the other six are right.  A NaN under a zero of the real-space mask is still NaN, as NaN * 0 is in the
    reference.  A short batch through the same plan afterwards -- the workspace behind its frames last held the NaN
    frame -- is right as well."""
    h, w = sig
    rng = np.random.default_rng(_seed('fft-nonfinite', sig))
    clean = (rng.normal(size=(8, h, w)) * 100).astype(np.float32)
    real = ((h / 2, w / 2), 4)
    ref, real_mask, half = _cryst_reference(clean, *_ring(sig), real)
    assert real_mask[h // 2, w // 2] == 0 and real_mask[2, 3] == 1
    plan = plans(h, w, 8)
    others = np.array([0, 1, 3, 4, 6, 7])
    with np.errstate(all='ignore'):
        for nan_at in ((2, 3), (h // 2, w // 2)):                      # an open pixel; a pixel the mask zeroes
            frames = clean.copy()
            frames[2][nan_at] = np.nan
            frames[5, h - 1, w - 1] = np.inf
            frames[7, 0, 0] = np.nan                                   # (the last slot of the plan's workspace)
            ref_nf = _cryst_reference(frames, *_ring(sig), real)[0]
            assert np.isnan(ref_nf[2]) and np.isnan(ref_nf[7]) and not np.isfinite(ref_nf[5])
            got, label = _cryst_run(hip, frames, real_mask, half, plan=plan)
            assert label == 'hipfft_r2c<float32> batch=8', label
            assert np.isnan(got[2]) and np.isnan(got[7]) and not np.isfinite(got[5]), got
            o = others[others != 7]
            assert np.all(np.isfinite(got[o]))
            assert np.all(np.abs(got[o] - ref[o]) <= F32_TOL * np.abs(ref).max()), (got, ref)
            got3, label3 = _cryst_run(hip, clean[:3], real_mask, half, plan=plan)      # 3 of 8: a short batch
            assert label3 == label
            assert np.all(np.abs(got3 - ref[:3]) <= F32_TOL * np.abs(ref).max()), (got3, ref[:3])


def test_one_plan_on_two_streams(hip, plans):
    """One plan called on the default stream, on a second stream and on the default stream again, different frames each
    time, one synchronisation at the end: the transform follows the stream of its call.  (Each stream is kept busy
    before its call, so a transform left on the other stream would run ahead of its input.)"""
    sig = (40, 48)
    rng = np.random.default_rng(_seed('fft-streams'))
    sets = [rng.integers(0, 4096, size=(8, 40, 48)).astype(np.uint16) for _ in range(3)]
    refs = [_cryst_reference(fr, *_ring(sig), None) for fr in sets]
    half = refs[0][2]
    plan = plans(40, 48, 8)
    default = torch.cuda.current_stream()
    second = torch.cuda.Stream()
    a = torch.ones((4096, 4096), device='cuda')
    busy = {None: torch.empty_like(a), second: torch.empty_like(a)}
    keep = []
    results = []
    for i, stream in enumerate((None, second, None)):
        with torch.cuda.stream(second if stream is not None else default):
            for _ in range(4):
                torch.mm(a, a, out=busy[stream])                         # this call's stream is busy for a while
        if stream is None:
            default.wait_stream(second)                                  # (the plan's workspace is one: calls in order)
        out, label, alive = _cryst_run(hip, sets[i], None, half, plan=plan, stream=stream, sync=False)
        assert label == 'hipfft_r2c<uint16> batch=8', label
        keep.append(alive)
        results.append(out)
    torch.cuda.synchronize()
    for out, (ref, _, _) in zip(results, refs):
        got = out.cpu().numpy()
        assert np.all(np.abs(got - ref) <= F32_TOL * np.abs(ref).max()), (got, ref)


FFT_PLAN_BYTES = 16777216


def test_plans_go_away_completely(hip):
    """64 plans made and closed in a row; free memory after cycle 64 less than ONE live plan below that after cycle 8
    (tests/plan_checks.py).  FFT_PLAN_BYTES = 16777216 bytes: torch.cuda.mem_get_info() before minus after one
    `hip.FFTPlan(0, 40, 48, 8)` on the MI355X, measured at the commit before `ltmi::FftHandle` (the
    plans then destroyed their hipFFT handles by hand); a second and a third plan made beside live ones cost the same.
    (40 x 48 is off the fused path: the plan holds its hipFFT handle and both workspaces from the start.)"""
    import plan_checks
    plan_checks.assert_plans_go_away(lambda: hip.FFTPlan(0, 40, 48, 8), FFT_PLAN_BYTES, 'FFTPlan')


# --- 2f: the switch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sig', [128, 256])
def test_switch_keeps_fused_shapes_on_hipfft(hip, sig):
    """LTMI_FFT_FUSED=0 at plan creation: the shapes of the fused kernels through hipFFT -- an independent check of
    those kernels.  Both routes within 1e-5 of the float64 reference and within 2e-5 of max|ref| of each other."""
    shape = (sig, sig)
    before = os.environ.get('LTMI_FFT_FUSED')
    os.environ['LTMI_FFT_FUSED'] = '0'
    try:
        plan_fft = hip.FFTPlan(0, sig, sig, 4)
    finally:
        if before is None:
            del os.environ['LTMI_FFT_FUSED']
        else:
            os.environ['LTMI_FFT_FUSED'] = before
    plan_fused = hip.FFTPlan(0, sig, sig, 4)
    try:
        rng = np.random.default_rng(_seed('fft-switch', sig))
        n = 9
        real = ((sig / 2, sig / 2), sig / 10)
        u16 = rng.integers(0, 4096, size=(n,) + shape).astype(np.uint16)
        f32 = (rng.normal(size=(n,) + shape) * 100).astype(np.float32)
        dark = rng.random(shape) * 6
        gain = rng.random(shape) * 0.6 + 0.7
        coords = [(0, 0), (sig - 1, sig - 1), (10, 40), (10, 41), (sig // 2, sig // 2)]
        cases = [('uint16', u16, u16, real, None),
                 ('float32', f32, f32, None, None),
                 ('uint16', u16, oc.correct(u16, shape, dark=dark, gain=gain, coords=coords), real,
                  _tables(shape, dark, gain, coords))]
        for dtype, frames, conv, rl, tables in cases:
            ref, real_mask, half = _cryst_reference(conv, *_ring(shape), rl)
            tol = F32_TOL * np.abs(ref).max()
            got_fft, label = _cryst_run(hip, frames, real_mask, half, tables=tables, plan=plan_fft)
            assert label == f'hipfft_r2c<{dtype}> batch=4', label
            got_fused, label_fused = _cryst_run(hip, frames, real_mask, half, tables=tables, plan=plan_fused)
            assert label_fused.startswith('k_cryst_'), label_fused
            assert ('corrected' in label_fused) == (tables is not None), label_fused
            print(f'switch {sig} {dtype} corrected={tables is not None}: hipFFT {_err(got_fft, ref):.3g}, '
                  f'{label_fused.split("<")[0]} {_err(got_fused, ref):.3g}, apart {_err(got_fft, got_fused, np.abs(ref).max()):.3g}')
            assert np.all(np.abs(got_fft - ref) <= tol), (got_fft, ref)
            assert np.all(np.abs(got_fused - ref) <= tol), (got_fused, ref)
            assert np.all(np.abs(got_fft - got_fused) <= 2 * tol)
    finally:
        torch.cuda.synchronize()
        plan_fft.close()
        plan_fused.close()


# --- 2g: argument errors of this entry point ------------------------------------------------------------------------------
def test_argument_errors_leave_the_output_alone(hip, plans):
    from libertem_amd.udf.crystallinity import mask_box
    h, w = 24, 40
    wc = w // 2 + 1
    plan = plans(h, w, 4)
    rng = np.random.default_rng(_seed('fft-errors'))
    frames = rng.integers(0, 4096, size=(3, h, w)).astype(np.uint16)
    ref, _, half = _cryst_reference(frames, *_ring((h, w)), None)
    t = torch.from_numpy(frames.view(np.int16)).cuda()
    hm = torch.from_numpy(np.ascontiguousarray(half.astype(np.float32))).cuda()
    out = torch.full((3,), 7.0, dtype=torch.float32, device='cuda')
    box = mask_box(half)
    tables = _tables((h, w), gain=np.ones((h, w)), coords=[(3, 3)])

    def call(dtype=np.uint16, n=3, ld=h * w, box=box):
        plan.crystallinity(t.data_ptr(), dtype, n, ld, None, hm.data_ptr(), box, out.data_ptr(), False)

    for kw, code, text in ((dict(box=(2, h + 1, 5)), -3, 'bad mask bounding box'),          # row_hi > h
                           (dict(box=(2, h - 2, wc + 1)), -3, 'bad mask bounding box'),      # n_cols > wc
                           (dict(box=(5, 4, 5)), -3, 'bad mask bounding box'),               # row_hi < row_lo
                           (dict(box=(-1, 4, 5)), -3, 'bad mask bounding box'),
                           (dict(ld=h * w - 1), -3, 'ld_tile < frame size'),
                           (dict(n=-1), -3, 'negative frame count'),
                           (dict(dtype=np.complex64), -2, 'unsupported tile dtype complex64')):
        with pytest.raises(ValueError, match=text) as e:
            call(**kw)
        assert f'(code {code})' in str(e.value), str(e.value)
    for missing in ('excl', 'env', 'cnt'):                                # n_excl > 0 with a null table
        broken = dict(tables)
        broken[missing] = None
        with pytest.raises(ValueError, match='bad repair tables') as e:
            plan.crystallinity_corrected(t.data_ptr(), np.uint16, 3, h * w, broken, None, hm.data_ptr(), box,
                                         out.data_ptr(), False)
        assert '(code -1)' in str(e.value), str(e.value)
    with pytest.raises(ValueError, match='null pointer') as e:
        plan.crystallinity(0, np.uint16, 3, h * w, None, hm.data_ptr(), box, out.data_ptr(), False)
    assert '(code -1)' in str(e.value), str(e.value)
    call(n=0)                                                             # an empty tile: OK, nothing written
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 7.0)
    call()
    torch.cuda.synchronize()
    assert plan.last_kernel() == 'hipfft_r2c<uint16> batch=4', plan.last_kernel()
    got = out.cpu().numpy()
    assert np.all(np.abs(got - ref) <= F32_TOL * np.abs(ref).max()), (got, ref)


# --- 3: more frames in a batch than the grid's y extent holds --------------------------------------------------------------
@pytest.mark.parametrize('corrected', [False, True], ids=['plain', 'gain'])
def test_more_frames_in_a_batch_than_grid_rows(hip, corrected):
    """70 000 frames of 8 x 8 uint8 in ONE batch: the frame count of a batch is the plan's max_batch, which nothing
    bounds (CrystallinityUDF sizes it from 2 GiB of workspace), and the prepare kernels index frames by the grid's y
    extent, which the device limits to 65 535: they walk the frames beyond it.  Every frame against the reference."""
    n, sig = 70000, (8, 8)
    rng = np.random.default_rng(_seed('fft-many-frames'))
    frames = rng.integers(0, 256, size=(n,) + sig).astype(np.uint8)
    frames[n - 1] = 0
    frames[65535, 3, 4] = 255
    gain = rng.random(sig) * 0.6 + 0.7 if corrected else None
    conv = oc.correct(frames, sig, gain=gain) if corrected else frames
    ref, real_mask, half = cryst_reference_many(conv, 1, 3, ((4, 4), 1))
    for kw in (dict(), dict(ld_pad=1)):                    # with gain: k_fft_prepare_corr, then k_fft_prepare
        got, label = _cryst_run(hip, frames, real_mask, half, batch=n, tables=_tables(sig, gain=gain) if corrected else None,
                                **kw)
        assert label == f'hipfft_r2c<uint8> batch={n}', label
        bad = np.flatnonzero(np.abs(got - ref) > F32_TOL * np.abs(ref).max())
        print(f'70 000 frames corrected={corrected} {kw}: max err {_err(got, ref):.3g}, {len(bad)} frames off')
        assert len(bad) == 0, (bad[:10], got[bad[:10]], ref[bad[:10]])
        assert got[n - 1] == 0
