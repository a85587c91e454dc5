"""
`ltmi_ceps_load`, `ltmi_ceps_store` and `ltmi_ceps_transform` on the MI355X through hip.ceps_load / hip.ceps_store /
hip.CepstrumPlan (csrc/ltmi_ceps.hip).  Every case has at most 7 frames.

k_ceps_store alone, BIT FOR BIT against the NumPy float32 model of tests/cepstrum_ref.py (itself checked against the
index-by-index restatement in tests/test_cepstrum_cpu.py) on seeded complex64 half spectra: two multiplies, an add, a
correctly rounded square root and one more multiply leave no rounding freedom.  Frame -> output:

    (16,16) -> (8,8)      even sizes, both halves of the columns
    (15,17) -> (7,5)      odd everything
    (16,12) -> (16,12)    output equal to the frame: every index, both halves, row 0 and both Nyquist lines
    (32,20) -> (6,9)      odd output of an even frame
    (16,16) -> (1,1)      a single element: the origin
    (9,8)   -> (9,1)      one column: the DC column, every row
    (8,9)   -> (8,9)      output equal to the frame, odd width

with 1 and 5 frames, padded ld_spec / ld_out, NaN around the spectra, poison around the results, zeros in `scale`.

k_ceps_load alone, elementwise within 3 eps32 (1 + |z|) |window| of float64 (one add, a logf of 1 ulp, one multiply):
uint8, int16 with negatives, uint16 with both ends of its range, float32, float64; 255 to 1028 pixels (less than one
block, several, a ragged last one), on the four-pixels-per-thread path (n_px and ld_tile multiples of 4, aligned base)
and on the one-pixel path (odd n_px, odd padding, a base off by one element).  The largest ratio seen is printed.

The whole plan on the same shapes against the float64 restatement, within the bound of tests/cepstrum_ref.py: uint16
and float32 tiles; n = 1, n = batch = 3 and n = 2 batch + 1 = 7 (a partial batch and the zeroed tail); padded ld_tile
and ld_out; guard bytes; bitwise repeats; the exact-delta frame; a NaN pixel; no frames; every error code; the
`last_kernel` string; one plan on two streams; plans that go away.
"""
import ctypes

import numpy as np
import pytest

import cepstrum_ref as cr
import guarded

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

EPS32 = cr.EPS32


# ---- k_ceps_store --------------------------------------------------------------------------------------------------------
def random_spectra(case, n):
    (h, w), _ = case
    rng = np.random.default_rng([5, n] + [int(v) for pair in case for v in pair])
    shape = (n, h, w // 2 + 1)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


def scale_for(case):
    """float32 scale without any symmetry, zero inside a radius of 1.5 around the origin and at one more element"""
    (h, w), (oh, ow) = case
    rng = np.random.default_rng([6] + [int(v) for pair in case for v in pair])
    s = rng.uniform(0.25, 1.0, (oh, ow)) * cr.keep((oh, ow), 1.5) / (h * w)
    s[oh - 1, 0] = 0
    return s.astype(np.float32)


class Store:
    """guarded half spectra, a guarded result and the scale on the device"""

    def __init__(self, case, n, pad_spec=0, pad_out=0):
        (h, w), (oh, ow) = self.case = case
        self.n = n
        self.spec_host = random_spectra(case, n)
        n_spec = h * (w // 2 + 1)
        self.spec = guarded.Region(n, n_spec, n_spec + pad_spec, np.complex64, init=self.spec_host.reshape((n, n_spec)),
                                   fill='nan')
        self.out = guarded.Region(n, oh * ow, oh * ow + pad_out, np.float32)
        self.scale_host = scale_for(case)
        self.scale = torch.from_numpy(self.scale_host.copy()).cuda()

    def run(self, **kw):
        from libertem_amd import hip
        (h, w), (oh, ow) = self.case
        args = dict(device=0, spec_ptr=self.spec.ptr, n_frames=self.n, h=h, w=w, ld_spec=self.spec.ld, out_h=oh,
                    out_w=ow, scale_ptr=self.scale.data_ptr(), out_ptr=self.out.ptr, ld_out=self.out.ld)
        args.update(kw)
        hip.ceps_store(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.out, 'out')
        guarded.unchanged(self.spec, 'spec')
        return self.out.result().reshape((self.n, oh, ow))


@pytest.mark.parametrize('n,pad_spec,pad_out', [(1, 0, 0), (5, 3, 2), (5, 0, 7)], ids=['1', '5-padded', '5-ld_out'])
@pytest.mark.parametrize('case', cr.CASES, ids=cr.case_id)
def test_store_bit_for_bit(case, n, pad_spec, pad_out):
    sig, out_shape = case
    call = Store(case, n, pad_spec, pad_out)
    got = call.run()
    ref = cr.store(call.spec_host, sig, out_shape, call.scale_host)
    assert got.dtype == np.float32
    assert got.tobytes() == ref.tobytes(), np.argwhere(got.view(np.uint32) != ref.view(np.uint32))[:4]
    assert np.all(got[:, call.scale_host == 0] == 0) and (call.scale_host == 0).any()
    assert call.run().tobytes() == got.tobytes()


def test_store_no_frames_and_error_codes():
    case = cr.CASES[3]
    (h, w), (oh, ow) = case
    empty = Store(case, 0)
    assert empty.run().shape == (0, oh, ow)
    call = Store(case, 2)
    n_spec = h * (w // 2 + 1)
    for kw in (dict(out_h=h + 1), dict(out_w=w + 1), dict(out_h=0), dict(out_w=-1), dict(ld_spec=n_spec - 1),
               dict(ld_out=oh * ow - 1), dict(n_frames=-1), dict(h=0), dict(w=0)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for name in ('spec_ptr', 'scale_ptr', 'out_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    # nothing of that reached the result, and the call still works
    assert call.run().tobytes() == cr.store(call.spec_host, (h, w), (oh, ow), call.scale_host).tobytes()


# ---- k_ceps_load ---------------------------------------------------------------------------------------------------------
def load_frames(dtype, n, n_px):
    rng = np.random.default_rng([7, n, n_px, np.dtype(dtype).itemsize, ord(np.dtype(dtype).kind)])
    dt = np.dtype(dtype)
    if dt == np.uint8:
        x = rng.integers(0, 255, (n, n_px), endpoint=True)
    elif dt == np.int16:
        x = rng.integers(-3000, 32767, (n, n_px), endpoint=True)
        x[0, :4] = (-32768, -1, 0, 32767)
    elif dt == np.uint16:
        x = rng.integers(0, 65535, (n, n_px), endpoint=True)
        x[0, :4] = (0, 65535, 1, 65534)
    else:
        x = (rng.random((n, n_px)) - 0.3) * 10.0 ** rng.integers(-3, 5, (n, n_px))
        x[0, :3] = (0.0, -0.0, -5.5)
    return x.astype(dt)


LOAD_RATIOS = []


# (pixels, pad of ld_tile, elements the tile's base lies behind a 256-byte boundary); the kernel converts four pixels per
# thread where n_px and ld_tile are multiples of 4 and the base is aligned for it, one otherwise
LOAD_SHAPES = [(255, 0, 0), (320, 3, 0), (600, 1, 0),          # one pixel per thread: odd n_px, odd ld_tile
               (320, 0, 0), (600, 4, 0), (1028, 0, 0),         # four: contiguous, padded by 4, a ragged second block
               (320, 0, 1)]                                    # one again: the base is off by an element


@pytest.mark.parametrize('n_px,pad,shift', LOAD_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('dtype', ['uint8', 'int16', 'uint16', 'float32', 'float64'])
def test_load_elementwise(dtype, n_px, pad, shift):
    from libertem_amd import hip
    n = 5
    frames = load_frames(dtype, n, n_px)
    if np.dtype(dtype).kind == 'i':
        assert (frames < 0).any()
    rng = np.random.default_rng([8, n_px])
    window_host = rng.uniform(-1.0, 1.0, n_px).astype(np.float32)
    window_host[:2] = (0.0, 1.0)
    window = torch.from_numpy(window_host.copy()).cuda()
    fill = 'nan' if frames.dtype.kind == 'f' else 'max'
    tile = guarded.Region(n, n_px, n_px + pad, frames.dtype, shift=shift, init=frames, fill=fill)
    out = guarded.Region(n, n_px, n_px, np.float32)
    worst = 0.0
    for offset in (1.0, 0.37):
        hip.ceps_load(0, tile.ptr, frames.dtype, n, tile.ld, n_px, offset, window.data_ptr(), out.ptr)
        torch.cuda.synchronize()
        guarded.unchanged_outside(out, 'out')
        guarded.unchanged(tile, 'tile')
        got = out.result()
        z = cr.log_frames(frames, offset)
        ref = z * window_host.astype(np.float64)[None]
        tol = EPS32 * (1.0 + np.abs(z)) * np.abs(window_host.astype(np.float64))[None]
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(np.isfinite(got))
        assert np.all(got[:, 0] == 0)                                    # (window 0)
        ratio = float((err[tol > 0] / tol[tol > 0]).max())
        worst = max(worst, ratio)
        print(f"k_ceps_load<{dtype}> {n_px} px offset {offset}: largest |dev - ref| / (eps32 (1 + |z|) |window|) = "
              f"{ratio:.4f} (allowed: 3)")
        assert np.all(err <= 3 * tol), (dtype, offset, ratio)
    LOAD_RATIOS.append(worst)
    print(f"k_ceps_load: largest ratio so far {max(LOAD_RATIOS):.4f}")


def test_load_no_frames_and_error_codes():
    from libertem_amd import hip
    n, n_px = 2, 300
    frames = load_frames('uint16', n, n_px)
    window = torch.ones(n_px, dtype=torch.float32, device='cuda')
    tile = guarded.Region(n, n_px, n_px, np.uint16, init=frames, fill='max')
    out = guarded.Region(n, n_px, n_px, np.float32)
    base = dict(device=0, tile_ptr=tile.ptr, tile_dtype=np.uint16, n_frames=n, ld_tile=n_px, n_px=n_px, offset=1.0,
                window_ptr=window.data_ptr(), out_ptr=out.ptr)

    def run(**kw):
        hip.ceps_load(**{**base, **kw})
        torch.cuda.synchronize()

    run(n_frames=0)
    guarded.unchanged_outside(out, 'out')
    assert out.result().tobytes() == out.view(out.host).tobytes()          # nothing was written
    for kw in (dict(n_frames=-1), dict(n_px=0), dict(ld_tile=n_px - 1)):
        with pytest.raises(ValueError, match=r'code -3'):
            run(**kw)
    for dt in (np.complex64, np.uint64):
        with pytest.raises(ValueError, match=r'code -2'):
            run(tile_dtype=dt)
    for offset in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match=r'offset.*code -1'):
            run(offset=offset)
    for name in ('tile_ptr', 'window_ptr', 'out_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            run(**{name: None})
    assert out.result().tobytes() == out.view(out.host).tobytes()
    run()
    ref = np.log(frames.astype(np.float64) + 1.0)
    assert np.all(np.abs(out.result() - ref) <= 3 * EPS32 * (1 + ref))


# ---- the whole route ----------------------------------------------------------------------------------------------------
OFFSET, DC = 0.75, 1.5


class Call:
    """one plan, a guarded tile and a guarded result"""

    def __init__(self, case, frames, max_batch, pad_tile=0, pad_out=0, offset=OFFSET, window='case', dc_radius=DC):
        from libertem_amd import hip
        (h, w), (oh, ow) = self.case = case
        n = frames.shape[0]
        self.n, self.frames, self.offset, self.dc_radius = n, frames, offset, dc_radius
        self.window = cr.window_for(case) if isinstance(window, str) else window
        self.plan = hip.CepstrumPlan(0, h, w, oh, ow, max_batch, offset, self.window, dc_radius)
        fill = 'nan' if frames.dtype.kind == 'f' else 'max'
        self.tile = guarded.Region(n, h * w, h * w + pad_tile, frames.dtype, init=frames.reshape((n, h * w)), fill=fill)
        self.out = guarded.Region(n, oh * ow, oh * ow + pad_out, np.float32)

    def run(self, **kw):
        args = dict(tile_ptr=self.tile.ptr, tile_dtype=self.frames.dtype, n_frames=self.n, ld_tile=self.tile.ld,
                    out_ptr=self.out.ptr, ld_out=self.out.ld)
        args.update(kw)
        self.plan.transform(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.out, 'cepstrum')
        guarded.unchanged(self.tile, 'tile')
        return self.out.result().reshape((self.n,) + self.case[1])

    def compare(self, got, skip_frames=(), what=''):
        ref = cr.reference(self.frames, self.case[1], self.offset, self.window, self.dc_radius)
        return cr.compare(got, ref, self.frames, self.offset, self.window, skip_frames, what)


BATCH = 3
# (tile dtype, frames, pad of ld_tile, pad of ld_out): one frame; a full batch; two batches and one frame more
VARIANTS = [('uint16', 1, 0, 0), ('uint16', BATCH, 3, 0), ('uint16', 2 * BATCH + 1, 0, 2),
            ('float32', 1, 1, 5), ('float32', BATCH, 0, 0), ('float32', 2 * BATCH + 1, 5, 1)]


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: f"{v[0]}-n{v[1]}-ld{v[2]}.{v[3]}")
@pytest.mark.parametrize('case', cr.CASES, ids=cr.case_id)
def test_transform_vs_definition(case, variant):
    dtype, n, pad_tile, pad_out = variant
    frames = cr.noise_frames(case[0], n, dtype)
    call = Call(case, frames, BATCH, pad_tile, pad_out)
    got = call.run()
    call.compare(got, what=f"{cr.case_id(case)} {dtype} n={n}")
    assert np.all(got[:, cr.keep(case[1], DC) == 0] == 0)
    assert call.plan.last_kernel() == f'k_ceps_load<{np.dtype(dtype).name}> + hipfft_r2c + k_ceps_store batch={BATCH}'
    # no atomics: a second call gives the same bytes
    assert call.run().tobytes() == got.tobytes()


def test_hann_window_by_default_shapes():
    # the window the UDF uses when none is given, on an odd and an even frame
    from libertem_amd.udf.cepstrum import hann_window
    for case in (cr.CASES[1], cr.CASES[3]):
        frames = cr.noise_frames(case[0], 4, 'uint16')
        call = Call(case, frames, BATCH, window=hann_window(case[0]), dc_radius=0.0)
        got = call.run()
        ref = cr.reference(frames, case[1], OFFSET, None, 0.0)
        cr.compare(got, ref, frames, OFFSET, None, what=f"hann {cr.case_id(case)}")


def test_exact_delta_frame():
    frame = cr.delta_frame()[None]
    ones = np.ones((16, 20), np.float32)
    call = Call(((16, 20), (16, 20)), frame, 1, offset=1e-30, window=ones, dc_radius=0.0)
    got = call.run()
    call.compare(got, what='exact delta')
    expected = np.zeros((16, 20))
    expected[8, 10] = 2.0
    expected[8 + 3, 10 + 5] = expected[8 - 3, 10 - 5] = 0.25
    # the closed form holds to 1e-6 in float64 (tests/test_cepstrum_cpu.py); the device adds its bound, in the 2-norm
    assert np.abs(got[0] - expected).max() < 1e-6 + cr.bound(frame, 1e-30, ones)[0]


def test_nan_pixel_stays_in_its_frame():
    case = cr.CASES[3]
    frames = cr.noise_frames(case[0], 3, 'float32')
    clean = Call(case, frames, BATCH).run()
    holed = frames.copy()
    holed[1, 7, 3] = np.nan
    call = Call(case, holed, BATCH)                              # (all three frames share one batch)
    got = call.run()
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()
    call.compare(got, skip_frames=[1], what='NaN pixel')


def test_no_frames_launches_nothing():
    case = cr.CASES[0]
    call = Call(case, np.zeros((0,) + case[0], np.float32), 4)
    assert call.run().shape == (0,) + case[1]
    assert call.plan.last_kernel() == ''


def test_error_codes():
    from libertem_amd import hip
    case = cr.CASES[3]
    (h, w), (oh, ow) = case
    frames = cr.noise_frames(case[0], 3, 'uint16')
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
    win = call.window
    for args in ((h, w, h + 1, ow, 2), (h, w, oh, w + 1, 2), (h, w, 0, ow, 2), (h, w, oh, ow, 2 ** 31 // (h * w) + 1)):
        with pytest.raises(ValueError, match=r'code -3'):
            hip.CepstrumPlan(0, *args, 1.0, win)
    with pytest.raises(ValueError, match=r'code -1'):
        hip.CepstrumPlan(0, h, w, oh, ow, 0, 1.0, win)
    for offset in (0.0, -2.0, np.inf, np.nan, 1e-60):
        with pytest.raises(ValueError, match=r'offset.*code -1'):
            hip.CepstrumPlan(0, h, w, oh, ow, 2, offset, win)
    for dc in (-0.5, np.nan):
        with pytest.raises(ValueError, match=r'dc_radius.*code -1'):
            hip.CepstrumPlan(0, h, w, oh, ow, 2, 1.0, win, dc)
    with pytest.raises(ValueError, match='window of shape'):
        hip.CepstrumPlan(0, h, w, oh, ow, 2, 1.0, win[:, :4])
    out = ctypes.c_void_p()
    rc = hip.lib().ltmi_ceps_plan_create(0, h, w, oh, ow, 2, 1.0, None, 0.0, ctypes.byref(out))
    assert rc == -1 and not out.value
    rc = hip.lib().ltmi_ceps_plan_create(0, h, w, oh, ow, 2, 1.0, win.ctypes.data_as(ctypes.c_void_p), 0.0, None)
    assert rc == -1
    with pytest.raises(ValueError, match=r'null plan.*code -1'):
        hip.check(hip.lib().ltmi_ceps_transform(None, call.tile.ptr, hip.dtype_code(np.uint16), 3, h * w, call.out.ptr,
                                                oh * ow, None), 'ltmi_ceps_transform')
    # nothing of that reached the result, and the plan still works
    call.compare(call.run(), what='after the errors')
    # ... and the creates that failed left nothing that keeps a new plan from working
    after = Call(case, frames, 2)
    after.compare(after.run(), what='a plan made after the errors')


# ---- one plan, two streams; plans that go away --------------------------------------------------------------------------
SMALLEST = min(cr.CASES, key=lambda c: c[0][0] * c[0][1])


def test_one_plan_on_two_streams():
    """One plan called on the default stream, on a second stream and on the default stream again, different frames each
    time, one synchronisation at the end (tests/plan_checks.py); the smallest case, 5 frames in batches of 2, so the
    memset of the tail runs too.  Every result is byte for byte what a fresh plan of the same arguments gives for the
    same frames on the default stream."""
    from libertem_amd import hip
    import plan_checks
    (h, w), (oh, ow) = SMALLEST
    window = cr.window_for(SMALLEST)
    sets = [cr.noise_frames((h, w), 5, 'uint16', seed=60 + i) for i in range(3)]
    tiles = [torch.from_numpy(s.view(np.int16).reshape(5, h * w)).cuda() for s in sets]

    def run(plan, tile, out, stream):
        plan.transform(tile.data_ptr(), np.uint16, 5, h * w, out.data_ptr(), oh * ow, stream=stream)

    outs = [torch.full((5, oh * ow), np.nan, dtype=torch.float32, device='cuda') for _ in range(3)]
    plan = hip.CepstrumPlan(0, h, w, oh, ow, 2, OFFSET, window, DC)
    plan_checks.three_calls_on_two_streams(lambda i, stream: run(plan, tiles[i], outs[i], stream))
    plan.close()
    for i in range(3):
        fresh = hip.CepstrumPlan(0, h, w, oh, ow, 2, OFFSET, window, DC)
        ref = torch.full((5, oh * ow), np.nan, dtype=torch.float32, device='cuda')
        run(fresh, tiles[i], ref, None)
        torch.cuda.synchronize()
        fresh.close()
        assert outs[i].cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), i
        assert np.all(np.isfinite(ref.cpu().numpy()))
        cr.compare(ref.cpu().numpy().reshape((5, oh, ow)), cr.reference(sets[i], (oh, ow), OFFSET, window, DC), sets[i],
                   OFFSET, window, what=f'two streams, set {i}')


# One live plan of SMALLEST with max_batch 2: the workspace is a few KiB, the hipFFT plan dominates.  The footprint of
# the holography plan of a frame of this size (tests/test_holo_kernels_gpu.py: 25165824 bytes, measured) is that of TWO
# hipFFT plans and more workspace: a cepstrum plan holds less, so 56 leaked ones would exceed it many times over.
CEPS_PLAN_BYTES = 25165824


def test_plans_go_away_completely():
    """64 plans made and closed in a row; free memory after cycle 64 less than ONE live plan below that after cycle 8
    (tests/plan_checks.py)."""
    from libertem_amd import hip
    import plan_checks
    (h, w), (oh, ow) = SMALLEST
    window = cr.window_for(SMALLEST)
    plan_checks.assert_plans_go_away(lambda: hip.CepstrumPlan(0, h, w, oh, ow, 2, OFFSET, window, DC), CEPS_PLAN_BYTES,
                                     'CepstrumPlan')
