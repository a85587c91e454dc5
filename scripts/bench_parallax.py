"""ParallaxUDF on the C2 scan shape: 256 x 256 positions of 256 x 256 uint16 frames resident in HBM (8 GiB), made by
`defocused_scan` (a 50 x 50 window around the disk, placed into zero frames on the device; the object is a normal field
low-passed at sigma 0.06 cycles per pixel, so that its features are wider than the shifts), a bright-field disk of
radius 24 pixels around (128, 128), max_shift 8, two iterations.  `ltmi_plx_plan_load`, `ltmi_plx_plan_iterate` and
`ltmi_plx_plan_sum` from HIP events, the whole job through `run_parallax` (host clock around a call that ends in a
synchronise), and beside it, from the same process, `run_ssb` on the same frames (the same gather, one pass over the
spectra).

Byte model, every pass reading and writing HBM once, N = Ny Nx scan positions, Nh = Ny (Nx / 2 + 1), P bright-field
pixels: the load moves per pixel 4 N + 4 N (transpose) and 4 N + 8 Nh (R2C into the store); one iteration reads the
store once for the sum (8 P Nh), and for the correlation reads it again, writes and reads the products (8 P Nh each)
and writes the maps (4 P N), of which the peak search reads the (2 m + 1)^2 window; a sum alone is 8 P Nh.

    python scripts/bench_parallax.py [--quick] [--out FILE]
        --quick: a 64 x 64 scan; --out: also append the lines to FILE
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.corrections.coordinates import rotate_deg
from libertem_amd.udf.parallax import (STORE_LIMIT_BYTES, parallax_aberrations, pixel_offsets, plan_batch,
                                       run_parallax)
from libertem_amd.udf.ssb import bf_pixels, run_ssb, wavelength
from libertem_amd.utils.generate import defocused_scan

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SIG = (256, 256)
NAV = (64, 64) if quick else (256, 256)
SEMICONV_PIX, CY, CX, MAX_SHIFT = 24., 128., 128., 8
ANGLE = 25.
MATRIX = 0.3 * rotate_deg(ANGLE) @ np.array([[1., .1], [.1, .9]])          # shifts up to 7.6 scan pixels
SSB = dict(lamb=wavelength(300), dpix=0.2e-10, semiconv=0.022, semiconv_pix=SEMICONV_PIX, cy=CY, cx=CX, cutoff=1)
WIN, W0 = 50, 103                                                          # the window [103, 153)^2 holds the disk


def say(line):
    print(line, flush=True)
    if out_file:
        with open(out_file, 'a') as f:
            f.write(line + '\n')


def t(fn, reps=10):
    fn(); torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


def whole_job(fn, reps=5):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return np.median(ts) * 1e3


rng = np.random.default_rng(7)
fy, fx = np.fft.fftfreq(NAV[0])[:, None], np.fft.fftfreq(NAV[1])[None, :]
low = np.fft.ifft2(np.fft.fft2(rng.standard_normal(NAV)) * np.exp(-(fy * fy + fx * fx) / (2 * 0.06 ** 2))).real
low -= low.mean()
obj = 1 + 0.4 * low / np.abs(low).max()
crop = defocused_scan(obj, MATRIX, (WIN, WIN), SEMICONV_PIX, CY - W0, CX - W0, counts=1000.)
n_frames, n_px = NAV[0] * NAV[1], SIG[0] * SIG[1]
frames = torch.zeros(NAV + SIG, dtype=torch.int16, device='cuda')
frames[:, :, W0:W0 + WIN, W0:W0 + WIN] = torch.from_numpy(np.rint(crop).astype(np.int16)).cuda()
del crop
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=frames, dtype=np.uint16, sig_dims=2, num_partitions=1)
idx = bf_pixels(SIG, SEMICONV_PIX, CY, CX)
P = int(idx.size)
n_half = NAV[0] * (NAV[1] // 2 + 1)
store = 8 * P * n_half
say(f"scan {NAV} of {SIG} uint16 ({frames.numel() * 2 / 2**30:.2f} GiB resident), semiconv_pix 24: P = {P}, "
    f"max_shift {MAX_SHIFT}, store {store / 2**20:.0f} MiB")
flat = frames.reshape(n_frames, n_px)
idx_dev = torch.from_numpy(idx).cuda()
bf = torch.empty((n_frames, P), dtype=torch.float32, device='cuda')
hip.ssb_gather(0, flat.data_ptr(), np.uint16, n_frames, n_px, n_px, idx_dev.data_ptr(), P, bf.data_ptr(), P)
batch = plan_batch(NAV, P)
plan = hip.ParallaxPlan(0, NAV[0], NAV[1], P, batch, MAX_SHIFT, STORE_LIMIT_BYTES)
load_model = P * (12 * n_frames + 8 * n_half)
ms = t(lambda: plan.load(bf.data_ptr(), P))
say(f"ltmi_plx_plan_load batch {batch}: {ms:.3f} ms  model {load_model / 2**30:.2f} GiB = {load_model / ms / 1e6:.0f} GB/s "
    f"({load_model / ms / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}")
sh = torch.zeros((P, 2), dtype=torch.float64, device='cuda')
half = torch.empty((NAV[0], NAV[1] // 2 + 1), dtype=torch.complex64, device='cuda')
iter_model = 4 * store + 4 * P * n_frames
ms = t(lambda: plan.iterate(sh.data_ptr()))            # (each call starts from the shifts of the one before)
say(f"ltmi_plx_plan_iterate: {ms:.3f} ms  model {iter_model / 2**30:.2f} GiB = {iter_model / ms / 1e6:.0f} GB/s "
    f"({iter_model / ms / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}")
ms = t(lambda: plan.sum(sh.data_ptr(), half.data_ptr()))
say(f"ltmi_plx_plan_sum: {ms:.3f} ms  model {store / 2**30:.2f} GiB = {store / ms / 1e6:.0f} GB/s "
    f"({store / ms / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}")
plan.close()
del bf
job = lambda: run_parallax(ctx, ds, SEMICONV_PIX, CY, CX, max_shift=MAX_SHIFT, iterations=2)      # noqa: E731
j_ms = whole_job(job)
say(f"ParallaxUDF whole job (run_parallax, two iterations, bf stays on the device): {j_ms:.2f} ms = "
    f"{n_frames / j_ms * 1e3:.0f} frames/s")
s_ms = whole_job(lambda: run_ssb(ctx, ds, **SSB))
say(f"SSBUDF whole job (run_ssb) on the same frames: {s_ms:.2f} ms = {n_frames / s_ms * 1e3:.0f} frames/s")
r_ms = whole_job(lambda: run_parallax(ctx, ds, SEMICONV_PIX, CY, CX, max_shift=MAX_SHIFT, iterations=2, regularize=True))
say(f"ParallaxUDF whole job with regularize=True (the shifts fitted on the host after each iteration): {r_ms:.2f} ms")
out = job()
true = pixel_offsets(SIG, idx, CY, CX) @ MATRIX.T
ab = parallax_aberrations(out['matrix'], SSB['dpix'], SSB['semiconv'], SEMICONV_PIX)
say(f"against the generator: largest shift error {np.abs(out['shifts'] - true).max():.3f} scan pixels, matrix error "
    f"{np.abs(out['matrix'] - MATRIX).max():.2e}, rotation {ab['rotation_deg']:.3f} deg (true {ANGLE}), defocus "
    f"{ab['defocus'] * 1e9:.2f} nm, image error {np.abs(out['image'] / 1000. - obj).max():.3f}, bright field "
    f"{np.abs(out['bright_field'] / 1000. - obj).max():.3f}")
ctx.close()
