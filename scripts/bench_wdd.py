"""WDDUDF beside SSBUDF on the C2 scan shape: 256 x 256 positions of 256 x 256 uint16 frames resident in HBM (8 GiB), a
bright-field disk of radius 24 pixels around (128, 128), a 64 x 64 window (K = 4096 pixels, of which P = 1789 lie in
the disk).  From one process, with HIP events: `ltmi_ssb_gather` with the window's list, `hip.WDDPlan` creation (the
build of F for all 65 536 Qs: 2 GiB; host clock around a call that ends in a synchronise), `ltmi_wdd_reconstruct`, and
the same for single-sideband (`ltmi_ssb_gather` with the disk's list, `ltmi_ssb_reconstruct`); then the whole jobs
`run_wdd` and `run_ssb` (host clock, plans cached).

Byte model of `ltmi_wdd_reconstruct`, every pass reading and writing HBM once, N = Ny Nx, Nh = Ny (Nx / 2 + 1): per
window pixel 4 N + 4 N (transpose), 4 N + 8 Nh (R2C), 8 Nh + 8 Nh (transpose), 8 N of spectra and 8 N of F in k_wdd_dot.
The filter build moves per Q 8 K (gamma) + 16 K (C2C) + 16 K (wiener) + 16 K (C2C).

    python scripts/bench_wdd.py [--quick] [--check] [--out FILE]
        --quick: a 64 x 64 scan; --check: also the NumPy definition (`reconstruct_window`, float64, one core) from
        the downloaded window pixels, and the device's distance from it; --out: also append the lines to FILE
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.udf import ssb, wdd
from libertem_amd.udf.ssb import run_ssb, wavelength
from libertem_amd.udf.wdd import run_wdd

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SIG = (256, 256)
NAV = (64, 64) if quick else (256, 256)
GEOMETRY = dict(lamb=wavelength(300), dpix=0.2e-10, semiconv=0.022, semiconv_pix=24., cy=128., cx=128.)
WINDOW, EPSILON = 64, 1e-2


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


H, W = SIG
n_frames, n_px = NAV[0] * NAV[1], H * W
g = torch.Generator(device='cuda').manual_seed(7)
frames = torch.empty((n_frames, n_px), dtype=torch.int16, device='cuda')
step = max(1, (1 << 30) // (n_px * 2))
for i in range(0, n_frames, step):
    j = min(n_frames, i + step)
    frames[i:j] = torch.randint(0, 4096, (j - i, n_px), generator=g, device='cuda', dtype=torch.int16)
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=frames.reshape(NAV + SIG), dtype=np.uint16, sig_dims=2, num_partitions=1)
pw = wdd.check_params(SIG, window=WINDOW, epsilon=EPSILON, **GEOMETRY)
ps = ssb.check_params(SIG, cutoff=1, **GEOMETRY)
geom = hip.ssb_geometry(pw['lamb'], (pw['dy'], pw['dx']), pw['semiconv'], pw['semiconv_pix'], pw['cy'], pw['cx'], pw['t'])
win_idx = wdd.window_pixels(SIG, WINDOW, pw['cy'], pw['cx'])
disk_idx = ssb.bf_pixels(SIG, ps['semiconv_pix'], ps['cy'], ps['cx'])
K, P = int(win_idx.size), int(disk_idx.size)
n_half = NAV[0] * (NAV[1] // 2 + 1)
say(f"scan {NAV} of {SIG} uint16 ({frames.numel() * 2 / 2**30:.2f} GiB resident), semiconv_pix 24: P = {P}; window "
    f"{WINDOW} x {WINDOW}: K = {K}, F = {n_frames * K * 8 / 2**30:.2f} GiB, epsilon {EPSILON}")
fourier = torch.empty(NAV, dtype=torch.complex64, device='cuda')


def gathered(idx):
    idx_dev = torch.from_numpy(idx).cuda()
    bf = torch.empty((n_frames, idx.size), dtype=torch.float32, device='cuda')
    ms = t(lambda: hip.ssb_gather(0, frames.data_ptr(), np.uint16, n_frames, n_px, n_px, idx_dev.data_ptr(), idx.size,
                                  bf.data_ptr(), idx.size))
    return bf, ms


# ---- WDD
bf_w, ms = gathered(win_idx)
say(f"WDD ltmi_ssb_gather ({K} window pixels): {ms:.3f} ms")
batch_w = ssb.plan_batch(NAV, K)
build_model = n_frames * K * 56
for what in ("first in the process", "second"):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = hip.WDDPlan(0, NAV[0], NAV[1], pw['window'], batch_w, geom, EPSILON)
    create_ms = (time.perf_counter() - t0) * 1e3
    say(f"WDD plan creation, {what}: {create_ms:.1f} ms (F for {n_frames} Qs, the workspace, the hipFFT plans)  "
        f"filter model {build_model / 2**30:.2f} GiB = {build_model / create_ms / 1e6:.0f} GB/s")
    if what != "second":
        plan.close()
ms_w = t(lambda: plan.reconstruct(bf_w.data_ptr(), K, fourier.data_ptr()))
got_w = fourier.cpu().numpy()
model_w = K * (8 * n_frames + 4 * n_frames + 8 * n_half + 16 * n_half + 16 * n_frames)
say(f"ltmi_wdd_reconstruct batch {batch_w}: {ms_w:.3f} ms  model {model_w / 2**30:.2f} GiB = "
    f"{model_w / ms_w / 1e6:.0f} GB/s ({model_w / ms_w / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}")
plan.close()
# ---- SSB, the same process
bf_s, ms = gathered(disk_idx)
say(f"SSB ltmi_ssb_gather ({P} bright-field pixels): {ms:.3f} ms")
batch_s = ssb.plan_batch(NAV, P)
plan = hip.SSBPlan(0, NAV[0], NAV[1], W, disk_idx, batch_s, geom, 1)
ms_s = t(lambda: plan.reconstruct(bf_s.data_ptr(), P, fourier.data_ptr()))
say(f"ltmi_ssb_reconstruct batch {batch_s}: {ms_s:.3f} ms   {plan.last_kernel()}")
plan.close()
say(f"reconstruct, WDD / SSB: {ms_w / ms_s:.2f} x for {K / P:.2f} x the pixels")
del bf_s
# ---- the whole jobs
j_w = whole_job(lambda: run_wdd(ctx, ds, window=WINDOW, epsilon=EPSILON, **GEOMETRY))
say(f"WDDUDF whole job (run_wdd, bf stays on the device, the plan cached): {j_w:.2f} ms = "
    f"{n_frames / j_w * 1e3:.0f} frames/s")
j_s = whole_job(lambda: run_ssb(ctx, ds, cutoff=1, **GEOMETRY))
say(f"SSBUDF whole job (run_ssb): {j_s:.2f} ms = {n_frames / j_s * 1e3:.0f} frames/s")
if '--check' in sys.argv:
    torch.set_num_threads(1)
    bf_host = bf_w.cpu().numpy()
    t0 = time.perf_counter()
    host = wdd.reconstruct_window(bf_host, NAV, SIG, window=WINDOW, epsilon=EPSILON, **GEOMETRY)
    say(f"reconstruct_window (NumPy, float64, one core) from the downloaded window pixels: "
        f"{time.perf_counter() - t0:.1f} s")
    ref = host['fourier'].astype(np.complex128)
    rest = np.ones(NAV, bool)
    rest[0, 0] = False
    err = np.abs(got_w - ref)
    say(f"device against NumPy: Q != 0 max error {err[rest].max():.3e} = "
        f"{err[rest].max() / np.abs(ref[rest]).max():.2e} of max|fourier[Q != 0]|, DC relative "
        f"{err[0, 0] / abs(ref[0, 0]):.2e}; zeros agree: {bool(np.array_equal(got_w == 0, ref == 0))}")
ctx.close()
