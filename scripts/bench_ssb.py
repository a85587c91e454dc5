"""SSBUDF on the C2 scan shape: 256 x 256 positions of 256 x 256 uint16 frames resident in HBM (8 GiB), a bright-field
disk of radius 24 pixels around (128, 128) (P = 1789 pixels in 47 detector rows).  `ltmi_ssb_gather` over the whole scan and
`ltmi_ssb_reconstruct` from HIP events, the whole job through `run_ssb` (host clock around a call that ends in a
synchronise), and beside them, from the same process: the NumPy branch (`reconstruct_bf`) on one core from the
downloaded bright-field pixels, and ApplyMasksUDF with the 16 dense float32 masks of bench.py's C2 as the cost of one
full read of those frames.

Byte model, every pass reading and writing HBM once, N = Ny Nx scan positions, Nh = Ny (Nx / 2 + 1), P bright-field
pixels: the gather reads the detector rows that cross the disk (2 r + 1 of h rows: whole 128-byte lines) and writes
4 N P; the plan moves per bright-field pixel 4 N + 4 N (transpose), 4 N + 8 Nh (R2C), 8 Nh + 8 Nh (transpose) and reads
8 N in k_ssb_trotter (a pixel outside both trotters of a Q is not loaded, so this is an upper bound).

    python scripts/bench_ssb.py [--quick] [--whole-job] [--out FILE]
        --quick: a 64 x 64 scan; --whole-job: only the device-resident whole job (for a
        `rocprofv3 --kernel-trace --stats` pass: the hipFFT executions and the kernels by name);
        --out: also append the lines to FILE
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.udf.masks import ApplyMasksUDF
from libertem_amd.udf.ssb import bf_pixels, check_params, plan_batch, reconstruct_bf, run_ssb, wavelength

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
whole_job_only = '--whole-job' in sys.argv
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SIG = (256, 256)
NAV = (64, 64) if quick else (256, 256)
# 300 kV, 22 mrad in 24 pixels, 0.2 A steps: the disks of the highest frequencies (beyond 2 semiconv / lamb) do not overlap
PARAMS = dict(lamb=wavelength(300), dpix=0.2e-10, semiconv=0.022, semiconv_pix=24., cy=128., cx=128., cutoff=1)


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
p = check_params(SIG, **PARAMS)
idx = bf_pixels(SIG, p['semiconv_pix'], p['cy'], p['cx'])
P = int(idx.size)
n_half = NAV[0] * (NAV[1] // 2 + 1)
rows = int(idx.max() // W - idx.min() // W + 1)
gather_model = n_frames * (rows * W * 2 + 4 * P)
plan_model = P * (8 * n_frames + 4 * n_frames + 8 * n_half + 16 * n_half + 8 * n_frames)
job = lambda: run_ssb(ctx, ds, **PARAMS)                                   # noqa: E731
if whole_job_only:
    say(f"SSBUDF whole job {NAV + SIG}, P = {P}: {whole_job(job):.2f} ms")
else:
    say(f"scan {NAV} of {SIG} uint16 ({frames.numel() * 2 / 2**30:.2f} GiB resident), semiconv_pix 24: P = {P}, "
        f"{rows} detector rows cross the disk")
    idx_dev = torch.from_numpy(idx).cuda()
    bf = torch.empty((n_frames, P), dtype=torch.float32, device='cuda')
    ms = t(lambda: hip.ssb_gather(0, frames.data_ptr(), np.uint16, n_frames, n_px, n_px, idx_dev.data_ptr(), P,
                                  bf.data_ptr(), P))
    say(f"ltmi_ssb_gather: {ms:.3f} ms  model {gather_model / 2**30:.2f} GiB = {gather_model / ms / 1e6:.0f} GB/s "
        f"({gather_model / ms / 1e6 / PEAK:.2f} of HBM); all of the frames in that time: "
        f"{frames.numel() * 2 / ms / 1e6:.0f} GB/s")
    fourier = torch.empty(NAV, dtype=torch.complex64, device='cuda')
    geom = hip.ssb_geometry(p['lamb'], (p['dy'], p['dx']), p['semiconv'], p['semiconv_pix'], p['cy'], p['cx'], p['t'])
    results = {}
    for batch in sorted({plan_batch(NAV, P), min(P, 256), P}):
        plan = hip.SSBPlan(0, NAV[0], NAV[1], W, idx, batch, geom, p['cutoff'])
        ms = t(lambda: plan.reconstruct(bf.data_ptr(), P, fourier.data_ptr()))
        results[batch] = fourier.cpu().numpy()
        ws = batch * (4 * n_frames + 16 * n_half) / 2**20
        say(f"ltmi_ssb_reconstruct batch {batch} ({ws:.0f} MiB workspace): {ms:.3f} ms  model "
            f"{plan_model / 2**30:.2f} GiB = {plan_model / ms / 1e6:.0f} GB/s ({plan_model / ms / 1e6 / PEAK:.2f} of HBM)"
            f"   {plan.last_kernel()}")
        plan.close()
    j_ms = whole_job(job)
    say(f"SSBUDF whole job (run_ssb, bf stays on the device, four (Ny, Nx) results on the host): {j_ms:.2f} ms = "
        f"{n_frames / j_ms * 1e3:.0f} frames/s")
    masks = np.random.default_rng(2).random((16,) + SIG).astype(np.float32)
    udf = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=16, mask_dtype=np.float32)
    m_ms = whole_job(lambda: ctx.run_udf(dataset=ds, udf=udf))
    say(f"ApplyMasksUDF, 16 dense float32 masks, the same frames, whole job: {m_ms:.2f} ms = "
        f"{n_frames / m_ms * 1e3:.0f} frames/s ({frames.numel() * 2 / m_ms / 1e6:.0f} GB/s of frames)")
    torch.set_num_threads(1)
    bf_host = bf.cpu().numpy()
    t0 = time.perf_counter()
    host = reconstruct_bf(bf_host, NAV, SIG, **PARAMS)
    n_s = time.perf_counter() - t0
    say(f"reconstruct_bf (NumPy, float64, one core) from the downloaded bright-field pixels: {n_s:.1f} s")
    ref = host['fourier'].astype(np.complex128)
    rest = np.ones(NAV, bool)
    rest[0, 0] = False
    for batch, got in results.items():
        err = np.abs(got - ref)
        say(f"device (batch {batch}) against NumPy: Q != 0 max error {err[rest].max():.3e} = "
            f"{err[rest].max() / np.abs(ref[rest]).max():.2e} of max|fourier[Q != 0]|, DC relative "
            f"{err[0, 0] / abs(ref[0, 0]):.2e}; zeros agree: {bool(np.array_equal(got == 0, ref == 0))}")
ctx.close()
