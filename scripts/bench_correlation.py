"""CorrelationUDF on a 128 x 128 scan of 256 x 256 uint16 frames (device resident), 32 peaks, crop_radius 8:
`ltmi_correlate_peaks` over the whole scan from HIP events for several batch sizes, the whole job through
Context.run_udf, the byte model and its fraction of 8 TB/s, and the NumPy branch on the CPU executor (a subset,
scaled up).

Byte model per pixel of a frame, every pass reading and writing HBM once: k_corr_load 2 + 4, R2C 4 + 4 (the half
spectrum has w/2+1 of w columns of 8 bytes), k_corr_mul 4 + 4, C2R 4 + 4, k_corr_peaks (2r+1)^2 n_peaks 4 / (h w):
30.6 bytes.

    python scripts/bench_correlation.py [--quick] [--whole-job]
        --quick: 1/16 of the scan; --whole-job: only the device-resident whole job (for a
        `rocprofv3 --kernel-trace --stats` pass: the two hipFFT executions and the three kernels by name)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip, masks
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.correlation import CorrelationUDF
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
whole_job_only = '--whole-job' in sys.argv
SIG = (256, 256)
NAV = (128 // (16 if quick else 1), 128)
N_PEAKS, R, Q = 32, 8, 1


def t(fn, reps=10):
    fn(); torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


def whole_job(ctx, ds, udf, reps=10):
    for _ in range(2):
        ctx.run_udf(dataset=ds, udf=udf)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.run_udf(dataset=ds, udf=udf); ts.append(time.perf_counter() - t0)
    return np.median(ts) * 1e3


H, W = SIG
n_frames, n_px = NAV[0] * NAV[1], H * W
# a 4 x 8 lattice of expected disks, 32 px apart, and a disk template of radius 6
peaks = np.array([(32 + 64 * i, 16 + 32 * j) for i in range(4) for j in range(8)], dtype=np.int32)
assert len(peaks) == N_PEAKS
template = masks.circular(centerX=W // 2, centerY=H // 2, imageSizeX=W, imageSizeY=H, radius=6).astype(np.float32)
g = torch.Generator(device='cuda').manual_seed(7)
fr = torch.randint(0, 4096, NAV + SIG, device='cuda', dtype=torch.int16, generator=g)
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
udf = CorrelationUDF(peaks=peaks, template=template, crop_radius=R, refine_radius=Q)
model = n_frames * (n_px * 30 + (2 * R + 1) ** 2 * N_PEAKS * 4)
if whole_job_only:
    print(f"CorrelationUDF whole job {NAV + SIG}: {whole_job(ctx, ds, udf):.2f} ms", flush=True)
else:
    per_frame = n_px * 4 + H * (W // 2 + 1) * 8
    dev_peaks = torch.from_numpy(peaks.reshape(-1).copy()).cuda()
    out = [torch.empty((n_frames, N_PEAKS, 2), device='cuda', dtype=torch.int32),
           torch.empty((n_frames, N_PEAKS, 2), device='cuda', dtype=torch.float32),
           torch.empty((n_frames, N_PEAKS), device='cuda', dtype=torch.float32),
           torch.empty((n_frames, N_PEAKS), device='cuda', dtype=torch.float32)]
    for batch in (32, 128, 255, CORR_WORKSPACE_BYTES // per_frame, 4096):
        batch = min(int(batch), n_frames)
        plan = hip.CorrPlan(0, H, W, batch, template)
        ms = t(lambda: plan.correlate_peaks(fr.data_ptr(), np.uint16, n_frames, n_px, dev_peaks.data_ptr(), N_PEAKS, R,
                                            Q, *(o.data_ptr() for o in out)))
        print(f"ltmi_correlate_peaks {NAV + SIG} batch {batch} ({batch * per_frame / 2**20:.0f} MiB workspace): "
              f"{ms:.2f} ms  {n_frames / ms * 1e3:.0f} frames/s  model {model / 2**30:.1f} GiB = "
              f"{model / ms / 1e6:.0f} GB/s ({model / ms / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}", flush=True)
        plan.close()
    j_ms = whole_job(ctx, ds, udf)
    cpu = Context(InlineJobExecutor())
    host_sub = fr[:1, :32].cpu().numpy().view(np.uint16)
    ds_cpu = cpu.load('memory', data=host_sub, sig_dims=2, num_partitions=1)
    cpu.run_udf(dataset=ds_cpu, udf=udf)
    t0 = time.perf_counter()
    cpu.run_udf(dataset=ds_cpu, udf=udf)
    cpu_fps = 32 / (time.perf_counter() - t0)
    print(f"CorrelationUDF whole job {NAV + SIG}: {j_ms:.2f} ms ({n_frames / j_ms * 1e3:.0f} frames/s)  "
          f"CPU NumPy {n_frames / cpu_fps * 1e3:.0f} ms (scaled, {cpu_fps:.0f} frames/s)", flush=True)
ctx.close()
