"""HoloReconstructUDF on a 16 x 32 stack of 1024 x 1024 uint16 holograms (device resident, 1 GiB) reconstructed to
256 x 256 with a smoothed disk aperture: `ltmi_holo_reconstruct` over the whole stack from HIP events for several batch
sizes, the whole job through Context.run_udf, the byte model and its fraction of 8 TB/s, and the NumPy branch on the
CPU executor (a subset, scaled up).

Byte model, every pass reading and writing HBM once: per frame pixel k_corr_load 2 + 4 and R2C 4 + 4 (the half spectrum
has w/2+1 of w columns of 8 bytes); per output pixel k_holo_crop 8 + 4 + 8, C2C 8 + 8 and k_holo_store 8 + 8:
14 h w + 52 oh ow bytes per frame.

    python scripts/bench_holo.py [--quick] [--whole-job]
        --quick: 1/8 of the stack; --whole-job: only the device-resident whole job (for a
        `rocprofv3 --kernel-trace --stats` pass: the hipFFT executions and the three kernels by name)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES
from libertem_amd.udf.holography import HoloReconstructUDF, disk_aperture
from libertem_amd.utils.generate import hologram_frame

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
whole_job_only = '--whole-job' in sys.argv
SIG = (1024, 1024)
OUT = (256, 256)
NAV = (16 // (8 if quick else 1), 32)
K = (205, 154)              # carrier, cycles per frame: a sampling of 4 pixels per fringe


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
n_frames, n_px, n_out = NAV[0] * NAV[1], H * W, OUT[0] * OUT[1]
# one simulated hologram of a smooth object, repeated with shot-noise-like offsets drawn on the device
yy, xx = np.mgrid[:H, :W]
amp = 0.7 + 0.2 * np.cos(2 * np.pi * yy / H)
phi = 3 * np.exp(-((yy - H / 2) ** 2 + (xx - W / 2) ** 2) / (2 * 150. ** 2))
fy, fx = K[0] / H, K[1] / W
base = hologram_frame(amp, phi, counts=4000., sampling=1 / np.hypot(fy, fx), visibility=0.5,
                      f_angle=float(np.degrees(np.arctan2(fx, fy))))
g = torch.Generator(device='cuda').manual_seed(7)
fr = torch.from_numpy(np.rint(base).astype(np.int16)).cuda()[None, None] + \
    torch.randint(0, 64, NAV + SIG, device='cuda', dtype=torch.int16, generator=g)
SB = ((-K[0]) % H, (-K[1]) % W)
aperture = disk_aperture(OUT, 64, 4.0)
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
udf = HoloReconstructUDF(out_shape=OUT, sb_position=SB, aperture=aperture)
model = n_frames * (14 * n_px + 52 * n_out)
if whole_job_only:
    print(f"HoloReconstructUDF whole job {NAV + SIG} -> {OUT}: {whole_job(ctx, ds, udf):.2f} ms", flush=True)
else:
    per_frame = 4 * n_px + 8 * H * (W // 2 + 1) + 8 * n_out
    out = torch.empty((n_frames, n_out), device='cuda', dtype=torch.complex64)
    for batch in (4, 16, CORR_WORKSPACE_BYTES // per_frame, 128):
        batch = min(int(batch), n_frames)
        plan = hip.HoloPlan(0, H, W, OUT[0], OUT[1], batch, SB[0], SB[1], aperture)
        ms = t(lambda: plan.reconstruct(fr.data_ptr(), np.uint16, n_frames, n_px, out.data_ptr(), n_out))
        print(f"ltmi_holo_reconstruct {NAV + SIG} -> {OUT} batch {batch} ({batch * per_frame / 2**20:.0f} MiB workspace): "
              f"{ms:.2f} ms  {n_frames / ms * 1e3:.0f} frames/s  model {model / 2**30:.2f} GiB = "
              f"{model / ms / 1e6:.0f} GB/s ({model / ms / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}", flush=True)
        plan.close()
    j_ms = whole_job(ctx, ds, udf)
    cpu = Context(InlineJobExecutor())
    host_sub = fr[:1, :4].cpu().numpy().view(np.uint16)
    ds_cpu = cpu.load('memory', data=host_sub, sig_dims=2, num_partitions=1)
    cpu.run_udf(dataset=ds_cpu, udf=udf)
    t0 = time.perf_counter()
    cpu.run_udf(dataset=ds_cpu, udf=udf)
    cpu_fps = 4 / (time.perf_counter() - t0)
    print(f"HoloReconstructUDF whole job {NAV + SIG} -> {OUT}: {j_ms:.2f} ms ({n_frames / j_ms * 1e3:.0f} frames/s)  "
          f"CPU NumPy {n_frames / cpu_fps * 1e3:.0f} ms (scaled, {cpu_fps:.1f} frames/s)", flush=True)
ctx.close()
