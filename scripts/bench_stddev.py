"""StdDevUDF: ltmi_moments_frames at the kernel level (8 GiB of frames, device resident, float64 and float32
results; ltmi_sum_frames on the same tiles for comparison), the whole job device-resident and host-streamed,
and the NumPy branch on the CPU executor.  Fractions of HBM peak count the frame bytes read, over 8 TB/s.

    python scripts/bench_stddev.py [--quick] [--whole-job]
        --quick: 1/16 of the sizes; --whole-job: only the device-resident whole job (for a
        `rocprofv3 --kernel-trace --stats` pass that splits it into kernels and the rest)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.stddev import StdDevUDF

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
whole_job_only = '--whole-job' in sys.argv
scale = 16 if quick else 1


def t(fn, reps=10):
    fn(); torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


n_px = 65536
for name, ndt, frames in () if whole_job_only else (('uint16', np.uint16, 65536 // scale), ('float32', np.float32, 32768 // scale)):
    if ndt == np.uint16:
        tile = torch.randint(0, 4096, (frames, n_px), device='cuda', dtype=torch.int16)
    else:
        tile = torch.rand((frames, n_px), device='cuda', dtype=torch.float32)
    nbytes = frames * n_px * tile.element_size()
    ws = torch.empty(max(hip.moments_workspace(frames, n_px, ndt), 16), device='cuda', dtype=torch.uint8)
    for rdt in (np.float64, np.float32):
        s = torch.zeros(n_px * 2, device='cuda', dtype=torch.float32 if rdt == np.float32 else torch.float64)
        v = torch.zeros(n_px, device='cuda', dtype=s.dtype)
        ms = t(lambda: hip.moments_frames(0, tile.data_ptr(), ndt, frames, n_px, n_px, 0, s.data_ptr(), rdt,
                                          v.data_ptr(), rdt, ws.data_ptr()))
        print(f"ltmi_moments_frames {name} -> {np.dtype(rdt).name}: {ms:.3f} ms  {nbytes / ms / 1e6:.0f} GB/s "
              f"({nbytes / ms / 1e6 / PEAK:.2f} of HBM peak)", flush=True)
    sws = torch.empty(max(hip.sum_frames_workspace(frames, n_px, np.float64), 16), device='cuda', dtype=torch.uint8)
    out = torch.zeros(n_px, device='cuda', dtype=torch.float64)
    ms = t(lambda: hip.sum_frames(0, tile.data_ptr(), ndt, frames, n_px, n_px, out.data_ptr(), np.float64,
                                  False, sws.data_ptr()))
    print(f"ltmi_sum_frames     {name} -> float64: {ms:.3f} ms  {nbytes / ms / 1e6:.0f} GB/s "
          f"({nbytes / ms / 1e6 / PEAK:.2f} of HBM peak)", flush=True)
    del tile, ws, sws

ctx = Context.make_with('hip', gpus=0)
nav = (256 // scale, 256)
fr = torch.randint(0, 4096, nav + (256, 256), device='cuda', dtype=torch.int16)
n_frames = nav[0] * nav[1]
nbytes = n_frames * 65536 * 2
ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
udf = StdDevUDF()
for _ in range(2):
    ctx.run_udf(dataset=ds, udf=udf)
ts = []
for _ in range(10):
    t0 = time.perf_counter(); ctx.run_udf(dataset=ds, udf=udf); ts.append(time.perf_counter() - t0)
ms = np.median(ts) * 1e3
print(f"StdDevUDF whole job, device resident uint16 {nav + (256, 256)}: {ms:.2f} ms  "
      f"{n_frames / ms / 1e3:.2f} Mframes/s  ({nbytes / ms / 1e6 / PEAK:.2f} of HBM peak)", flush=True)
if whole_job_only:
    ctx.close()
    sys.exit(0)
host = fr.cpu().numpy().view(np.uint16)
del fr, ds
torch.cuda.empty_cache()
ds_h = ctx.load('memory', data=host, sig_dims=2)
for _ in range(2):
    ctx.run_udf(dataset=ds_h, udf=udf)
ts = []
for _ in range(5):
    t0 = time.perf_counter(); ctx.run_udf(dataset=ds_h, udf=udf); ts.append(time.perf_counter() - t0)
ms = np.median(ts) * 1e3
print(f"StdDevUDF whole job, host streamed uint16: {ms:.2f} ms  {n_frames / ms / 1e3:.2f} Mframes/s  "
      f"({nbytes / ms / 1e6:.0f} GB/s of frames)", flush=True)
ctx.close()

cpu = Context(InlineJobExecutor())
sub = host[:4]                           # a nav subset: 1024 frames
ds_c = cpu.load('memory', data=sub, sig_dims=2, num_partitions=1)
cpu.run_udf(dataset=ds_c, udf=StdDevUDF())
t0 = time.perf_counter()
cpu.run_udf(dataset=ds_c, udf=StdDevUDF())
dt = time.perf_counter() - t0
print(f"StdDevUDF NumPy branch, CPU executor, {sub.shape}: {sub.shape[0] * sub.shape[1] / dt:.0f} frames/s", flush=True)
