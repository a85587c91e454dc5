"""FEMUDF and LogsumUDF on the C2 dataset (256 x 256 scan of 256 x 256 uint16 frames, device resident):
kernel time from HIP events, the whole job, the byte model and its fraction of 8 TB/s, and the NumPy branch
on the CPU executor (a subset, scaled up).  FEM also on 16 384 frames of 512 x 512.

Byte model: FEM reads the 128-byte lines its ring's spans touch, per frame; logsum reads every frame once
(the chunk's second pass is meant to hit the cache) plus the float32 buffer.

    python scripts/bench_framestats.py [--quick] [--whole-job]
        --quick: 1/16 of the scan; --whole-job: only the device-resident whole jobs (for a
        `rocprofv3 --kernel-trace --stats` pass)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.FEM import FEMUDF, ring_mask, ring_spans
from libertem_amd.udf.logsum import LogsumUDF

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


def touched_line_bytes(spans, width, itemsize):
    """bytes of the distinct 128-byte lines the spans of one frame touch (frames start on a line)"""
    lines = set()
    for r, x0, x1 in spans:
        a, b = (int(r) * width + int(x0)) * itemsize, (int(r) * width + int(x1)) * itemsize
        lines.update(range(a // 128, (b - 1) // 128 + 1))
    return 128 * len(lines)


def whole_job(ctx, ds, udf, reps=10):
    for _ in range(2):
        ctx.run_udf(dataset=ds, udf=udf)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.run_udf(dataset=ds, udf=udf); ts.append(time.perf_counter() - t0)
    return np.median(ts) * 1e3


def report(name, kernel_ms, job_ms, nbytes, cpu_fps, n_frames):
    line = f"{name}: kernel {kernel_ms:.3f} ms  {nbytes / kernel_ms / 1e6:.0f} GB/s ({nbytes / kernel_ms / 1e6 / PEAK:.2f} of HBM)"
    line += f"  whole job {job_ms:.2f} ms ({job_ms / kernel_ms:.2f} x kernel)  model {nbytes / 2**30:.2f} GiB"
    if cpu_fps:
        line += f"  CPU NumPy {n_frames / cpu_fps * 1e3:.0f} ms (scaled, {cpu_fps:.0f} frames/s)"
    print(line, flush=True)


def cpu_rate(host_sub, udf):
    cpu = Context(InlineJobExecutor())
    ds = cpu.load('memory', data=host_sub, sig_dims=2, num_partitions=1)
    cpu.run_udf(dataset=ds, udf=udf)
    t0 = time.perf_counter()
    cpu.run_udf(dataset=ds, udf=udf)
    return host_sub.shape[0] * host_sub.shape[1] / (time.perf_counter() - t0)


ctx = Context.make_with('hip', gpus=0)
for sig, nav in (((256, 256), (256 // scale, 256)), ((512, 512), (64 // scale, 256))):
    H, W = sig
    n_frames = nav[0] * nav[1]
    n_px = H * W
    g = torch.Generator(device='cuda').manual_seed(7)
    fr = torch.randint(0, 4096, nav + sig, device='cuda', dtype=torch.int16, generator=g)
    ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
    center, rad_in, rad_out = (H / 2, W / 2), H / 8, 3 * H / 8
    mask = ring_mask(center, rad_in, rad_out, sig)
    spans = ring_spans(mask)
    fem_bytes = n_frames * touched_line_bytes(spans, W, 2)
    fem = FEMUDF(center=center, rad_in=rad_in, rad_out=rad_out)
    if not whole_job_only:
        sp = torch.from_numpy(spans.reshape(-1).copy()).cuda()
        out = torch.empty(n_frames, device='cuda', dtype=torch.float32)
        k_ms = t(lambda: hip.ring_moments(0, fr.data_ptr(), np.uint16, n_frames, W, n_px, sp.data_ptr(),
                                          len(spans), int(mask.sum()), out.data_ptr()))
    j_ms = whole_job(ctx, ds, fem)
    if whole_job_only:
        print(f"FEMUDF whole job {nav + sig}: {j_ms:.2f} ms", flush=True)
    else:
        host_sub = fr[:1].cpu().numpy().view(np.uint16)
        report(f"FEM {nav + sig} center {center} r {rad_in}..{rad_out}", k_ms, j_ms, fem_bytes,
               cpu_rate(host_sub, FEMUDF(center=center, rad_in=rad_in, rad_out=rad_out)), n_frames)
    if sig == (256, 256):
        log_bytes = n_frames * n_px * 2 + n_px * 4 * 2
        logsum = LogsumUDF()
        if not whole_job_only:
            out = torch.zeros(n_px, device='cuda', dtype=torch.float32)
            ws = torch.empty(max(16, hip.logsum_workspace(n_frames, n_px, np.uint16)), device='cuda', dtype=torch.uint8)
            k_ms = t(lambda: hip.logsum_frames(0, fr.data_ptr(), np.uint16, n_frames, n_px, n_px, out.data_ptr(),
                                               ws.data_ptr()))
        j_ms = whole_job(ctx, ds, logsum)
        if whole_job_only:
            print(f"LogsumUDF whole job {nav + sig}: {j_ms:.2f} ms", flush=True)
        else:
            host_sub = fr[:1, :64].cpu().numpy().view(np.uint16)
            report(f"logsum {nav + sig}", k_ms, j_ms, log_bytes, cpu_rate(host_sub, LogsumUDF()), n_frames)
    del fr, ds
    torch.cuda.empty_cache()
ctx.close()
