"""PeakFindUDF on the scan of scripts/bench_correlation.py -- 128 x 128 positions of 256 x 256 uint16 frames (device
resident), disk template of radius 6 --: `run_peakfind` with num_peaks 32 and min_distance 8 against `run_correlation`
with 32 given peaks and crop_radius 8 on the same data, alternating in one process (what searching the whole map costs
over looking at 32 windows), and `ltmi_find_peaks_maps` alone on the correlation maps of one tile from HIP events.

Byte model of the search per pixel of a map: 4 read by k_pf_cells; the keys are 16 bytes per (d+1)^2 cell written and
about as much read again (0.4 bytes per pixel at d = 8), the windows of the found peaks (2d+1)^2 N 4 / (h w).  The
correlation in front of it moves about 30 bytes per pixel.

    python scripts/bench_peakfind.py [--quick] [--whole-job]
        --quick: 1/16 of the scan; --whole-job: only the device-resident PeakFindUDF job (for a
        `rocprofv3 --kernel-trace --stats` pass: the two hipFFT executions and the six kernels by name)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip, masks
from libertem_amd.api import Context
from libertem_amd.udf import correlation
from libertem_amd.udf.correlation import CorrelationUDF
from libertem_amd.udf.peakfind import PeakFindUDF

quick = '--quick' in sys.argv
whole_job_only = '--whole-job' in sys.argv
SIG = (256, 256)
NAV = (128 // (16 if quick else 1), 128)
N_PEAKS, D, Q = 32, 8, 1


def whole_job(ctx, ds, udf, reps=10, **kw):
    for _ in range(2):
        ctx.run_udf(dataset=ds, udf=udf, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.run_udf(dataset=ds, udf=udf, **kw); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return np.median(ts) * 1e3, np.min(ts) * 1e3, np.max(ts) * 1e3


H, W = SIG
n_frames = NAV[0] * NAV[1]
peaks = np.array([(32 + 64 * i, 16 + 32 * j) for i in range(4) for j in range(8)], dtype=np.int32)
template = masks.circular(centerX=W // 2, centerY=H // 2, imageSizeX=W, imageSizeY=H, radius=6).astype(np.float32)
g = torch.Generator(device='cuda').manual_seed(7)
fr = torch.randint(0, 4096, NAV + SIG, device='cuda', dtype=torch.int16, generator=g)
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
find = PeakFindUDF(template=template, num_peaks=N_PEAKS, min_distance=D, refine_radius=Q)
corr = CorrelationUDF(peaks=peaks, template=template, crop_radius=D, refine_radius=Q)
if whole_job_only:
    print(f"PeakFindUDF whole job {NAV + SIG}: {whole_job(ctx, ds, find)[0]:.2f} ms", flush=True)
    ctx.close()
    sys.exit(0)
# alternating, so that both see the same machine
times = {'find': [], 'corr': [], 'find_dev': [], 'corr_dev': []}
for _ in range(3):
    times['find'].append(whole_job(ctx, ds, find))
    times['corr'].append(whole_job(ctx, ds, corr))
    times['find_dev'].append(whole_job(ctx, ds, find, result_where='device'))
    times['corr_dev'].append(whole_job(ctx, ds, corr, result_where='device'))
for name, label in (('find', 'run_peakfind (PeakFindUDF)'), ('corr', 'run_correlation (CorrelationUDF)'),
                    ('find_dev', "PeakFindUDF, result_where='device'"),
                    ('corr_dev', "CorrelationUDF, result_where='device'")):
    med = [t[0] for t in times[name]]
    print(f"{label} whole job {NAV + SIG}: medians of 10 runs, three rounds: "
          f"{' / '.join(f'{m:.2f}' for m in med)} ms (fastest and slowest single run "
          f"{min(t[1] for t in times[name]):.2f} / {max(t[2] for t in times[name]):.2f} ms)", flush=True)
m_find, m_corr = np.median([t[0] for t in times['find']]), np.median([t[0] for t in times['corr']])
print(f"the search takes {m_find - m_corr:+.3f} ms = {100 * (m_find - m_corr) / m_corr:+.1f} % over {m_corr:.2f} ms "
      f"({n_frames / m_find * 1e3:.0f} frames/s with it)", flush=True)
d_find, d_corr = np.median([t[0] for t in times['find_dev']]), np.median([t[0] for t in times['corr_dev']])
print(f"with the results left on the device {d_find - d_corr:+.3f} ms = {100 * (d_find - d_corr) / d_corr:+.1f} % "
      f"over {d_corr:.2f} ms", flush=True)
plans = [p for p in correlation._PLANS.values() if p.sig == SIG]
batch = plans[0].max_batch
print(f"tiles of {batch} frames: {-(-n_frames // batch)} calls per run   {plans[0].last_kernel()}", flush=True)
res = ctx.run_udf(dataset=ds, udf=find)
found = np.asarray(res['n_found'].data)
print(f"n_found: {found.min()} .. {found.max()} of {N_PEAKS} slots per frame", flush=True)

# the search alone: on maps with the statistics of a correlation (smoothed noise), one tile's worth
n_maps = min(batch, n_frames)
maps = torch.randn((n_maps, 1, H, W), device='cuda', generator=g)
maps = torch.nn.functional.avg_pool2d(maps, 9, stride=1, padding=4).reshape((n_maps, H, W)).contiguous()
out = [torch.empty((n_maps,), device='cuda', dtype=torch.int32),
       torch.empty((n_maps, N_PEAKS, 2), device='cuda', dtype=torch.int32),
       torch.empty((n_maps, N_PEAKS, 2), device='cuda', dtype=torch.float32),
       torch.empty((n_maps, N_PEAKS), device='cuda', dtype=torch.float32),
       torch.empty((n_maps, N_PEAKS), device='cuda', dtype=torch.float32)]


def search():
    hip.find_peaks_maps(0, maps.data_ptr(), n_maps, H, W, H * W, N_PEAKS, D, 0, 0.0, 0.0, Q,
                        *(o.data_ptr() for o in out))


for _ in range(3):
    search()
torch.cuda.synchronize()
evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
for e0, e1 in evs:
    e0.record(); search(); e1.record()
torch.cuda.synchronize()
ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
model = n_maps * H * W * 4
print(f"ltmi_find_peaks_maps {n_maps} maps of {H} x {W}, N = {N_PEAKS}, d = {D}: median of 20 calls "
      f"{ms[10] * 1e3:.0f} us (fastest {ms[0] * 1e3:.0f}, slowest {ms[-1] * 1e3:.0f}); one read of the maps "
      f"{model / 2**20:.0f} MiB = {model / ms[10] / 1e6:.0f} GB/s   {hip.find_peaks_last_kernel()}", flush=True)
ctx.close()
