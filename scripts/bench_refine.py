"""LatticeRefineUDF on the scan of scripts/bench_correlation.py -- 128 x 128 positions of 256 x 256 uint16 frames
(device resident), 32 peaks on a lattice, crop_radius 8 --: the whole `run_refine` job and `CorrelationUDF` alone on the
same data in the same process (what the fit adds to a run), `ltmi_lattice_fit` alone over the whole scan from HIP
events (3 warm-up calls, the median of 20), and the NumPy branch's `fit_lattice` on the downloaded arrays on one core.

Byte model of the fit per (frame, peak): 8 (refineds) + 4 (weight) read, 1 (selector) written = 13 bytes, plus 28
bytes of results per frame; the correlation in front of it moves about 30 bytes per PIXEL.

    python scripts/bench_refine.py [--quick]        --quick: 1/16 of the scan
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip, masks
from libertem_amd.api import Context
from libertem_amd.udf import correlation
from libertem_amd.udf.correlation import CorrelationUDF
from libertem_amd.udf.lattice import LatticeRefineUDF, fit_lattice

quick = '--quick' in sys.argv
SIG = (256, 256)
NAV = (128 // (16 if quick else 1), 128)
N_PEAKS, R, Q = 32, 8, 1
ZERO, A, B = (32., 16.), (64., 0.), (0., 32.)           # peaks (32 + 64 i, 16 + 32 j), i < 4, j < 8


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
indices = np.array([(i, j) for i in range(4) for j in range(8)], dtype=np.int32)
assert len(indices) == N_PEAKS
template = masks.circular(centerX=W // 2, centerY=H // 2, imageSizeX=W, imageSizeY=H, radius=6).astype(np.float32)
g = torch.Generator(device='cuda').manual_seed(7)
fr = torch.randint(0, 4096, NAV + SIG, device='cuda', dtype=torch.int16, generator=g)
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
refine = LatticeRefineUDF(indices=indices, zero=ZERO, a=A, b=B, template=template, crop_radius=R, refine_radius=Q,
                          tolerance=R)
corr = CorrelationUDF(peaks=refine._peaks(), template=template, crop_radius=R, refine_radius=Q)
# alternating, so that both see the same machine
times = {'refine': [], 'corr': [], 'refine_dev': [], 'corr_dev': []}
for _ in range(3):
    times['refine'].append(whole_job(ctx, ds, refine))
    times['corr'].append(whole_job(ctx, ds, corr))
    times['refine_dev'].append(whole_job(ctx, ds, refine, result_where='device'))
    times['corr_dev'].append(whole_job(ctx, ds, corr, result_where='device'))
for name, label in (('refine', 'run_refine (LatticeRefineUDF)'), ('corr', 'CorrelationUDF alone'),
                    ('refine_dev', "LatticeRefineUDF, result_where='device'"),
                    ('corr_dev', "CorrelationUDF alone, result_where='device'")):
    med = [t[0] for t in times[name]]
    print(f"{label} whole job {NAV + SIG}: medians of 10 runs, three rounds: "
          f"{' / '.join(f'{m:.2f}' for m in med)} ms (fastest and slowest single run "
          f"{min(t[1] for t in times[name]):.2f} / {max(t[2] for t in times[name]):.2f} ms)", flush=True)
m_ref, m_corr = np.median([t[0] for t in times['refine']]), np.median([t[0] for t in times['corr']])
print(f"the fit adds {m_ref - m_corr:.3f} ms = {100 * (m_ref - m_corr) / m_corr:.1f} % to {m_corr:.2f} ms "
      f"({n_frames / m_ref * 1e3:.0f} frames/s with it)", flush=True)
d_ref, d_corr = np.median([t[0] for t in times['refine_dev']]), np.median([t[0] for t in times['corr_dev']])
print(f"with the results left on the device it adds {d_ref - d_corr:.3f} ms = {100 * (d_ref - d_corr) / d_corr:.1f} % "
      f"to {d_corr:.2f} ms", flush=True)
plans = [p for p in correlation._PLANS.values() if p.sig == SIG]
print(f"tiles of {plans[0].max_batch} frames: {-(-n_frames // plans[0].max_batch)} calls of each entry per run",
      flush=True)

# the kernel alone, on the results of a run left on the device
res = ctx.run_udf(dataset=ds, udf=refine, result_where='device')
refineds, elevations = (res[k].device_data for k in ('refineds', 'peak_elevations'))
dev_idx = torch.from_numpy(indices.reshape(-1).copy()).cuda()
out = [torch.empty((n_frames, 2), device='cuda', dtype=torch.float32) for _ in range(3)]
sel = torch.empty((n_frames, N_PEAKS), device='cuda', dtype=torch.uint8)
err = torch.empty((n_frames,), device='cuda', dtype=torch.float32)
start = np.concatenate([ZERO, A, B])


def fit():
    hip.lattice_fit(0, refineds.data_ptr(), elevations.data_ptr(), None, n_frames, N_PEAKS, dev_idx.data_ptr(), start,
                    R, *(o.data_ptr() for o in out), sel.data_ptr(), err.data_ptr())


for _ in range(3):
    fit()
torch.cuda.synchronize()
evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
for e0, e1 in evs:
    e0.record(); fit(); e1.record()
torch.cuda.synchronize()
ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
model = n_frames * (N_PEAKS * 13 + 28)
print(f"ltmi_lattice_fit {n_frames} frames x {N_PEAKS} peaks: median of 20 calls {ms[10] * 1e3:.1f} us "
      f"(fastest {ms[0] * 1e3:.1f}, slowest {ms[-1] * 1e3:.1f}); model {model / 2**20:.1f} MiB = "
      f"{model / ms[10] / 1e6:.0f} GB/s   {hip.lattice_last_kernel()}", flush=True)
selected = float(sel.float().mean().cpu())
fitted = float((~torch.isnan(err)).float().mean().cpu())
print(f"selected {100 * selected:.1f} % of the (frame, peak) pairs, a fit exists on {100 * fitted:.1f} % of the frames",
      flush=True)

# the NumPy branch on the downloaded arrays, one core
h_ref = np.asarray(res['refineds'].data).reshape((n_frames, N_PEAKS, 2))
h_el = np.asarray(res['peak_elevations'].data).reshape((n_frames, N_PEAKS))
from threadpoolctl import threadpool_limits
with threadpool_limits(limits=1):
    fit_lattice(h_ref, h_el, None, indices, ZERO, A, B, R)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); host = fit_lattice(h_ref, h_el, None, indices, ZERO, A, B, R)
        ts.append(time.perf_counter() - t0)
print(f"fit_lattice (NumPy, one core) on the downloaded arrays: median of 5 calls {np.median(ts) * 1e3:.1f} ms = "
      f"{np.median(ts) / n_frames * 1e6:.2f} us per frame", flush=True)
same = np.array_equal(host[3], sel.cpu().numpy().astype(bool))
print(f"selector of the two: {'equal' if same else 'DIFFERENT'}; largest |zero| difference "
      f"{np.nanmax(np.abs(host[0] - out[0].cpu().numpy())):.3g} px", flush=True)
ctx.close()
