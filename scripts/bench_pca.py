"""WeightedSumUDF's kernel and run_pca on the C2 scan shape: 256 x 256 positions of 256 x 256 uint16 frames resident in
HBM (8 GiB).  From one process, with HIP events: `ltmi_wsum_frames` with k = 16 (and 1, 17, 32, 64) beside
`ltmi_sum_frames` over the same bytes; then the whole jobs `run_weighted_sum` and `run_pca` (n_components = 16, the
defaults otherwise: 24 columns, 2 power iterations, 7 frame passes) with its split into frame passes and small algebra
(host clock).

Byte model of `ltmi_wsum_frames` and `ltmi_sum_frames`: N P itemsize bytes read, the output negligible.

    python scripts/bench_pca.py [--quick] [--out FILE]
        --quick: a 64 x 64 scan; --out: also append the lines to FILE
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.udf.pca import run_pca
from libertem_amd.udf.weightedsum import run_weighted_sum

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SIG = (256, 256)
NAV = (64, 64) if quick else (256, 256)
K = 16


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


n_frames, n_px = NAV[0] * NAV[1], SIG[0] * SIG[1]
g = torch.Generator(device='cuda').manual_seed(7)
frames = torch.empty((n_frames, n_px), dtype=torch.int16, device='cuda')
step = max(1, (1 << 30) // (n_px * 2))
for i in range(0, n_frames, step):
    j = min(n_frames, i + step)
    frames[i:j] = torch.randint(0, 4096, (j - i, n_px), generator=g, device='cuda', dtype=torch.int16)
nbytes = frames.numel() * 2
say(f"scan {NAV} of {SIG} uint16 ({nbytes / 2**30:.2f} GiB resident), uniform counts in [0, 4096)")

# ---- the kernels, the same bytes
out = torch.empty((n_px,), dtype=torch.float32, device='cuda')
ws = torch.empty((max(16, hip.sum_frames_workspace(n_frames, n_px, np.float32)),), dtype=torch.uint8, device='cuda')
ms_sum = t(lambda: hip.sum_frames(0, frames.data_ptr(), np.uint16, n_frames, n_px, n_px, out.data_ptr(), np.float32,
                                  False, ws.data_ptr()))
say(f"ltmi_sum_frames -> float32: {ms_sum:.3f} ms = {nbytes / ms_sum / 1e6:.0f} GB/s "
    f"({nbytes / ms_sum / 1e6 / PEAK:.2f} of HBM by the model)")
del ws
for k in (K, 1, 17, 32, 64):
    w = torch.randn((n_frames, k), generator=g, device='cuda', dtype=torch.float32)
    outk = torch.empty((k, n_px), dtype=torch.float32, device='cuda')
    need = hip.wsum_workspace(n_frames, n_px, k)
    wsk = torch.empty((need,), dtype=torch.uint8, device='cuda')
    ms = t(lambda: hip.wsum_frames(0, frames.data_ptr(), np.uint16, n_frames, n_px, n_px, w.data_ptr(), k, k,
                                   outk.data_ptr(), n_px, False, wsk.data_ptr()))
    tf = 2.0 * n_frames * n_px * 16 * ((k + 15) // 16) / ms / 1e9
    say(f"ltmi_wsum_frames k = {k}: {ms:.3f} ms = {nbytes / ms / 1e6:.0f} GB/s ({nbytes / ms / 1e6 / PEAK:.2f} of HBM by "
        f"the model), {ms / ms_sum:.2f} x ltmi_sum_frames; {tf:.0f} TF of f32 MFMA on {16 * ((k + 15) // 16)} columns; "
        f"workspace {need / 2**20:.0f} MiB = {need // (4 * k * n_px)} slabs")
    del w, outk, wsk

# ---- the whole jobs
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=frames.reshape(NAV + SIG), dtype=np.uint16, sig_dims=2, num_partitions=1)
weights = np.random.default_rng(3).standard_normal(NAV + (K,)).astype(np.float32)
for _ in range(2):
    run_weighted_sum(ctx, ds, weights)
ts = []
for _ in range(5):
    t0 = time.perf_counter(); run_weighted_sum(ctx, ds, weights); ts.append(time.perf_counter() - t0)
say(f"WeightedSumUDF whole job (run_weighted_sum, k = {K}, weights uploaded per run): {np.median(ts) * 1e3:.2f} ms = "
    f"{n_frames / np.median(ts):.0f} frames/s")
run_pca(ctx, ds, K)
runs = []
for _ in range(3):
    t0 = time.perf_counter(); res = run_pca(ctx, ds, K); runs.append((time.perf_counter() - t0, res['timings']))
wall, split = sorted(runs, key=lambda r: r[0])[1]
say(f"run_pca n_components = {K} (24 columns, n_iter = 2: StdDevUDF + 3 x ApplyMasksUDF + 3 x WeightedSumUDF): "
    f"{wall * 1e3:.1f} ms = frame passes {split['frame_passes'] * 1e3:.1f} ms + small algebra (NumPy float64 on the "
    f"host: 3 QR of N x 24, 2 QR of P x 24, the SVD of 24 x P) {split['algebra'] * 1e3:.1f} ms")
say(f"  7 passes over {nbytes / 2**30:.2f} GiB at the HBM rate would take {7 * nbytes / PEAK / 1e6:.1f} ms")
ctx.close()
