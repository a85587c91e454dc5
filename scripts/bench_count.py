"""Electron counting on the C2 scan shape: 256 x 256 positions of 256 x 256 uint16 frames resident in HBM (8 GiB),
made by `electron_frames(rate=0.05)` -- about 205 events per frame -- and counted with background_threshold = 10,
xray_threshold = 1000 and the generator's dark frame.  4096 frames are generated on the host and repeated 16 times on
the device: generating all 65536 on one core takes minutes and the kernels' time does not depend on it.

From HIP events, the median of 10: `ltmi_count_events` alone, `ltmi_store_events` alone, and `ltmi_sum_sig` on the same
frames in the same process -- the project's plain read stream over the same bytes, the yardstick.  From the host
clock: `count_events` end to end (two runs over the frames, the D2H copies and the files), `count_frames` (NumPy, one
core) on 256 frames, and the point of the exercise, ApplyMasksUDF with the 16 dense float32 masks of bench.py's C2 on
the dense dataset and on the raw_csr dataset `count_events` wrote.

Byte model: each kernel reads the pixel bytes once plus the halo rows at 2 / strip_rows (and
the dark frame through L2); the count kernel writes 4 bytes per frame, the store kernel 4 + 1 bytes per event.

    python scripts/bench_count.py [--quick] [--out FILE]
        --quick: a 64 x 64 scan; --out: also append the lines to FILE
"""
import os, shutil, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.udf.counting import count_events, count_frames
from libertem_amd.udf.masks import ApplyMasksUDF
from libertem_amd.utils.generate import electron_frames

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SIG = (256, 256)
NAV = (64, 64) if quick else (256, 256)
UNIQUE = 1024 if quick else 4096
T_BG, T_X = 10., 1000.


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


def whole_job(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return np.median(ts) * 1e3


H, W = SIG
n_frames, n_px = NAV[0] * NAV[1], H * W
frames = torch.empty((n_frames, n_px), dtype=torch.int16, device='cuda')
host_sample = None
planted = 0
for i in range(0, UNIQUE, 1024):
    part, dark, (indptr, _) = electron_frames(1024, SIG, 0.05, 100 + i)
    if host_sample is None:
        host_sample = part[:256].copy()
    planted += int(indptr[-1])
    frames[i:i + 1024] = torch.from_numpy(part.reshape((1024, n_px)).view(np.int16)).cuda()
for i in range(UNIQUE, n_frames, UNIQUE):
    frames[i:i + UNIQUE] = frames[:UNIQUE]
planted *= n_frames // UNIQUE
dark_dev = torch.from_numpy(dark).cuda()
pixel_bytes = frames.numel() * 2
strip = hip.count_strip_rows(H, W)
read_model = pixel_bytes * (1 + 2 / strip)
say(f"scan {NAV} of {SIG} uint16 ({pixel_bytes / 2**30:.2f} GiB resident, {UNIQUE} different frames), "
    f"{planted} planted events = {planted / n_frames:.1f} per frame = {planted / frames.numel() * 100:.2f} % of the "
    f"pixels; strips of {strip} rows")

ptr = frames.data_ptr()
n_events = torch.empty(n_frames, dtype=torch.int32, device='cuda')
sums = torch.empty(n_frames, dtype=torch.float32, device='cuda')
s_ms = t(lambda: hip.sum_sig(0, ptr, np.uint16, n_frames, n_px, n_px, sums.data_ptr(), np.float32, False))
say(f"ltmi_sum_sig (the read stream): {s_ms:.3f} ms = {pixel_bytes / s_ms / 1e6:.0f} GB/s ({pixel_bytes / s_ms / 1e6 / PEAK:.2f} of HBM)")
c_ms = t(lambda: hip.count_events(0, ptr, np.uint16, n_frames, H, W, n_px, dark_dev.data_ptr(), None, T_BG, T_X,
                                  n_events.data_ptr()))
say(f"ltmi_count_events: {c_ms:.3f} ms  model {read_model / 2**30:.2f} GiB = {read_model / c_ms / 1e6:.0f} GB/s "
    f"({read_model / c_ms / 1e6 / PEAK:.2f} of HBM), {c_ms / s_ms:.2f} x ltmi_sum_sig   {hip.count_last_kernel()}")
counts = n_events.cpu().numpy()
assert int(counts.sum()) == planted, (int(counts.sum()), planted)
row_ptr = torch.zeros(n_frames + 1, dtype=torch.int64, device='cuda')
row_ptr[1:] = torch.cumsum(n_events.to(torch.int64), 0)
nnz = int(row_ptr[-1])
indices = torch.empty(nnz, dtype=torch.int32, device='cuda')
values = torch.empty(nnz, dtype=torch.uint8, device='cuda')
status = torch.zeros(1, dtype=torch.int32, device='cuda')
w_ms = t(lambda: hip.store_events(0, ptr, np.uint16, n_frames, H, W, n_px, dark_dev.data_ptr(), None, T_BG, T_X,
                                  row_ptr.data_ptr(), 0, nnz, indices.data_ptr(), values.data_ptr(), np.uint8,
                                  status.data_ptr()))
assert int(status[0]) == 0
store_model = read_model + 5 * nnz + 8 * n_frames
say(f"ltmi_store_events (uint8 values): {w_ms:.3f} ms  model {store_model / 2**30:.2f} GiB = "
    f"{store_model / w_ms / 1e6:.0f} GB/s ({store_model / w_ms / 1e6 / PEAK:.2f} of HBM), {w_ms / s_ms:.2f} x "
    f"ltmi_sum_sig   {hip.count_last_kernel()}")

ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=frames.reshape(NAV + SIG), dtype=np.uint16, sig_dims=2, num_partitions=1)
tmp = tempfile.mkdtemp(prefix='bench_count_')
try:
    path = os.path.join(tmp, 'counted.toml')
    res = {}
    def job():
        res.update(count_events(ctx, ds, path, T_BG, T_X, dark=dark))
    j_ms = whole_job(job)
    assert res['nnz'] == planted
    written = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
    say(f"count_events end to end (two runs, D2H, {written / 2**20:.0f} MiB of files): {j_ms:.1f} ms = "
        f"{n_frames / j_ms * 1e3:.0f} frames/s")
    masks = np.random.default_rng(2).random((16,) + SIG).astype(np.float32)
    udf = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=16, mask_dtype=np.float32)
    d_ms = whole_job(lambda: ctx.run_udf(dataset=ds, udf=udf), reps=5, warm=2)
    say(f"ApplyMasksUDF, 16 dense float32 masks, the dense frames, whole job: {d_ms:.2f} ms = "
        f"{n_frames / d_ms * 1e3:.0f} frames/s")
    counted = ctx.load('raw_csr', path=path)
    udf2 = ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=16, mask_dtype=np.float32)
    r_ms = whole_job(lambda: ctx.run_udf(dataset=counted, udf=udf2), reps=5, warm=2)
    kernels = sorted({h.last_kernel() for h in udf2.masks._handle_cache.values()})
    say(f"ApplyMasksUDF, the same masks, the counted raw_csr dataset, whole job: {r_ms:.2f} ms = "
        f"{n_frames / r_ms * 1e3:.0f} frames/s, {d_ms / r_ms:.1f} x the dense run   {kernels}")
finally:
    shutil.rmtree(tmp, ignore_errors=True)
torch.set_num_threads(1)
t0 = time.perf_counter()
ref = count_frames(host_sample, T_BG, T_X, dark=dark)
n_s = time.perf_counter() - t0
say(f"count_frames (NumPy, one core) on {len(host_sample)} frames: {n_s * 1e3:.0f} ms = "
    f"{len(host_sample) / n_s:.0f} frames/s, {n_s / len(host_sample) * n_frames:.0f} s for the scan")
assert np.array_equal(np.diff(ref[0]), counts[:len(host_sample)])
ctx.close()
