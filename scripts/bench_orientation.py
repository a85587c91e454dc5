"""Orientation matching on a 128 x 128 scan of 256 x 256 uint16 frames resident in HBM (2 GiB), made by
`spot_pattern_frames`: polar images of n_r = 64 x n_phi = 360, a library of 1000 templates of 20 spots, n_best = 1.
64 frames are generated on the host and repeated on the device: the kernel's time does not depend on the pixels.

From HIP events, the median of 10: `ltmi_orient_match`, `ltmi_orient_polar` alone (stage 1 written to global memory),
and `ltmi_sum_sig` on the same frames in the same process -- the project's plain read stream over the same bytes.  From
the host clock: `polar_frames` + `match_polar` (NumPy, one core) on the 64 different frames.

Model: stage 2 reads n_frames x (spots of the library) x n_phi words of LDS; the aggregate
rate of 4-byte LDS reads is about 75 TB/s.  It also issues vector instructions for every word -- the multiply and the
add are separate by definition -- so the LDS rate is a bound, not an expectation.

    python scripts/bench_orientation.py [--quick] [--out FILE]
        --quick: a 32 x 32 scan; --out: also append the lines to FILE
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.udf.orientation import match_polar, polar_frames, polar_library, polar_table
from libertem_amd.utils.generate import spot_pattern_frames

LDS_B32 = 75e12             # bytes/s, 4-byte LDS reads, every CU streaming
PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
SIG, CENTER = (256, 256), (127.3, 128.6)
NAV = (32, 32) if quick else (128, 128)
N_R, N_PHI, N_TEMPLATES, N_SPOTS, UNIQUE = 64, 360, 1000, 20, 64


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


rng = np.random.default_rng(7)
spot_lists = []
for _ in range(N_TEMPLATES):
    r, a = rng.uniform(4, N_R - 1, N_SPOTS), rng.uniform(0, 2 * np.pi, N_SPOTS)
    spot_lists.append((r * np.sin(a), r * np.cos(a), rng.uniform(0.3, 1, N_SPOTS)))
library = polar_library(spot_lists, N_R, N_PHI)
tap_idx, tap_w = polar_table(SIG, CENTER, N_R, N_PHI)
truth = np.stack([rng.integers(0, N_TEMPLATES, UNIQUE), rng.integers(0, N_PHI, UNIQUE)], axis=1)
host = spot_pattern_frames(spot_lists, [(tt, 2 * np.pi * k / N_PHI) for tt, k in truth], SIG, CENTER, seed=1)

H, W = SIG
n_frames, n_px = NAV[0] * NAV[1], H * W
frames = torch.empty((n_frames, n_px), dtype=torch.int16, device='cuda')
frames[:UNIQUE] = torch.from_numpy(host.reshape((UNIQUE, n_px)).view(np.int16)).cuda()
for i in range(UNIQUE, n_frames, UNIQUE):
    frames[i:i + UNIQUE] = frames[:UNIQUE]
pixel_bytes = frames.numel() * 2
n_spots = int(library[0][-1])
say(f"scan {NAV} of {SIG} uint16 ({pixel_bytes / 2**30:.2f} GiB resident, {UNIQUE} different frames), polar images of "
    f"{N_R} x {N_PHI}, {N_TEMPLATES} templates with {n_spots} spots, n_best 1")

plan = hip.OrientPlan(0, H, W, tap_idx, tap_w, library, 1)
ptr = frames.data_ptr()
tmpl = torch.empty(n_frames, dtype=torch.int32, device='cuda')
rot = torch.empty(n_frames, dtype=torch.int32, device='cuda')
corr = torch.empty(n_frames, dtype=torch.float32, device='cuda')
norm = torch.empty(n_frames, dtype=torch.float32, device='cuda')
sums = torch.empty(n_frames, dtype=torch.float32, device='cuda')
polar = torch.empty((n_frames, N_R * N_PHI), dtype=torch.float32, device='cuda')

s_ms = t(lambda: hip.sum_sig(0, ptr, np.uint16, n_frames, n_px, n_px, sums.data_ptr(), np.float32, False))
say(f"ltmi_sum_sig (the read stream): {s_ms:.3f} ms = {pixel_bytes / s_ms / 1e6:.0f} GB/s "
    f"({pixel_bytes / s_ms / 1e6 / PEAK:.2f} of HBM)")
p_ms = t(lambda: plan.polar(ptr, np.uint16, n_frames, n_px, polar.data_ptr(), N_R * N_PHI))
say(f"ltmi_orient_polar (stage 1 to global memory, {polar.numel() * 4 / 2**30:.2f} GiB written): {p_ms:.3f} ms, "
    f"{p_ms / s_ms:.2f} x ltmi_sum_sig   {plan.last_kernel()}")
m_ms = t(lambda: plan.match(ptr, np.uint16, n_frames, n_px, tmpl.data_ptr(), rot.data_ptr(), corr.data_ptr(),
                            norm.data_ptr()))
lds_bytes = 4. * n_frames * n_spots * N_PHI
model_ms = lds_bytes / LDS_B32 * 1e3
say(f"ltmi_orient_match: {m_ms:.3f} ms = {n_frames / m_ms * 1e3:.0f} frames/s = "
    f"{n_frames * N_TEMPLATES * N_PHI / m_ms / 1e6:.1f} G candidates/s; stage 2 reads {lds_bytes / 1e9:.1f} GB of LDS: "
    f"{model_ms:.3f} ms at 75 TB/s, the kernel runs at {model_ms / m_ms:.2f} of that "
    f"({lds_bytes / m_ms / 1e9:.1f} TB/s)   {plan.last_kernel()}")
got_t, got_r = tmpl.cpu().numpy(), rot.cpu().numpy()
say(f"recovered (template, rotation) of {int(((got_t[:UNIQUE] == truth[:, 0]) & (got_r[:UNIQUE] == truth[:, 1])).sum())} "
    f"of the {UNIQUE} different frames")

torch.set_num_threads(1)
t0 = time.perf_counter()
ref = match_polar(polar_frames(host, tap_idx, tap_w), library, 1)
n_s = time.perf_counter() - t0
say(f"polar_frames + match_polar (NumPy, one core) on {UNIQUE} frames: {n_s * 1e3:.0f} ms = {UNIQUE / n_s:.0f} frames/s, "
    f"{n_s / UNIQUE * n_frames:.0f} s for the scan, {n_s / UNIQUE * n_frames * 1e3 / m_ms:.0f} x the kernel")
assert np.array_equal(ref[0][:, 0], got_t[:UNIQUE]) and np.array_equal(ref[1][:, 0], got_r[:UNIQUE])
assert np.array_equal(ref[2][:, 0], corr.cpu().numpy()[:UNIQUE])
