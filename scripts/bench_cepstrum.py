"""CepstrumUDF on a 128 x 128 scan of 256 x 256 uint16 frames of a strained lattice (device resident, 2 GiB) cropped
to 64 x 64: `ltmi_ceps_transform` over the whole scan from HIP events for several batch sizes; beside it, in the same
process and over the same bytes, `ltmi_holo_reconstruct` to 64 x 64 (the same k_corr_load-sized read and the same
batched R2C, then a crop, a small C2C and a store) and `ltmi_sum_sig` (one read of the scan: the HBM read stream);
the whole job through Context.run_udf with the result left on the device; the byte model and its fraction of 8 TB/s.

Byte model, every pass reading and writing HBM once: per frame pixel k_ceps_load 2 + 4 and R2C 4 + 4 (the half spectrum
has w/2+1 of w columns of 8 bytes); per output pixel k_ceps_store 8 + 4: 14 h w + 12 oh ow bytes per frame.  The window
and the scale stay in cache.

    python scripts/bench_cepstrum.py [--quick] [--whole-job]
        --quick: 1/8 of the scan; --whole-job: only the device-resident whole job (for a
        `rocprofv3 --kernel-trace --stats` pass: the hipFFT execution and the two kernels by name)
"""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libertem_amd import hip
from libertem_amd.api import Context
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES
from libertem_amd.udf.cepstrum import CepstrumUDF, hann_window
from libertem_amd.udf.holography import disk_aperture
from libertem_amd.utils.generate import strained_lattice_scan

PEAK = 8000.                # GB/s
quick = '--quick' in sys.argv
whole_job_only = '--whole-job' in sys.argv
SIG = (256, 256)
OUT = (64, 64)
NAV = (128 // (8 if quick else 1), 128)


def t(fn, reps=10):
    fn(); torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


def whole_job(ctx, ds, udf, reps=10):
    for _ in range(2):
        ctx.run_udf(dataset=ds, udf=udf, result_where='device')
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); ctx.run_udf(dataset=ds, udf=udf, result_where='device'); ts.append(time.perf_counter() - t0)
    return np.median(ts) * 1e3


H, W = SIG
n_frames, n_px, n_out = NAV[0] * NAV[1], H * W, OUT[0] * OUT[1]
# one row of the scan with a strain that varies along it, repeated with shot-noise-like offsets drawn on the device
strain = np.zeros((1, NAV[1], 2, 2))
strain[0, :, 0, 0] = np.linspace(-0.03, 0.03, NAV[1])
strain[0, :, 1, 1] = np.linspace(0.02, -0.02, NAV[1])
row = strained_lattice_scan((1, NAV[1]), SIG, (21, 4), (-5, 18), strain=strain, counts=2000.)[0]
g = torch.Generator(device='cuda').manual_seed(7)
fr = torch.from_numpy(row.astype(np.int16)).cuda() + \
    torch.randint(0, 16, NAV + SIG, device='cuda', dtype=torch.int16, generator=g)
ctx = Context.make_with('hip', gpus=0)
ds = ctx.load('memory', data=fr, dtype=np.uint16, sig_dims=2, num_partitions=1)
udf = CepstrumUDF(out_shape=OUT, dc_radius=3.5)
model = n_frames * (14 * n_px + 12 * n_out)
if whole_job_only:
    print(f"CepstrumUDF whole job {NAV + SIG} -> {OUT}, result on the device: {whole_job(ctx, ds, udf):.2f} ms", flush=True)
else:
    per_frame = 4 * n_px + 8 * H * (W // 2 + 1)
    out = torch.empty((n_frames, n_out), device='cuda', dtype=torch.float32)
    window = hann_window(SIG)
    for batch in (64, 256, CORR_WORKSPACE_BYTES // per_frame, 4096):
        batch = min(int(batch), n_frames)
        plan = hip.CepstrumPlan(0, H, W, OUT[0], OUT[1], batch, 1.0, window, 3.5)
        ms = t(lambda: plan.transform(fr.data_ptr(), np.uint16, n_frames, n_px, out.data_ptr(), n_out))
        print(f"ltmi_ceps_transform {NAV + SIG} -> {OUT} batch {batch} ({batch * per_frame / 2**20:.0f} MiB workspace): "
              f"{ms:.2f} ms  {n_frames / ms * 1e3:.0f} frames/s  model {model / 2**30:.2f} GiB = "
              f"{model / ms / 1e6:.0f} GB/s ({model / ms / 1e6 / PEAK:.2f} of HBM)   {plan.last_kernel()}", flush=True)
        plan.close()
    # the same bytes through the holography plan (sideband at the origin: the same 64 x 64 corner of the spectrum)
    batch = min(int(CORR_WORKSPACE_BYTES // (per_frame + 8 * n_out)), n_frames)
    wave = torch.empty((n_frames, n_out), device='cuda', dtype=torch.complex64)
    holo = hip.HoloPlan(0, H, W, OUT[0], OUT[1], batch, 0, 0, disk_aperture(OUT, 24, 2.0))
    ms = t(lambda: holo.reconstruct(fr.data_ptr(), np.uint16, n_frames, n_px, wave.data_ptr(), n_out))
    holo_model = n_frames * (14 * n_px + 52 * n_out)
    print(f"ltmi_holo_reconstruct {NAV + SIG} -> {OUT} batch {batch}: {ms:.2f} ms  {n_frames / ms * 1e3:.0f} frames/s  "
          f"model {holo_model / 2**30:.2f} GiB = {holo_model / ms / 1e6:.0f} GB/s ({holo_model / ms / 1e6 / PEAK:.2f} of HBM)",
          flush=True)
    holo.close()
    del wave
    # ... and one read of them
    sums = torch.empty((n_frames,), device='cuda', dtype=torch.float32)
    ms = t(lambda: hip.sum_sig(0, fr.data_ptr(), np.uint16, n_frames, n_px, n_px, sums.data_ptr(), np.float32, False))
    read = n_frames * n_px * 2
    print(f"ltmi_sum_sig over the same scan: {ms:.2f} ms  {read / 2**30:.2f} GiB = {read / ms / 1e6:.0f} GB/s "
          f"({read / ms / 1e6 / PEAK:.2f} of HBM)", flush=True)
    j_ms = whole_job(ctx, ds, udf)
    print(f"CepstrumUDF whole job {NAV + SIG} -> {OUT}, result on the device: {j_ms:.2f} ms "
          f"({n_frames / j_ms * 1e3:.0f} frames/s)", flush=True)
ctx.close()
