"""Sparse frames against a dense 16-mask float32 stack on one MI355X, per step of 65 536 frames of 256 x 256
uint16 data with uniformly random events at 1 %, 5 % and 20 % density, the CSR triple resident in HBM:

  direct       ltmi_apply_masks_csr (stored entries only)
  materialise  ltmi_csr_densify into a dense window + ltmi_apply_masks on it (what every stack that the direct
               kernel does not take costs)
  dense        ltmi_apply_masks alone on the densified, resident frames (the dense yardstick)

HIP-event times over `--reps` launches after `--warmup`, and bytes/s over the bytes of the triple.

    python scripts/bench_raw_csr.py [--frames 65536] [--out profiles/raw_csr.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from libertem_amd import hip                                   # noqa: E402
from libertem_amd.common.hiparray import HipArray              # noqa: E402

SIG = (256, 256)
N_MASKS = 16


def random_triple(n_frames, density, seed):
    """canonical CSR triple on the device: every pixel of every frame holds an event with probability `density`"""
    n_px = SIG[0] * SIG[1]
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(seed)
    counts, cols = [], []
    for f0 in range(0, n_frames, 1024):
        n = min(1024, n_frames - f0)
        hit = torch.rand((n, n_px), device='cuda:0', generator=gen) < density
        counts.append(hit.sum(dim=1))
        cols.append(hit.nonzero()[:, 1].to(torch.int32))       # (row-major: ascending inside a frame)
        del hit
    indptr = torch.zeros(n_frames + 1, dtype=torch.int64, device='cuda:0')
    indptr[1:] = torch.cumsum(torch.cat(counts), 0)
    indices = torch.cat(cols)
    values = torch.randint(1, 4096, (indices.shape[0],), device='cuda:0', generator=gen, dtype=torch.int16)
    return indptr, indices, values


def timed(fn, warmup, reps):
    s = torch.cuda.current_stream(0)
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=65536)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n, n_px = args.frames, SIG[0] * SIG[1]
    rng = np.random.default_rng(0)
    masks = rng.random((N_MASKS, n_px)).astype(np.float32)
    lines = [f"{n} frames of {SIG[0]}x{SIG[1]} uint16, {N_MASKS} float32 masks, {hip.device_info(0)['name']}; "
             f"ms per step (HIP events, {args.reps} launches after {args.warmup})",
             "density   nnz/frame  triple GiB   direct ms  (GB/s of triple)   materialise ms  (GB/s)   "
             "dense ms   kernels"]
    dense = HipArray.empty((n, n_px), np.uint16, 0)
    for density in (0.01, 0.05, 0.20):
        indptr, indices, values = random_triple(n, density, seed=int(density * 100))
        nnz = int(indices.shape[0])
        triple_bytes = indptr.numel() * 8 + nnz * (4 + 2)
        h = hip.MaskHandle.dense(0, masks, np.float32)
        out = torch.empty((n, N_MASKS), dtype=torch.float32, device='cuda:0')

        def direct():
            assert h.apply_csr(indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), np.uint16, 0, 0, n,
                               out.data_ptr(), N_MASKS, False)

        def densify():
            hip.csr_densify(0, indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), np.uint16, 0, 0, n, n_px,
                            dense.data_ptr(), n_px)

        def dense_only():
            h.apply(dense.data_ptr(), np.uint16, n, n_px, out.data_ptr(), N_MASKS, False)

        def materialise():
            densify()
            dense_only()

        t_direct = timed(direct, args.warmup, args.reps)
        k_direct = h.last_kernel()
        ref = out.clone()
        t_mat = timed(materialise, args.warmup, args.reps)
        t_dense = timed(dense_only, args.warmup, args.reps)
        k_dense = h.last_kernel()
        # the two routes compute the same product (float32 round-off apart)
        err = float(((out - ref).abs().max() / ref.abs().max()).cpu())
        assert err < 1e-4, err
        lines.append(f"{density:7.2f} {nnz / n:11.1f} {triple_bytes / 2**30:11.3f} {t_direct:11.3f} "
                     f"{triple_bytes / t_direct / 1e6:12.1f} {t_mat:20.3f} {triple_bytes / t_mat / 1e6:9.1f} "
                     f"{t_dense:10.3f}   {k_direct.split(' grid')[0]} | {k_dense.split(' grid')[0]}")
        print(lines[-1], flush=True)
        h.close()
        del indptr, indices, values, out, ref
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
