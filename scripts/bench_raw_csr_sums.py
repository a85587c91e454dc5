"""SumSigUDF's and SumUDF's kernels on sparse frames on one MI355X, per step of 65 536 frames of uint16 data, the
CSR triple resident in HBM:

  sum_sig     ltmi_csr_sum_sig (stored entries only)       against ltmi_csr_densify + ltmi_sum_sig
  sum_frames  ltmi_csr_sum_frames (stored entries only)    against ltmi_csr_densify + ltmi_sum_frames

The second of each pair is what a tile cost before the sparse kernels existed.  Cases: 256 x 256 frames with
uniformly random events at 1 %, 5 % and 20 % fill, 512 x 512 at 0.5 %, and 256 x 256 at 1 % with 1 % of every frame's
events on 16 central pixels (a beam: the pixels that every frame hits).  HIP-event times over `--reps` launches
after `--warmup`, the four routes in turn, `--rounds` times: the median of the rounds, and the largest distance of
a round from its median as the spread.  Every pair is checked for equal results.

    python scripts/bench_raw_csr_sums.py [--frames 65536] [--out profiles/raw_csr_sums.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..'), HERE]
from libertem_amd import hip                                   # noqa: E402
from libertem_amd.common.hiparray import HipArray              # noqa: E402
from bench_raw_csr import timed                                # noqa: E402  (scripts/, next to this file)

# (name, sig, fill, beam)
CASES = (('1 %', (256, 256), 0.01, False), ('5 %', (256, 256), 0.05, False), ('20 %', (256, 256), 0.20, False),
         ('512x512 0.5 %', (512, 512), 0.005, False), ('1 % + beam', (256, 256), 0.01, True))


def random_triple(n_frames, sig, fill, beam, seed):
    """canonical CSR triple on the device: every pixel of every frame holds an event with probability `fill`;
    beam: each of the 16 central pixels (4 x 4) is hit with the probability that puts 1 % of a frame's events there"""
    n_px = sig[0] * sig[1]
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(seed)
    prob = torch.full((n_px,), fill, device='cuda:0')
    if beam:
        cy, cx = sig[0] // 2, sig[1] // 2
        centre = (torch.arange(cy - 2, cy + 2, device='cuda:0')[:, None] * sig[1]
                  + torch.arange(cx - 2, cx + 2, device='cuda:0')[None, :]).reshape(-1)
        prob[centre] = min(1.0, 0.01 * fill * n_px / 16)
    step = max(1, (1 << 26) // n_px)
    counts, cols = [], []
    for f0 in range(0, n_frames, step):
        n = min(step, n_frames - f0)
        hit = torch.rand((n, n_px), device='cuda:0', generator=gen) < prob
        counts.append(hit.sum(dim=1))
        cols.append(hit.nonzero()[:, 1].to(torch.int32))       # (row-major: ascending inside a frame)
        del hit
    indptr = torch.zeros(n_frames + 1, dtype=torch.int64, device='cuda:0')
    indptr[1:] = torch.cumsum(torch.cat(counts), 0)
    indices = torch.cat(cols)
    values = torch.randint(1, 4096, (indices.shape[0],), device='cuda:0', generator=gen, dtype=torch.int16)
    return indptr, indices, values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=65536)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    n = args.frames
    lines = [f"{n} frames of uint16, float32 results, {hip.device_info(0)['name']}; ms per step (HIP events, "
             f"{args.reps} launches after {args.warmup}, median of {args.rounds} alternating rounds); dense route = "
             "ltmi_csr_densify + the dense kernel; GB/s over the bytes of the triple; spread = largest distance of "
             "a round from its median",
             "case             nnz/frame  triple GiB |  csr_sum_sig  (GB/s)  dense route   ratio |  "
             "csr_sum_frames  (GB/s)  dense route   ratio | spread"]
    for k, (name, sig, fill, beam) in enumerate(CASES):
        n_px = sig[0] * sig[1]
        indptr, indices, values = random_triple(n, sig, fill, beam, seed=k + 1)
        nnz = int(indices.shape[0])
        triple_bytes = indptr.numel() * 8 + nnz * (4 + 2)
        dense = HipArray.empty((n, n_px), np.uint16, 0)
        sig_a = torch.empty(n, dtype=torch.float32, device='cuda:0')
        sig_b = torch.empty(n, dtype=torch.float32, device='cuda:0')
        img_a = torch.empty(n_px, dtype=torch.float32, device='cuda:0')
        img_b = torch.empty(n_px, dtype=torch.float32, device='cuda:0')
        ws_csr = torch.empty(hip.csr_sum_frames_workspace(n_px), dtype=torch.uint8, device='cuda:0')
        ws_dense = torch.empty(max(16, hip.sum_frames_workspace(n, n_px, np.float32)), dtype=torch.uint8,
                               device='cuda:0')
        triple = (indptr.data_ptr(), indices.data_ptr(), values.data_ptr(), np.uint16, 0, 0, n, n_px)

        def densify():
            hip.csr_densify(0, *triple, dense.data_ptr(), n_px)

        def csr_sig():
            hip.csr_sum_sig(0, *triple, sig_a.data_ptr(), np.float32, False)

        def dense_sig():
            densify()
            hip.sum_sig(0, dense.data_ptr(), np.uint16, n, n_px, n_px, sig_b.data_ptr(), np.float32, False)

        def csr_frames():
            hip.csr_sum_frames(0, *triple, img_a.data_ptr(), np.float32, False, ws_csr.data_ptr())

        def dense_frames():
            densify()
            hip.sum_frames(0, dense.data_ptr(), np.uint16, n, n_px, n_px, img_b.data_ptr(), np.float32, False,
                           ws_dense.data_ptr())

        fns = (csr_sig, dense_sig, csr_frames, dense_frames)
        rounds = [{fn.__name__: timed(fn, args.warmup, args.reps) for fn in fns} for _ in range(args.rounds)]
        t = {fn.__name__: float(np.median([r[fn.__name__] for r in rounds])) for fn in fns}
        spread = max(abs(r[k] - t[k]) / t[k] for r in rounds for k in t)
        # the two routes compute the same sums (the dense kernels sum in float32: round-off apart)
        for a, b in ((sig_a, sig_b), (img_a, img_b)):
            err = float(((a - b).abs().max() / b.abs().max()).cpu())
            assert err < 1e-4, err
        gbs = lambda ms: triple_bytes / ms / 1e6                  # noqa: E731
        lines.append(f"{name:16s} {nnz / n:9.1f} {triple_bytes / 2**30:11.3f} | {t['csr_sig']:12.3f} "
                     f"{gbs(t['csr_sig']):7.0f} {t['dense_sig']:12.3f} {t['dense_sig'] / t['csr_sig']:7.1f} | "
                     f"{t['csr_frames']:15.3f} {gbs(t['csr_frames']):7.0f} {t['dense_frames']:12.3f} "
                     f"{t['dense_frames'] / t['csr_frames']:7.1f} | {100 * spread:5.1f} %")
        print(lines[-1], flush=True)
        del indptr, indices, values, dense, sig_a, sig_b, img_a, img_b, ws_csr, ws_dense
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
