#!/usr/bin/env python
"""
Speed of the device transposition (ltmi_transpose2d, csrc/ltmi_transpose.hip) and of the transposed-data converter
built on it.  One process, HIP events for the kernel, wall clock for the conversion.

Kernel: a rows x cols array (default 4096 x 65536) of 1-, 2-, 4- and 8-byte elements, the median of 20 launches
after 3 warm-ups, as 2 * rows * cols * item_bytes / time in TB/s and as a fraction of the 8 TB/s HBM peak; in the
same run `torch.Tensor.t().contiguous()` on the same buffer, the yardstick.

End to end: `convert_transposed` of a 1 GiB uint16 (sig, nav) MemoryDataSet into a .npy file in /dev/shm (a
temporary directory if there is none), once on the hip executor and once on `Context(InlineJobExecutor())`, where
the UDF runs the reference's NumPy lines.

    python scripts/bench_transpose.py [--rows R --cols C] [--gib G] [--skip-e2e]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12


def median_ms(fn, torch, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times))


def bench_kernel(rows, cols):
    import torch
    from libertem_amd import hip
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    print(f"kernel: {rows} x {cols}, median of 20 launches after 3 warm-ups")
    for ib in (1, 2, 4, 8):
        src = torch.randint(0, 127, (rows, cols), dtype=torch.uint8, device='cuda:0').to(tdt[ib])
        dst = torch.empty((cols, rows), dtype=tdt[ib], device='cuda:0')
        stream = torch.cuda.current_stream().cuda_stream
        sp, dp = src.data_ptr(), dst.data_ptr()
        ours, ours_min = median_ms(lambda: hip.transpose2d(0, sp, cols, rows, cols, ib, dp, rows, stream), torch)
        assert torch.equal(dst, src.t())
        ref, ref_min = median_ms(lambda: src.t().contiguous(), torch)
        nbytes = 2 * rows * cols * ib
        rate, ref_rate = nbytes / (ours * 1e-3), nbytes / (ref * 1e-3)
        print(f"  item_bytes={ib}  {hip.transpose_last_kernel():<16} {ours:8.3f} ms (min {ours_min:.3f})  "
              f"{rate / 1e12:6.3f} TB/s  {100 * rate / HBM_PEAK:5.1f} % of peak   |  torch t().contiguous() "
              f"{ref:8.3f} ms (min {ref_min:.3f})  {ref_rate / 1e12:6.3f} TB/s   |  kernel / torch time "
              f"{ours / ref:5.2f}", flush=True)
        del src, dst
        torch.cuda.empty_cache()


def bench_convert(gib):
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    from libertem_amd.contrib.convert_transposed import convert_transposed
    n_sig_px = 128 * 128                                    # detector pixels S: the nav axes of the stored order
    n_nav = int(gib * (1 << 30)) // (2 * n_sig_px)          # scan positions N
    shape = (128, 128, n_nav // 256, 256)
    data = (np.arange(int(np.prod(shape)), dtype=np.uint32) % 4093).astype(np.uint16).reshape(shape)
    tmp_root = '/dev/shm' if os.path.isdir('/dev/shm') else None
    print(f"convert_transposed: uint16 {shape} = {data.nbytes / (1 << 30):.2f} GiB, 8 partitions, output in "
          f"{tmp_root or tempfile.gettempdir()}")
    for label, make in (('hip executor', lambda: Context.make_with('hip', gpus=0)),
                        ('inline executor (NumPy)', lambda: Context(executor=InlineJobExecutor()))):
        ctx = make()
        try:
            with tempfile.TemporaryDirectory(dir=tmp_root) as tmp:
                ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=8)
                times = []
                for rep in range(2):
                    path = os.path.join(tmp, f'out{rep}.npy')
                    t0 = time.perf_counter()
                    convert_transposed(ctx, ds, path)
                    times.append(time.perf_counter() - t0)
                    if rep == 0:
                        out = np.load(path, mmap_mode='r')
                        assert out.shape == shape[2:] + shape[:2]
                        probe = out.reshape(-1, n_sig_px)[::4099]
                        assert np.array_equal(probe, data.reshape(n_sig_px, -1).T[::4099])
                        del out, probe
                    os.unlink(path)
                print(f"  {label:<26} " + '  '.join(f"run {i + 1}: {t:7.2f} s ({data.nbytes / t / 1e9:5.2f} GB/s)"
                                                     for i, t in enumerate(times)), flush=True)
        finally:
            ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--cols', type=int, default=65536)
    ap.add_argument('--gib', type=float, default=1.0)
    ap.add_argument('--skip-e2e', action='store_true')
    args = ap.parse_args()
    import torch
    print(f"device: {torch.cuda.get_device_name(0)}")
    bench_kernel(args.rows, args.cols)
    if not args.skip_e2e:
        bench_convert(args.gib)


if __name__ == '__main__':
    main()
