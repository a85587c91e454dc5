"""FRMS6 load and decode, for the record: a synthetic set of N frames of the real detector's
size (132 x 528 raw -> 264 x 264) written to a local directory, then
  - the whole load: decode_bytes / decode_seconds of ctx.load('frms6', ...) (second load: bounce buffers
    page-locked, files in the page cache), to compare with the staged host-to-device rate (README);
  - the kernel alone: HIP events around ltmi_frms6_decode on resident bytes (vector kernel; the pixel-per-lane
    kernel on the same bytes moved by 2), next to a device-to-device copy of the same bytes and to
    ltmi_mib_decode on 16-bit frames with the same output bytes.

    python scripts/bench_frms6.py [--frames 7680] [--kernel-frames 4096] [--dir /tmp/frms6_bench]
"""
import os
import sys
import argparse

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import frms6_synth as synth  # noqa: E402
from libertem_amd import hip  # noqa: E402
from libertem_amd.api import Context  # noqa: E402

H, W = 132, 528                     # raw (folded) frame
SIG = (2 * H, W // 2)
STRIDE = synth.FRAME_HEADER + H * W * 2
PEAK = 8e12                         # HBM, bytes / s


def median_ms(fn, reps=9):
    for _ in range(3):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


def report(what, ms, moved):
    print(f"{what}: {ms:.3f} ms = {moved / ms / 1e6:.0f} GB/s read + written "
          f"({moved / ms * 1e3 / PEAK * 100:.1f} % of 8 TB/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=7680)          # 1.0 GiB of records
    ap.add_argument('--kernel-frames', type=int, default=4096)   # at most; 535 MB in and out at the defaults: past the 256 MiB L3
    ap.add_argument('--dir', default='/tmp/frms6_bench')
    args = ap.parse_args()
    n = args.frames
    os.makedirs(args.dir, exist_ok=True)
    # 16 different frames, repeated; two signal files
    raw = synth.random_raw(16, H, W, 1)
    half = n // 2
    synth.write_set(args.dir, 'bench', synth.random_raw(16, H, W, 2, high=256),
                    [raw[np.arange(half) % 16], raw[np.arange(n - half) % 16]], (n,), 1)
    hdr = os.path.join(args.dir, 'bench.hdr')
    ctx = Context.make_with('hip', gpus=0)
    for attempt in ('first load', 'second load'):
        ds = ctx.load('frms6', path=hdr)
        print(f"{attempt}: {ds.decode_bytes / 2**30:.2f} GiB of files in {ds.decode_seconds * 1e3:.0f} ms = "
              f"{ds.decode_bytes / ds.decode_seconds / 1e9:.1f} GB/s (decode_bytes / decode_seconds)")
        del ds
    # the kernel on resident bytes
    m = min(half, args.kernel_frames)
    host = np.fromfile(os.path.join(args.dir, 'bench_001.frms6'), dtype=np.uint8, count=m * STRIDE,
                       offset=synth.FILE_HEADER)
    buf = torch.empty(m * STRIDE + 16, dtype=torch.uint8, device='cuda:0')
    out = torch.empty(m * SIG[0] * SIG[1], dtype=torch.int16, device='cuda:0')
    payload = m * H * W * 2
    for shift, kernel in ((0, 'k_frms6_unfold16'), (2, 'k_frms6_unfold2')):
        buf[shift:shift + m * STRIDE] = torch.from_numpy(host).cuda()
        ptr = buf.data_ptr() + shift + synth.FRAME_HEADER
        ms = median_ms(lambda: hip.frms6_decode(0, ptr, STRIDE, m, H, W, 1, out.data_ptr(), np.uint16))
        assert hip.frms6_last_kernel() == kernel
        report(f"ltmi_frms6_decode ({kernel}), {m} frames", ms, 2 * payload)
    want = synth.unfold(raw[np.arange(4) % 16], 1)
    assert np.array_equal(out[:4 * SIG[0] * SIG[1]].cpu().numpy().view(np.uint16).reshape(want.shape), want)
    # a device-to-device copy of the same bytes
    src = torch.empty(payload, dtype=torch.uint8, device='cuda:0')
    dst = out.view(torch.uint8)
    ms = median_ms(lambda: dst.copy_(src))
    report(f"device-to-device copy, {payload / 1e6:.0f} MB", ms, 2 * payload)
    # ltmi_mib_decode, 16-bit big-endian integers, the same output bytes
    stride = 384 + SIG[0] * SIG[1] * 2
    mib = torch.zeros(m * stride, dtype=torch.uint8, device='cuda:0')
    ms = median_ms(lambda: hip.mib_decode(0, mib.data_ptr(), stride, 384, 'u', 16, False, m, SIG[0], SIG[1],
                                          out.data_ptr(), np.uint16))
    report(f"ltmi_mib_decode u16, {m} frames", ms, 2 * payload)
    ctx.close()
    for f in os.listdir(args.dir):
        if f.startswith('bench'):
            os.remove(os.path.join(args.dir, f))


if __name__ == '__main__':
    main()
