"""K2IS load and decode, for the record: a synthetic acquisition of N frames written to a
local directory, then
  - the whole load: decode_bytes / decode_seconds of ctx.load('k2is', ...) (second load: bounce buffers
    page-locked, files in the page cache), to compare with the staged host-to-device rate (README);
  - the kernel alone: HIP events around ltmi_k2is_decode on resident bytes, next to ltmi_mib_decode on raw
    12-bit frames with the same output bytes.

    python scripts/bench_k2is.py [--frames 256] [--dir /tmp/k2is_bench]
"""
import os
import sys
import argparse

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import k2is_synth as synth  # noqa: E402
from libertem_amd import hip  # noqa: E402
from libertem_amd.api import Context  # noqa: E402

H, W = synth.FRAME_SHAPE


def median_ms(fn, reps=7):
    for _ in range(2):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--dir', default='/tmp/k2is_bench')
    args = ap.parse_args()
    n = args.frames
    os.makedirs(args.dir, exist_ok=True)
    # 8 different frames, repeated: the headers (frame ids, block counts) run through all n
    frames = synth.random_frames(8, 1)[np.arange(n) % 8]
    paths = synth.write_k2is(args.dir, frames, name='bench')
    del frames
    ctx = Context.make_with('hip', gpus=0)
    for attempt in ('first load', 'second load'):
        ds = ctx.load('k2is', path=paths[0])
        print(f"{attempt}: {ds.decode_bytes / 2**30:.2f} GiB of files in {ds.decode_seconds * 1e3:.0f} ms = "
              f"{ds.decode_bytes / ds.decode_seconds / 1e9:.1f} GB/s (decode_bytes / decode_seconds)")
        del ds
    # the kernel on resident bytes (32 frames: 183 MB in, 244 MB out)
    m = min(n, 32)
    part = m * synth.BLOCKS_PER_FRAME * synth.BLOCK_SIZE
    raw = torch.empty(8 * part, dtype=torch.uint8, device='cuda:0')
    for s, p in enumerate(paths):
        raw[s * part:(s + 1) * part] = torch.from_numpy(np.fromfile(p, dtype=np.uint8, count=part)).cuda()
    out = torch.empty(m * H * W, dtype=torch.int16, device='cuda:0')
    ptrs = [raw.data_ptr() + s * part for s in range(8)]
    ms = median_ms(lambda: hip.k2is_decode(0, ptrs, m, out.data_ptr(), np.uint16))
    moved = 8 * part + m * H * W * 2
    print(f"ltmi_k2is_decode: {m} frames in {ms:.3f} ms = {moved / ms / 1e6:.0f} GB/s read + written "
          f"({moved / ms / 1e6 / 80:.1f} % of 8 TB/s)")
    # ltmi_mib_decode, raw 12 bit (4 pixels per 64-bit word), the same output bytes
    stride = 384 + H * W * 2
    mib = torch.zeros(m * stride, dtype=torch.uint8, device='cuda:0')
    ms = median_ms(lambda: hip.mib_decode(0, mib.data_ptr(), stride, 384, 'r', 12, False, m, H, W,
                                          out.data_ptr(), np.uint16))
    moved = 2 * m * H * W * 2
    print(f"ltmi_mib_decode r12: {m} frames in {ms:.3f} ms = {moved / ms / 1e6:.0f} GB/s read + written "
          f"({moved / ms / 1e6 / 80:.1f} % of 8 TB/s)")
    ctx.close()
    for p in paths:
        os.remove(p)


if __name__ == '__main__':
    main()
