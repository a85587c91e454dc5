"""Record-file load and gather, for the record.

  --loads    the whole load of three real geometries, files written to --dir and read back from the page cache:
             decode_bytes / decode_seconds of ctx.load(...) (second load: bounce buffers page-locked), to compare
             with the 38 - 41 GB/s of .mib and K2IS loads.  EMPAD 256 x 256 scan; SEQ 1024 x 1024 uint16 with an
             8-byte footer, 4096 frames; BLO 144 x 144 uint8, 256 x 256 scan.
  --kernels  the kernel alone on resident bytes past the 256 MiB Infinity Cache: k_records<16> on EMPAD's records,
             k_records<2> on BLO's, each next to a hipMemcpy2DAsync device-to-device copy of the same geometry;
             HIP events here, and the launches are few and plain so that a kernel trace of this run can be read.

    python scripts/bench_records.py --loads [--scale 1.0] [--dir /tmp/records_bench]
    python scripts/bench_records.py --kernels
"""
import os
import sys
import ctypes
import argparse

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import records_synth as synth  # noqa: E402
from libertem_amd import hip  # noqa: E402
from libertem_amd.api import Context  # noqa: E402

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
          f"({moved / ms * 1e3 / PEAK * 100:.1f} % of 8 TB/s)", flush=True)


def write_repeated(path, head, block, n_blocks, tail):
    with open(path, 'wb') as f:
        f.write(head)
        for _ in range(n_blocks):
            f.write(block)
        f.write(tail)


def write_empad(dirpath, scale, rng):
    ny = max(2, int(256 * scale))
    frames = rng.integers(0, 4096, (64, 128, 128)).astype(np.float32)
    write_repeated(os.path.join(dirpath, 'bench_empad.raw'), b'', synth.records(frames, 0, 1024).tobytes(),
                   ny * 256 // 64, b'')
    xml = synth.write_empad_xml(os.path.join(dirpath, 'bench_empad.xml'), 'bench_empad.raw', acquire=(ny, 256))
    return 'EMPAD %d x 256 scan' % ny, 'empad', dict(path=xml), frames, ny * 256


def write_seq(dirpath, scale, rng):
    n = max(64, int(4096 * scale) // 64 * 64)
    frames = rng.integers(0, 4096, (64, 1024, 1024)).astype(np.uint16)
    data = synth.seq_bytes(frames, 8)
    path = os.path.join(dirpath, 'bench.seq')
    write_repeated(path, data[:8192].tobytes(), data[8192:].tobytes(), n // 64, b'')
    return 'SEQ 1024 x 1024 uint16, %d frames' % n, 'seq', dict(path=path, nav_shape=(n,)), frames, n


def write_blo(dirpath, scale, rng):
    ny = max(2, int(256 * scale))
    frames = rng.integers(0, 256, (64, 144, 144)).astype(np.uint8)
    data, offset = synth.blo_bytes(frames, (1, 64), magic=258)
    head = data[:offset].copy()
    fields = head[:240].view(synth.blo_header_dtype('<'))
    fields['NY'], fields['NX'] = ny, 256
    path = os.path.join(dirpath, 'bench.blo')
    write_repeated(path, head.tobytes(), synth.records(frames, 6, 0).tobytes(), ny * 256 // 64, b'')
    return 'BLO 144 x 144 uint8, %d x 256 scan' % ny, 'blo', dict(path=path), frames, ny * 256


def loads(args):
    """64 different frames per file, repeated; one file at a time"""
    os.makedirs(args.dir, exist_ok=True)
    rng = np.random.default_rng(1)
    ctx = Context.make_with('hip', gpus=0)
    for write in (write_empad, write_seq, write_blo):
        try:
            name, kind, kwargs, frames, n = write(args.dir, args.scale, rng)
            for attempt in ('first load', 'second load', 'third load'):
                ds = ctx.load(kind, **kwargs)
                print(f"{name}, {attempt}: {ds.decode_bytes / 2**30:.2f} GiB of file in "
                      f"{ds.decode_seconds * 1e3:.0f} ms = {ds.decode_bytes / ds.decode_seconds / 1e9:.1f} GB/s "
                      f"(decode_bytes / decode_seconds), {hip.records_last_kernel()}", flush=True)
                for local0, want in ((0, frames[:2]), (n - 1, frames[63:])):
                    arr, row0 = ds.device_frames(local0, len(want))
                    got = arr.rows(row0, row0 + len(want)).cpu().reshape(want.shape)
                    assert np.array_equal(got, want), (name, local0)
                del ds, arr, got
        finally:
            for f in os.listdir(args.dir):
                if f.startswith('bench'):
                    os.remove(os.path.join(args.dir, f))
    ctx.close()


def kernels(args):
    rt = ctypes.CDLL('libamdhip64.so')
    rt.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    device_to_device = 3
    torch.cuda.init()
    # (frame header, payload, footer, frames, source shift): > 500 MB in and out each
    for what, frame_header, payload, footer, n, shift in (('EMPAD records', 0, 65536, 1024, 8192, 0),
                                                          ('BLO 144 x 144 records', 6, 20736, 0, 25600, 0)):
        stride = frame_header + payload + footer
        src = torch.randint(0, 256, (n * stride + 16,), dtype=torch.uint8, device='cuda:0')
        dst = torch.zeros(n * payload, dtype=torch.uint8, device='cuda:0')
        ptr = src.data_ptr() + shift + frame_header
        ms = median_ms(lambda: hip.records_gather(0, ptr, stride, n, payload, dst.data_ptr()))
        kernel = hip.records_last_kernel()
        report(f"ltmi_records_gather ({kernel}), {what}, {n} frames", ms, 2 * n * payload)
        first = src[shift + frame_header:shift + frame_header + payload]
        last = src[shift + frame_header + (n - 1) * stride:][:payload]
        assert torch.equal(dst[:payload], first) and torch.equal(dst[(n - 1) * payload:], last)
        stream = torch.cuda.current_stream().cuda_stream

        def copy2d():
            rc = rt.hipMemcpy2DAsync(dst.data_ptr(), payload, ptr, stride, payload, n, device_to_device, stream)
            assert rc == 0, rc
        dst.zero_()
        ms = median_ms(copy2d)
        report(f"hipMemcpy2DAsync device-to-device, {what}, {n} rows", ms, 2 * n * payload)
        assert torch.equal(dst[(n - 1) * payload:], last)
        del src, dst


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--loads', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--dir', default='/tmp/records_bench')
    a = ap.parse_args()
    if a.loads:
        loads(a)
    if a.kernels:
        kernels(a)
