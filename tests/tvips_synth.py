"""
Synthetic TVIPS series for the tests (a helper, not a test): a seeded writer of `name_000.tvips`, `name_001.tvips`,
... and a plain NumPy decoder that strips the framing file by file -- the CPU yardstick of the TVIPS tests, which
tests/test_tvips_cpu.py pins to the reference's reader through tests/golden/tvips.npz.

The format: `_000` starts with the series header, 256 bytes: thirteen little-endian int32 (header
size 256, version 1 or 2, width, height, bits per pixel, x and y offset, x and y binning, pixel size, high tension,
magnification, image header bytes) and padding; then, in every file, records [image header | pixels].  An image
header has 12 bytes in version 1 and the series header's count in version 2, where it holds the scan position as
float32: Scan_x at byte 68, Scan_y at byte 72.

Image headers and the padding of the series header are written as seeded non-zero noise, so that framing read as
pixels, or a scan position read from the wrong place, shows.
"""
import os

import numpy as np

import records_synth

SERIES_HEADER_SIZE = 256
SERIES_WORDS = ('size', 'version', 'xdim', 'ydim', 'bpp', 'xoff', 'yoff', 'xbin', 'ybin', 'pixel_size_nm',
                'high_tension_kv', 'mag_total', 'frame_header_bytes')
V1_FRAME_HEADER = 12
SCAN_X_AT, SCAN_Y_AT = 68, 72


def noise(rng, shape):
    return rng.integers(1, 256, shape).astype(np.uint8)


def series_header(rng, version, height, width, bpp, frame_header, override=None):
    """-> 256 bytes.  `override`: words to write differently (size=..., version=..., bpp=...)"""
    words = dict(size=SERIES_HEADER_SIZE, version=version, xdim=width, ydim=height, bpp=bpp, xoff=3, yoff=5, xbin=2,
                 ybin=4, pixel_size_nm=7, high_tension_kv=300, mag_total=12000,
                 frame_header_bytes=frame_header if version == 2 else 0)
    words.update(override or {})
    head = noise(rng, SERIES_HEADER_SIZE)
    head[:4 * len(SERIES_WORDS)] = np.array([words[k] for k in SERIES_WORDS], dtype='<i4').view(np.uint8)
    return head


def image_headers(rng, n, frame_header, scan=None):
    """-> (n, frame_header) bytes of noise; scan: n positions (y, x) written as float32 where version 2 keeps them"""
    heads = noise(rng, (n, frame_header))
    if scan is not None:
        assert len(scan) == n and frame_header >= SCAN_Y_AT + 4
        for i, (y, x) in enumerate(scan):
            heads[i, SCAN_X_AT:SCAN_X_AT + 4] = np.array([x], dtype='<f4').view(np.uint8)
            heads[i, SCAN_Y_AT:SCAN_Y_AT + 4] = np.array([y], dtype='<f4').view(np.uint8)
    return heads


def write_series(dirpath, name, frames, version, frame_header, counts, scan=None, seed=0, numbers=None, override=None):
    """frames (n, height, width) uint8 / uint16 -> the files `<name>_%03d.tvips` holding `counts` frames each ->
    their paths.  `frame_header`: image header bytes (version 1: 12); `scan`: (y, x) per frame, version 2;
    `numbers`: the files' numbers (default 0, 1, ...); `override`: series header words"""
    frames = np.ascontiguousarray(frames)
    frames = frames.astype(frames.dtype.newbyteorder('<'))
    n, height, width = frames.shape
    assert sum(counts) == n and (version == 2 or frame_header == V1_FRAME_HEADER)
    rng = np.random.default_rng(seed)
    head = series_header(rng, version, height, width, 8 * frames.dtype.itemsize, frame_header, override)
    heads = image_headers(rng, n, frame_header, scan if version == 2 else None)
    records = np.concatenate([heads, frames.reshape(n, -1).view(np.uint8)], axis=1)
    numbers = list(range(len(counts))) if numbers is None else list(numbers)
    paths, first = [], 0
    for number, count in zip(numbers, counts):
        path = os.path.join(dirpath, "%s_%03d.tvips" % (name, number))
        with open(path, 'wb') as f:
            if number == 0:
                f.write(head.tobytes())
            f.write(records[first:first + count].tobytes())
        paths.append(path)
        first += count
    return paths


def strip_series(paths, counts, frame_header, dtype, frame_shape):
    """the files of a series, by hand -> frames (sum(counts),) + frame_shape: 256 bytes of series header in the first
    file, then records of `frame_header` bytes and one frame each"""
    dtype = np.dtype(dtype)
    payload = int(np.prod(frame_shape)) * dtype.itemsize
    parts = []
    for i, (path, count) in enumerate(zip(paths, counts)):
        data = np.fromfile(path, dtype=np.uint8)
        file_header = SERIES_HEADER_SIZE if i == 0 else 0
        assert len(data) == file_header + count * (frame_header + payload), path
        parts.append(records_synth.strip(data, file_header, frame_header, payload, 0, count, dtype, frame_shape))
    return np.concatenate(parts)
