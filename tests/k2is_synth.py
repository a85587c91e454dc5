"""
Synthetic Gatan K2 IS acquisitions for the tests (a helper, not a test): a writer of the 8 sector files from
an array of frames, and a plain NumPy decoder of such files -- the CPU yardstick of the K2IS tests, which
tests/test_k2is_cpu.py pins to the reference's decoder through tests/golden/k2is.npz.

The format (written from its description, see DESIGN.md "K2IS"): sector s (file `*_{s+1}.bin`) holds the
frame columns [256 s, 256 s + 256) as blocks of 0x5758 bytes = a 40-byte big-endian header + 930 rows x 16
pixels packed 12 bit little-endian (a = b0 | (b1 & 0x0F) << 8, b = b1 >> 4 | b2 << 4); a frame is 32
consecutive blocks per sector, block k covers the rows [930 (k // 16), +930) and the sector columns
[16 (15 - k % 16), +16).
"""
import os

import numpy as np


def _frames_in_mappings_of_their_own():
    """Frames are 7.6 MB, sets of them up to 61 MB.  glibc raises its mmap threshold to the size of the first
    such array that is freed (up to 32 MiB) and serves the later ones from the heap, which then keeps tens of
    MB of free chunks for the rest of the process -- and tests/test_runtime_cpu.py expects a fresh 40 MiB array
    to get a mapping of its own.  A fixed threshold keeps these arrays out of the heap altogether."""
    import ctypes
    try:
        ctypes.CDLL(None).mallopt(-3, 1 << 20)          # M_MMAP_THRESHOLD
    except (AttributeError, OSError):                   # not glibc
        pass


_frames_in_mappings_of_their_own()

HEADER_SIZE = 40
BLOCK_SIZE = 0x5758
DATA_SIZE = BLOCK_SIZE - HEADER_SIZE
BLOCKS_PER_FRAME = 32
NUM_SECTORS = 8
FRAME_SHAPE = (1860, 2048)
SYNC_WORD = 0xFFFF0055

HEADER_DTYPE = np.dtype([
    ('sync', '>u4'), ('pad1', 'V4'), ('version', 'u1'), ('flags', 'u1'), ('pad2', 'V6'),
    ('block_count', '>u4'), ('width', '>u2'), ('height', '>u2'), ('frame_id', '>u4'),
    ('pixel_x_start', '>u2'), ('pixel_y_start', '>u2'), ('pixel_x_end', '>u2'), ('pixel_y_end', '>u2'),
    ('block_size', '>u4'),
])
assert HEADER_DTYPE.itemsize == HEADER_SIZE


def random_frames(n, seed):
    """(n, 1860, 2048) uint16 with values < 4096 from a seed"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4096, (n,) + FRAME_SHAPE, dtype=np.uint16)


def pack_uint12(px):
    """(..., 2 m) uint16 < 4096 -> (..., 3 m) uint8"""
    px = np.asarray(px, dtype=np.uint16)
    a, b = px[..., 0::2], px[..., 1::2]
    out = np.empty(px.shape[:-1] + (px.shape[-1] // 2, 3), dtype=np.uint8)
    out[..., 0] = a & 0xFF
    out[..., 1] = (a >> 8) | ((b & 0xF) << 4)
    out[..., 2] = b >> 4
    return out.reshape(px.shape[:-1] + (px.shape[-1] // 2 * 3,))


def unpack_uint12(raw):
    """(..., 3 m) uint8 -> (..., 2 m) uint16"""
    t = np.asarray(raw, dtype=np.uint8).reshape(raw.shape[:-1] + (raw.shape[-1] // 3, 3)).astype(np.uint16)
    out = np.empty(t.shape[:-1] + (2,), dtype=np.uint16)
    out[..., 0] = t[..., 0] | ((t[..., 1] & 0x0F) << 8)
    out[..., 1] = (t[..., 1] >> 4) | (t[..., 2] << 4)
    return out.reshape(raw.shape[:-1] + (raw.shape[-1] // 3 * 2,))


def sector_payload(frames, s):
    """payload bytes of sector `s`: (n, 32, 22320) uint8, block k of every frame in file order"""
    frames = np.asarray(frames)
    n = frames.shape[0]
    strip = frames[:, :, 256 * s:256 * (s + 1)].reshape(n, 2, 930, 16, 16)      # (n, half, row, j, px)
    blocks = strip.transpose(0, 1, 3, 2, 4)[:, :, ::-1]                        # (n, half, 15 - j, row, px)
    return pack_uint12(np.ascontiguousarray(blocks).reshape(n, BLOCKS_PER_FRAME, 930, 16)).reshape(
        n, BLOCKS_PER_FRAME, DATA_SIZE)


def block_headers(frame_ids, flags, first_block_count, k=None):
    """headers of the blocks `k` (default 0 ... 31) of the frames `frame_ids`, block_count running per block"""
    frame_ids = np.asarray(frame_ids)
    k = np.arange(BLOCKS_PER_FRAME) if k is None else np.asarray(k)
    h = np.zeros((len(frame_ids), len(k)), dtype=HEADER_DTYPE)
    h['sync'] = SYNC_WORD
    h['version'] = 1
    h['flags'] = np.asarray(flags)[:, None]
    h['block_count'] = first_block_count + np.arange(h.size).reshape(h.shape)
    h['width'], h['height'] = 256, 1860
    h['frame_id'] = frame_ids[:, None]
    h['pixel_x_start'] = 16 * (15 - k % 16)
    h['pixel_y_start'] = 930 * (k // 16)
    h['pixel_x_end'] = h['pixel_x_start'] + 15
    h['pixel_y_end'] = h['pixel_y_start'] + 929
    h['block_size'] = BLOCK_SIZE
    return h


def write_k2is(dirpath, frames, name='k2', lead=0, extra=None, trailing=None, first_frame_id=1000):
    """
    Write `{name}_1.bin` ... `{name}_8.bin` -> list of the 8 paths.

    frames : (n, 1860, 2048) uint16 < 4096; the first `lead` of them without the shutter flag
    extra : per sector, blocks of the frame before the first one that precede it in the file (the tail of a
        frame whose head was not recorded: an unsynchronised start)
    trailing : per sector, blocks of a frame after the last one (a truncated last frame)
    """
    frames = np.asarray(frames)
    n = frames.shape[0]
    extra = [0] * NUM_SECTORS if extra is None else list(extra)
    trailing = [0] * NUM_SECTORS if trailing is None else list(trailing)
    ids = first_frame_id + np.arange(n)
    flags = (np.arange(n) >= lead).astype(np.uint8)
    first_count = 5000 + max(extra)                         # block_count of block 0 of frame 0, every sector
    paths = []
    for s in range(NUM_SECTORS):
        rec = np.zeros((n, BLOCKS_PER_FRAME), dtype=[('h', HEADER_DTYPE), ('d', np.uint8, DATA_SIZE)])
        rec['h'] = block_headers(ids, flags, first_count)
        rec['d'] = sector_payload(frames, s)
        path = os.path.join(dirpath, f'{name}_{s + 1}.bin')
        with open(path, 'wb') as f:
            for count, frame_id, ks, first in (
                    (extra[s], first_frame_id - 1, np.arange(32 - extra[s], 32), first_count - extra[s]),
                    (None, None, None, None),
                    (trailing[s], first_frame_id + n, np.arange(trailing[s]), first_count + 32 * n)):
                if count is None:
                    rec.tofile(f)
                elif count:
                    part = np.zeros(count, dtype=rec.dtype)
                    part['h'] = block_headers([frame_id], [0], first, k=ks)[0]
                    part['d'] = 0x5A
                    part.tofile(f)
        paths.append(path)
    return paths


def read_headers(path):
    """all block headers of a sector file (whole blocks only)"""
    n = os.path.getsize(path) // BLOCK_SIZE
    raw = np.memmap(path, dtype=np.uint8, mode='r', shape=(n, BLOCK_SIZE))
    return np.ascontiguousarray(raw[:, :HEADER_SIZE]).view(HEADER_DTYPE).reshape(n)


def decode_blocks(blocks):
    """(n, 32, 22360) uint8 blocks of ONE sector (headers included) -> (n, 1860, 256) uint16"""
    blocks = np.asarray(blocks)
    n = blocks.shape[0]
    px = unpack_uint12(blocks[:, :, HEADER_SIZE:].reshape(n, 2, 16, 930, 24))  # (n, half, k % 16, row, 16 px)
    px = px[:, :, ::-1].transpose(0, 1, 3, 2, 4)                               # (n, half, row, strip, px)
    return np.ascontiguousarray(px).reshape(n, 1860, 256)


def decode_files(paths):
    """
    The whole frames of a synthetic set, found by their headers alone: a frame is whole if every sector holds
    32 blocks with its frame_id.  -> (frames (m, 1860, 2048) uint16, shutter (m,) bool, frame_ids (m,))
    """
    paths = sorted(paths)
    assert len(paths) == NUM_SECTORS
    heads = [read_headers(p) for p in paths]
    whole = None
    for h in heads:
        ids, counts = np.unique(h['frame_id'], return_counts=True)
        mine = set(ids[counts == BLOCKS_PER_FRAME].tolist())
        whole = mine if whole is None else whole & mine
    ids = np.array(sorted(whole), dtype=np.int64)
    frames = np.zeros((len(ids),) + FRAME_SHAPE, dtype=np.uint16)
    shutter = np.zeros(len(ids), dtype=bool)
    for s, (p, h) in enumerate(zip(paths, heads)):
        raw = np.memmap(p, dtype=np.uint8, mode='r', shape=(len(h), BLOCK_SIZE))
        for i, frame_id in enumerate(ids):
            idx = np.flatnonzero(h['frame_id'] == frame_id)
            assert np.array_equal(idx, idx[0] + np.arange(BLOCKS_PER_FRAME))
            frames[i, :, 256 * s:256 * (s + 1)] = decode_blocks(raw[idx][None])[0]
            shutter[i] = bool(h['flags'][idx[0]] & 1)
    return frames, shutter, ids


def positioned(frames, n_nav, sync_offset):
    """frame g at scan position g - sync_offset, zero frames elsewhere -> (n_nav, 1860, 2048)"""
    out = np.zeros((n_nav,) + FRAME_SHAPE, dtype=np.uint16)
    for p in range(n_nav):
        if 0 <= p + sync_offset < len(frames):
            out[p] = frames[p + sync_offset]
    return out
