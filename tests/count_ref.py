"""
Electron counting: the definition (libertem_amd/udf/counting.py) as the plain loop over pixels
and neighbours in float32, written without a look at `count_frames`, and the inputs the counting tests share.

`CASES` is the table of inputs: name -> builder of (frames (n, h, w), t_bg, t_x, dark, gain).  `reference(name,
values)` computes the loop once per process and hands out the same read-only arrays afterwards.
"""
import functools
import zlib

import numpy as np

DTYPES = ('uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32')
SHAPES = ((1, 1), (1, 7), (7, 1), (3, 3), (16, 16), (33, 35), (70, 66), (130, 64), (5, 515))
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def seed(*what):
    return zlib.crc32(repr(what).encode())


def count_ref(frames, t_bg, t_x=np.inf, dark=None, gain=None, values='count'):
    """-> (indptr int64, indices int32, data uint8 | float32), pixel by pixel"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    t_bg, t_x = np.float32(t_bg), np.float32(t_x)
    indptr, indices, data = [0], [], []
    with np.errstate(all='ignore'):
        for f in range(n):
            u = [[0.0] * w for _ in range(h)]
            for y in range(h):
                for x in range(w):
                    v = np.float32(frames[f, y, x])
                    if dark is not None:
                        v = np.float32(v - np.float32(dark[y, x]))
                    if gain is not None:
                        v = np.float32(v * np.float32(gain[y, x]))
                    u[y][x] = float(v) if v <= t_x else 0.0     # (float32 -> Python float is exact)
            bg = float(t_bg)
            for y in range(h):
                for x in range(w):
                    c = u[y][x]
                    if not c > bg:
                        continue
                    event = True
                    for dy, dx in NEIGHBOURS:
                        yy, xx = y + dy, x + dx
                        if not (0 <= yy < h and 0 <= xx < w):
                            continue
                        earlier = yy * w + xx < y * w + x
                        if (earlier and not c > u[yy][xx]) or (not earlier and not c >= u[yy][xx]):
                            event = False
                            break
                    if event:
                        indices.append(y * w + x)
                        data.append(c)
            indptr.append(len(indices))
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    if values == 'count':
        return indptr, indices, np.ones(len(indices), dtype=np.uint8)
    assert values == 'intensity'
    return indptr, indices, np.asarray(data, dtype=np.float32)


def dense_event_images(indptr, indices, data, shape):
    """the CSR rows as dense frames (n, h, w) of the data's dtype"""
    n = len(indptr) - 1
    out = np.zeros((n, shape[0] * shape[1]), dtype=data.dtype)
    for f in range(n):
        out[f, indices[indptr[f]:indptr[f + 1]]] = data[indptr[f]:indptr[f + 1]]
    return out.reshape((n,) + tuple(shape))


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _random(dtype, shape=(33, 35), n=2):
    """values 0 .. 50 (signed dtypes: -25 .. 50, float32: fractional), many local maxima above t_bg = 30"""
    rng = np.random.default_rng(seed('random', dtype, shape))
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        frames = ((rng.random((n,) + shape) - 0.3) * 70).astype(dt)
    else:
        frames = rng.integers(-25 if dt.kind == 'i' else 0, 50, (n,) + shape, endpoint=True).astype(dt)
    return frames, 30.0, np.inf, None, None


def _large_ints(dtype):
    """32-bit integers that float32 rounds: neighbours that differ as integers and tie as float32"""
    rng = np.random.default_rng(seed('large', dtype))
    base = 2 ** 31 - 300 if dtype == 'int32' else 2 ** 32 - 300
    frames = (base - rng.integers(0, 600, (2, 16, 16))).astype(dtype)
    return frames, 1000.0, np.inf, None, None


def _ties(shape, n):
    """values 0 .. 3: equal maxima side by side everywhere, so on both sides of every strip and chunk boundary"""
    rng = np.random.default_rng(seed('ties', shape))
    return rng.integers(0, 3, (n,) + shape, endpoint=True).astype(np.uint8), 0.5, np.inf, None, None


def _special():
    """t_bg = 5, t_x = 100 on 9 x 9 float32 frames"""
    rng = np.random.default_rng(seed('special'))
    frames = rng.random((3, 9, 9)).astype(np.float32)
    a, b, c = frames
    a[2, 2] = 5.0                      # v == t_bg: no event
    a[2, 6] = 100.0                    # v == t_x: kept, an event
    a[6, 2], a[6, 3] = 200.0, 50.0     # v > t_x: zeroed, and its neighbour becomes the event
    a[6, 6], a[5, 6] = np.nan, 7.0     # NaN becomes 0; its neighbour counts
    b[1, 1] = np.inf                   # > t_x: zeroed
    b[1, 2] = 6.0
    b[4, 4] = -np.inf
    b[4, 5] = 8.0
    b[7, 7], b[7, 8], b[8, 7] = 9.0, 9.0, 9.0      # three equal neighbours: the first wins
    c[:] = np.nan                      # a frame without a number: no event
    return frames, 5.0, 100.0, None, None


def _special_inf():
    """t_x = +inf: +Inf stays and is an event, of two adjacent ones the first; t_bg = -inf: everything is above the
    background but -Inf itself"""
    rng = np.random.default_rng(seed('special-inf'))
    frames = rng.random((2, 9, 9)).astype(np.float32)
    a, b = frames
    a[3, 3], a[3, 4], a[4, 2] = np.inf, np.inf, np.inf
    a[0, 0] = np.nan
    a[8, 8] = -np.inf
    b[:] = -np.inf
    b[4, 4] = np.nan                   # becomes 0, the one value above -inf
    return frames, -np.inf, np.inf, None, None


def _dark_gain(dtype):
    rng = np.random.default_rng(seed('dark-gain', dtype))
    shape = (33, 35)
    frames, _, _, _, _ = _random(dtype, shape, 2)
    dark = (rng.random(shape) * 3).astype(np.float32)
    gain = (0.5 + rng.random(shape)).astype(np.float32)
    gain[5, 5] = 0                     # a dead pixel
    gain[20, 7] = 40                   # a hot one: above t_x after the multiplication
    return frames, 20.0, 90.0, dark, gain


def _dark_only():
    frames, _, _, _, _ = _random('uint16', (16, 16), 2)
    dark = np.full((16, 16), 10.25, dtype=np.float32)
    return frames, 20.0, np.inf, dark, None


def _gain_only():
    frames, _, _, _, _ = _random('int16', (16, 16), 2)
    gain = np.linspace(0.25, 2.0, 256, dtype=np.float32).reshape((16, 16))
    return frames, 20.0, np.inf, None, gain


def _lattice():
    """isolated maxima on a stride-2 lattice: the largest number of events a frame can hold, far more than 64 in
    every 256 pixels"""
    frames = np.zeros((2, 70, 66), dtype=np.uint8)
    frames[:, ::2, ::2] = 9
    frames[1, ::2, ::2] = np.arange(35 * 33).reshape((35, 33)) % 7 + 2
    return frames, 1.0, np.inf, None, None


def _empty_between():
    frames, _, _, _, _ = _ties((16, 16), 3)
    frames[1] = 0
    return frames, 0.5, np.inf, None, None


def strip_edge(strip, w=64):
    """frames of 2 strip + 3 rows with events, ties and near-events on the first and the last row of every strip"""
    h = 2 * strip + 3
    rng = np.random.default_rng(seed('strip-edge', strip, w))
    frames = rng.integers(0, 3, (2, h, w), endpoint=True).astype(np.uint8)
    for k, y in enumerate((strip - 1, strip, 2 * strip - 1, 2 * strip)):
        frames[0, y, 3 + 8 * k] = 9                              # a lone maximum on the edge row
        frames[0, y, 40] = 7                                     # a column of equal values across the edges
    frames[1, strip - 1, 10], frames[1, strip, 11] = 8, 8        # equal, diagonal across the edge: the first wins
    frames[1, strip, 20], frames[1, strip - 1, 21] = 8, 8
    frames[1, 2 * strip, 30], frames[1, 2 * strip - 1, 30] = 6, 5
    return frames, 0.5, np.inf, None, None


CASES = {}
for _dt in DTYPES:
    CASES[f'random-{_dt}'] = functools.partial(_random, _dt)
for _dt in ('uint32', 'int32'):
    CASES[f'large-{_dt}'] = functools.partial(_large_ints, _dt)
for _shape in SHAPES:
    # 7 frames where the loop over them stays short, 1 elsewhere
    CASES['ties-%dx%d' % _shape] = functools.partial(_ties, _shape, 7 if _shape[0] * _shape[1] <= 256 else 1)
CASES['special'] = _special
CASES['special-inf'] = _special_inf
for _dt in ('uint16', 'float32'):
    CASES[f'dark-gain-{_dt}'] = functools.partial(_dark_gain, _dt)
CASES['dark-only'] = _dark_only
CASES['gain-only'] = _gain_only
CASES['lattice'] = _lattice
CASES['empty-between'] = _empty_between


@functools.lru_cache(maxsize=None)
def case(name):
    frames, t_bg, t_x, dark, gain = CASES[name]()
    for a in (frames, dark, gain):
        if a is not None:
            a.setflags(write=False)
    return frames, t_bg, t_x, dark, gain


@functools.lru_cache(maxsize=None)
def reference(name, values='count'):
    """(indptr, indices, data) of a case by the loop, computed once and read-only"""
    if values == 'count':
        indptr, indices, data = reference(name, 'intensity')
        out = (indptr, indices, np.ones(len(indices), dtype=np.uint8))
    else:
        out = count_ref(*case(name), values='intensity')
    for a in out:
        a.setflags(write=False)
    return out
