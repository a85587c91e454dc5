"""
Ground truth of the cepstrum tests: the definition of CepstrumUDF restated in float64 index by
index -- explicit DFT phases at the SIGNED quefrency of every output element, no fft2, roll, fftshift or crop, so a
mistake in the index arithmetic of the code under test cannot be made here a second time --, the case table of the
kernel tests, seeded frame makers and the comparison the device tests share.

Output element (u, v) of an (oh, ow) output holds the signed quefrency (qy, qx) = (u - oh // 2, v - ow // 2).  For a
frame y of (h, w) (rounded to float32 first), the float32 offset and the float32 window:

    z         = log(max(y, 0) + offset)
    out[u, v] = |sum_mn z[m, n] window[m, n] exp(-2 pi i (qy m / h + qx n / w))| / (h w) * keep[u, v]
    keep[u, v] = 0 if hypot(qy, qx) < dc_radius else 1

The bound of the device results, per frame in the 2-norm over the whole output:

    |dev - ref|_2 <= C eps32 (log2(h w) + 2) |(1 + |z|) window|_2 / sqrt(h w),        C = 8

from the normwise error of one float32 FFT (eps32 log2(N) of the norm of what it transforms; |C|_2 <= |t|_2 / sqrt(h w)
over all h w quefrencies), an input error of at most 3 eps32 (1 + |z|) |window| per pixel (one add, a 1-ulp logf and
one multiply: the add's relative error eps32 / 2 of the argument moves the logarithm by eps32 / 2 absolutely, hence the
1 beside |z|) and three more roundings for the square root and the scale: log2(h w) + 2 covers them with C = 8, the
constant tests/holo_ref.py uses.  On the CPU a float32 NumPy path (float32 rfft2, then `store` below) stays at 0.0025
to 0.0076 of the bound on these shapes with `noise_frames`, and an output shifted by one row exceeds it 68 000 times.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
C_BOUND = 8.0

# (h, w), (oh, ow): even and odd sizes; output equal to the frame (both halves, row 0, both Nyquist lines); a single
# element; one column
CASES = [((16, 16), (8, 8)), ((15, 17), (7, 5)), ((16, 12), (16, 12)), ((32, 20), (6, 9)), ((16, 16), (1, 1)),
         ((9, 8), (9, 1)), ((8, 9), (8, 9))]


def case_id(case):
    (h, w), (oh, ow) = case
    return f"{h}x{w}-{oh}x{ow}"


def quefrencies(n_out):
    """the signed quefrency of every index of an output axis of n_out: index n_out // 2 holds 0"""
    return np.array([i - n_out // 2 for i in range(n_out)], dtype=np.int64)


def _phases(q, n):
    """exp(-2 pi i q[a] m / n) for m in [0, n): (len(q), n); the integer product is reduced mod n first"""
    qm = (np.asarray(q, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    return np.exp(-2j * np.pi * qm / n)


def hann(sig):
    """the periodic Hann window, element by element in float64 -> float32 (h, w)"""
    h, w = sig
    out = np.empty((h, w), dtype=np.float64)
    for i in range(h):
        for j in range(w):
            out[i, j] = (0.5 - 0.5 * np.cos(2 * np.pi * i / h)) * (0.5 - 0.5 * np.cos(2 * np.pi * j / w))
    return out.astype(np.float32)


def keep(out_shape, dc_radius):
    oh, ow = out_shape
    out = np.ones((oh, ow), dtype=np.float64)
    for u in range(oh):
        for v in range(ow):
            if np.hypot(float(u - oh // 2), float(v - ow // 2)) < dc_radius:
                out[u, v] = 0.0
    return out


def window_for(case, seed=0):
    """a float32 window without any symmetry, values in [0.25, 1]: a transposed or mirrored index shows"""
    rng = np.random.default_rng([seed, 1] + [int(v) for pair in case for v in pair])
    return rng.uniform(0.25, 1.0, case[0]).astype(np.float32)


def log_frames(frames, offset):
    """z of the definition in float64: (n, h, w)"""
    y = np.asarray(frames).astype(np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        return np.log(np.maximum(y, 0.0) + float(np.float32(offset)))


def reference(frames, out_shape, offset, window, dc_radius=0.0):
    """the definition for frames (n, h, w) -> float64 (n, oh, ow); `window`: float32 (h, w) or None for the Hann
    window.  A frame with a non-finite pixel gives NaN."""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    oh, ow = out_shape
    win = (hann((h, w)) if window is None else np.asarray(window, dtype=np.float32)).astype(np.float64)
    t = log_frames(frames, offset) * win[None]
    e_y = _phases(quefrencies(oh), h)                        # (oh, h)
    e_x = _phases(quefrencies(ow), w)                        # (ow, w)
    k = keep(out_shape, dc_radius)
    out = np.empty((n, oh, ow), dtype=np.float64)
    with np.errstate(all='ignore'):
        for f in range(n):
            out[f] = np.abs(e_y @ t[f] @ e_x.T) / (h * w) * k
    return out


def noise_frames(sig, n, dtype, seed=0):
    """seeded frames (n, h, w) of `dtype` with power at every frequency: integers over a good part of the dtype's
    range (negative ones too, where it has them), floats in [-15, 35)"""
    rng = np.random.default_rng([seed, 3, n] + [int(v) for v in sig])
    dt = np.dtype(dtype)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        return rng.integers(max(info.min, -2000), min(info.max, 4000), (n,) + tuple(sig), endpoint=True).astype(dt)
    return ((rng.random((n,) + tuple(sig)) - 0.3) * 50).astype(dt)


def delta_frame():
    """exp(2 + 0.5 cos(2 pi (3 i / 16 + 5 j / 20))) as float32 (16, 20): with no window and a negligible offset its
    cepstrum is 2 at the origin, 0.25 at +-(3, 5) and nothing elsewhere"""
    i = np.arange(16, dtype=np.float64)[:, None]
    j = np.arange(20, dtype=np.float64)[None, :]
    return np.exp(2 + 0.5 * np.cos(2 * np.pi * (3 * i / 16 + 5 * j / 20))).astype(np.float32)


def bound(frames, offset, window):
    """the bound of the module docstring, per frame -> (n,); `window`: float32 (h, w) or None for the Hann window"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    win = (hann((h, w)) if window is None else np.asarray(window, dtype=np.float32)).astype(np.float64)
    z = log_frames(frames, offset)
    with np.errstate(all='ignore'):
        norm = np.sqrt((((1.0 + np.abs(z)) * win[None]) ** 2).reshape((n, -1)).sum(axis=1))
    return C_BOUND * EPS32 * (np.log2(h * w) + 2) * norm / np.sqrt(h * w)


def compare(dev, ref, frames, offset, window, skip_frames=(), what=''):
    """every frame of the device result (n, oh, ow) within the bound of the float64 reference; the frames in
    `skip_frames` (a non-finite pixel: unspecified) are left out.  -> the largest |error|_2 / bound"""
    dev = np.asarray(dev)
    n = ref.shape[0]
    assert dev.shape == ref.shape and dev.dtype == np.float32, (dev.shape, dev.dtype, ref.shape)
    take = np.ones(n, bool)
    take[list(skip_frames)] = False
    b = bound(frames, offset, window)
    with np.errstate(all='ignore'):
        err = np.sqrt(((dev.astype(np.float64) - ref).reshape((n, -1)) ** 2).sum(axis=1))
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err == 0, 0., np.inf))
    ratio = ratio[take]
    if ratio.size == 0:
        return 0.0
    print(f"cepstrum {what}: largest |dev - ref|_2 / bound = {ratio.max():.5f}")
    assert np.all(np.isfinite(dev[take]))
    assert ratio.max() <= 1.0, (what, float(ratio.max()))
    return float(ratio.max())


def store(spec, sig, out_shape, scale):
    """k_ceps_store in NumPy float32, bit for bit: spec (n, h, w // 2 + 1) complex64, `scale` float32 (oh, ow) as the
    kernel gets it.  Element (u, v) reads ky = (u - oh // 2) mod h, kx = (v - ow // 2) mod w: spec[ky, kx] for
    kx <= w // 2, else spec[(h - ky) mod h, w - kx]; sqrt(re * re + im * im) * scale, each operation rounded to
    float32."""
    h, w = sig
    oh, ow = out_shape
    out = np.empty((spec.shape[0], oh, ow), dtype=np.float32)
    s = np.asarray(scale, dtype=np.float32)
    for u in range(oh):
        ky = (u - oh // 2) % h
        for v in range(ow):
            kx = (v - ow // 2) % w
            c = spec[:, ky, kx] if kx <= w // 2 else spec[:, (h - ky) % h, w - kx]
            re, im = c.real.astype(np.float32), c.imag.astype(np.float32)
            out[:, u, v] = np.sqrt(re * re + im * im) * s[u, v]
    return out
