"""
Ground truth of the holography tests: the definition of HoloReconstructUDF restated in float64
WITHOUT an index -- two matrix products with explicit exponentials, no fft, roll, fftshift or crop, so a mistake in the
index arithmetic of the code under test cannot be made here a second time --, the case table of the kernel tests,
seeded frame makers and the comparison the device tests share.

With s(i, n) = i if i <= (n - 1) // 2 else i - n, a frame y of (h, w) (rounded to float32 first), the sideband
(sy, sx), the output shape (oh, ow) and the aperture:

    G    = (E_y y E_x^T) / (h w) * aperture      E_y[u, n] = exp(-2 pi i (sy + s(u, oh)) n / h), E_x likewise
    wave = D_y G D_x^T                           D_y[i, u] = exp(+2 pi i i s(u, oh) / oh), D_x likewise
    wave /= reference_wave                       where given

The bound of the device results, per frame in the 2-norm over the output:

    |dev - ref|_2 <= C eps32 (log2(h w) + log2(oh ow)) sqrt(oh ow / (h w)) max|aperture| |y|_2,        C = 8

from the normwise error of a float32 FFT (eps32 log2(N) of the norm of what it transforms), |F|_2 = |y|_2 / sqrt(h w)
and |wave|_2 = sqrt(oh ow) |G|_2; C = 8 is the constant section 4.6b uses for three float32 transforms.  With a
reference wave the bound is multiplied by max|1 / reference| and 4 eps32 |ref result|_2 is added: one cast of the
inverse to complex64 and one complex float32 multiply, each below 1.2 eps32, doubled.
"""
import numpy as np

from correlation_ref import EXTREMES, POOL

EPS32 = float(np.finfo(np.float32).eps)
C_BOUND = 8.0

# (h, w), (oh, ow), (sy, sx): what the rows probe is said in tests/test_holo_kernels_gpu.py
CASES = [
    ((16, 16), (8, 8), (3, 12)),         # the mirrored half only
    ((16, 16), (8, 8), (0, 8)),          # straddles the Nyquist column and row 0
    ((15, 17), (7, 5), (14, 9)),         # odd everything, wraps in y
    ((16, 12), (16, 12), (0, 6)),        # output equal to the frame: every index, both halves
    ((32, 20), (6, 9), (16, 10)),        # both Nyquist lines
    ((16, 16), (1, 1), (5, 0)),          # a single output element
    ((9, 8), (9, 1), (0, 0)),            # the DC column
]


def case_id(case):
    (h, w), (oh, ow), (sy, sx) = case
    return f"{h}x{w}-{oh}x{ow}-sb{sy}.{sx}"


def signed(n):
    """s(i, n) for i in [0, n), written out: the non-negative frequencies, then the negative ones"""
    return np.array([i if i <= (n - 1) // 2 else i - n for i in range(n)], dtype=np.int64)


def _phases(k, n, sign):
    """exp(sign 2 pi i k[a] m / n) for m in [0, n): (len(k), n); the integer product is reduced mod n first"""
    km = (np.asarray(k, dtype=np.int64)[:, None] * np.arange(n, dtype=np.int64)[None, :]) % n
    return np.exp(sign * 2j * np.pi * km / n)


def reference(frames, out_shape, sb_position, aperture, reference_wave=None, round_input=True):
    """the definition for frames (n, h, w) -> complex128 (n, oh, ow); a frame with a non-finite pixel gives NaN.
    round_input=False leaves float64 frames as they are: the operation itself, without the definition's float32 step"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    oh, ow = out_shape
    sy, sx = sb_position
    y = frames.astype(np.float32).astype(np.float64) if round_input else frames.astype(np.float64)
    e_y = _phases(sy + signed(oh), h, -1)                    # (oh, h)
    e_x = _phases(sx + signed(ow), w, -1)                    # (ow, w)
    d_y = _phases(signed(oh), oh, +1).T                      # [i, u]
    d_x = _phases(signed(ow), ow, +1).T                      # [j, v]
    a = np.asarray(aperture, dtype=np.float32).astype(np.float64)
    out = np.empty((n, oh, ow), dtype=np.complex128)
    with np.errstate(all='ignore'):
        for f in range(n):
            g = (e_y @ y[f] @ e_x.T) / (h * w) * a
            out[f] = d_y @ g @ d_x.T
        if reference_wave is not None:
            out = out / np.asarray(reference_wave).astype(np.complex128)[None]
    return out


def aperture_for(case, seed=0):
    """a float32 aperture without any symmetry, values in [0.25, 1]: a transposed or mirrored index shows"""
    rng = np.random.default_rng([seed, 1] + [int(v) for pair in case for v in pair])
    return rng.uniform(0.25, 1.0, case[1]).astype(np.float32)


def reference_wave_for(case, seed=0):
    """complex128 of modulus in [0.5, 2] and any phase"""
    rng = np.random.default_rng([seed, 2] + [int(v) for pair in case for v in pair])
    return rng.uniform(0.5, 2.0, case[1]) * np.exp(2j * np.pi * rng.random(case[1]))


def noise_frames(sig, n, dtype, seed=0):
    """seeded frames (n, h, w) of `dtype` with power at every frequency: integers over a good part of the dtype's
    range, floats in [-15, 35)"""
    rng = np.random.default_rng([seed, 3, n] + [int(v) for v in sig])
    dt = np.dtype(dtype)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        return rng.integers(max(info.min, -2000), min(info.max, 4000), (n,) + tuple(sig), endpoint=True).astype(dt)
    return ((rng.random((n,) + tuple(sig)) - 0.3) * 50).astype(dt)


def typed_frames(sig, n, dtype, seed=0):
    """noise_frames, and for uint32 (n >= 3) the values of EXTREMES in frame 2: the ends of the range, 2^31 and its
    neighbours, 2^24 + 1"""
    frames = noise_frames(sig, n, dtype, seed)
    if np.dtype(dtype).name == 'uint32' and n >= 3:
        v = np.array(EXTREMES['uint32']).astype(frames.dtype)
        at = np.linspace(0, sig[0] * sig[1] - 1, len(v)).astype(int)
        frames[2].reshape(-1)[at] = v
    return frames


# tiles of many frames drawn from a pool (correlation_ref.pool_index): 8 x 8 -> 4 x 4, the sideband in the mirrored
# half: columns 6, 7 and 5 are mirrored ones, 4 is the stored Nyquist column
POOL_CASE = ((8, 8), (4, 4), (1, 6))


def pool_frames():
    return noise_frames(POOL_CASE[0], POOL, 'uint8', seed=9)


def pool_spectra():
    """POOL random complex64 half spectra (8, 5)"""
    rng = np.random.default_rng([9, 5])
    shape = (POOL, POOL_CASE[0][0], POOL_CASE[0][1] // 2 + 1)
    return (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)


def carrier_params(sig, k):
    """`sampling` and `f_angle` of hologram_frame whose carrier has k = (ky, kx) cycles per frame of `sig`"""
    fy, fx = k[0] / sig[0], k[1] / sig[1]
    return 1.0 / np.hypot(fy, fx), float(np.degrees(np.arctan2(fx, fy)))


def hologram_frames(sig, n, k, dtype='uint16', counts=4000., visibility=0.5, seed=0):
    """n holograms (libertem_amd.utils.generate.hologram_frame) of smooth random objects, carrier on the integer
    frequency k, rounded into `dtype`"""
    from libertem_amd.utils.generate import hologram_frame
    rng = np.random.default_rng([seed, 4, n] + [int(v) for v in sig])
    h, w = sig
    yy, xx = np.mgrid[:h, :w]
    sampling, f_angle = carrier_params(sig, k)
    frames = np.empty((n, h, w), dtype=np.float64)
    for f in range(n):
        a, b, c = rng.uniform(-1, 1, 3)
        amp = 0.7 + 0.2 * np.cos(2 * np.pi * (yy / h + a))
        phi = 2 * np.pi * (a * yy / h + b * xx / w) + c
        frames[f] = hologram_frame(amp, phi, counts=counts, sampling=sampling, visibility=visibility, f_angle=f_angle)
    dt = np.dtype(dtype)
    return np.rint(frames).astype(dt) if dt.kind in 'iu' else frames.astype(dt)


def bound(frames, out_shape, aperture, reference_wave=None, ref_result=None):
    """the bound of the module docstring, per frame -> (n,)"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    oh, ow = out_shape
    y = frames.astype(np.float32).astype(np.float64).reshape((n, -1))
    with np.errstate(all='ignore'):
        ny = np.sqrt((y * y).sum(axis=1))
    b = (C_BOUND * EPS32 * (np.log2(h * w) + np.log2(oh * ow)) * np.sqrt(oh * ow / (h * w))
         * float(np.abs(np.asarray(aperture, dtype=np.float64)).max()) * ny)
    if reference_wave is not None:
        ref_inv = (1.0 / np.asarray(reference_wave).astype(np.complex128)).astype(np.complex64)
        with np.errstate(all='ignore'):
            nr = np.sqrt((np.abs(ref_result.reshape((n, -1))) ** 2).sum(axis=1))
        b = b * float(np.abs(ref_inv).max()) + 4 * EPS32 * nr
    return b


def compare(dev, ref, frames, aperture, reference_wave=None, skip_frames=(), what=''):
    """every frame of the device result (n, oh, ow) within the bound of the float64 reference; the frames in
    `skip_frames` (a non-finite pixel: unspecified) are left out.  -> the largest |error|_2 / bound * C"""
    dev = np.asarray(dev)
    n = ref.shape[0]
    assert dev.shape == ref.shape and dev.dtype == np.complex64, (dev.shape, dev.dtype, ref.shape)
    keep = np.ones(n, bool)
    keep[list(skip_frames)] = False
    b = bound(frames, ref.shape[1:], aperture, reference_wave, ref)
    with np.errstate(all='ignore'):
        err = np.sqrt((np.abs(dev.astype(np.complex128) - ref).reshape((n, -1)) ** 2).sum(axis=1))
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1) * C_BOUND, np.where(err == 0, 0., np.inf))
    ratio = ratio[keep]
    if ratio.size == 0:
        return 0.0
    print(f"holography {what}: largest |dev - ref|_2 / (bound / C) = {ratio.max():.4f} (bound C = {C_BOUND})")
    assert np.all(np.isfinite(dev[keep]))
    assert ratio.max() <= C_BOUND, (what, float(ratio.max()))
    return float(ratio.max())


def gather(spec, sig, out_shape, sb_position, aperture):
    """The half-spectrum gather of k_holo_crop in NumPy, bit for bit: spec (n, h, w // 2 + 1) complex64, the aperture
    float32 as the kernel gets it.  Element (u, v) reads ky = (sy + s(u)) mod h, kx = (sx + s(v)) mod w: spec[ky, kx]
    for kx <= w // 2, else conj(spec[(h - ky) mod h, w - kx]); each component times the aperture, in float32."""
    h, w = sig
    oh, ow = out_shape
    sy, sx = sb_position
    out = np.empty((spec.shape[0], oh, ow), dtype=np.complex64)
    a = np.asarray(aperture, dtype=np.float32)
    for u in range(oh):
        ky = (sy + int(signed(oh)[u])) % h
        for v in range(ow):
            kx = (sx + int(signed(ow)[v])) % w
            if kx <= w // 2:
                re, im = spec[:, ky, kx].real, spec[:, ky, kx].imag
            else:
                re, im = spec[:, (h - ky) % h, w - kx].real, -spec[:, (h - ky) % h, w - kx].imag
            out[:, u, v].real = re.astype(np.float32) * a[u, v]
            out[:, u, v].imag = im.astype(np.float32) * a[u, v]
    return out
