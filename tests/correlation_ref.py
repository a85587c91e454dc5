"""
Ground truth of the correlation tests: the definition of CorrelationUDF restated frame by
frame in float64 NumPy, a seeded frame maker, the case table of the kernel tests and the comparison they share.

Definition, for a frame x as float32 y, a float32 template t centred at (h // 2, w // 2), peaks (py, px), r, q:
    corr = irfft2(rfft2(y) * conj(rfft2(ifftshift(t))), s=(h, w))
    W = corr[py - r:py + r + 1, px - r:px + r + 1] clipped to the frame
    peak_values = max(W); centers = first maximum of W, row-major, frame coordinates
    refineds = centre of mass of N - min(N), N the (2q + 1)^2 neighbourhood of centers clipped to the frame
               (centers if the weights sum to 0)
    peak_elevations = (max(W) - mean(W)) / std(W), ddof 0 (0 if the std is 0)
    a frame with a non-finite pixel: peak_values NaN, the rest unspecified
"""
import numpy as np

from cryst_ref import EXTREMES

EPS32 = float(np.finfo(np.float32).eps)
C_BOUND = 8.0              # |gpu - ref| <= C eps32 log2(h w) |y|_2 |t|_2 for every correlation value
REFINED_TOL = 0.02         # pixels
ELEVATION_RTOL = 1e-3


def disk_template(sig, radius=4.0):
    """a disk of ones centred at (h // 2, w // 2), float32"""
    h, w = sig
    yy, xx = np.mgrid[:h, :w]
    return (((yy - h // 2) ** 2 + (xx - w // 2) ** 2) <= radius ** 2).astype(np.float32)


def _disk_at(sig, cy, cx, radius):
    h, w = sig
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= radius ** 2).astype(np.float64)       # (clipped, no wrap-around)


def make_frames(sig, peaks, r, n_frames, seed, dtype='float32', n_blurred=0, radius=4.0):
    """-> frames (n_frames, h, w) of `dtype`, shifts (n_frames, n_peaks, 2) int, frac (n_frames, 2) float.
    Noise N(0, 0.05) plus, for every peak, a disk of amplitude 1 at peaks[k] + shift, shift an integer in
    [-r + 1, r - 1]^2 per (frame, peak).  The last `n_blurred` frames are blurred by a fractional shift frac in
    [0.2, 0.8]^2 (bilinear: the disks' true position is peaks[k] + shift + frac); frac is 0 for the others.
    Integer dtypes store offset + scale * (noise + disks), rounded and clipped to the dtype: uint8 10 + 60 x,
    uint16 2000 + 20000 x, int16 8000 x (a small offset: it adds to |y| and so to the bound, not to the signal), int8
    50 x, uint32 1e8 + 1e9 x and int32 5e8 x (the scale of the planted extremes); bool stores x > 0.5."""
    rng = np.random.default_rng(seed)
    peaks = np.asarray(peaks)
    h, w = sig
    shifts = rng.integers(-r + 1, r, (n_frames, len(peaks), 2))
    shifts = np.clip(peaks[None] + shifts, 0, (h - 1, w - 1)) - peaks[None]      # (every disk's centre inside the frame)
    frac = np.zeros((n_frames, 2))
    if n_blurred:
        frac[n_frames - n_blurred:] = rng.uniform(0.2, 0.8, (n_blurred, 2))
    x = rng.normal(0., 0.05, (n_frames, h, w))
    for f in range(n_frames):
        fy, fx = frac[f]
        for k in range(len(peaks)):
            cy, cx = peaks[k] + shifts[f, k]
            if fy == 0 and fx == 0:
                x[f] += _disk_at(sig, cy, cx, radius)
            else:
                x[f] += ((1 - fy) * (1 - fx) * _disk_at(sig, cy, cx, radius)
                         + fy * (1 - fx) * _disk_at(sig, cy + 1, cx, radius)
                         + (1 - fy) * fx * _disk_at(sig, cy, cx + 1, radius)
                         + fy * fx * _disk_at(sig, cy + 1, cx + 1, radius))
    return store(x, dtype), shifts, frac


STORED = {'uint8': (10, 60), 'uint16': (2000, 20000), 'int16': (0, 8000), 'int8': (0, 50), 'uint32': (1e8, 1e9),
          'int32': (0, 5e8)}


def store(x, dtype):
    """float64 frames in units of a disk -> `dtype`: offset + scale * x rounded and clipped for the integers (STORED),
    x > 0.5 for bool, a cast for the floats"""
    dt = np.dtype(dtype)
    if dt.kind == 'b':
        return x > 0.5
    if dt.kind in 'iu':
        offset, scale = STORED[dt.name]
        info = np.iinfo(dt)
        x = np.clip(np.rint(offset + scale * x), info.min, info.max)
    return x.astype(dt)


def _span(p, radius, size):
    return max(int(p) - radius, 0), min(int(p) + radius, size - 1) + 1


def correlation(frame, template):
    """float64 circular cross-correlation of one frame (rounded to float32 first) with the template"""
    y = np.asarray(frame).astype(np.float32).astype(np.float64)
    t = np.asarray(template, dtype=np.float32).astype(np.float64)
    return np.fft.irfft2(np.fft.rfft2(y) * np.conj(np.fft.rfft2(np.fft.ifftshift(t))), s=y.shape)


def reference(frames, template, peaks, r, q=1):
    """The definition, frame by frame and peak by peak.  -> dict of float64 / int64 arrays: centers, refineds
    (n, n_peaks, 2), peak_values, peak_elevations (n, n_peaks); and what the tolerances are derived from: `gap`
    (largest minus second largest value of W), `wsum` (sum of the refinement weights), `std` and `rise`
    (max(W) - mean(W)), all (n, n_peaks)."""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    k_n = len(peaks)
    out = {'centers': np.zeros((n, k_n, 2), np.int64), 'refineds': np.zeros((n, k_n, 2)),
           'peak_values': np.zeros((n, k_n)), 'peak_elevations': np.zeros((n, k_n)), 'gap': np.zeros((n, k_n)),
           'wsum': np.zeros((n, k_n)), 'std': np.zeros((n, k_n)), 'rise': np.zeros((n, k_n))}
    for f in range(n):
        if not np.isfinite(frames[f].astype(np.float64)).all():
            out['peak_values'][f] = np.nan
            continue
        corr = correlation(frames[f], template)
        for k, (py, px) in enumerate(peaks):
            ya, yb = _span(py, r, h)
            xa, xb = _span(px, r, w)
            win = corr[ya:yb, xa:xb]
            first = int(np.argmax(win))                     # (first maximum in row-major order)
            cy, cx = ya + first // win.shape[1], xa + first % win.shape[1]
            top = win.reshape(-1)[first]
            ordered = np.sort(win.reshape(-1))
            out['gap'][f, k] = ordered[-1] - ordered[-2] if ordered.size > 1 else np.inf
            out['centers'][f, k] = (cy, cx)
            out['peak_values'][f, k] = top
            std = win.std()
            out['std'][f, k] = std
            out['rise'][f, k] = top - win.mean()
            out['peak_elevations'][f, k] = (top - win.mean()) / std if std > 0 else 0.
            na, nb = _span(cy, q, h)
            ma, mb = _span(cx, q, w)
            wgt = corr[na:nb, ma:mb] - corr[na:nb, ma:mb].min()
            total = wgt.sum()
            out['wsum'][f, k] = total
            if total > 0:
                yy, xx = np.mgrid[na:nb, ma:mb]
                out['refineds'][f, k] = ((wgt * yy).sum() / total, (wgt * xx).sum() / total)
            else:
                out['refineds'][f, k] = (cy, cx)
    return out


def value_bound(frames, template):
    """per frame: C eps32 log2(h w) |y|_2 |t|_2 -- three float32 transforms each lose eps32 log2(h w) of the norm of
    what they transform, and every correlation value is an inner product bounded by |y| |t|"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    y = frames.astype(np.float32).astype(np.float64).reshape((n, -1))
    with np.errstate(all='ignore'):
        ny = np.sqrt((y * y).sum(axis=1))
    nt = np.sqrt((np.asarray(template, dtype=np.float64) ** 2).sum())
    return C_BOUND * EPS32 * np.log2(h * w) * ny * nt


def compare(got, ref, frames, template, q=1, skip_frames=(), bound=None, max_skipped=0.02):
    """The checks the device results share.  got: dict of the four arrays (n, n_peaks[, 2]).
    peak_values within the bound for every pair; centers equal, refineds and peak_elevations within their tolerances
    for every pair whose top-two gap exceeds twice the bound, at most `max_skipped` of the pairs below it.  `bound`:
    value_bound per frame where the caller has it already (a tile drawn from a pool), else taken from the frames.
    -> dict(ratio=largest |error| / bound * C, skipped=share of pairs below the gap, derived_refined /
    derived_elevation=pairs that use the derived tolerance)."""
    n, k_n = ref['peak_values'].shape
    keep = np.ones(n, bool)
    keep[list(skip_frames)] = False
    bound = (value_bound(frames, template) if bound is None else np.asarray(bound))[:, None] * np.ones((1, k_n))
    err = np.abs(np.asarray(got['peak_values'], np.float64) - ref['peak_values'])
    with np.errstate(all='ignore'):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1) * C_BOUND, np.where(err == 0, 0., np.inf))
    ratio = ratio[keep]
    print(f"correlation: largest peak_values error / (eps32 log2(hw) |y| |t|) = {ratio.max():.4f} (bound C = {C_BOUND})")
    assert ratio.max() <= C_BOUND, ratio.max()
    gapped = (ref['gap'] > 2 * bound) & keep[:, None]
    skipped = 1.0 - gapped[keep].mean()
    print(f"correlation: {100 * skipped:.2f} % of the (frame, peak) pairs lie below the gap")
    assert skipped <= max_skipped, skipped
    assert np.array_equal(np.asarray(got['centers'])[gapped], ref['centers'][gapped])
    # refined = sum(w p) / sum(w), w = N - min(N): each weight is off by at most 2 bound, and to first order
    # d refined = sum(dw (p - refined)) / sum(w) with |p - refined| <= 2 q, so |d refined| <= (2q+1)^2 4 q bound / sum(w).
    # For the seeded disks (bound ~1e-3 of a weight sum of ~50 at q = 1) that is ~1e-3 px, below REFINED_TOL; where
    # a window holds no disk the weight sum is small and the derived value is the larger one: it is used there.
    with np.errstate(all='ignore'):
        d_ref = (2 * q + 1) ** 2 * 4 * q * bound / ref['wsum']
        # elevation = rise / std: rise and std are each off by at most 2 bound -> relative error
        # 2 bound (1 / rise + 1 / std); ~4e-4 for the seeded disks (std ~10), below ELEVATION_RTOL
        d_el = 2 * bound * (1 / ref['rise'] + 1 / ref['std'])
    tol_ref = np.maximum(REFINED_TOL, np.where(np.isfinite(d_ref), d_ref, REFINED_TOL))
    tol_el = np.maximum(ELEVATION_RTOL, np.where(np.isfinite(d_el), d_el, ELEVATION_RTOL))
    e_ref = np.abs(np.asarray(got['refineds'], np.float64) - ref['refineds']).max(axis=2)
    assert np.all(e_ref[gapped] <= tol_ref[gapped]), (e_ref[gapped] / tol_ref[gapped]).max()
    e_el = np.abs(np.asarray(got['peak_elevations'], np.float64) - ref['peak_elevations'])
    lim = tol_el * np.abs(ref['peak_elevations'])
    assert np.all(e_el[gapped] <= lim[gapped]), (e_el[gapped] / lim[gapped]).max()
    return {'ratio': float(ratio.max()), 'skipped': float(skipped),
            'derived_refined': int((tol_ref[gapped] > REFINED_TOL).sum()),
            'derived_elevation': int((tol_el[gapped] > ELEVATION_RTOL).sum())}


def border_peaks(sig):
    """one peak whose window is clipped at each border, one at a corner, two inside"""
    h, w = sig
    return np.array([(0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1), (0, 0), (h // 2, w // 2),
                     (h // 4 + 1, w // 4 + 2)], dtype=np.int32)


# the kernel cases: (id, sig, n_frames, max_batch, dtype, peaks ('one' | 'border'), r, q, pad of ld_tile, seed).
# The seeds are picked so that no (frame, peak) pair lies below the gap of the comparison (a disk whose maximum sits on
# a clipped border can tie with its neighbour): tests/test_correlation_cpu.py checks that, in float64, on the CPU.
KERNEL_CASES = [
    ('32x32-f4', (32, 32), 8, 8, 'float32', 'border', 6, 1, 0, 2),
    ('32x32-u2-ld', (32, 32), 8, 8, 'uint16', 'border', 6, 2, 24, 2),
    ('32x32-u1-r1', (32, 32), 8, 3, 'uint8', 'border', 1, 1, 0, 2),
    ('32x32-i2-one', (32, 32), 8, 8, 'int16', 'one', 6, 1, 3, 2),
    ('36x50-f4', (36, 50), 5, 4, 'float32', 'border', 6, 2, 0, 1),
    ('36x51-u2', (36, 51), 5, 5, 'uint16', 'border', 6, 1, 1, 3),
    ('36x51-f4-one-r1', (36, 51), 5, 2, 'float32', 'one', 1, 2, 0, 2),
    ('64x64-u2-batches', (64, 64), 70, 32, 'uint16', 'border', 6, 1, 0, 8),
    # the other pixel types k_corr_load takes, each on its vector path (32 x 32, contiguous rows) and on its scalar
    # path (36 x 51, padded rows), 5 frames in batches of 2, the values of PLANTED inside a window of frame 2
    # (bool: one disk of ones on zeros; a binary disk at a clipped border ties with its neighbour whatever the seed)
    ('32x32-b1', (32, 32), 5, 2, 'bool', 'one', 6, 1, 0, 2),
    ('36x51-b1-ld', (36, 51), 5, 2, 'bool', 'one', 6, 1, 5, 2),
    ('32x32-i1', (32, 32), 5, 2, 'int8', 'border', 6, 1, 0, 2),
    ('36x51-i1-ld', (36, 51), 5, 2, 'int8', 'one', 6, 1, 5, 2),
    ('32x32-u4', (32, 32), 5, 2, 'uint32', 'border', 6, 1, 0, 2),
    ('36x51-u4-ld', (36, 51), 5, 2, 'uint32', 'one', 6, 2, 5, 2),
    ('32x32-i4', (32, 32), 5, 2, 'int32', 'border', 6, 2, 0, 2),
    ('36x51-i4-ld', (36, 51), 5, 2, 'int32', 'one', 6, 1, 5, 2),
]

# the ends of the range, 2^31 and its neighbours (a signed or unsigned slip) and 2^24 + 1 (the conversion's rounding)
PLANTED = {'uint32': EXTREMES['uint32'], 'int32': EXTREMES['int32'], 'int8': [-128, 127]}
# where they go, relative to the one peak / the inner peak (h // 2, w // 2) of the border list: inside its window, r = 6
PLANTED_AT = ((-1, 2), (2, -1), (0, 3), (-3, 0), (3, 3), (-2, -3), (4, 1), (1, -4))


def plant(frames, dtype, peak, frame=2):
    """PLANTED[dtype] into `frames[frame]` around `peak`, in place"""
    for v, (dy, dx) in zip(PLANTED.get(np.dtype(dtype).name, ()), PLANTED_AT):
        frames[frame, peak[0] + dy, peak[1] + dx] = v


def kernel_case(case):
    """-> frames, template, peaks, r, q of a row of KERNEL_CASES"""
    _, sig, n, _, dtype, which, r, q, _, seed = case
    peaks = border_peaks(sig) if which == 'border' else np.array([(sig[0] // 2 - 2, sig[1] // 2 + 3)], np.int32)
    frames, _, _ = make_frames(sig, peaks, r, n, seed, dtype=dtype, n_blurred=n // 4)
    plant(frames, dtype, peaks[5] if which == 'border' else peaks[0])
    return frames, disk_template(sig), peaks, r, q


# ---- tiles of many frames drawn from a pool --------------------------------------------------------------------------
# The restatements are per-frame Python loops: they run on POOL distinct members once, frame f of a tile is member
# idx[f], and what is expected of frame f is what the restatement gives for that member.
POOL = 61                  # prime: no common factor with the 8 frames of a k_corr_mul group, 32768 or 65535
GRID_ROWS = 65535          # the largest gridDim.y the launchers use
POOL_SIG = (8, 8)
POOL_PEAKS = np.array([(2, 2), (5, 5)], dtype=np.int32)
POOL_R, POOL_Q = 2, 1
POOL_RADIUS = 1.5          # a 3 x 3 block


def pool_index(n, extra=(), seed=7, members=POOL):
    """-> idx (n,): seeded members in [0, members); the frames on both sides of the grid-row limit, the first, the
    last and those in `extra` get a member that differs from both neighbours', so that a frame taken from the slot
    before or behind shows"""
    rng = np.random.default_rng([seed, n])
    idx = rng.integers(0, members, n)
    for f in sorted({0, GRID_ROWS - 1, GRID_ROWS, GRID_ROWS + 1, n - 1, *extra}):
        if 0 <= f < n:
            near = {int(idx[g]) for g in (f - 1, f + 1) if 0 <= g < n}
            idx[f] = next(m % members for m in range(int(idx[f]), int(idx[f]) + members) if m % members not in near)
    return idx


def through(ref, idx):
    """the restatement's arrays of the pool -> those of the tile"""
    return {name: a[idx] for name, a in ref.items()}


def pool_template():
    return disk_template(POOL_SIG, POOL_RADIUS)


def pool_frames(seed=3):
    """POOL frames of 8 x 8 uint8 (10 + 60 x): two 3 x 3 blocks of amplitude 1 and 0.75, their centres in [2, 5]^2 (no
    block and no correlation peak wraps around) and at least 3 apart, on noise N(0, 0.05); every fourth member blurred
    by a fractional shift as in make_frames"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0., 0.05, (POOL,) + POOL_SIG)
    for m in range(POOL):
        while True:
            c = rng.integers(2, 6, (2, 2))
            if np.abs(c[0] - c[1]).max() >= 3:
                break
        fy, fx = rng.uniform(0.2, 0.8, 2) if m % 4 == 3 else (0., 0.)
        for (cy, cx), a in zip(c, (1.0, 0.75)):
            cy, cx = min(cy, 5 - (fy > 0)), min(cx, 5 - (fx > 0))
            x[m] += a * ((1 - fy) * (1 - fx) * _disk_at(POOL_SIG, cy, cx, POOL_RADIUS)
                         + fy * (1 - fx) * _disk_at(POOL_SIG, cy + 1, cx, POOL_RADIUS)
                         + (1 - fy) * fx * _disk_at(POOL_SIG, cy, cx + 1, POOL_RADIUS)
                         + fy * fx * _disk_at(POOL_SIG, cy + 1, cx + 1, POOL_RADIUS))
    return store(x, 'uint8')
