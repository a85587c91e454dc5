"""
Ground truth of the peak-finding tests: the definition of PeakFindUDF restated map by map and
pixel by pixel in plain loops (nothing from libertem_amd), seeded frames of disks with pairwise distinct amplitudes,
the case tables of the GPU tests, and `decided`: whether an error of at most B per correlation value can change which
peaks a frame keeps.

Definition, for a map c of (h, w), N = num_peaks, d = min_distance, b = border, q = refine_radius:
    1. p is a candidate iff over every other p' with |y'-y| <= d, |x'-x| <= d inside the frame: c[p] > c[p'] where p'
       precedes p in row-major order, c[p] >= c[p'] where it follows
    2. eligible iff b <= y < h-b, b <= x < w-b and c[p] > float32(threshold_abs)
    3. eligible candidates by value descending, index ascending; v0 the first value; if v0 > 0 those with
       c[p] < float32(threshold_rel) * v0 (one multiply in the map's dtype) go; the first N of the rest are kept
    4. centers = (y, x); peak_values = c[p]; refineds = centre of mass of Nb - min(Nb), Nb the (2q+1)^2 neighbourhood
       clipped to the frame (the centre where the weights sum to 0); peak_elevations = (max(W) - mean(W)) / std(W),
       ddof 0 (0 where the std is 0), W the window of radius d clipped to the frame
    5. slots from n_found on: centers (-1, -1), the rest NaN
    6. a map with a non-finite value keeps nothing
"""
import numpy as np

import correlation_ref as cr

REFINED_TOL = cr.REFINED_TOL
ELEVATION_RTOL = cr.ELEVATION_RTOL
NAMES = ('n_found', 'centers', 'refineds', 'peak_values', 'peak_elevations')


def params(num_peaks, min_distance, border=0, threshold_abs=0.0, threshold_rel=0.0, refine_radius=1):
    return dict(num_peaks=num_peaks, min_distance=min_distance, border=border, threshold_abs=threshold_abs,
                threshold_rel=threshold_rel, refine_radius=refine_radius)


def _span(p, radius, size):
    return max(int(p) - radius, 0), min(int(p) + radius, size - 1) + 1


def candidates(c, d):
    """step 1 by brute force -> [(y, x)] in row-major order"""
    h, w = c.shape
    out = []
    for y in range(h):
        ya, yb = _span(y, d, h)
        for x in range(w):
            xa, xb = _span(x, d, w)
            v = c[y, x]
            if not v >= c[ya:yb, xa:xb].max():               # (not the largest of its neighbourhood: no candidate)
                continue
            ok = True
            for yy in range(ya, yb):
                for xx in range(xa, xb):
                    if (yy, xx) < (y, x):
                        ok = ok and v > c[yy, xx]
                    elif (yy, xx) > (y, x):
                        ok = ok and v >= c[yy, xx]
            if ok:
                out.append((y, x))
    return out


def ranked(c, d, b, threshold_abs, threshold_rel):
    """steps 1 - 3 without the cut at N -> [(value, y, x)] in the order of step 3, and v0 (None: nothing eligible)"""
    h, w = c.shape
    t_abs = np.float32(threshold_abs)
    el = [(c[y, x], y, x) for y, x in candidates(c, d) if b <= y < h - b and b <= x < w - b and c[y, x] > t_abs]
    el.sort(key=lambda e: (-e[0], e[1] * w + e[2]))
    if not el:
        return [], None
    v0 = el[0][0]
    if v0 > 0:
        t = c.dtype.type(np.float32(threshold_rel)) * v0
        el = [e for e in el if not e[0] < t]
    return el, v0


def reference(maps, num_peaks, min_distance, border=0, threshold_abs=0.0, threshold_rel=0.0, refine_radius=1):
    """The definition, map by map.  -> dict: n_found (n,) int64, centers (n, N, 2) int64, refineds (n, N, 2),
    peak_values, peak_elevations (n, N) float64"""
    maps = np.asarray(maps)
    n, h, w = maps.shape
    N, d, q = num_peaks, min_distance, refine_radius
    out = {'n_found': np.zeros(n, np.int64), 'centers': np.full((n, N, 2), -1, np.int64),
           'refineds': np.full((n, N, 2), np.nan), 'peak_values': np.full((n, N), np.nan),
           'peak_elevations': np.full((n, N), np.nan)}
    for f in range(n):
        c = maps[f]
        if not np.isfinite(c).all():
            continue
        kept = ranked(c, d, border, threshold_abs, threshold_rel)[0][:N]
        out['n_found'][f] = len(kept)
        c64 = c.astype(np.float64)
        for k, (v, y, x) in enumerate(kept):
            out['centers'][f, k] = (y, x)
            out['peak_values'][f, k] = v
            ya, yb = _span(y, d, h)
            xa, xb = _span(x, d, w)
            win = c64[ya:yb, xa:xb]
            std = win.std()
            out['peak_elevations'][f, k] = (win.max() - win.mean()) / std if std > 0 else 0.
            na, nb = _span(y, q, h)
            ma, mb = _span(x, q, w)
            wgt = c64[na:nb, ma:mb] - c64[na:nb, ma:mb].min()
            total = wgt.sum()
            if total > 0:
                yy, xx = np.mgrid[na:nb, ma:mb]
                out['refineds'][f, k] = ((wgt * yy).sum() / total, (wgt * xx).sum() / total)
            else:
                out['refineds'][f, k] = (y, x)
    return out


def decided(corr64, p, bound):
    """True iff no perturbation of the map by at most `bound` per value can change n_found or centers: every pixel
    within 2 bound of its neighbourhood maximum either is a kept peak whose neighbourhood gap, threshold gaps and rank
    gaps (to the next kept peak, and the N-th to the best peak left out) all exceed 2 bound, or misses being kept by
    more than 2 bound (a threshold, or the N-th kept value), or lies in the border strip."""
    c = np.asarray(corr64, dtype=np.float64)
    if not np.isfinite(c).all():
        return True
    h, w = c.shape
    N, d, b = p['num_peaks'], p['min_distance'], p['border']
    t_abs, t_rel = float(np.float32(p['threshold_abs'])), float(np.float32(p['threshold_rel']))
    g = 2 * bound
    el, v0 = ranked(c, d, b, t_abs, t_rel)
    kept = el[:N]
    if v0 is not None and abs(v0) <= g:                      # (the sign of v0 switches the relative threshold)
        return False
    t = t_rel * v0 if v0 is not None and v0 > 0 else -np.inf
    kept_at = {(y, x): k for k, (_, y, x) in enumerate(kept)}
    for k in range(len(kept) - 1):
        if not kept[k][0] - kept[k + 1][0] > g:
            return False
    if len(el) > N and not kept[-1][0] - el[N][0] > g:
        return False
    last = kept[-1][0] if len(kept) == N else -np.inf
    for y in range(h):
        ya, yb = _span(y, d, h)
        for x in range(w):
            xa, xb = _span(x, d, w)
            win = c[ya:yb, xa:xb]
            v = c[y, x]
            if v < win.max() - g:
                continue
            if (y, x) in kept_at:
                others = np.delete(win.reshape(-1), (y - ya) * (xb - xa) + (x - xa))
                gap = v - others.max() if others.size else np.inf
                if not (gap > g and v - t_abs > g and v - t > g):
                    return False
            else:
                inner = b <= y < h - b and b <= x < w - b
                if inner and not (v < t_abs - g or v < t - g or v < last - g):
                    return False
    return True


# ---- maps for the search alone (exact float32 values: every decision is exact) --------------------------------------
MAP_SIGS = ((32, 32), (33, 35), (48, 40))


def quantised_maps(sig, n, seed, dtype='float32'):
    """integers in [-2, 6], a quarter of the pixels raised by another 0 .. 3: ties and plateaus everywhere"""
    rng = np.random.default_rng(seed)
    shape = (n,) + tuple(sig)
    m = rng.integers(-2, 4, shape) + rng.integers(0, 4, shape) * (rng.random(shape) < 0.25)
    return m.astype(dtype)


def special_maps(sig, d):
    """float32 maps (7, h, w) for a search with min_distance d, whose kernel works on aligned (d+1)^2 cells:
    0 constant; 1 distinct maxima in the four corners, on every edge, inside a border strip of 3 and in the middle;
    2 equal values on both sides of cell boundaries, next to each other, d apart (the first wins) and d + 1 apart
    (both stay), along both axes; 3 the values 8, 4, 2, 1 (threshold_rel 0.5 sits exactly on 4) and a plateau;
    4 a NaN among finite values; 5 a copy of map 1; 6 an Inf"""
    h, w = sig
    d1 = d + 1
    m = np.zeros((7, h, w), np.float32)
    m[0] = 1.5
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2 + 1), (h // 2, 0),
             (h // 2 + 1, w - 1), (2, min(w // 2 + d1, w - 3)), (h // 2, w // 2)]
    for k, (y, x) in enumerate(spots):
        m[1, y, x] = 3 + k
    yb = d1 * max(1, (h // 2) // d1)                        # a cell boundary in each axis
    xb = d1 * max(1, (w // 2) // d1)
    if yb < h and xb + d1 < w:
        m[2, yb - 1, 1] = m[2, yb, 1] = 5                   # neighbours across the row boundary
        m[2, 1, xb - 1 + d1] = m[2, 1, xb + d1] = 5         # ... across a column boundary
    if yb + d < h and xb + 3 * d + 2 < w and xb + 2 * d1 < w:
        m[2, yb - 1, xb] = m[2, yb - 1 + d, xb] = 6         # d apart: one peak
        m[2, yb - 1, xb + 2 * d1] = m[2, yb + d, xb + 2 * d1] = 7                   # d + 1 apart: two
        m[2, h - 1, xb - 1] = m[2, h - 1, xb - 1 + d] = 6
        m[2, h - 1, xb + 2 * d + 1] = m[2, h - 1, xb + 3 * d + 2] = 7
    for v, (y, x) in zip((8, 4, 2, 1), ((3, 3), (3, w - 4), (h - 4, 3), (h - 4, w - 4))):
        m[3, y, x] = v
    m[3, h // 2 - 1:h // 2 + 2, w // 2 - 2:w // 2 + 1] = 3  # a 3 x 3 plateau
    m[4] = quantised_maps(sig, 1, 5)[0]
    m[4, h // 3, w // 3] = np.nan
    m[5] = m[1]
    m[6] = m[1]
    m[6, h - 2, 2] = np.inf
    return m


POOL_MAPS = (((8, 8), 41), ((64, 64), 42))     # (sig, seed) of the two tiles of many maps


def pool_maps(sig, seed):
    """cr.POOL quantised float32 maps for tiles of many maps (cr.pool_index); member 7 is constant, member 23 holds a
    NaN (it keeps nothing)"""
    m = quantised_maps(sig, cr.POOL, seed)
    m[7] = 1.5
    m[23, sig[0] // 3, sig[1] // 3] = np.nan
    return m


def comb_map(n=256, step=3):
    """(1, n, n): one pixel in every step x step block carries a value of its own, the rest is 0: with d = 1 every
    one of them is a peak -- (n // step)^2 of them, more than the selection ranks in one go"""
    k = n // step
    i, j = np.mgrid[:k, :k]
    m = np.zeros((1, n, n), np.float32)
    m[0, 1 + step * i, 1 + step * j] = 1 + ((i * k + j) * 7919 % (k * k)).astype(np.float32)
    return m


# ---- seeded frames --------------------------------------------------------------------------------------------------
RADIUS = 3.0


def template(sig):
    return cr.disk_template(sig, radius=RADIUS)


def make_frames(sig, n_frames, seed, dtype='float32', noise=0.01):
    """-> frames (n_frames, h, w) of `dtype`, positions (n_frames, 9, 2), amplitudes (9,).  Nine disks of radius 3 per
    frame on a 3 x 3 grid, each moved by up to 2 px per frame, with the pairwise distinct amplitudes 1, 0.92, ...,
    0.36 (assigned to the grid places in a seeded order), on noise N(0, `noise`).  Integer dtypes are stored as
    tests/correlation_ref.py stores them: offset + scale * x."""
    rng = np.random.default_rng(seed)
    h, w = sig
    amps = 1.0 - 0.08 * np.arange(9)
    gy = np.linspace(6, h - 7, 3).round().astype(int)
    gx = np.linspace(6, w - 7, 3).round().astype(int)
    grid = np.array([(y, x) for y in gy for x in gx])
    pos = grid[None] + rng.integers(-2, 3, (n_frames, 9, 2))
    x = rng.normal(0., noise, (n_frames, h, w))
    for f in range(n_frames):
        for k, a in zip(rng.permutation(9), amps):
            x[f] += a * cr._disk_at(sig, pos[f, k, 0], pos[f, k, 1], RADIUS)
    dt = np.dtype(dtype)
    if dt.kind in 'iu':
        offset, scale = {'uint8': (10, 60), 'uint16': (2000, 20000), 'int16': (0, 8000)}[dt.name]
        info = np.iinfo(dt)
        x = np.clip(np.rint(offset + scale * x), info.min, info.max)
    return x.astype(dt), pos, amps


def threshold_for(frames, tmpl):
    """threshold_abs between the noise and the weakest disk: the correlation of a flat frame at the frames' median
    level plus 0.18 of a full-amplitude disk's rise (the weakest disk rises by 0.36)"""
    dt = np.asarray(frames).dtype
    offset, scale = {'uint8': (10, 60), 'uint16': (2000, 20000), 'int16': (0, 8000)}.get(dt.name, (0, 1))
    area = float(np.asarray(tmpl, dtype=np.float64).sum())
    return float(np.float32((offset + 0.18 * scale) * area))


# the cases of `CorrPlan.find_peaks` in tests/test_peakfind_kernels_gpu.py:
# (id, sig, n_frames, max_batch, dtype, pad of ld_tile, seed, search parameters without threshold_abs)
PLAN_CASES = [
    ('48x40-u2-batches', (48, 40), 7, 3, 'uint16', 0, 3, dict(num_peaks=12, min_distance=5)),
    ('48x40-u1-n7', (48, 40), 7, 3, 'uint8', 5, 4, dict(num_peaks=7, min_distance=2, border=3)),
    ('33x35-i2-n1', (33, 35), 4, 4, 'int16', 3, 5, dict(num_peaks=1, min_distance=5, refine_radius=2)),
    ('32x32-f4-rel', (32, 32), 5, 2, 'float32', 0, 6, dict(num_peaks=12, min_distance=1, threshold_rel=0.5)),
]

# the scan of tests/test_peakfind_gpu.py: 4 x 5 positions of 48 x 40 uint16
SCAN_SIG, SCAN_NAV, SCAN_SEED = (48, 40), (4, 5), 12
SCAN_PARAMS = dict(num_peaks=12, min_distance=5, refine_radius=1)


def plan_case(case):
    """-> frames, template, search parameters (threshold_abs filled in) of a row of PLAN_CASES"""
    _, sig, n, _, dtype, _, seed, search = case
    frames, _, _ = make_frames(sig, n, seed, dtype=dtype)
    tmpl = template(sig)
    return frames, tmpl, params(threshold_abs=threshold_for(frames, tmpl), **search)


def scan_case():
    frames, pos, _ = make_frames(SCAN_SIG, SCAN_NAV[0] * SCAN_NAV[1], SCAN_SEED, dtype='uint16')
    tmpl = template(SCAN_SIG)
    return frames, tmpl, params(threshold_abs=threshold_for(frames, tmpl), **SCAN_PARAMS), pos


def corrected_scan():
    """the scan's frames after a dark frame and a gain map (one rounding to float32), and those two"""
    frames = scan_case()[0]
    rng = np.random.default_rng(21)
    dark = rng.uniform(0., 500., SCAN_SIG)
    gain = rng.uniform(0.95, 1.05, SCAN_SIG)
    return ((frames.astype(np.float64) - dark) * gain).astype(np.float32), dark, gain


def pool_case():
    """the pool of tests/correlation_ref.py searched with d = 1 for up to 3 peaks: -> frames (cr.POOL, 8, 8) uint8,
    template, parameters.  threshold_abs as threshold_for has it, between a flat frame and the weaker block."""
    frames, tmpl = cr.pool_frames(), cr.pool_template()
    return frames, tmpl, params(num_peaks=3, min_distance=1, threshold_abs=threshold_for(frames, tmpl))


def undecided_frame():
    """one noisy uint16 frame (noise 0.5 of a disk) searched without thresholds: its noise maxima are kept, and some
    lie closer to each other than the error bound"""
    frames, _, _ = make_frames(SCAN_SIG, 1, 99, dtype='uint16', noise=0.5)
    return frames, template(SCAN_SIG), params(num_peaks=64, min_distance=1)


def all_decided(frames, tmpl, p):
    """per frame: `decided` on the float64 correlation with correlation_ref's bound"""
    bound = cr.value_bound(frames, tmpl)
    return np.array([decided(cr.correlation(frames[f], tmpl), p, bound[f]) for f in range(len(frames))])
