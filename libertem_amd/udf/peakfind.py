"""
PeakFindUDF on MI355X: the strongest correlation maxima of every frame, the step that produces the `peaks` of
CorrelationUDF and LatticeRefineUDF -- and, run on every frame, the disk positions of polycrystalline samples, where
no fixed peak list exists.

Every frame is cross-correlated with one template as in CorrelationUDF; on the correlation map `c` of (h, w)
(DESIGN.md section 4.6d), with N = num_peaks, d = min_distance, b = border, q = refine_radius:

    1. p = (y, x) is a candidate iff, over every other p' with |y' - y| <= d and |x' - x| <= d inside the frame,
       c[p] > c[p'] where p' precedes p in row-major order and c[p] >= c[p'] where it follows (of equal values the
       first wins; two candidates are more than d apart);
    2. a candidate is eligible iff b <= y < h - b, b <= x < w - b and c[p] > threshold_abs;
    3. the eligible candidates by value descending, then row-major index ascending; v0 the first value; if v0 > 0,
       those with c[p] < float32(threshold_rel) * v0 (one multiply in the map's dtype) go; the first N of the rest
       are kept: n_found;
    4. for k < n_found: centers[k] = (y, x), peak_values[k] = c[p], refineds[k] and peak_elevations[k] as
       CorrelationUDF defines them for the peak centers[k], crop_radius = d and refine_radius = q;
    5. for k >= n_found: centers (-1, -1), the rest NaN;
    6. a frame with a non-finite pixel has n_found = 0.

On the device a tile goes through `ltmi_correlate_find` (csrc/ltmi_corr.hip, csrc/ltmi_peakfind.hip); on a CPU executor
NumPy computes the definition in float64 and casts at the end.  Guessing a lattice from the found peaks is not part of
this module.
"""
import numpy as np

from libertem_amd.udf.correlation import plan_for
from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, quiet_floats, runs_on_hip

#: what `ltmi_correlate_find` takes (csrc/ltmi_peakfind.hip)
MAX_PEAKS = 1024
MAX_WIDTH = 8192
NAMES = ('n_found', 'centers', 'refineds', 'peak_values', 'peak_elevations')


def check_params(sig, num_peaks, min_distance, border, threshold_abs, threshold_rel, refine_radius):
    """-> the parameters as (N, d, b, threshold_abs, threshold_rel, q); ValueError names the value that is off"""
    n, d, b, q = int(num_peaks), int(min_distance), int(border), int(refine_radius)
    t_abs, t_rel = float(threshold_abs), float(threshold_rel)
    if not 1 <= n <= MAX_PEAKS:
        raise ValueError(f"num_peaks {num_peaks} must lie in [1, {MAX_PEAKS}]")
    if d < 1:
        raise ValueError(f"min_distance {min_distance} must be at least 1")
    if q < 1:
        raise ValueError(f"refine_radius {refine_radius} must be at least 1")
    if b < 0 or 2 * b >= min(sig):
        raise ValueError(f"border {border} must be at least 0 and leave a pixel of the {tuple(sig)} frame")
    if not 0 <= t_rel <= 1:
        raise ValueError(f"threshold_rel {threshold_rel} must lie in [0, 1]")
    if t_abs != t_abs:
        raise ValueError(f"threshold_abs {threshold_abs} is not a number")
    return n, d, b, t_abs, t_rel, q


def _first_maximum(val, idx, d, axis):
    """per pixel, the largest value within d along `axis` and the smallest index that holds it"""
    best_v, best_i = val.copy(), idx.copy()
    for s in range(1, min(d, val.shape[axis] - 1) + 1):
        for dst, src in ((slice(s, None), slice(None, -s)), (slice(None, -s), slice(s, None))):
            at = (slice(None),) * axis + (dst,)
            frm = (slice(None),) * axis + (src,)
            bv, bi, ov, oi = best_v[at], best_i[at], val[frm], idx[frm]
            take = (ov > bv) | ((ov == bv) & (oi < bi))
            best_v[at] = np.where(take, ov, bv)
            best_i[at] = np.where(take, oi, bi)
    return best_v, best_i


def _windows(maps, f, cy, cx, radius):
    """values (n_sel, (2 radius + 1)^2) of the windows around (cy, cx) in the frames f, which of them lie inside
    the frame, and their rows and columns"""
    _, h, w = maps.shape
    radius = min(radius, max(h, w))
    off = np.arange(-radius, radius + 1)
    shape = (len(f), off.size, off.size)
    yy = np.broadcast_to(cy[:, None, None] + off[None, :, None], shape).reshape((len(f), -1))
    xx = np.broadcast_to(cx[:, None, None] + off[None, None, :], shape).reshape((len(f), -1))
    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    win = maps[f[:, None], np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float64)
    return win, inside, yy, xx


def find_in_maps(maps, num_peaks, min_distance, border=0, threshold_abs=0.0, threshold_rel=0.0, refine_radius=1):
    """Steps 1 - 6 on maps (n, h, w) of any float dtype: the decisions on the values as given (the relative threshold
    is one multiply in the maps' dtype), the statistics in float64, cast at the end.
    -> n_found (n,) int32, centers (n, N, 2) int32, refineds (n, N, 2) float32, peak_values, peak_elevations (n, N)
    float32"""
    maps = np.asarray(maps)
    if maps.ndim != 3 or maps.dtype.kind != 'f':
        raise ValueError(f"maps must be floats of shape (n, h, w), not {maps.dtype} {maps.shape}")
    n, h, w = maps.shape
    n_peaks, d, b, t_abs, t_rel, q = check_params((h, w), num_peaks, min_distance, border, threshold_abs,
                                                  threshold_rel, refine_radius)
    n_found = np.zeros(n, dtype=np.int32)
    centers = np.full((n, n_peaks, 2), -1, dtype=np.int32)
    refineds = np.full((n, n_peaks, 2), np.nan, dtype=np.float32)
    values = np.full((n, n_peaks), np.nan, dtype=np.float32)
    elevations = np.full((n, n_peaks), np.nan, dtype=np.float32)
    if n == 0:
        return n_found, centers, refineds, values, elevations
    with quiet_floats():
        finite = np.isfinite(maps).all(axis=(1, 2))
        idx = np.broadcast_to(np.arange(h * w, dtype=np.int64).reshape((1, h, w)), maps.shape)
        best_v, best_i = _first_maximum(maps, idx, d, axis=2)
        best_v, best_i = _first_maximum(best_v, best_i, d, axis=1)
        yy, xx = np.mgrid[:h, :w]
        inner = (yy >= b) & (yy < h - b) & (xx >= b) & (xx < w - b)
        eligible = (best_i == idx) & inner[None] & (maps > np.float32(t_abs)) & finite[:, None, None]
        f, p = np.nonzero(eligible.reshape((n, -1)))
        v = maps.reshape((n, -1))[f, p]
        order = np.lexsort((p, -v, f))                       # frame, value descending, index ascending
        f, p, v = f[order], p[order], v[order]
        v0 = v[np.searchsorted(f, f)]                        # (f is sorted: the first entry of its frame)
        keep = ~((v0 > 0) & (v < maps.dtype.type(np.float32(t_rel)) * v0))
        f, p, v = f[keep], p[keep], v[keep]
        rank = np.arange(len(f)) - np.searchsorted(f, f)
        top = rank < n_peaks
        f, p, v, rank = f[top], p[top], v[top], rank[top]
        np.add.at(n_found, f, 1)
        cy, cx = p // w, p % w
        centers[f, rank, 0], centers[f, rank, 1] = cy, cx
        values[f, rank] = v
        if len(f):
            win, inside, _, _ = _windows(maps, f, cy, cx, d)
            cnt = inside.sum(axis=1)
            mean = (win * inside).sum(axis=1) / cnt
            std = np.sqrt((inside * (win - mean[:, None]) ** 2).sum(axis=1) / cnt)
            elevations[f, rank] = np.where(std > 0, (v.astype(np.float64) - mean) / np.where(std > 0, std, 1), 0)
            nb, inside, ny, nx = _windows(maps, f, cy, cx, q)
            wgt = (nb - np.where(inside, nb, np.inf).min(axis=1)[:, None]) * inside
            total = wgt.sum(axis=1)
            safe = np.where(total > 0, total, 1)
            refineds[f, rank, 0] = np.where(total > 0, (wgt * ny).sum(axis=1) / safe, cy)
            refineds[f, rank, 1] = np.where(total > 0, (wgt * nx).sum(axis=1) / safe, cx)
    return n_found, centers, refineds, values, elevations


def _correlation_maps(frames64, template):
    t_spec = np.conj(np.fft.rfft2(np.fft.ifftshift(np.asarray(template, dtype=np.float32).astype(np.float64))))
    return np.fft.irfft2(np.fft.rfft2(frames64) * t_spec[None], s=frames64.shape[1:])


def find_peaks(frame, template, num_peaks, min_distance, border=0, threshold_abs=0.0, threshold_rel=0.0,
               refine_radius=1):
    """The peaks of ONE host frame -- a `run_logsum` or SumUDF result, say -- in float64 on the CPU: integer
    (n_found, 2) positions (y, x), strongest first, ready for `CorrelationUDF(peaks=...)`."""
    frame = np.asarray(frame, dtype=np.float64)
    if frame.ndim != 2 or np.shape(template) != frame.shape:
        raise ValueError(f"template of shape {np.shape(template)} for a frame of {frame.shape}")
    with quiet_floats():
        maps = _correlation_maps(frame[None], template)
    n_found, centers, _, _, _ = find_in_maps(maps, num_peaks, min_distance, border, threshold_abs, threshold_rel,
                                             refine_radius)
    return centers[0, :int(n_found[0])].copy()


class PeakFindUDF(WholeFrameUDF):
    """
    Parameters
    ----------
    template : array of float, shape of a frame
        real template centred at (h // 2, w // 2), used as float32
    num_peaks : int
        N, the number of result slots per frame, 1 to 1024
    min_distance : int
        d, at least 1: a peak is the first maximum of its (2d + 1)^2 neighbourhood
    border : int
        peaks closer than this to an edge are not kept
    threshold_abs, threshold_rel : float
        a peak's value exceeds threshold_abs and is not below threshold_rel (in [0, 1]) times the strongest one
    refine_radius : int
        half edge of the centre-of-mass neighbourhood, at least 1

    Results (nav, on the device): 'n_found' (int32), 'centers' (int32, (N, 2)), 'refineds' (float32, (N, 2)),
    'peak_values' and 'peak_elevations' (float32, (N,)); slots from n_found on hold (-1, -1) and NaN.
    """

    def __init__(self, template, num_peaks, min_distance, border=0, threshold_abs=0.0, threshold_rel=0.0,
                 refine_radius=1):
        super().__init__(template=template, num_peaks=num_peaks, min_distance=min_distance, border=border,
                         threshold_abs=threshold_abs, threshold_rel=threshold_rel, refine_radius=refine_radius)

    def get_result_buffers(self):
        n = int(self.params.num_peaks)
        if n < 1:
            raise ValueError(f"num_peaks {self.params.num_peaks} must lie in [1, {MAX_PEAKS}]")
        return {
            'n_found': self.buffer(kind='nav', dtype='int32', where='device'),
            'centers': self.buffer(kind='nav', dtype='int32', extra_shape=(n, 2), where='device'),
            'refineds': self.buffer(kind='nav', dtype='float32', extra_shape=(n, 2), where='device'),
            'peak_values': self.buffer(kind='nav', dtype='float32', extra_shape=(n,), where='device'),
            'peak_elevations': self.buffer(kind='nav', dtype='float32', extra_shape=(n,), where='device'),
        }

    def get_dist_merge(self):
        return {k: 'disjoint' for k in NAMES}

    def get_task_data(self):
        check_whole_frames(self)
        sig = tuple(int(s) for s in self.meta.dataset_shape.sig)
        if len(sig) != 2:
            raise ValueError(f"PeakFindUDF needs 2D frames, not {sig}")
        template = np.ascontiguousarray(self.params.template, dtype=np.float32)
        if template.shape != sig:
            raise ValueError(f"template of shape {template.shape} for frames of {sig}")
        p = self.params
        n, d, b, t_abs, t_rel, q = check_params(sig, p.num_peaks, p.min_distance, p.border, p.threshold_abs,
                                                p.threshold_rel, p.refine_radius)
        td = {'sig': sig, 'template': template, 'search': (n, d, b, t_abs, t_rel, q)}
        if runs_on_hip(self):
            if sig[1] > MAX_WIDTH:
                raise ValueError(f"frames of {sig[1]} columns: the device search takes at most {MAX_WIDTH}")
            td.update(plan=plan_for(self, sig, template))
        return td

    def _process_tile_numpy(self, tile):
        td = self.task_data
        with quiet_floats():
            maps = _correlation_maps(np.asarray(tile).astype(np.float32).astype(np.float64), td.template)
        res = find_in_maps(maps, *td.search)
        for name, value in zip(NAMES, res):
            getattr(self.results, name)[:] = value

    def _process_tile_hip(self, tile):
        r = self.results
        check_device_args(self, tile, r.n_found, r.centers, r.refineds, r.peak_values, r.peak_elevations)
        td = self.task_data
        td.plan.find_peaks(tile.data_ptr(), tile.dtype, tile.shape[0], tile.ld, *td.search,
                           r.n_found.data_ptr(), r.centers.data_ptr(), r.refineds.data_ptr(),
                           r.peak_values.data_ptr(), r.peak_elevations.data_ptr(), stream=self.meta.stream_ptr)


def run_peakfind(ctx, dataset, template, num_peaks, min_distance, border=0, threshold_abs=0.0, threshold_rel=0.0,
                 refine_radius=1, roi=None):
    """The num_peaks strongest correlation maxima of every frame of `dataset`; -> the five result buffers by name."""
    udf = PeakFindUDF(template=template, num_peaks=num_peaks, min_distance=min_distance, border=border,
                      threshold_abs=threshold_abs, threshold_rel=threshold_rel, refine_radius=refine_radius)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)
