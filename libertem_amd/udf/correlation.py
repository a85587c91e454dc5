"""
CorrelationUDF on MI355X: template matching at given peaks, the first step of strain and orientation mapping.

Every frame is cross-correlated with one template (a disk, `libertem_amd.masks.circular`, or a background-subtracting
one, `background_subtraction` / `radial_gradient_background_subtraction`); around every expected peak position the
maximum of the correlation is located in a small window and refined to sub-pixel precision.  The operation
(DESIGN.md section 4.6b), for a frame `x` as float32 `y`, a real float32 template `t` centred at (h // 2, w // 2),
integer peaks (py, px), `crop_radius` r and `refine_radius` q:

    corr = irfft2(rfft2(y) * conj(rfft2(ifftshift(t))), s=(h, w))          circular cross-correlation
    W    = corr[py - r:py + r + 1, px - r:px + r + 1], clipped to the frame (no wrap-around)
    peak_values[k]     = max(W)
    centers[k]         = (y, x) of the first maximum of W in row-major order, in frame coordinates
    refineds[k]        = centre of mass of N - min(N), N the (2q + 1)^2 neighbourhood of centers[k] clipped to the
                         frame; centers[k] where the weights sum to 0
    peak_elevations[k] = (max(W) - mean(W)) / std(W), ddof 0; 0 where std(W) is 0

A frame with a non-finite pixel has peak_values NaN for every peak; its other results are unspecified.

On the device a whole tile goes through two batched hipFFTs and three kernels (`ltmi_correlate_peaks`,
csrc/ltmi_corr.hip); on a CPU executor NumPy computes the definition in float64 and casts at the end.
"""
import numpy as np

from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, quiet_floats, runs_on_hip
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES, PlanCache, array_digest, frame_batch, udf_device

_PLANS = PlanCache(8, owned=False)          # (device, h, w, batch, template digest) -> hip.CorrPlan


def _plan(device, sig, batch, template):
    from libertem_amd import hip
    key = (int(device), int(sig[0]), int(sig[1]), int(batch), array_digest(template))
    return _PLANS.get_or_make(key, lambda: hip.CorrPlan(device, sig[0], sig[1], batch, template))


def plan_for(udf, sig, template):
    """the cached plan of a UDF's device, frame shape, template and batch: as many frames as the workspace budget,
    the tile depth and the partition allow"""
    per_frame = sig[0] * sig[1] * 4 + sig[0] * (sig[1] // 2 + 1) * 8
    return _plan(udf_device(udf), sig, frame_batch(udf, per_frame, CORR_WORKSPACE_BYTES), template)


def _window(p, radius, size):
    return max(p - radius, 0), min(p + radius, size - 1) + 1


def correlate_frames(frames, template, peaks, crop_radius, refine_radius=1):
    """The definition in NumPy for frames (n, h, w): float64 transforms and statistics, results cast at the end.
    -> centers (n, n_peaks, 2) int32, refineds (n, n_peaks, 2) float32, peak_values, peak_elevations (n, n_peaks)
    float32"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    n_peaks = len(peaks)
    centers = np.zeros((n, n_peaks, 2), dtype=np.int32)
    refineds = np.zeros((n, n_peaks, 2), dtype=np.float32)
    values = np.zeros((n, n_peaks), dtype=np.float32)
    elevations = np.zeros((n, n_peaks), dtype=np.float32)
    t_spec = np.conj(np.fft.rfft2(np.fft.ifftshift(np.asarray(template, dtype=np.float32).astype(np.float64))))
    with quiet_floats():
        y = frames.astype(np.float32).astype(np.float64)
        corr = np.fft.irfft2(np.fft.rfft2(y) * t_spec[None], s=(h, w))
        bad = ~np.isfinite(y).all(axis=(1, 2))
        for k, (py, px) in enumerate(peaks):
            ya, yb = _window(int(py), crop_radius, h)
            xa, xb = _window(int(px), crop_radius, w)
            win = corr[:, ya:yb, xa:xb].reshape((n, -1))
            first = np.argmax(win, axis=1)
            top = win[np.arange(n), first]
            cy, cx = ya + first // (xb - xa), xa + first % (xb - xa)
            centers[:, k, 0], centers[:, k, 1] = cy, cx
            values[:, k] = top
            std = win.std(axis=1)
            elevations[:, k] = np.where(std > 0, (top - win.mean(axis=1)) / np.where(std > 0, std, 1), 0)
            for f in range(n):
                na, nb = _window(int(cy[f]), refine_radius, h)
                ma, mb = _window(int(cx[f]), refine_radius, w)
                wgt = corr[f, na:nb, ma:mb] - corr[f, na:nb, ma:mb].min()
                total = wgt.sum()
                if total > 0:
                    refineds[f, k] = ((wgt.sum(axis=1) * np.arange(na, nb)).sum() / total,
                                      (wgt.sum(axis=0) * np.arange(ma, mb)).sum() / total)
                else:
                    refineds[f, k] = (cy[f], cx[f])
        values[bad] = np.nan
    return centers, refineds, values, elevations


class CorrelationUDF(WholeFrameUDF):
    """
    Parameters
    ----------
    peaks : array of int, shape (n_peaks, 2)
        expected peak positions (y, x) inside the frame
    template : array of float, shape of a frame
        real template centred at (h // 2, w // 2), used as float32
    crop_radius : int
        half edge of the search window around every peak, at least 1
    refine_radius : int
        half edge of the centre-of-mass neighbourhood around the maximum, at least 1

    Results (nav, on the device): 'centers' (int32, (n_peaks, 2)), 'refineds' (float32, (n_peaks, 2)), 'peak_values'
    and 'peak_elevations' (float32, (n_peaks,)).
    """

    def __init__(self, peaks, template, crop_radius, refine_radius=1):
        super().__init__(peaks=peaks, template=template, crop_radius=crop_radius, refine_radius=refine_radius)

    def _peaks(self):
        peaks = np.asarray(self.params.peaks)
        if peaks.ndim != 2 or peaks.shape[1] != 2 or peaks.dtype.kind not in 'iu':
            raise ValueError(f"peaks must be integers of shape (n_peaks, 2), not {peaks.dtype} {peaks.shape}")
        return peaks.astype(np.int32)

    def get_result_buffers(self):
        n_peaks = len(self._peaks())
        return {
            'centers': self.buffer(kind='nav', dtype='int32', extra_shape=(n_peaks, 2), where='device'),
            'refineds': self.buffer(kind='nav', dtype='float32', extra_shape=(n_peaks, 2), where='device'),
            'peak_values': self.buffer(kind='nav', dtype='float32', extra_shape=(n_peaks,), where='device'),
            'peak_elevations': self.buffer(kind='nav', dtype='float32', extra_shape=(n_peaks,), where='device'),
        }

    def get_dist_merge(self):
        return {k: 'disjoint' for k in ('centers', 'refineds', 'peak_values', 'peak_elevations')}

    def get_task_data(self):
        check_whole_frames(self)
        sig = tuple(int(s) for s in self.meta.dataset_shape.sig)
        if len(sig) != 2:
            raise ValueError(f"CorrelationUDF needs 2D frames, not {sig}")
        template = np.ascontiguousarray(self.params.template, dtype=np.float32)
        if template.shape != sig:
            raise ValueError(f"template of shape {template.shape} for frames of {sig}")
        peaks = self._peaks()
        inside = (peaks >= 0) & (peaks < np.array(sig))
        if not inside.all():
            k = int(np.flatnonzero(~inside.all(axis=1))[0])
            raise ValueError(f"peak {k} at {tuple(int(v) for v in peaks[k])} lies outside the {sig} frame")
        r, q = int(self.params.crop_radius), int(self.params.refine_radius)
        if r < 1 or q < 1:
            raise ValueError(f"crop_radius {r} and refine_radius {q} must be at least 1")
        td = {'sig': sig, 'template': template, 'peaks': peaks, 'r': r, 'q': q}
        if runs_on_hip(self):
            td.update(plan=plan_for(self, sig, template), device_peaks={})
        return td

    def process_tile(self, tile):
        if len(self.task_data.peaks):
            super().process_tile(tile)

    def _process_tile_numpy(self, tile):
        td = self.task_data
        res = correlate_frames(np.asarray(tile), td.template, td.peaks, td.r, td.q)
        self.results.centers[:] = res[0]
        self.results.refineds[:] = res[1]
        self.results.peak_values[:] = res[2]
        self.results.peak_elevations[:] = res[3]

    def _process_tile_hip(self, tile):
        r = self.results
        check_device_args(self, tile, r.centers, r.refineds, r.peak_values, r.peak_elevations)
        td = self.task_data
        peaks = td.device_peaks.get(tile.device)
        if peaks is None:
            import torch
            peaks = td.device_peaks[tile.device] = torch.from_numpy(td.peaks.reshape(-1).copy()).to(
                f'cuda:{tile.device}')
        td.plan.correlate_peaks(tile.data_ptr(), tile.dtype, tile.shape[0], tile.ld, peaks.data_ptr(),
                                len(td.peaks), td.r, td.q, r.centers.data_ptr(), r.refineds.data_ptr(),
                                r.peak_values.data_ptr(), r.peak_elevations.data_ptr(),
                                stream=self.meta.stream_ptr)


def run_correlation(ctx, dataset, peaks, template, crop_radius, refine_radius=1, roi=None):
    """Template matching at `peaks` for every frame of `dataset`; -> the four result buffers by name."""
    udf = CorrelationUDF(peaks=peaks, template=template, crop_radius=crop_radius, refine_radius=refine_radius)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)
