"""
LatticeRefineUDF on MI355X: the lattice that fits the matched peaks of every frame, the second step of strain and
orientation mapping (the first: `CorrelationUDF`, whose four results it keeps).

Per frame, for P peaks with refined positions r_k (`refineds`, float32 (y, x)), weights w_k (`peak_elevations` with
`weighted=True`, 1 otherwise), integer lattice indices (i_k, j_k), a start lattice zero0, a0, b0 and a `tolerance`
tau >= 0 in pixels; all arithmetic is float64, the results are cast once at the end:

    p_k         = zero0 + i_k a0 + j_k b0
    selector[k] = r_k finite, w_k finite, w_k > 0 and |r_k - p_k|_2 <= tau
                  (`weighted=False`: peak_values[k] finite takes the place of the two conditions on w_k)
    a fit EXISTS iff the index pairs of the selected peaks are not collinear -- decided on the integers: k0 the first
                  selected peak, k1 the first selected one with another index pair, some selected k with
                  (i_k - i_k0)(j_k1 - j_k0) - (j_k - j_k0)(i_k1 - i_k0) != 0
    zero, a, b  = argmin sum_sel w_k |zero + i_k a + j_k b - r_k|^2      (NaN where no fit exists)
    error       = sqrt(sum_sel w_k |res_k|^2 / sum_sel w_k)              (NaN where no fit exists)

The weight multiplies the SQUARED residual (a weighted least-squares fit with weights w_k, i.e. rows scaled by
sqrt(w_k)); other packages may scale the rows by w_k itself.

On the device one launch of `k_lattice_fit` follows the correlation of a tile on the same stream (`ltmi_lattice_fit`,
csrc/ltmi_lattice.hip); on a CPU executor `fit_lattice` computes the definition for all frames of a tile at once.
`lattice_strain` turns the fitted vectors into strain and rotation maps.
"""
import numpy as np

from libertem_amd.udf.correlation import CorrelationUDF
from libertem_amd.udf.device import check_device_args, quiet_floats

MAX_INDEX = 2**20
LATTICE_NAMES = ('zero', 'a', 'b', 'selector', 'error')


def _pair(v, name):
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (2,) or not np.all(np.isfinite(v)):
        raise ValueError(f"{name} must be a finite (y, x) pair, not {v!r}")
    return v


def _indices(indices):
    idx = np.asarray(indices)
    if idx.ndim != 2 or idx.shape[1] != 2 or idx.dtype.kind not in 'iu' or len(idx) < 1:
        raise ValueError(f"indices must be integers of shape (n_peaks, 2) with at least one row, not {idx.dtype} "
                         f"{idx.shape}")
    if np.abs(idx.astype(np.int64)).max() > MAX_INDEX:
        raise ValueError(f"indices must lie in [-2^20, 2^20], not up to {np.abs(idx.astype(np.int64)).max()}")
    return idx.astype(np.int32)


def _tolerance(tolerance):
    tol = float(tolerance)
    if not (tol >= 0 and np.isfinite(tol)):
        raise ValueError(f"tolerance must be finite and at least 0, not {tolerance}")
    return tol


def fit_lattice(refineds, weights, peak_values, indices, zero, a, b, tolerance):
    """The definition in NumPy for refineds (n, P, 2), weights and peak_values (n, P) or None, indices (P, 2): masked
    float64 sums and one batched solve over the frames whose fit exists, results cast at the end.
    -> zero, a, b (n, 2) float32, selector (n, P) bool, error (n,) float32"""
    r = np.asarray(refineds, dtype=np.float32).astype(np.float64)
    n, n_peaks = r.shape[:2]
    idx = np.asarray(indices).astype(np.int64).reshape((n_peaks, 2))
    zero, a, b = (np.asarray(v, dtype=np.float64) for v in (zero, a, b))
    w = np.ones((n, n_peaks)) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    pred = zero[None] + idx[:, :1] * a[None] + idx[:, 1:] * b[None]
    with quiet_floats():
        d = r - pred[None]
        sel = (np.isfinite(r).all(axis=2) & np.isfinite(w) & (w > 0)
               & (np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) <= float(tolerance)))
        if peak_values is not None:
            sel &= np.isfinite(np.asarray(peak_values, dtype=np.float32))
    # the first selected peak, the first selected one with another index pair, a third one off their line
    rows = np.arange(n)
    d0 = idx[None] - idx[np.argmax(sel, axis=1)][:, None, :]
    k1 = np.argmax(sel & (d0 != 0).any(axis=2), axis=1)
    d1 = d0[rows, k1]
    exists = (sel & (d0[..., 0] * d1[:, None, 1] - d0[..., 1] * d1[:, None, 0] != 0)).any(axis=1)
    out = {name: np.full((n, 2), np.nan, dtype=np.float32) for name in ('zero', 'a', 'b')}
    error = np.full(n, np.nan, dtype=np.float32)
    if exists.any():
        design = np.concatenate([np.ones((n_peaks, 1)), idx.astype(np.float64)], axis=1)
        ws = np.where(sel, w, 0.)[exists]
        rs = np.where(sel[..., None], r, 0.)[exists]
        normal = np.einsum('fk,kp,kq->fpq', ws, design, design)
        rhs = np.einsum('fk,kp,fkc->fpc', ws, design, rs)
        x = np.linalg.solve(normal, rhs)
        res = design[None] @ x - rs
        error[exists] = np.sqrt((ws * (res ** 2).sum(axis=2)).sum(axis=1) / ws.sum(axis=1))
        out['zero'][exists], out['a'][exists], out['b'][exists] = x[:, 0], x[:, 1], x[:, 2]
    return out['zero'], out['a'], out['b'], sel, error


def lattice_peaks(sig, zero, a, b, max_index, margin=0):
    """All (i, j) in [-max_index, max_index]^2, in row-major order, whose rounded position rint(zero + i a + j b)
    lies at least `margin` pixels inside a frame of shape `sig`.  -> indices, peaks: int32 (P, 2)"""
    zero, a, b = _pair(zero, 'zero'), _pair(a, 'a'), _pair(b, 'b')
    span = np.arange(-int(max_index), int(max_index) + 1)
    idx = np.stack(np.meshgrid(span, span, indexing='ij'), axis=-1).reshape((-1, 2))
    pos = np.rint(zero[None] + idx[:, :1] * a[None] + idx[:, 1:] * b[None])
    inside = ((pos >= margin) & (pos <= np.array(sig) - 1 - margin)).all(axis=1)
    return idx[inside].astype(np.int32), pos[inside].astype(np.int32)


def lattice_strain(a, b, ref_a, ref_b):
    """Strain and rotation of the lattices (a, b), arrays of shape (..., 2) of (y, x) vectors, against the reference
    lattice (ref_a, ref_b), in float64: F = [a b] [ref_a ref_b]^-1 with the vectors as columns and (y, x) as rows,
    F = [[F_yy, F_yx], [F_xy, F_xx]].  -> dict of e_yy = F_yy - 1, e_xx = F_xx - 1, e_yx = (F_yx + F_xy) / 2 and
    rotation = (F_yx - F_xy) / 2, the small rotation angle in radians: positive turns the x axis towards the y axis
    (counter-clockwise with x to the right and y upwards, clockwise on a displayed image, whose y points down).
    NaN lattices give NaN."""
    a, b, ra, rb = (np.asarray(v, dtype=np.float64) for v in (a, b, ref_a, ref_b))
    with quiet_floats():
        det = ra[..., 0] * rb[..., 1] - rb[..., 0] * ra[..., 1]
        f_yy = (a[..., 0] * rb[..., 1] - b[..., 0] * ra[..., 1]) / det
        f_yx = (b[..., 0] * ra[..., 0] - a[..., 0] * rb[..., 0]) / det
        f_xy = (a[..., 1] * rb[..., 1] - b[..., 1] * ra[..., 1]) / det
        f_xx = (b[..., 1] * ra[..., 0] - a[..., 1] * rb[..., 0]) / det
    return {'e_yy': f_yy - 1, 'e_xx': f_xx - 1, 'e_yx': (f_yx + f_xy) / 2, 'rotation': (f_yx - f_xy) / 2}


class LatticeRefineUDF(CorrelationUDF):
    """
    Parameters
    ----------
    indices : array of int, shape (n_peaks, 2)
        lattice indices (i, j) of the peaks, at least one, |value| <= 2^20; the expected peak positions of the
        correlation are rint(zero + i a + j b) and must lie inside the frame
    zero, a, b : (y, x) pairs
        the start lattice
    template, crop_radius, refine_radius
        as for CorrelationUDF
    tolerance : float
        largest distance in pixels of a refined position from the start lattice's prediction at which the peak takes
        part in the fit; default: crop_radius
    weighted : bool
        weight every peak's squared residual with its peak_elevation (default), or with 1

    Results (nav, on the device): the four of CorrelationUDF, and 'zero', 'a', 'b' (float32, (2,)), 'selector' (bool,
    (n_peaks,)), 'error' (float32): NaN lattices and errors where no fit exists.
    """

    def __init__(self, indices, zero, a, b, template, crop_radius, refine_radius=1, tolerance=None, weighted=True):
        super(CorrelationUDF, self).__init__(indices=indices, zero=zero, a=a, b=b, template=template,
                                             crop_radius=crop_radius, refine_radius=refine_radius,
                                             tolerance=tolerance, weighted=weighted)

    def _lattice(self):
        """-> indices int32 (n_peaks, 2), start (zero0, a0, b0 as 6 float64), tolerance"""
        p = self.params
        start = np.concatenate([_pair(p.zero, 'zero'), _pair(p.a, 'a'), _pair(p.b, 'b')])
        return _indices(p.indices), start, _tolerance(p.crop_radius if p.tolerance is None else p.tolerance)

    def _peaks(self):
        idx, start, _ = self._lattice()
        return np.rint(start[None, 0:2] + idx[:, :1] * start[None, 2:4] + idx[:, 1:] * start[None, 4:6]).astype(
            np.int32)

    def get_result_buffers(self):
        n_peaks = len(self._peaks())
        bufs = super().get_result_buffers()
        for name in ('zero', 'a', 'b'):
            bufs[name] = self.buffer(kind='nav', dtype='float32', extra_shape=(2,), where='device')
        bufs['selector'] = self.buffer(kind='nav', dtype='bool', extra_shape=(n_peaks,), where='device')
        bufs['error'] = self.buffer(kind='nav', dtype='float32', where='device')
        return bufs

    def get_dist_merge(self):
        return dict(super().get_dist_merge(), **{name: 'disjoint' for name in LATTICE_NAMES})

    def get_task_data(self):
        td = super().get_task_data()
        idx, start, tol = self._lattice()
        td.update(indices=idx, start=start, tol=tol, device_indices={})
        return td

    def _process_tile_numpy(self, tile):
        super()._process_tile_numpy(tile)
        td, r = self.task_data, self.results
        weighted = bool(self.params.weighted)
        res = fit_lattice(np.asarray(r.refineds), np.asarray(r.peak_elevations) if weighted else None,
                          None if weighted else np.asarray(r.peak_values), td.indices, td.start[0:2],
                          td.start[2:4], td.start[4:6], td.tol)
        for name, value in zip(LATTICE_NAMES, res):
            getattr(r, name)[:] = value

    def _process_tile_hip(self, tile):
        super()._process_tile_hip(tile)
        from libertem_amd import hip
        td, r = self.task_data, self.results
        weighted = bool(self.params.weighted)
        check_device_args(self, tile, r.zero, r.a, r.b, r.selector, r.error)
        indices = td.device_indices.get(tile.device)
        if indices is None:
            import torch
            indices = td.device_indices[tile.device] = torch.from_numpy(td.indices.reshape(-1).copy()).to(
                f'cuda:{tile.device}')
        hip.lattice_fit(tile.device, r.refineds.data_ptr(), r.peak_elevations.data_ptr() if weighted else None,
                        None if weighted else r.peak_values.data_ptr(), tile.shape[0], len(td.indices),
                        indices.data_ptr(), td.start, td.tol, r.zero.data_ptr(), r.a.data_ptr(), r.b.data_ptr(),
                        r.selector.data_ptr(), r.error.data_ptr(), stream=self.meta.stream_ptr)


def run_refine(ctx, dataset, zero, a, b, indices, template, crop_radius, refine_radius=1, tolerance=None,
               weighted=True, roi=None):
    """Template matching at the lattice positions `indices` of (zero, a, b) and the lattice fit to the matches, for
    every frame of `dataset`; -> the nine result buffers by name."""
    udf = LatticeRefineUDF(indices=indices, zero=zero, a=a, b=b, template=template, crop_radius=crop_radius,
                           refine_radius=refine_radius, tolerance=tolerance, weighted=weighted)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)
