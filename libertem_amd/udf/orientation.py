"""
OrientationMatchUDF on MI355X: orientation mapping of a polycrystalline scan by template matching in polar coordinates
(Cautaerts et al., Ultramicroscopy 237 (2022) 113517).  Every frame is resampled once to a polar image; an in-plane
rotation of a template is then a cyclic shift along phi, and every frame is scored against (templates x rotations)
candidates, of which the best few templates and their rotations are kept.

The definition (tests/orientation_ref.py restates it as loops).  Every float32 operation is
rounded on its own, so NumPy and the kernels give the same bytes for everything but `polar_norm`:

    1. `polar_table`: polar point (i, j) lies at r_i = r_min + i delta_r, phi_j = 2 pi j / n_phi, that is at
       y = cy + r_i sin phi_j, x = cx + r_i cos phi_j; its four taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
       (y0 + 1, x0 + 1) around it carry the bilinear weights, computed in float64 and rounded to float32; a tap outside
       the frame has index 0 and weight 0.
    2. P[i, j] = (w0 v0 + w1 v1) + (w2 v2 + w3 v3), v = float32(pixel); a tap of weight 0 is not read, its v is +0.
    3. `polar_library`: template t holds spots (spot_r, spot_phi, spot_w) sorted by (r, phi), unit 2-norm.
    4. score of template t at rotation k: acc = +0, then acc = acc + spot_w[s] * P[spot_r[s], (spot_phi[s] + k) mod
       n_phi] over its spots in stored order; c[t] = max over k, rot[t] = the smallest k that reaches it.
    5. the templates by c descending, then t ascending; the first n_best are the result, further slots hold
       template -1, rotation -1, correlation NaN.
    6. polar_norm = float32(sqrt(sum of float64(P)^2)).
    7. a frame with a non-finite pixel at a tap of non-zero weight: every slot -1 / -1 / NaN, polar_norm NaN.
       (P is then non-finite too, which is how `match_polar` sees it; frames whose P or scores overflow float32
       without such a pixel are outside the definition.)

On the device a tile goes through `ltmi_orient_match` (csrc/ltmi_orient.hip); on a CPU executor `polar_frames` and
`match_polar` compute the same.  The normalised correlation index is correlation / polar_norm, by the caller.
Not built: a pre-filter on the radial profile, sub-bin rotation refinement, a centre per frame, intensity transforms.
"""
import math

import numpy as np

from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, quiet_floats, runs_on_hip
from libertem_amd.udf.plans import PlanCache, array_digest, udf_device

#: what `ltmi_orient_plan_create` takes (csrc/ltmi_orient.hip); MAX_POLAR_WORDS is `hip.orient_max_polar_words()`: the
#: polar image shares the 160 KiB of LDS of a CU with 8 KiB of scores and 192 bytes of reduction scratch
MAX_BEST = 16
MAX_PHI = 1024
MAX_POLAR_WORDS = 38864
NAMES = ('template', 'rotation', 'correlation', 'polar_norm')
_PLANS = PlanCache(8, owned=False)          # (device, h, w, n_best, digest of table and library) -> hip.OrientPlan


def check_params(n_r, n_phi, n_best=1):
    """-> (n_r, n_phi, n_best) as ints; ValueError names the value that is off"""
    r, p, b = int(n_r), int(n_phi), int(n_best)
    if not 1 <= b <= MAX_BEST:
        raise ValueError(f"n_best {n_best} must lie in [1, {MAX_BEST}]")
    if not 1 <= p <= MAX_PHI:
        raise ValueError(f"n_phi {n_phi} must lie in [1, {MAX_PHI}]")
    if r < 1:
        raise ValueError(f"n_r {n_r} must be at least 1")
    if r * p > MAX_POLAR_WORDS:
        raise ValueError(f"a polar image of n_r {n_r} x n_phi {n_phi} = {r * p} values: at most {MAX_POLAR_WORDS} "
                         "fit the LDS of a CU next to the kernel's scores")
    return r, p, b


def check_library(library, n_r, n_phi):
    """-> (indptr int64, spot_r int32, spot_phi int32, spot_w float32), contiguous; ValueError names what is off"""
    try:
        indptr, spot_r, spot_phi, spot_w = library
    except (TypeError, ValueError):
        raise ValueError("a library is the quadruple (indptr, spot_r, spot_phi, spot_w) of `polar_library`")
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    spot_r = np.ascontiguousarray(spot_r, dtype=np.int32)
    spot_phi = np.ascontiguousarray(spot_phi, dtype=np.int32)
    spot_w = np.ascontiguousarray(spot_w, dtype=np.float32)
    if indptr.ndim != 1 or indptr.size < 2:
        raise ValueError(f"a library of {max(indptr.size - 1, 0) if indptr.ndim == 1 else indptr.shape} templates: "
                         "at least 1 is needed")
    if indptr[0] != 0 or np.any(np.diff(indptr) < 0):
        raise ValueError("indptr must start at 0 and never fall")
    n = int(indptr[-1])
    if not (spot_r.shape == spot_phi.shape == spot_w.shape == (n,)):
        raise ValueError(f"indptr ends at {n}, the spot arrays have shapes {spot_r.shape}, {spot_phi.shape} and "
                         f"{spot_w.shape}")
    if n:
        if spot_r.min() < 0 or spot_r.max() >= n_r:
            off = spot_r[(spot_r < 0) | (spot_r >= n_r)][0]
            raise ValueError(f"spot_r {off} lies outside [0, {n_r})")
        if spot_phi.min() < 0 or spot_phi.max() >= n_phi:
            off = spot_phi[(spot_phi < 0) | (spot_phi >= n_phi)][0]
            raise ValueError(f"spot_phi {off} lies outside [0, {n_phi})")
        if not np.all(np.isfinite(spot_w)):
            raise ValueError(f"spot_w {spot_w[~np.isfinite(spot_w)][0]} is not finite")
    return indptr, spot_r, spot_phi, spot_w


def polar_table(sig_shape, center, n_r, n_phi, r_min=1.0, delta_r=1.0):
    """Step 1 for frames of `sig_shape` = (h, w) and `center` = (cy, cx), floats.
    -> tap_idx int32 (n_r, n_phi, 4) of y * w + x, tap_w float32 (n_r, n_phi, 4)"""
    sig = tuple(int(s) for s in sig_shape)
    if len(sig) != 2 or min(sig) < 1:
        raise ValueError(f"polar_table needs 2D frames, not {tuple(sig_shape)}")
    h, w = sig
    n_r, n_phi, _ = check_params(n_r, n_phi)
    cy, cx = (float(c) for c in center)
    r = float(r_min) + np.arange(n_r, dtype=np.float64) * float(delta_r)
    phi = 2 * np.pi * np.arange(n_phi, dtype=np.float64) / n_phi
    y = cy + r[:, None] * np.sin(phi)[None, :]
    x = cx + r[:, None] * np.cos(phi)[None, :]
    if not (np.all(np.isfinite(y)) and np.all(np.isfinite(x))):
        raise ValueError(f"center {tuple(center)}, r_min {r_min} and delta_r {delta_r} must be finite")
    y0, x0 = np.floor(y), np.floor(x)
    fy, fx = y - y0, x - x0
    ty = np.stack([y0, y0, y0 + 1, y0 + 1], axis=-1)
    tx = np.stack([x0, x0 + 1, x0, x0 + 1], axis=-1)
    wgt = np.stack([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], axis=-1)
    inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
    tap_idx = np.where(inside, ty * w + tx, 0).astype(np.int32)
    tap_w = np.where(inside, wgt, 0).astype(np.float32)
    return tap_idx, tap_w


def polar_library(spot_lists, n_r, n_phi, r_min=1.0, delta_r=1.0):
    """Step 3 from one (qy, qx, intensity) triple of arrays per template, positions in pixels relative to the centre:
    r = rint((hypot(qy, qx) - r_min) / delta_r), phi = rint(atan2(qy, qx) n_phi / 2 pi) mod n_phi; spots with r outside
    [0, n_r) are dropped, spots of one bin added in float64 in the order given, a template's weights divided by
    their 2-norm in float64 (the root of the correctly rounded sum of squares) and rounded to float32, its spots
    sorted by (r, phi).  A template may end up empty; mirrored patterns are further templates.
    -> (indptr int64 (T + 1,), spot_r int32, spot_phi int32, spot_w float32)"""
    n_r, n_phi, _ = check_params(n_r, n_phi)
    indptr, rs, phis, ws = [0], [], [], []
    for spots in spot_lists:
        qy, qx, inten = (np.asarray(a, dtype=np.float64).reshape(-1) for a in spots)
        if not (qy.shape == qx.shape == inten.shape):
            raise ValueError(f"a template's qy, qx and intensity have shapes {qy.shape}, {qx.shape}, {inten.shape}")
        if not (np.all(np.isfinite(qy)) and np.all(np.isfinite(qx)) and np.all(np.isfinite(inten))):
            raise ValueError("spot positions and intensities must be finite")
        r = np.rint((np.hypot(qy, qx) - float(r_min)) / float(delta_r)).astype(np.int64)
        phi = np.rint(np.arctan2(qy, qx) * n_phi / (2 * np.pi)).astype(np.int64) % n_phi
        keep = (r >= 0) & (r < n_r)
        bins = r[keep] * n_phi + phi[keep]
        uniq, inverse = np.unique(bins, return_inverse=True)          # (sorted: by r, then phi)
        total = np.zeros(len(uniq), dtype=np.float64)
        np.add.at(total, inverse, inten[keep])                        # (unbuffered: in the order given)
        norm = math.sqrt(math.fsum(total * total))               # (the correctly rounded sum of the squares)
        if norm > 0:
            total = total / norm
        rs.append(uniq // n_phi)
        phis.append(uniq % n_phi)
        ws.append(total.astype(np.float32))
        indptr.append(indptr[-1] + len(uniq))
    if len(indptr) < 2:
        raise ValueError("a library of 0 templates: at least 1 is needed")
    return (np.asarray(indptr, dtype=np.int64), np.concatenate(rs).astype(np.int32),
            np.concatenate(phis).astype(np.int32), np.concatenate(ws).astype(np.float32))


def polar_frames(frames, tap_idx, tap_w):
    """Step 2 for frames (n, h, w) of any real dtype -> P float32 (n, n_r, n_phi)"""
    frames = np.asarray(frames)
    if frames.ndim != 3:
        raise ValueError(f"frames must have shape (n, h, w), not {frames.shape}")
    tap_idx, tap_w = np.asarray(tap_idx), np.asarray(tap_w, dtype=np.float32)
    with quiet_floats():
        v = frames.reshape((frames.shape[0], -1))[:, tap_idx].astype(np.float32)
        v = np.where(tap_w[None] != 0, v, np.float32(0))
        prod = tap_w[None] * v
        return (prod[..., 0] + prod[..., 1]) + (prod[..., 2] + prod[..., 3])


def match_polar(P, library, n_best=1):
    """Steps 4 - 7 on polar images P float32 (n, n_r, n_phi), vectorised over frames and rotations, in float32.
    -> template int32 (n, n_best), rotation int32 (n, n_best), correlation float32 (n, n_best), polar_norm
    float32 (n,)"""
    P = np.asarray(P)
    if P.ndim != 3 or P.dtype != np.float32:
        raise ValueError(f"P must be float32 of shape (n, n_r, n_phi), not {P.dtype} {P.shape}")
    n, n_r, n_phi = P.shape
    _, _, n_best = check_params(n_r, n_phi, n_best)
    indptr, spot_r, spot_phi, spot_w = check_library(library, n_r, n_phi)
    n_t = len(indptr) - 1
    template = np.full((n, n_best), -1, dtype=np.int32)
    rotation = np.full((n, n_best), -1, dtype=np.int32)
    correlation = np.full((n, n_best), np.nan, dtype=np.float32)
    norm = np.full(n, np.nan, dtype=np.float32)
    if n == 0:
        return template, rotation, correlation, norm
    with quiet_floats():
        good = np.isfinite(P).all(axis=(1, 2))
        twice = np.concatenate([P, P], axis=2)                        # row[(phi + k) mod n_phi] = twice[phi + k]
        c = np.zeros((n, n_t), dtype=np.float32)
        rot = np.zeros((n, n_t), dtype=np.int32)
        for t in range(n_t):
            acc = np.zeros((n, n_phi), dtype=np.float32)
            for s in range(indptr[t], indptr[t + 1]):
                acc = acc + spot_w[s] * twice[:, spot_r[s], spot_phi[s]:spot_phi[s] + n_phi]
            rot[:, t] = np.argmax(acc, axis=1)                        # (the first maximum)
            c[:, t] = acc[np.arange(n), rot[:, t]]
        order = np.argsort(-c, axis=1, kind='stable')[:, :n_best]     # (stable: of equal scores the lower t)
        k = order.shape[1]
        rows = np.arange(n)[:, None]
        template[:, :k], rotation[:, :k], correlation[:, :k] = order, rot[rows, order], c[rows, order]
        norm[:] = np.sqrt((P.astype(np.float64) ** 2).sum(axis=(1, 2))).astype(np.float32)
        template[~good], rotation[~good], correlation[~good], norm[~good] = -1, -1, np.nan, np.nan
    return template, rotation, correlation, norm


def rotation_angles(rotation, n_phi):
    """the in-plane rotation in radians, 2 pi rotation / n_phi, of `rotation` results; NaN where a slot is empty (-1)"""
    rotation = np.asarray(rotation)
    return np.where(rotation >= 0, 2 * np.pi * rotation / int(n_phi), np.nan)


def plan_for(udf, sig, tap_idx, tap_w, library, n_best):
    """the cached plan of a UDF's device, frame shape, sampling table, library and n_best"""
    from libertem_amd import hip
    device = udf_device(udf)
    key = (int(device), int(sig[0]), int(sig[1]), int(n_best), array_digest(tap_idx, tap_w, *library))
    return _PLANS.get_or_make(key, lambda: hip.OrientPlan(device, sig[0], sig[1], tap_idx, tap_w, library, n_best))


class OrientationMatchUDF(WholeFrameUDF):
    """
    Parameters
    ----------
    library : (indptr, spot_r, spot_phi, spot_w)
        the templates, as `polar_library` builds them for the same n_r, n_phi, r_min and delta_r
    center : (cy, cx)
        the pattern centre in pixels, floats, the same for every frame
    n_r, n_phi : int
        shape of the polar image: radii r_min + i delta_r, angles 2 pi j / n_phi (n_phi at most 1024)
    n_best : int
        result slots per frame, 1 to 16
    r_min, delta_r : float
        first radius and radial step in pixels

    Results (nav, on the device): 'template' and 'rotation' (int32, (n_best,)), 'correlation' (float32, (n_best,), the
    raw score), 'polar_norm' (float32); slots from the number of templates on hold -1, -1 and NaN.
    """

    def __init__(self, library, center, n_r, n_phi, n_best=1, r_min=1.0, delta_r=1.0):
        super().__init__(library=library, center=center, n_r=n_r, n_phi=n_phi, n_best=n_best, r_min=r_min,
                         delta_r=delta_r)

    def get_result_buffers(self):
        p = self.params
        _, _, n = check_params(p.n_r, p.n_phi, p.n_best)
        return {
            'template': self.buffer(kind='nav', dtype='int32', extra_shape=(n,), where='device'),
            'rotation': self.buffer(kind='nav', dtype='int32', extra_shape=(n,), where='device'),
            'correlation': self.buffer(kind='nav', dtype='float32', extra_shape=(n,), where='device'),
            'polar_norm': self.buffer(kind='nav', dtype='float32', where='device'),
        }

    def get_dist_merge(self):
        return {k: 'disjoint' for k in NAMES}

    def get_task_data(self):
        check_whole_frames(self)
        sig = tuple(int(s) for s in self.meta.dataset_shape.sig)
        if len(sig) != 2:
            raise ValueError(f"OrientationMatchUDF needs 2D frames, not {sig}")
        p = self.params
        n_r, n_phi, n_best = check_params(p.n_r, p.n_phi, p.n_best)
        library = check_library(p.library, n_r, n_phi)
        tap_idx, tap_w = polar_table(sig, p.center, n_r, n_phi, p.r_min, p.delta_r)
        td = {'sig': sig, 'tap_idx': tap_idx, 'tap_w': tap_w, 'library': library, 'n_best': n_best}
        if runs_on_hip(self):
            td.update(plan=plan_for(self, sig, tap_idx, tap_w, library, n_best))
        return td

    def _process_tile_numpy(self, tile):
        td = self.task_data
        res = match_polar(polar_frames(np.asarray(tile), td.tap_idx, td.tap_w), td.library, td.n_best)
        for name, value in zip(NAMES, res):
            getattr(self.results, name)[:] = value

    def _process_tile_hip(self, tile):
        r = self.results
        check_device_args(self, tile, r.template, r.rotation, r.correlation, r.polar_norm)
        self.task_data.plan.match(tile.data_ptr(), tile.dtype, tile.shape[0], tile.ld, r.template.data_ptr(),
                                  r.rotation.data_ptr(), r.correlation.data_ptr(), r.polar_norm.data_ptr(),
                                  stream=self.meta.stream_ptr)


def run_orientation_match(ctx, dataset, library, center, n_r, n_phi, n_best=1, r_min=1.0, delta_r=1.0, roi=None):
    """The n_best best templates and their rotations for every frame of `dataset`; -> the four result buffers by
    name."""
    udf = OrientationMatchUDF(library=library, center=center, n_r=n_r, n_phi=n_phi, n_best=n_best, r_min=r_min,
                              delta_r=delta_r)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)
