"""
SSBUDF on MI355X: single-sideband ptychography of a focused-probe 4D-STEM scan (Rodenburg, McCallum & Nellist,
Ultramicroscopy 48 (1993) 304; Pennycook et al., Ultramicroscopy 151 (2015) 160; Strauch et al., Microsc. Microanal.
27 (2021) 1078), the consumer of `libertem_amd.utils.generate.weak_phase_scan`.

The operation, for a scan (Ny, Nx) of real frames (h, w), the wavelength `lamb`, the scan
step `dpix` = (dy, dx) in the unit of `lamb`, the convergence semi-angle `semiconv` in rad and its radius on the
detector `semiconv_pix` in pixels, the disk centre (cy, cx), a 2 x 2 `transformation` T acting on (y, x), an integer
`cutoff` >= 1 and the signed frequency s(i, n) = i if i <= (n - 1) // 2 else i - n (NumPy's fftfreq order):

    A(y, x)      = (y - cy)^2 + (x - cx)^2 < semiconv_pix^2       the bright-field pixels K, P of them, row-major
    G[K, iy, ix] = sum_R I[R, K] exp(-2 pi i (s(iy) ry / Ny + s(ix) rx / Nx))      np.fft.fft2 over the scan axes
    for Q = (iy, ix) != (0, 0):
      q   = (s(iy) / (Ny dy), s(ix) / (Nx dx))
      d   = T q lamb semiconv_pix / semiconv                      the shift of the diffracted disks in detector pixels
      A+- = the same disk centred at (cy, cx) +- d
      pos = A and A+ and not A-,   neg = A and A- and not A+      the two "trotters"
      fourier[Q] = (sum_pos G[K, Q] / |pos| - sum_neg G[K, Q] / |neg|) / 2  if |pos| >= cutoff and |neg| >= cutoff,
                   else 0
    fourier[0, 0] = sum_A G[K, 0] / P
    complex = ifft2(fourier),  phase = angle(complex),  amplitude = |complex|

The three predicates are float64, every product, quotient and sum rounded on its own in the order written (products
and quotients left to right): the device and NumPy agree on them bit for bit.  Every Q is computed from its own d --
`fourier` is not antisymmetric at the Nyquist index of an even scan axis, where s = -n / 2.  A region of interest is
a ValueError (the transform needs the full rectangle), as are P = 0 and cutoff < 1.  A frame with a non-finite pixel
inside the disk gives an unspecified result; pixels outside the disk are never read.

The published UDF forms frame . mask_Q for every Q and multiplies by a DFT phase: O(N^2 P) for N scan positions.  Here
the bright-field pixels of every frame are gathered once (`ltmi_ssb_gather`, the only pass over the frames), and
`fourier` comes from one batched FFT over the scan axes per bright-field pixel and one kernel that evaluates the
trotters analytically (`ltmi_ssb_reconstruct`, csrc/ltmi_ssb.hip): O(P N log N), no mask stack.  On a CPU executor
NumPy computes the definition in float64 / complex128 and casts at the end.  The inverse transform of the one
(Ny, Nx) image is NumPy's in complex128 in both cases.
Not part of this module: sub-pixel trotter masks, aberration correction, WDD and iterative ptychography.
"""
import contextlib

import numpy as np

from libertem_amd.common.hiparray import HipArray
from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, quiet_floats, runs_on_hip
from libertem_amd.udf.holography import signed_frequencies
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES, PlanCache, udf_device

# (device, Ny, Nx, w, batch, cutoff, the geometry and the list as bytes) -> hip.SSBPlan; a plan holds up to the
# workspace budget of HBM
_PLANS = PlanCache(2, owned=True)

#: (name, dtype, extra shape) of the results of SSBUDF and WDDUDF; 'nav': the scan shape
IMAGE_RESULTS = (('fourier', 'complex64', 'nav'), ('complex', 'complex64', 'nav'), ('phase', 'float32', 'nav'),
                 ('amplitude', 'float32', 'nav'))
RESULTS = tuple(name for name, _, _ in IMAGE_RESULTS)


def wavelength(kilovolts):
    """The relativistic de Broglie wavelength of an electron accelerated through `kilovolts` kV, in metres:
    h / sqrt(2 m e U (1 + e U / (2 m c^2))) with the CODATA 2018 constants (300 kV: 1.9687 pm)."""
    planck, mass, charge, light = 6.62607015e-34, 9.1093837015e-31, 1.602176634e-19, 299792458.
    energy = charge * float(kilovolts) * 1e3
    return planck / np.sqrt(2 * mass * energy * (1 + energy / (2 * mass * light ** 2)))


def check_params(sig, lamb, dpix, semiconv, semiconv_pix, cy=None, cx=None, transformation=None, cutoff=1):
    """-> dict(lamb, dy, dx, semiconv, semiconv_pix, cy, cx, t (2 x 2 float64), cutoff) with the defaults filled in;
    ValueError names the value that is off"""
    if len(sig) != 2:
        raise ValueError(f"SSBUDF needs 2D frames, not {tuple(sig)}")
    h, w = (int(s) for s in sig)
    try:
        dy, dx = (float(dpix), float(dpix)) if np.ndim(dpix) == 0 else (float(v) for v in dpix)
    except (TypeError, ValueError):
        raise ValueError(f"dpix {dpix!r} must be a number or (dy, dx)")
    values = dict(lamb=float(lamb), dy=dy, dx=dx, semiconv=float(semiconv), semiconv_pix=float(semiconv_pix))
    for name, v in values.items():
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} {v!r} must be positive and finite")
    cy = h / 2 if cy is None else float(cy)
    cx = w / 2 if cx is None else float(cx)
    if not (np.isfinite(cy) and np.isfinite(cx)):
        raise ValueError(f"the disk centre {(cy, cx)} must be finite")
    t = np.eye(2) if transformation is None else np.asarray(transformation, dtype=np.float64)
    if t.shape != (2, 2):
        raise ValueError(f"transformation of shape {t.shape} must be a 2 x 2 matrix acting on (y, x)")
    if not np.all(np.isfinite(t)):
        raise ValueError("transformation must be finite")
    if int(cutoff) != cutoff or int(cutoff) < 1:
        raise ValueError(f"cutoff {cutoff!r} must be an integer >= 1")
    return dict(values, cy=cy, cx=cx, t=np.ascontiguousarray(t), cutoff=int(cutoff))


def bf_pixels(sig, semiconv_pix, cy, cx):
    """the row-major indices of the detector pixels with (y - cy)^2 + (x - cx)^2 < semiconv_pix^2 -> int32 (P)"""
    h, w = (int(s) for s in sig)
    y = np.arange(h, dtype=np.float64)[:, None]
    x = np.arange(w, dtype=np.float64)[None, :]
    inside = (y - cy) * (y - cy) + (x - cx) * (x - cx) < float(semiconv_pix) * float(semiconv_pix)
    return np.flatnonzero(inside.reshape(-1)).astype(np.int32)


def disk_pixels(sig, p):
    """`bf_pixels` of the checked parameters p; ValueError for an empty disk"""
    idx = bf_pixels(sig, p['semiconv_pix'], p['cy'], p['cx'])
    if idx.size == 0:
        raise ValueError(f"no detector pixel lies within semiconv_pix {p['semiconv_pix']} of {(p['cy'], p['cx'])}: "
                         f"P = 0")
    return idx


def _shifts(p, nav_shape, iy):
    """d of the Qs (iy, 0 .. Nx - 1) -> (d_y, d_x), float64 (Nx) each"""
    ny, nx = nav_shape
    qy = float(signed_frequencies(ny)[iy]) / (float(ny) * p['dy'])
    qx = signed_frequencies(nx).astype(np.float64) / (float(nx) * p['dx'])
    t = p['t']
    ty = t[0, 0] * qy + t[0, 1] * qx
    tx = t[1, 0] * qy + t[1, 1] * qx
    return (ty * p['lamb'] * p['semiconv_pix'] / p['semiconv'], tx * p['lamb'] * p['semiconv_pix'] / p['semiconv'])


def _trotters(p, nav_shape, iy, y, x):
    """(pos, neg), bool (Nx, len(y)), of the Qs of row iy over the pixels (y, x) of the disk"""
    d_y, d_x = _shifts(p, nav_shape, iy)
    r2 = p['semiconv_pix'] * p['semiconv_pix']

    def inside(oy, ox):
        v, u = y[None, :] - oy[:, None], x[None, :] - ox[:, None]
        return v * v + u * u < r2

    in_p = inside(p['cy'] + d_y, p['cx'] + d_x)
    in_m = inside(p['cy'] - d_y, p['cx'] - d_x)
    return in_p & ~in_m, in_m & ~in_p


def trotter_masks(sig, q_index, nav_shape, **params):
    """The (pos, neg) boolean detector masks (h, w) of the spatial frequency Q = q_index = (iy, ix) of a scan of
    `nav_shape`, on the host, for inspection; **params as for `SSBUDF`."""
    p = check_params(sig, **params)
    h, w = (int(s) for s in sig)
    iy, ix = (int(v) for v in q_index)
    ny, nx = (int(v) for v in nav_shape)
    if not (0 <= iy < ny and 0 <= ix < nx):
        raise ValueError(f"q_index {(iy, ix)} lies outside the {(ny, nx)} scan")
    idx = bf_pixels(sig, p['semiconv_pix'], p['cy'], p['cx'])
    pos, neg = _trotters(p, (ny, nx), iy, (idx // w).astype(np.float64), (idx % w).astype(np.float64))
    out = np.zeros((2, h * w), bool)
    out[0, idx], out[1, idx] = pos[ix], neg[ix]
    return out[0].reshape(h, w), out[1].reshape(h, w)


def _images(fourier, scale=1.0):
    """fourier (complex64 or complex128, unshifted) -> the four results in their result dtypes; complex =
    scale ifft2(fourier)"""
    with quiet_floats():
        cplx = np.fft.ifft2(np.asarray(fourier).astype(np.complex128))
        if scale != 1.0:
            cplx = cplx * scale         # (not by 1: a complex product turns -0 into +0, which `angle` tells apart)
        return {'fourier': np.asarray(fourier).astype(np.complex64), 'complex': cplx.astype(np.complex64),
                'phase': np.angle(cplx).astype(np.float32), 'amplitude': np.abs(cplx).astype(np.float32)}


def reconstruct_bf(bf, nav_shape, sig, lamb, dpix, semiconv, semiconv_pix, cy=None, cx=None, transformation=None,
                   cutoff=1):
    """The definition in NumPy from bf (Ny Nx, P), the bright-field pixels `bf_pixels(sig, ...)` of every frame:
    float64 / complex128 throughout, cast at the end.  -> dict of 'fourier', 'complex' (complex64), 'phase',
    'amplitude' (float32), each (Ny, Nx)"""
    p = check_params(sig, lamb, dpix, semiconv, semiconv_pix, cy, cx, transformation, cutoff)
    ny, nx = (int(v) for v in nav_shape)
    w = int(sig[1])
    idx = disk_pixels(sig, p)
    bf = np.asarray(bf)
    if bf.shape != (ny * nx, idx.size):
        raise ValueError(f"bf of shape {bf.shape} for a scan of {(ny, nx)} and {idx.size} bright-field pixels")
    y, x = (idx // w).astype(np.float64), (idx % w).astype(np.float64)
    with quiet_floats():
        # (P, Ny, Nx): the scan image of every bright-field pixel, transformed over its own two axes
        g = np.fft.fft2(np.ascontiguousarray(bf.T, dtype=np.float64).reshape(idx.size, ny, nx))
        fourier = np.zeros((ny, nx), np.complex128)
        for iy in range(ny):
            pos, neg = _trotters(p, (ny, nx), iy, y, x)
            n_pos, n_neg = pos.sum(axis=1), neg.sum(axis=1)
            row = g[:, iy, :].T                                       # (Nx, P)
            s_pos = np.where(pos, row, 0).sum(axis=1)
            s_neg = np.where(neg, row, 0).sum(axis=1)
            ok = (n_pos >= p['cutoff']) & (n_neg >= p['cutoff'])
            fourier[iy] = np.where(ok, (s_pos / np.maximum(n_pos, 1) - s_neg / np.maximum(n_neg, 1)) / 2, 0)
        fourier[0, 0] = g[:, 0, 0].sum() / idx.size
    return _images(fourier)


def _plan(device, nav_shape, sig_w, idx, batch, p):
    from libertem_amd import hip
    geom = hip.ssb_geometry(p['lamb'], (p['dy'], p['dx']), p['semiconv'], p['semiconv_pix'], p['cy'], p['cx'], p['t'])
    key = (int(device), nav_shape[0], nav_shape[1], int(sig_w), int(batch), p['cutoff'], geom.tobytes(), idx.tobytes())
    return _PLANS.get_or_make(key, lambda: hip.SSBPlan(device, nav_shape[0], nav_shape[1], sig_w, idx, batch, geom,
                                                       p['cutoff']))


def release_plans(device=None):
    """Destroy the cached plans of `device` (None: of every device) and free their workspace."""
    _PLANS.release(device)


def plan_batch(nav_shape, n_idx):
    """bright-field pixels per hipFFT execution: as many as the workspace budget (the one measured for correlation
    plans) allows -- per pixel the float32 scan image, its half spectrum and the transposed copy of that, after the
    40 bytes per Q of the accumulator and the list itself"""
    ny, nx = nav_shape
    per_pixel = 4 * ny * nx + 2 * 8 * ny * (nx // 2 + 1)
    budget = CORR_WORKSPACE_BYTES - 40 * ny * nx - 4 * n_idx
    return int(max(1, min(budget // per_pixel, n_idx)))


@contextlib.contextmanager
def device_stream(device, stream=None):
    """`device` as torch's current one, and the stream to launch on: `stream`, or -- after everything enqueued on the
    device has finished: the rows of bf were written on the executor's stream -- torch's current stream"""
    import torch
    with torch.cuda.device(device):
        if stream is None:
            torch.cuda.synchronize(device)
            stream = torch.cuda.current_stream(device)
        yield stream


def plan_fourier(plan, bf, nav_shape, stream=None):
    """`plan.reconstruct` (an SSBPlan's or a WDDPlan's) of a device-resident bf -> complex64 (Ny, Nx) on the host"""
    with device_stream(bf.device, stream) as stream:
        fourier = HipArray.empty(tuple(nav_shape), np.complex64, bf.device)
        plan.reconstruct(bf.data_ptr(), bf.ld, fourier.data_ptr(), stream=stream)
        stream.synchronize()
        return fourier.cpu()


def reconstruct_device(bf, nav_shape, sig_w, idx, p, stream=None):
    """`fourier` of a device-resident bf (HipArray (Ny Nx, P) float32) through the native plan -> complex64 (Ny, Nx)
    on the host"""
    ny, nx = nav_shape
    if tuple(bf.shape) != (ny * nx, idx.size) or bf.dtype != np.float32:
        raise ValueError(f"bf {bf.shape} {bf.dtype} for a scan of {(ny, nx)} and {idx.size} bright-field pixels")
    plan = _plan(bf.device, (ny, nx), sig_w, idx, plan_batch((ny, nx), idx.size), p)
    return plan_fourier(plan, bf, (ny, nx), stream)


class ScanPixelsUDF(WholeFrameUDF):
    """
    What the UDFs share that reconstruct one image from a list of detector pixels of every frame of a 2D scan.  The
    listed pixels are gathered into the buffer 'bf' (nav, on the device, float32 (len(list),)), the only pass over the
    frames; `get_results` reconstructs from the whole of it.  Positions a sync_offset leaves without a frame keep zero
    rows in 'bf', on the device as on the host.

    A subclass gives `_geometry() -> sig, nav, p, idx` (the frame and scan shapes, its checked parameters, the pixel
    list as int32 frame indices), `_reconstruct_device(bf, sig, nav, p, idx)` for a HipArray bf (Ny Nx, len(idx)) and
    `_reconstruct_host` for a NumPy one, both -> the dict of its results, and SINGLE_RESULTS where they are not the
    four images.
    """

    #: (name, dtype, extra shape) of the results; 'nav': the scan shape, 'P' in a shape: len(idx)
    SINGLE_RESULTS = IMAGE_RESULTS

    def _shapes(self):
        shape = self.meta.dataset_shape
        return tuple(int(s) for s in shape.sig), tuple(int(s) for s in shape.nav)

    def check_scan_geometry(self, min_positions):
        """ValueError for a scan that is not 2D or holds fewer than `min_positions` positions, and for a roi"""
        name, nav = type(self).__name__, self._shapes()[1]
        if len(nav) != 2 or nav[0] * nav[1] < min_positions:
            raise ValueError(f"{name} needs a 2D scan of at least {min_positions} positions, not {nav}")
        if self.meta.roi is not None:
            raise ValueError(f"{name} cannot take a roi: the transform over the scan needs the full rectangle")

    def get_result_buffers(self):
        _, nav, _, idx = self._geometry()
        n_idx = int(idx.size)
        bufs = {'bf': self.buffer(kind='nav', dtype='float32', extra_shape=(n_idx,), where='device')}
        for name, dtype, shape in self.SINGLE_RESULTS:
            shape = nav if shape == 'nav' else tuple(n_idx if s == 'P' else s for s in shape)
            bufs[name] = self.buffer(kind='single', dtype=dtype, extra_shape=shape, use='result_only')
        return bufs

    def get_dist_merge(self):
        return {'bf': 'disjoint'}

    def get_write_once_buffers(self):
        """whole-frame tiles: every row of 'bf' is written by one gather call (see SumSigUDF.get_write_once_buffers),
        so a partition's rows may go straight into the buffer of the whole scan"""
        ts = self.meta.tiling_scheme if self.meta is not None else None
        if self.meta is not None and self.meta.array_backend == self.BACKEND_NUMPY:
            return ()
        if ts is None or len(ts) != 1 or getattr(self.meta, 'sig_sliced_tiles', False):
            return ()
        return ('bf',)

    def get_task_data(self):
        check_whole_frames(self)
        sig, _, _, idx = self._geometry()
        td = {'sig': sig, 'idx': idx}
        if runs_on_hip(self):
            td.update(idx_dev=HipArray.from_numpy(idx, udf_device(self)))
        return td

    def _process_tile_numpy(self, tile):
        self.results.bf[:] = np.asarray(tile).reshape((tile.shape[0], -1))[:, self.task_data.idx]

    def _process_tile_hip(self, tile):
        from libertem_amd import hip
        td, bf = self.task_data, self.results.bf
        check_device_args(self, tile, bf)
        hip.ssb_gather(tile.device, tile.data_ptr(), tile.dtype, tile.shape[0], tile.ld, td.sig[0] * td.sig[1],
                       td.idx_dev.data_ptr(), td.idx.size, bf.data_ptr(), bf.ld, stream=self.meta.stream_ptr)

    def get_results(self):
        sig, nav, p, idx = self._geometry()
        bf = self.results.get_buffer('bf').result_array
        if isinstance(bf, HipArray):
            # a run with result_where='device': bf never left HBM
            return self._reconstruct_device(bf.reshape((nav[0] * nav[1], idx.size)), sig, nav, p, idx)
        return self._reconstruct_host(np.asarray(bf).reshape((nav[0] * nav[1], idx.size)), sig, nav, p, idx)


class SSBUDF(ScanPixelsUDF):
    """
    Parameters
    ----------
    lamb : float
        wavelength, e.g. `wavelength(300)` in metres
    dpix : float or (float, float)
        scan step (dy, dx), in the unit of `lamb`
    semiconv : float
        convergence semi-angle in rad
    semiconv_pix : float
        radius of the bright-field disk on the detector, in pixels
    cy, cx : float or None
        centre of the disk; None: (h / 2, w / 2)
    transformation : 2 x 2 array or None
        acts on (y, x) of the scan's spatial frequencies, e.g. `libertem_amd.corrections.coordinates.rotate_deg`;
        None: the identity
    cutoff : int
        a spatial frequency whose trotters hold fewer pixels than this is set to zero

    Results (single, extra shape = the scan shape): 'fourier', 'complex' (complex64), 'phase', 'amplitude' (float32).
    Buffer 'bf' (nav, on the device): the bright-field pixels of every frame, float32 (P).
    """

    def __init__(self, lamb, dpix, semiconv, semiconv_pix, cy=None, cx=None, transformation=None, cutoff=1):
        super().__init__(lamb=lamb, dpix=dpix, semiconv=semiconv, semiconv_pix=semiconv_pix, cy=cy, cx=cx,
                         transformation=transformation, cutoff=cutoff)

    def _geometry(self):
        """-> sig, nav, the checked parameters, the bright-field list; ValueError for what the operation cannot take"""
        pr = self.params
        sig, nav = self._shapes()
        p = check_params(sig, pr.lamb, pr.dpix, pr.semiconv, pr.semiconv_pix, pr.cy, pr.cx, pr.transformation,
                         pr.cutoff)
        self.check_scan_geometry(2)
        return sig, nav, p, disk_pixels(sig, p)

    def _reconstruct_device(self, bf, sig, nav, p, idx):
        return _images(reconstruct_device(bf, nav, sig[1], idx, p))

    def _reconstruct_host(self, bf, sig, nav, p, idx):
        pr = self.params
        return reconstruct_bf(bf, nav, sig, pr.lamb, pr.dpix, pr.semiconv, pr.semiconv_pix, pr.cy, pr.cx,
                              pr.transformation, pr.cutoff)


def _run_on_device(ctx, dataset, udf, names, keep_bf):
    """`udf` on a HIP context with 'bf' left on the device -> dict of the results `names` as host arrays, and with
    keep_bf 'bf', the HipArray"""
    res = ctx.run_udf(dataset=dataset, udf=udf, result_where='device')
    out = {name: np.asarray(res[name].data) for name in names}
    if keep_bf:
        out['bf'] = res['bf'].device_data
    return out


def run_ssb(ctx, dataset, lamb, dpix, semiconv, semiconv_pix, cy=None, cx=None, transformation=None, cutoff=1,
            keep_bf=False):
    """The single-sideband reconstruction of `dataset` on a HIP context, with the bright-field pixels left on the
    device (`result_where='device'`): they never cross the host link.  -> dict of 'fourier', 'complex', 'phase',
    'amplitude' as host arrays (Ny, Nx), and with keep_bf 'bf', the HipArray (Ny, Nx, P)."""
    udf = SSBUDF(lamb=lamb, dpix=dpix, semiconv=semiconv, semiconv_pix=semiconv_pix, cy=cy, cx=cx,
                 transformation=transformation, cutoff=cutoff)
    return _run_on_device(ctx, dataset, udf, RESULTS, keep_bf)
