"""
WDDUDF on MI355X: Wigner-distribution deconvolution ptychography of a focused-probe 4D-STEM scan (Rodenburg & Bates,
Phil. Trans. R. Soc. A 339 (1992) 521; Yang et al., Ultramicroscopy 180 (2017) 173), the step after
`libertem_amd.udf.ssb`: the same data, the same geometry, the same transform over the scan axes, but no weak-phase
assumption -- the probe's own Wigner function is deconvolved with a Wiener filter in place of the +-1 trotter masks,
and the result is the complex object (phase and amplitude).

The operation, with s(i, n), the shift d(Q), the disk A and the float64 predicates of
`libertem_amd.udf.ssb`, a `window` (By, Bx) of detector pixels and `epsilon` > 0:

    y0 = floor(cy) - By // 2,  x0 = floor(cx) - Bx // 2       the window [y0, y0 + By) x [x0, x0 + Bx), row-major,
                                                              K = (v, u); it lies in the frame and holds all of A
    P  = |A|
    G[K, Q] = np.fft.fft2 over the scan axes of I[R, K]       for the window pixels
    for every Q = (iy, ix), the DC included:
      Gamma[K] = A[K] and A-[K]                               A- = the disk centred at (cy, cx) - d(Q)
      chi[rho] = sum_K Gamma[K] exp(+2 pi i (v rho_y / By + u rho_x / Bx))
      W[rho]   = conj(chi[rho]) / (|chi[rho]|^2 + epsilon P^2)
      H[rho]   = sum_K G[K, Q] exp(+2 pi i (v rho_y / By + u rho_x / Bx))
      S[Q]     = sum_rho H[rho] W[rho] / (By Bx)
    fourier[Q] = conj(S[-Q mod (Ny, Nx)]) / |S[0, 0]|
    complex = Ny Nx ifft2(fourier)  (the object, mean 1),  phase = angle(complex),  amplitude = |complex|

A Q whose two disks do not overlap has Gamma = 0 and S = 0 exactly: there is no cutoff.  A region of interest is a
ValueError; all-zero frames give NaN.  `weak_phase_scan(phi, ...)` reconstructs +phi.

Device and NumPy both use S[Q] = sum_K G[K, Q] F[K, Q] / (By Bx) with F[K, Q] = sum_rho W[rho] exp(+2 pi i ...): F
depends on the geometry alone and G is never transformed over the detector.  On the device the window pixels of every
frame are gathered once (`ltmi_ssb_gather` with the window's list), the native plan (`hip.WDDPlan`, csrc/ltmi_wdd.hip)
builds and keeps F (Ny Nx By Bx complex64) and sums G F per Q in float64; the inverse transform of the one (Ny, Nx)
image is NumPy's.  `epsilon` = 0.01 is a default, not a tuned value: a smaller one recovers more of the phase scale of
a noise-free scan and amplifies noise.
Not part of this module: F streamed or halved by symmetry, the dark-field rows k' != 0, aberrations and defocus in
the probe, the inverse transform on the device, iterative ptychography.
"""
import numpy as np

from libertem_amd.udf import ssb
from libertem_amd.udf.device import quiet_floats
from libertem_amd.udf.plans import PlanCache

# (device, Ny, Nx, batch, epsilon, the geometry and the window as bytes) -> hip.WDDPlan; a plan holds F and the
# workspace in HBM
_PLANS = PlanCache(2, owned=True)


def check_params(sig, lamb, dpix, semiconv, semiconv_pix, window, epsilon=0.01, cy=None, cx=None,
                 transformation=None):
    """-> dict(lamb, dy, dx, semiconv, semiconv_pix, cy, cx, t, window=(y0, x0, By, Bx), epsilon) with the defaults
    filled in, by the rules of `ssb.check_params`; ValueError names the value that is off"""
    p = ssb.check_params(sig, lamb, dpix, semiconv, semiconv_pix, cy, cx, transformation)
    del p['cutoff']
    h, w = (int(s) for s in sig)
    y0, x0, by, bx = _window_at(window, p['cy'], p['cx'])
    try:
        eps = float(epsilon)
    except (TypeError, ValueError):
        raise ValueError(f"epsilon {epsilon!r} must be a number")
    if not (np.isfinite(eps) and eps > 0):
        raise ValueError(f"epsilon {epsilon!r} must be positive and finite")
    if y0 < 0 or y0 + by > h:
        raise ValueError(f"window rows [{y0}, {y0 + by}) (By = {by} around cy = {p['cy']}) leave the frame of {h} rows")
    if x0 < 0 or x0 + bx > w:
        raise ValueError(f"window columns [{x0}, {x0 + bx}) (Bx = {bx} around cx = {p['cx']}) leave the frame of "
                         f"{w} columns")
    disk = ssb.disk_pixels(sig, p)
    y, x = disk // w, disk % w
    outside = (y < y0) | (y >= y0 + by) | (x < x0) | (x >= x0 + bx)
    if outside.any():
        k = int(np.flatnonzero(outside)[0])
        raise ValueError(f"window {(by, bx)} at {(y0, x0)} does not hold the disk pixel {(int(y[k]), int(x[k]))}: "
                         f"semiconv_pix {p['semiconv_pix']} needs a larger window")
    return dict(p, window=(y0, x0, by, bx), epsilon=eps)


def window_pixels(sig, window, cy=None, cx=None):
    """the row-major frame indices of the window (By, Bx) around the centre (None: (h / 2, w / 2)), [y0, y0 + By) x
    [x0, x0 + Bx) with y0 = floor(cy) - By // 2, x0 = floor(cx) - Bx // 2 -> int32 (By Bx); ValueError for a window
    that leaves the frame"""
    h, w = (int(s) for s in sig)
    cy = h / 2 if cy is None else float(cy)
    cx = w / 2 if cx is None else float(cx)
    return _window_list((h, w), _window_at(window, cy, cx))


def _window_at(window, cy, cx):
    """-> (y0, x0, By, Bx) of the window (By, Bx), or of one integer for both, around the centre (cy, cx)"""
    try:
        by, bx = (window, window) if np.ndim(window) == 0 else window
        if int(by) != by or int(bx) != bx or int(by) < 1 or int(bx) < 1:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"window {window!r} must be an integer or (By, Bx), each >= 1")
    by, bx = int(by), int(bx)
    return int(np.floor(cy)) - by // 2, int(np.floor(cx)) - bx // 2, by, bx


def _window_list(sig, window):
    y0, x0, by, bx = window
    if by < 1 or bx < 1 or y0 < 0 or x0 < 0 or y0 + by > sig[0] or x0 + bx > sig[1]:
        raise ValueError(f"window rows [{y0}, {y0 + by}) x columns [{x0}, {x0 + bx}) leave the frame {tuple(sig)}")
    rows = (np.arange(y0, y0 + by, dtype=np.int64) * sig[1])[:, None]
    return (rows + np.arange(x0, x0 + bx, dtype=np.int64)[None, :]).reshape(-1).astype(np.int32)


def _filters(p, nav_shape, iy):
    """F of the Qs (iy, 0 .. Nx - 1) -> complex128 (Nx, By, Bx)"""
    y0, x0, by, bx = p['window']
    d_y, d_x = ssb._shifts(p, nav_shape, iy)
    r2 = p['semiconv_pix'] * p['semiconv_pix']
    y = np.arange(y0, y0 + by, dtype=np.float64)[None, :, None]
    x = np.arange(x0, x0 + bx, dtype=np.float64)[None, None, :]

    def inside(oy, ox):
        v, u = y - np.reshape(oy, (-1, 1, 1)), x - np.reshape(ox, (-1, 1, 1))
        return v * v + u * u < r2

    in_a = inside(np.array([p['cy']]), np.array([p['cx']]))
    gamma = in_a & inside(p['cy'] - d_y, p['cx'] - d_x)
    n_disk = float(in_a.sum())
    chi = np.fft.ifft2(gamma.astype(np.float64)) * (by * bx)            # the unnormalised exp(+i) transform
    wiener = np.conj(chi) / (np.abs(chi) ** 2 + p['epsilon'] * n_disk * n_disk)
    return np.fft.ifft2(wiener) * (by * bx)


def wdd_filter(sig, q_index, nav_shape, **params):
    """The Wiener filter F[K] (complex128 (By, Bx)) of the spatial frequency Q = q_index = (iy, ix) of a scan of
    `nav_shape`, on the host, for inspection; **params as for `WDDUDF`."""
    p = check_params(sig, **params)
    iy, ix = (int(v) for v in q_index)
    ny, nx = (int(v) for v in nav_shape)
    if not (0 <= iy < ny and 0 <= ix < nx):
        raise ValueError(f"q_index {(iy, ix)} lies outside the {(ny, nx)} scan")
    return _filters(p, (ny, nx), iy)[ix]


def reconstruct_window(bf, nav_shape, sig, lamb, dpix, semiconv, semiconv_pix, window, epsilon=0.01, cy=None, cx=None,
                       transformation=None):
    """The definition in NumPy from bf (Ny Nx, By Bx), the window pixels `window_pixels(sig, window, cy, cx)` of every
    frame: float64 / complex128 throughout, in the F form, cast at the end.  -> dict of 'fourier', 'complex'
    (complex64), 'phase', 'amplitude' (float32), each (Ny, Nx)"""
    p = check_params(sig, lamb, dpix, semiconv, semiconv_pix, window, epsilon, cy, cx, transformation)
    ny, nx = (int(v) for v in nav_shape)
    _, _, by, bx = p['window']
    bf = np.asarray(bf)
    if bf.shape != (ny * nx, by * bx):
        raise ValueError(f"bf of shape {bf.shape} for a scan of {(ny, nx)} and {by * bx} window pixels")
    with quiet_floats():
        # (K, Ny, Nx): the scan image of every window pixel, transformed over its own two axes
        g = np.fft.fft2(np.ascontiguousarray(bf.T, dtype=np.float64).reshape(by * bx, ny, nx))
        s = np.zeros((ny, nx), np.complex128)
        for iy in range(ny):
            f = _filters(p, (ny, nx), iy).reshape(nx, by * bx)
            s[iy] = (g[:, iy, :].T * f).sum(axis=1) / (by * bx)
        mirrored = s[(-np.arange(ny)) % ny][:, (-np.arange(nx)) % nx]
        fourier = np.conj(mirrored) / np.abs(s[0, 0])
    return ssb._images(fourier, fourier.size)


def _plan(device, nav_shape, batch, p):
    from libertem_amd import hip
    geom = hip.ssb_geometry(p['lamb'], (p['dy'], p['dx']), p['semiconv'], p['semiconv_pix'], p['cy'], p['cx'], p['t'])
    window = np.asarray(p['window'], dtype=np.int32)
    key = (int(device), nav_shape[0], nav_shape[1], int(batch), p['epsilon'], geom.tobytes(), window.tobytes())
    return _PLANS.get_or_make(key, lambda: hip.WDDPlan(device, nav_shape[0], nav_shape[1], window, batch, geom,
                                                       p['epsilon']))


def release_plans(device=None):
    """Destroy the cached plans of `device` (None: of every device) and free their filters and workspace."""
    _PLANS.release(device)


def reconstruct_device(bf, nav_shape, p, stream=None):
    """`fourier` of a device-resident bf (HipArray (Ny Nx, By Bx) float32) through the native plan -> complex64
    (Ny, Nx) on the host"""
    ny, nx = nav_shape
    n_window = p['window'][2] * p['window'][3]
    if tuple(bf.shape) != (ny * nx, n_window) or bf.dtype != np.float32:
        raise ValueError(f"bf {bf.shape} {bf.dtype} for a scan of {(ny, nx)} and {n_window} window pixels")
    plan = _plan(bf.device, (ny, nx), ssb.plan_batch((ny, nx), n_window), p)
    return ssb.plan_fourier(plan, bf, (ny, nx), stream)


class WDDUDF(ssb.ScanPixelsUDF):
    """
    Parameters
    ----------
    lamb, dpix, semiconv, semiconv_pix, cy, cx, transformation
        as for `SSBUDF`
    window : int or (int, int)
        (By, Bx), the detector window around the disk centre that is deconvolved; it must hold the whole disk
    epsilon : float
        the Wiener filter's regularisation, relative to P^2 = |chi(0)|^2 at Q = 0; 0.01 is not tuned

    Results (single, extra shape = the scan shape): 'fourier', 'complex' (complex64), 'phase', 'amplitude' (float32).
    Buffer 'bf' (nav, on the device): the window pixels of every frame, float32 (By Bx).
    """

    def __init__(self, lamb, dpix, semiconv, semiconv_pix, window, epsilon=0.01, cy=None, cx=None,
                 transformation=None):
        super().__init__(lamb=lamb, dpix=dpix, semiconv=semiconv, semiconv_pix=semiconv_pix, window=window,
                         epsilon=epsilon, cy=cy, cx=cx, transformation=transformation)

    def _geometry(self):
        """-> sig, nav, the checked parameters, the window's list; ValueError for what the operation cannot take"""
        pr = self.params
        sig, nav = self._shapes()
        p = check_params(sig, pr.lamb, pr.dpix, pr.semiconv, pr.semiconv_pix, pr.window, pr.epsilon, pr.cy, pr.cx,
                         pr.transformation)
        self.check_scan_geometry(2)
        return sig, nav, p, _window_list(sig, p['window'])

    def _reconstruct_device(self, bf, sig, nav, p, idx):
        fourier = reconstruct_device(bf, nav, p)
        return ssb._images(fourier, fourier.size)

    def _reconstruct_host(self, bf, sig, nav, p, idx):
        pr = self.params
        return reconstruct_window(bf, nav, sig, pr.lamb, pr.dpix, pr.semiconv, pr.semiconv_pix, pr.window, pr.epsilon,
                                  pr.cy, pr.cx, pr.transformation)


def run_wdd(ctx, dataset, lamb, dpix, semiconv, semiconv_pix, window, epsilon=0.01, cy=None, cx=None,
            transformation=None, keep_bf=False):
    """The Wigner-distribution deconvolution of `dataset` on a HIP context, with the window pixels left on the device
    (`result_where='device'`): they never cross the host link.  -> dict of 'fourier', 'complex', 'phase', 'amplitude'
    as host arrays (Ny, Nx), and with keep_bf 'bf', the HipArray (Ny, Nx, By Bx)."""
    udf = WDDUDF(lamb=lamb, dpix=dpix, semiconv=semiconv, semiconv_pix=semiconv_pix, window=window, epsilon=epsilon,
                 cy=cy, cx=cx, transformation=transformation)
    return ssb._run_on_device(ctx, dataset, udf, ssb.RESULTS, keep_bf)
