"""
ParallaxUDF on MI355X: tilt-corrected bright-field imaging of a defocused-probe 4D-STEM scan, also called "parallax" or
tcBF-STEM (Lupini, Chi & Jesse, J. Microsc. 263 (2016) 43; the parallax reconstruction of py4DSTEM), the consumer of
`libertem_amd.utils.generate.defocused_scan`.

Under defocus every bright-field detector pixel K records a complete scan image I_K(r), shifted against the others by
s_K = A (k - c) for the pixel's position k on the detector.  The shifts are measured by cross-correlation with the
aligned mean, undone and the images summed; the 2 x 2 matrix A is fitted.  Its rotation part is the rotation between
the scan axes and the detector axes (what `SSBUDF` and `WDDUDF` take as `transformation`), its symmetric part defocus
and astigmatism (`parallax_aberrations`).

The operation, for a scan (Ny, Nx) of real frames (h, w), the radius `semiconv_pix` and the
centre (cy, cx) of the bright-field disk, an integer `max_shift` = m >= 1 with 2 m + 1 <= Ny, Nx, `iterations` >= 1,
the signed frequency s(i, n) of `SSBUDF` and Nxc = Nx // 2 + 1:

    K            = the P bright-field pixels `ssb.bf_pixels`, row-major
    G[K, iy, ix] = rfft2 over the scan axes of I[., K]                                   (P, Ny, Nxc)
    ey[K, iy]    = exp(2 pi i (s(iy, Ny) sh[K, 0] / Ny)),  ex[K, ix] = exp(2 pi i (s(ix, Nx) sh[K, 1] / Nx))
    S(sh)[iy, ix] = (1 / P) sum_K G[K, iy, ix] (ey[K, iy] ex[K, ix])
    sh_0 = 0
    for it in 1 .. iterations:
        R        = S(sh_{it-1});  R[0, 0] = 0
        C_K      = irfft2(G[K] conj(R), s=(Ny, Nx))         C_K[t] = sum_r I_K(r + t) ref(r), up to a constant factor
        (ty, tx) = the first maximum of C_K[ty mod Ny, tx mod Nx] over -m <= ty, tx <= m in row-major (ty, tx) order
        sub(c-, c0, c+) = clip((c- - c+) / (2 d), -0.5, 0.5) if d = c- - 2 c0 + c+ < 0 else 0
        sh_it[K] = (ty + sub along y, tx + sub along x)      the neighbours c-, c+ at indices mod Ny, Nx
        if regularize: sh_it = M (k - c) + b, the least-squares affine fit of sh_it, at every K
    matrix, offset = M, b of the fit of the last sh (always computed);  shifts = the last sh
    image = irfft2(S(shifts), s=(Ny, Nx));  bright_field = irfft2(S(0), s=(Ny, Nx))

irfft2 is NumPy's: of the columns ix = 0 and ix = Nx / 2 of a half spectrum, which pair with themselves, it takes the
Hermitian part (X[iy] + conj(X[-iy])) / 2 and nothing else -- at the Nyquist index a fractional shift acts as its
cosine.  I_K(r) = O(r - s_K) peaks at t = s_K, and the ramp exp(+2 pi i ...) undoes it.  A bright-field pixel whose
scan image is constant has an unspecified shift inside the window (its correlation map is zero everywhere, up to
rounding).  A region of interest is a ValueError (the transform needs the full rectangle), as are P = 0, a scan axis
shorter than 2 m + 1 and tiles that are not whole frames.

On the device the bright-field pixels of every frame are gathered once (`ltmi_ssb_gather`, the only pass over the
frames), their spectra are kept in a plan-owned store of 8 P Ny Nxc bytes, and every iteration is two streams over that
store (csrc/ltmi_parallax.hip): float32 transforms, float64 sums and parabolas.  The shifts stay on the device
between iterations unless `regularize` fits them on the host (P x 2 doubles each way).  The inverse transforms of the
two (Ny, Nx) images are NumPy's in float64.  On a CPU executor NumPy computes the definition in float64 / complex128
and casts at the end.
Not part of this module: upsampled output, higher-order aberration fits, band-pass filters on the correlation and a
multi-GPU split of the transform.  A store above `STORE_LIMIT_BYTES` is an error; recomputing the spectra per
iteration is not built.
"""
import numpy as np

from libertem_amd.common.hiparray import HipArray
from libertem_amd.udf.device import quiet_floats
from libertem_amd.udf.holography import signed_frequencies
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES, PlanCache
from libertem_amd.udf.ssb import ScanPixelsUDF, _run_on_device, device_stream, disk_pixels

# (device, Ny, Nx, P, batch, max_shift) -> hip.ParallaxPlan; a plan holds the spectra and the workspace in HBM
_PLANS = PlanCache(2, owned=True)

RESULTS = ('shifts', 'matrix', 'offset', 'image', 'bright_field')

#: the largest store of spectra (8 P Ny Nxc bytes) a plan may hold: 8 GiB, about 3 % of the MI355X's HBM -- the
#: 256 x 256 scan with 1789 bright-field pixels of scripts/bench_parallax.py takes 0.47 GB
STORE_LIMIT_BYTES = 8 << 30


def check_params(sig, semiconv_pix, cy=None, cx=None, max_shift=4, iterations=2):
    """-> dict(semiconv_pix, cy, cx, max_shift, iterations) with the defaults filled in; ValueError names the value
    that is off"""
    if len(sig) != 2:
        raise ValueError(f"ParallaxUDF needs 2D frames, not {tuple(sig)}")
    h, w = (int(s) for s in sig)
    semiconv_pix = float(semiconv_pix)
    if not (np.isfinite(semiconv_pix) and semiconv_pix > 0):
        raise ValueError(f"semiconv_pix {semiconv_pix!r} must be positive and finite")
    cy = h / 2 if cy is None else float(cy)
    cx = w / 2 if cx is None else float(cx)
    if not (np.isfinite(cy) and np.isfinite(cx)):
        raise ValueError(f"the disk centre {(cy, cx)} must be finite")
    if int(max_shift) != max_shift or int(max_shift) < 1:
        raise ValueError(f"max_shift {max_shift!r} must be an integer >= 1")
    if int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"iterations {iterations!r} must be an integer >= 1")
    return dict(semiconv_pix=semiconv_pix, cy=cy, cx=cx, max_shift=int(max_shift), iterations=int(iterations))


def check_scan(nav, max_shift):
    """a 2D scan whose axes both hold the 2 m + 1 shifts of the window, else ValueError"""
    if len(nav) != 2:
        raise ValueError(f"ParallaxUDF needs a 2D scan, not {tuple(nav)}")
    if min(nav) < 2 * max_shift + 1:
        raise ValueError(f"both axes of the {tuple(nav)} scan must be at least 2 * max_shift + 1 = {2 * max_shift + 1}")


def pixel_offsets(sig, idx, cy, cx):
    """k - c of the listed detector pixels -> float64 (P, 2), (y, x)"""
    w = int(sig[1])
    idx = np.asarray(idx)
    return np.stack([(idx // w).astype(np.float64) - cy, (idx % w).astype(np.float64) - cx], axis=1)


def fit_shifts(shifts, offsets):
    """The least-squares affine fit shifts[K] ~ M offsets[K] + b in float64 -> (M (2, 2), b (2,), fitted (P, 2)).
    With fewer than three pixels, or all of them on one line, the fit of least norm."""
    shifts = np.asarray(shifts, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.float64)
    if shifts.ndim != 2 or shifts.shape[1] != 2 or offsets.shape != shifts.shape:
        raise ValueError(f"shifts {shifts.shape} and offsets {offsets.shape} must both be (P, 2)")
    design = np.concatenate([offsets, np.ones((len(offsets), 1))], axis=1)
    coeff = np.linalg.lstsq(design, shifts, rcond=None)[0]              # (3, 2): column j fits component j
    return np.ascontiguousarray(coeff[:2].T), coeff[2].copy(), design @ coeff


def parallax_aberrations(matrix, dpix, semiconv, semiconv_pix):
    """
    What the fitted `matrix` (scan pixels of shift per detector pixel of tilt) says about the geometry and the probe.
    With the scan step `dpix` = (dy, dx) (or one number) in a unit of length and the angle of one detector pixel,
    semiconv / semiconv_pix rad, the matrix in that unit per rad is diag(dy, dx) matrix / (semiconv / semiconv_pix);
    its polar decomposition R S has a proper rotation R and a symmetric S = C1 1 + A1 [[cos 2a, sin 2a], [sin 2a,
    -cos 2a]].  S is taken with its larger eigenvalue positive: a defocus of the other sign shows as a rotation that is
    off by 180 degrees.

    -> dict of 'rotation_deg' (R = `corrections.coordinates.rotate_deg(rotation_deg)`, detector to scan),
    'transformation' (R transposed, scan to detector: what `SSBUDF` and `WDDUDF` take), 'defocus' (C1 = trace(S) / 2;
    for one number dpix that is trace of the pixel-unit S / 2 * dpix / (semiconv / semiconv_pix)), 'astigmatism'
    (A1 >= 0) and 'astigmatism_axis_deg' (a in (-90, 90]), lengths in the unit of dpix.
    """
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (2, 2) or not np.all(np.isfinite(m)):
        raise ValueError(f"matrix must be a finite 2 x 2 array, not {m!r}")
    try:
        dy, dx = (float(dpix), float(dpix)) if np.ndim(dpix) == 0 else (float(v) for v in dpix)
    except (TypeError, ValueError):
        raise ValueError(f"dpix {dpix!r} must be a number or (dy, dx)")
    for name, v in dict(dy=dy, dx=dx, semiconv=float(semiconv), semiconv_pix=float(semiconv_pix)).items():
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} {v!r} must be positive and finite")
    phys = np.diag([dy, dx]) @ m / (float(semiconv) / float(semiconv_pix))
    u, sv, vt = np.linalg.svd(phys)
    if np.linalg.det(u @ vt) < 0:
        # a proper rotation and an indefinite S instead of a reflection and a positive one
        u = u * np.array([1., -1.])
        sv = sv * np.array([1., -1.])
    rot = u @ vt
    sym = vt.T @ np.diag(sv) @ vt
    a, b = (sym[0, 0] - sym[1, 1]) / 2, (sym[0, 1] + sym[1, 0]) / 2
    # rotate_deg(t) = [[cos t, sin t], [-sin t, cos t]] on (y, x)
    return {'rotation_deg': float(np.degrees(np.arctan2(rot[0, 1], rot[0, 0]))),
            'transformation': np.ascontiguousarray(rot.T),
            'defocus': float((sym[0, 0] + sym[1, 1]) / 2),
            'astigmatism': float(np.hypot(a, b)),
            'astigmatism_axis_deg': float(np.degrees(np.arctan2(b, a)) / 2)}


def _sub(cm, c0, cp):
    """the vertex of the parabola through (-1, cm), (0, c0), (1, cp), clipped to half a pixel; 0 without a maximum"""
    d = cm - 2. * c0 + cp
    with np.errstate(all='ignore'):
        v = np.clip((cm - cp) / (2. * d), -0.5, 0.5)
    return np.where(d < 0, v, 0.)


def find_shifts(maps, max_shift):
    """maps (n, Ny, Nx) circular correlation maps -> float64 (n, 2): the first maximum within max_shift of the origin
    in row-major (ty, tx) order, plus the parabola vertex per axis from the neighbours at indices mod (Ny, Nx)"""
    maps = np.asarray(maps)
    n, ny, nx = maps.shape
    m = int(max_shift)
    t = np.arange(-m, m + 1)
    window = maps[:, (t % ny)[:, None], (t % nx)[None, :]].reshape(n, -1)
    best = np.argmax(window, axis=1)
    ty, tx = best // (2 * m + 1) - m, best % (2 * m + 1) - m
    k = np.arange(n)
    c0 = maps[k, ty % ny, tx % nx].astype(np.float64)
    sub_y = _sub(maps[k, (ty - 1) % ny, tx % nx].astype(np.float64), c0, maps[k, (ty + 1) % ny, tx % nx].astype(np.float64))
    sub_x = _sub(maps[k, ty % ny, (tx - 1) % nx].astype(np.float64), c0, maps[k, ty % ny, (tx + 1) % nx].astype(np.float64))
    return np.stack([ty + sub_y, tx + sub_x], axis=1)


def ramps(sh, nav_shape):
    """-> ey (P, Ny), ex (P, Nxc), complex128"""
    ny, nx = nav_shape
    sh = np.asarray(sh, dtype=np.float64)
    sy = signed_frequencies(ny).astype(np.float64)
    sx = signed_frequencies(nx).astype(np.float64)[:nx // 2 + 1]
    ay = 2 * np.pi * (sy[None, :] * sh[:, 0:1] / float(ny))
    ax = 2 * np.pi * (sx[None, :] * sh[:, 1:2] / float(nx))
    return np.cos(ay) + 1j * np.sin(ay), np.cos(ax) + 1j * np.sin(ax)


def _results(shifts, offsets, nav, half_image, half_bf, image_dtype=np.float32):
    """the five results in their result dtypes from the last shifts and the half spectra S(shifts), S(0)"""
    matrix, offset, _ = fit_shifts(shifts, offsets)
    with quiet_floats():
        image = np.fft.irfft2(np.asarray(half_image).astype(np.complex128), s=nav)
        bright = np.fft.irfft2(np.asarray(half_bf).astype(np.complex128), s=nav)
    return {'shifts': np.asarray(shifts, dtype=np.float64), 'matrix': matrix, 'offset': offset,
            'image': image.astype(image_dtype), 'bright_field': bright.astype(image_dtype)}


def parallax_bf(bf, nav_shape, sig, semiconv_pix, cy=None, cx=None, max_shift=4, iterations=2, regularize=False,
                image_dtype=np.float32):
    """The definition in NumPy from bf (Ny Nx, P), the bright-field pixels `ssb.bf_pixels(sig, ...)` of every frame:
    float64 / complex128 throughout, cast at the end.  -> dict of 'shifts' (P, 2), 'matrix' (2, 2), 'offset' (2,)
    (float64), 'image', 'bright_field' (`image_dtype` (Ny, Nx): float32 as the UDF's results, or float64 uncast)"""
    p = check_params(sig, semiconv_pix, cy, cx, max_shift, iterations)
    nav = tuple(int(v) for v in nav_shape)
    check_scan(nav, p['max_shift'])
    ny, nx = nav
    idx = disk_pixels(sig, p)
    bf = np.asarray(bf)
    if bf.shape != (ny * nx, idx.size):
        raise ValueError(f"bf of shape {bf.shape} for a scan of {(ny, nx)} and {idx.size} bright-field pixels")
    offsets = pixel_offsets(sig, idx, p['cy'], p['cx'])
    with quiet_floats():
        g = np.fft.rfft2(np.ascontiguousarray(bf.T, dtype=np.float64).reshape(idx.size, ny, nx))

        def mean(sh):
            ey, ex = ramps(sh, nav)
            return np.einsum('kyx,ky,kx->yx', g, ey, ex) / idx.size

        sh = np.zeros((idx.size, 2))
        for _ in range(p['iterations']):
            ref = mean(sh)
            ref[0, 0] = 0
            sh = find_shifts(np.fft.irfft2(g * np.conj(ref)[None], s=nav), p['max_shift'])
            if regularize:
                sh = fit_shifts(sh, offsets)[2]
        return _results(sh, offsets, nav, mean(sh), mean(np.zeros((idx.size, 2))), image_dtype)


def plan_batch(nav_shape, n_idx):
    """bright-field pixels per hipFFT execution: as many as the workspace budget (the one measured for correlation
    plans) allows -- per pixel the float32 scan image / correlation map and one complex64 half spectrum"""
    ny, nx = nav_shape
    per_pixel = 4 * ny * nx + 8 * ny * (nx // 2 + 1)
    return int(max(1, min(CORR_WORKSPACE_BYTES // per_pixel, n_idx)))


def _plan(device, nav_shape, n_idx, batch, max_shift):
    from libertem_amd import hip
    key = (int(device), nav_shape[0], nav_shape[1], int(n_idx), int(batch), int(max_shift))
    return _PLANS.get_or_make(key, lambda: hip.ParallaxPlan(device, nav_shape[0], nav_shape[1], n_idx, batch, max_shift,
                                                            STORE_LIMIT_BYTES))


def release_plans(device=None):
    """Destroy the cached plans of `device` (None: of every device) and free their spectra and workspace."""
    _PLANS.release(device)


def parallax_device(bf, nav_shape, offsets, max_shift, iterations=2, regularize=False, stream=None):
    """The results of a device-resident bf (HipArray (Ny Nx, P) float32) through the native plan; offsets: k - c of
    the P pixels (`pixel_offsets`).  -> the dict of `parallax_bf`"""
    ny, nx = nav_shape
    n_idx = len(offsets)
    if tuple(bf.shape) != (ny * nx, n_idx) or bf.dtype != np.float32:
        raise ValueError(f"bf {bf.shape} {bf.dtype} for a scan of {(ny, nx)} and {n_idx} bright-field pixels")
    check_scan((ny, nx), max_shift)
    device = bf.device
    plan = _plan(device, (ny, nx), n_idx, plan_batch((ny, nx), n_idx), max_shift)
    with device_stream(device, stream) as stream:
        plan.load(bf.data_ptr(), bf.ld, stream=stream)
        zeros = HipArray.zeros((n_idx, 2), np.float64, device)
        sh = HipArray.zeros((n_idx, 2), np.float64, device)
        for _ in range(int(iterations)):
            plan.iterate(sh.data_ptr(), stream=stream)
            if regularize:
                stream.synchronize()
                sh = HipArray.from_numpy(fit_shifts(sh.cpu(), offsets)[2], device)
        halves = HipArray.empty((2, ny, nx // 2 + 1), np.complex64, device)
        plan.sum(sh.data_ptr(), halves.data_ptr(), stream=stream)
        plan.sum(zeros.data_ptr(), halves.data_ptr() + 8 * ny * (nx // 2 + 1), stream=stream)
        stream.synchronize()
        half_image, half_bf = halves.cpu()
        return _results(sh.cpu(), offsets, (ny, nx), half_image, half_bf)


class ParallaxUDF(ScanPixelsUDF):
    """
    Parameters
    ----------
    semiconv_pix : float
        radius of the bright-field disk on the detector, in pixels
    cy, cx : float or None
        centre of the disk; None: (h / 2, w / 2)
    max_shift : int
        m: the shifts are searched in [-m, m] scan pixels per axis; both scan axes must be at least 2 m + 1
    iterations : int
        rounds of aligning the reference and measuring again; the first measures against the plain mean
    regularize : bool
        replace the shifts of every round by their affine fit

    Results (single): 'shifts' (P, 2), 'matrix' (2, 2), 'offset' (2,) (float64); 'image', 'bright_field' (float32,
    the scan shape).  Buffer 'bf' (nav, on the device): the bright-field pixels of every frame, float32 (P).
    """

    SINGLE_RESULTS = (('shifts', 'float64', ('P', 2)), ('matrix', 'float64', (2, 2)), ('offset', 'float64', (2,)),
                      ('image', 'float32', 'nav'), ('bright_field', 'float32', 'nav'))

    def __init__(self, semiconv_pix, cy=None, cx=None, max_shift=4, iterations=2, regularize=False):
        super().__init__(semiconv_pix=semiconv_pix, cy=cy, cx=cx, max_shift=max_shift, iterations=iterations,
                         regularize=bool(regularize))

    def _geometry(self):
        """-> sig, nav, the checked parameters, the bright-field list; ValueError for what the operation cannot take"""
        pr = self.params
        sig, nav = self._shapes()
        p = check_params(sig, pr.semiconv_pix, pr.cy, pr.cx, pr.max_shift, pr.iterations)
        check_scan(nav, p['max_shift'])
        self.check_scan_geometry(2)
        return sig, nav, p, disk_pixels(sig, p)

    def _reconstruct_device(self, bf, sig, nav, p, idx):
        return parallax_device(bf, nav, pixel_offsets(sig, idx, p['cy'], p['cx']), p['max_shift'], p['iterations'],
                               self.params.regularize)

    def _reconstruct_host(self, bf, sig, nav, p, idx):
        return parallax_bf(bf, nav, sig, p['semiconv_pix'], p['cy'], p['cx'], p['max_shift'], p['iterations'],
                           self.params.regularize)


def run_parallax(ctx, dataset, semiconv_pix, cy=None, cx=None, max_shift=4, iterations=2, regularize=False,
                 keep_bf=False):
    """The tilt-corrected bright-field reconstruction of `dataset` on a HIP context, with the bright-field pixels left
    on the device (`result_where='device'`): they never cross the host link.  -> dict of 'shifts', 'matrix', 'offset',
    'image', 'bright_field' as host arrays, and with keep_bf 'bf', the HipArray (Ny, Nx, P)."""
    udf = ParallaxUDF(semiconv_pix=semiconv_pix, cy=cy, cx=cx, max_shift=max_shift, iterations=iterations,
                      regularize=regularize)
    return _run_on_device(ctx, dataset, udf, RESULTS, keep_bf)
