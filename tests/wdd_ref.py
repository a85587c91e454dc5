"""
Wigner-distribution deconvolution ptychography restated index by index in float64 / complex128 (DESIGN.md section
4.6i): a double loop over the spatial frequencies Q of the scan, per Q one boolean window image and two transforms over
the window, in the rho-space form -- the package and the device use the F form, so the two share no derivation.

    window = [y0, y0 + By) x [x0, x0 + Bx),  y0 = floor(cy) - By // 2,  x0 = floor(cx) - Bx // 2,  K = (v, u)
    A      = (y - cy)^2 + (x - cx)^2 < semiconv_pix^2,  P = |A|,  A- = the same disk centred at (cy, cx) - d(Q)
    G[K, Q]  = np.fft.fft2 over the scan axes of I[R, K]
    Gamma[K] = A[K] and A-[K]
    chi[rho] = sum_K Gamma[K] exp(+2 pi i (v rho_y / By + u rho_x / Bx))           (By Bx np.fft.ifft2)
    W[rho]   = conj(chi[rho]) / (|chi[rho]|^2 + epsilon P^2)
    H[rho]   = sum_K G[K, Q] exp(+2 pi i (v rho_y / By + u rho_x / Bx))
    S[Q]     = sum_rho H[rho] W[rho] / (By Bx)
    fourier[Q] = conj(S[-Q mod (Ny, Nx)]) / |S[0, 0]|,  complex = Ny Nx ifft2(fourier)

`single=True` runs the same steps in float32 / complex64 (the predicates stay float64): its distance from the float64
run is what single precision costs on a fixture, and decides the tolerance (`atol_rule`).

The geometry, the shifts, the fixtures, `rim_margin` and `phase_agreement` are those of tests/ssb_ref.py; `reference`
and `filters` assert a rim margin of 1e-6 on whatever fixture they are given.
"""
import numpy as np

import ssb_ref as sr

#: the windows of the generic fixture (12 x 10 scan of 24 x 28, centre 11.6 / 14.2, radius 7.3): the disk spans rows
#: 5 .. 18 and columns 7 .. 21, the windows start at (3, 6), (3, 5) and (1, 6)
WINDOWS = ((16, 16), (16, 18), (20, 16))
GENERIC = {k: v for k, v in sr.GENERIC.items() if k != 'cutoff'}
GENERIC_EPSILON = 1e-2
PHYS_WINDOW = 24
PHYS_EPSILON = 1e-4


def physical_params():
    return {k: v for k, v in sr.physical_params().items() if k != 'cutoff'}


def window_origin(p, window):
    by, bx = (window, window) if np.isscalar(window) else window
    return int(np.floor(p['cy'])) - by // 2, int(np.floor(p['cx'])) - bx // 2, int(by), int(bx)


def gamma(sig, nav, iy, ix, p):
    """A and A- of Q = (iy, ix) as a boolean detector image"""
    d_y, d_x = sr.shift(p, nav, iy, ix)
    r2 = p['semiconv_pix'] * p['semiconv_pix']
    return sr.disk(sig, p) & (sr.distance2(sig, p['cy'] - d_y, p['cx'] - d_x) < r2)


def _backward(a, single):
    """sum_K a[K] exp(+2 pi i (v rho_y / By + u rho_x / Bx)) over the last two axes"""
    a = np.asarray(a, dtype=np.complex64 if single else np.complex128)
    out = np.fft.ifft2(a) * a.dtype.type(a.shape[-2] * a.shape[-1])
    assert out.dtype == a.dtype
    return out


def wiener(sig, nav, iy, ix, p, window, epsilon, single=False):
    """W[rho] of Q = (iy, ix), (By, Bx)"""
    y0, x0, by, bx = window_origin(p, window)
    n_disk = int(sr.disk(sig, p).sum())
    real = np.float32 if single else np.float64
    chi = _backward(gamma(sig, nav, iy, ix, p)[y0:y0 + by, x0:x0 + bx], single)
    return np.conj(chi) / (np.abs(chi) ** 2 + real(epsilon * n_disk * n_disk))


def filters(sig, nav, window, epsilon, single=False, **params):
    """F[Q, K] = sum_rho W[rho] exp(+2 pi i ...) for every Q -> (Ny, Nx, By Bx): what ltmi_wdd_filter builds"""
    p = sr.full_params(sig, **params)
    assert sr.rim_margin(sig, nav, p) >= 1e-6
    _, _, by, bx = window_origin(p, window)
    out = np.zeros(nav + (by * bx,), np.complex64 if single else np.complex128)
    for iy in range(nav[0]):
        for ix in range(nav[1]):
            out[iy, ix] = _backward(wiener(sig, nav, iy, ix, p, window, epsilon, single), single).reshape(-1)
    return out


def reference(frames, window, epsilon, single=False, **params):
    """frames (Ny, Nx, h, w) -> dict(fourier, complex, phase, amplitude, s, overlap), complex128 / float64 (complex64
    / float32 with `single`); s is S[Q] before the mirror and the normalisation, overlap the pixel count of Gamma"""
    frames = np.asarray(frames)
    ny, nx, h, w = frames.shape
    p = sr.full_params((h, w), **params)
    y0, x0, by, bx = window_origin(p, window)
    a = sr.disk((h, w), p)
    assert a.sum() > 0 and y0 >= 0 and x0 >= 0 and y0 + by <= h and x0 + bx <= w
    assert a[y0:y0 + by, x0:x0 + bx].sum() == a.sum()
    # no pixel within 1e-6 (in distance squared) of a rim of any Q: Gamma does not hang on the predicates' last bits
    assert sr.rim_margin((h, w), (ny, nx), p) >= 1e-6
    cplx_t = np.complex64 if single else np.complex128
    g = np.fft.fft2(frames[:, :, y0:y0 + by, x0:x0 + bx].astype(np.float32 if single else np.float64), axes=(0, 1))
    assert g.dtype == cplx_t
    s = np.zeros((ny, nx), cplx_t)
    overlap = np.zeros((ny, nx), np.int64)
    for iy in range(ny):
        for ix in range(nx):
            overlap[iy, ix] = gamma((h, w), (ny, nx), iy, ix, p).sum()
            wien = wiener((h, w), (ny, nx), iy, ix, p, window, epsilon, single)
            hh = _backward(g[iy, ix], single)
            s[iy, ix] = (hh * wien).sum() / (by * bx)
    fourier = np.zeros((ny, nx), cplx_t)
    with np.errstate(all='ignore'):
        for iy in range(ny):
            for ix in range(nx):
                fourier[iy, ix] = np.conj(s[(-iy) % ny, (-ix) % nx]) / np.abs(s[0, 0])
    cplx = np.fft.ifft2(fourier) * (ny * nx)
    return dict(fourier=fourier, complex=cplx, phase=np.angle(cplx), amplitude=np.abs(cplx), s=s, overlap=overlap)


def dot(spec_half, filt, nav):
    """sum_K G[K, Q] F[Q, K] on half spectra (Ny, Nx // 2 + 1, K) completed by G[iy, ix] = conj(G[-iy mod Ny,
    Nx - ix]), filt (Ny, Nx, K) -- what ltmi_wdd_dot computes.  -> complex128 (Ny, Nx)"""
    ny, nx = nav
    spec_half = np.asarray(spec_half).astype(np.complex128)
    filt = np.asarray(filt).astype(np.complex128)
    out = np.zeros((ny, nx), np.complex128)
    for iy in range(ny):
        for ix in range(nx):
            g = spec_half[iy, ix] if ix <= nx // 2 else np.conj(spec_half[(-iy) % ny, nx - ix])
            out[iy, ix] = (g * filt[iy, ix]).sum()
    return out


def finish(s_sum, n_window):
    """fourier of the raw sums: conj(S[-Q]) / |S[0, 0]|, S = s_sum / n_window"""
    ny, nx = s_sum.shape
    s = s_sum / n_window
    mirrored = s[(-np.arange(ny)) % ny][:, (-np.arange(nx)) % nx]
    return np.conj(mirrored) / np.abs(s[0, 0])


# ---- tolerances -------------------------------------------------------------------------------------------------
def rest_scale(ref):
    """max |ref| over Q != 0"""
    rest = np.ones(ref.shape, bool)
    rest[0, 0] = False
    return float(np.abs(ref[rest]).max()) if rest.any() else 0.


def atol_rule(ref, ref_single):
    """SSB's atol, 1e-5 max|ref over Q != 0| -- unless the float32 restatement itself reaches a quarter of it on this
    fixture: then 8 x the float32 restatement's error against the float64 one"""
    base = 1e-5 * rest_scale(ref)
    single_err = float(np.abs(np.asarray(ref_single).astype(np.complex128) - ref).max())
    return (base if single_err < base / 4 else 8 * single_err), base, single_err


def assert_filter(got, ref, ref_single, what=''):
    """F of a set of Qs against `filters`: rtol 1e-5 and atol 1e-5 max|ref|, or, where the float32 restatement
    reaches a quarter of that, 8 x its error -- the rule of `atol_rule` with the scale taken over all of F"""
    got, ref = np.asarray(got).astype(np.complex128), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    base = 1e-5 * float(np.abs(ref).max())
    single_err = float(np.abs(np.asarray(ref_single).astype(np.complex128) - ref).max())
    atol = base if single_err < base / 4 else 8 * single_err
    err = np.abs(got - ref)
    print(f"{what}: max error {err.max():.3e} (atol {atol:.3e}, SSB's rule {base:.3e}, float32 restatement "
          f"{single_err:.3e})")
    assert np.all(err <= atol + 1e-5 * np.abs(ref)), (what, float(err.max()), atol)


def assert_fourier(got, ref, what='', atol=None):
    """SSB's rule: Q != 0 to rtol 1e-5 and atol (default 1e-5 max|ref over Q != 0|), DC to rtol 1e-6 (the DC of
    `fourier` is conj(S[0]) / |S[0]|, of modulus 1: its error is a phase error)"""
    got, ref = np.asarray(got).astype(np.complex128), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rest = np.ones(ref.shape, bool)
    rest[0, 0] = False
    atol = 1e-5 * rest_scale(ref) if atol is None else atol
    err = np.abs(got - ref)
    print(f"{what}: Q != 0 max error {err[rest].max() if rest.any() else 0.:.3e} (atol {atol:.3e}), "
          f"DC relative error {err[0, 0] / abs(ref[0, 0]):.3e}")
    assert np.all(err[rest] <= atol + 1e-5 * np.abs(ref[rest])), (what, float(err[rest].max()), atol)
    assert err[0, 0] <= 1e-6 * abs(ref[0, 0]), (what, float(err[0, 0]), abs(ref[0, 0]))


def assert_images(got, ref, what='', atol=None):
    """`complex`, `phase` and `amplitude` against the restatement.  complex = Ny Nx ifft2(fourier) = sum_Q fourier[Q]
    exp(...): a fourier within `assert_fourier` moves it by at most sum_Q |error[Q]| <= tol = N (atol + 1e-5
    max|fourier ref|) per pixel (triangle inequality), the amplitude by as much, and the phase by at most
    asin(tol / |complex|) < 2 tol / min|complex ref| wherever that is small."""
    atol = 1e-5 * rest_scale(ref['fourier']) if atol is None else atol
    tol = ref['fourier'].size * (atol + 1e-5 * np.abs(ref['fourier']).max())
    c = np.asarray(got['complex']).astype(np.complex128)
    assert np.abs(c - ref['complex']).max() <= tol, (what, float(np.abs(c - ref['complex']).max()), tol)
    assert np.abs(np.asarray(got['amplitude'], dtype=np.float64) - ref['amplitude']).max() <= \
        tol + 1e-6 * ref['amplitude'].max(), what
    small = 2 * tol / np.abs(ref['complex']).min()
    assert small < 0.1, (what, small)
    dphi = np.angle(np.exp(1j * (np.asarray(got['phase'], dtype=np.float64) - ref['phase'])))
    assert np.abs(dphi).max() <= small + 1e-6, (what, float(np.abs(dphi).max()), small)
