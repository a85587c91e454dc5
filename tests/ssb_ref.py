"""
Single-sideband ptychography restated index by index in float64 / complex128: a double loop
over the spatial frequencies Q of the scan, one pair of boolean detector masks per Q, no code shared with the package.

    G[K, iy, ix] = sum_R I[R, K] exp(-2 pi i (s(iy) ry / Ny + s(ix) rx / Nx))        (np.fft.fft2 over the scan axes)
    A   = (y - cy)^2 + (x - cx)^2 < semiconv_pix^2
    d   = T q lamb semiconv_pix / semiconv,  q = (s(iy) / (Ny dy), s(ix) / (Nx dx))
    A+- = the same disk centred at (cy, cx) +- d
    pos = A and A+ and not A-,  neg = A and A- and not A+
    fourier[Q] = (sum_pos G / |pos| - sum_neg G / |neg|) / 2 if both counts reach the cutoff, else 0
    fourier[0] = sum_A G[K, 0] / P

Also here: the fixtures of the ssb tests (the generic Poisson scan, the simulated weak phase object), the smallest
distance of any pixel from any rim, and the tolerances the issue sets.
"""
import numpy as np

#: the generic fixture: a 12 x 10 scan of 24 x 28 frames, a rotated, anisotropic geometry
GENERIC = dict(lamb=2.0e-12, dpix=(0.31e-10, 0.27e-10), semiconv=0.022, semiconv_pix=7.3, cy=11.6, cx=14.2, cutoff=4,
               transformation=np.array([[np.cos(np.deg2rad(25.)), -np.sin(np.deg2rad(25.))],
                                        [np.sin(np.deg2rad(25.)), np.cos(np.deg2rad(25.))]]))
GENERIC_NAV = (12, 10)
GENERIC_SIG = (24, 28)


def signed(i, n):
    """the signed frequency of index i of an axis of n (fftfreq order; for even n, index n / 2 is -n / 2)"""
    return i if i <= (n - 1) // 2 else i - n


def full_params(sig, lamb, dpix, semiconv, semiconv_pix, cy=None, cx=None, transformation=None, cutoff=1):
    """the defaults filled in: dpix as (dy, dx), the centre (h / 2, w / 2), the identity"""
    dy, dx = (dpix, dpix) if np.isscalar(dpix) else dpix
    cy = sig[0] / 2 if cy is None else cy
    cx = sig[1] / 2 if cx is None else cx
    t = np.eye(2) if transformation is None else np.asarray(transformation, dtype=np.float64)
    return dict(lamb=float(lamb), dy=float(dy), dx=float(dx), semiconv=float(semiconv),
                semiconv_pix=float(semiconv_pix), cy=float(cy), cx=float(cx), t=t, cutoff=int(cutoff))


def shift(p, nav, iy, ix):
    """d of Q = (iy, ix), in detector pixels"""
    ny, nx = nav
    qy = float(signed(iy, ny)) / (float(ny) * p['dy'])
    qx = float(signed(ix, nx)) / (float(nx) * p['dx'])
    ty = p['t'][0, 0] * qy + p['t'][0, 1] * qx
    tx = p['t'][1, 0] * qy + p['t'][1, 1] * qx
    return (ty * p['lamb'] * p['semiconv_pix'] / p['semiconv'], tx * p['lamb'] * p['semiconv_pix'] / p['semiconv'])


def distance2(sig, cy, cx):
    """(y - cy)^2 + (x - cx)^2 of every detector pixel"""
    y = np.arange(sig[0], dtype=np.float64)[:, None]
    x = np.arange(sig[1], dtype=np.float64)[None, :]
    return (y - cy) * (y - cy) + (x - cx) * (x - cx)


def disk(sig, p):
    return distance2(sig, p['cy'], p['cx']) < p['semiconv_pix'] * p['semiconv_pix']


def masks(sig, nav, iy, ix, p):
    """(pos, neg) of Q = (iy, ix) as boolean detector images"""
    d_y, d_x = shift(p, nav, iy, ix)
    r2 = p['semiconv_pix'] * p['semiconv_pix']
    a = disk(sig, p)
    a_p = distance2(sig, p['cy'] + d_y, p['cx'] + d_x) < r2
    a_m = distance2(sig, p['cy'] - d_y, p['cx'] - d_x) < r2
    return a & a_p & ~a_m, a & a_m & ~a_p


def rim_margin(sig, nav, p):
    """the smallest |distance^2 - semiconv_pix^2| over every pixel, the disk and both shifted disks of every Q"""
    r2 = p['semiconv_pix'] * p['semiconv_pix']
    margin = np.abs(distance2(sig, p['cy'], p['cx']) - r2).min()
    for iy in range(nav[0]):
        for ix in range(nav[1]):
            d_y, d_x = shift(p, nav, iy, ix)
            for sgn in (1., -1.):
                margin = min(margin, np.abs(distance2(sig, p['cy'] + sgn * d_y, p['cx'] + sgn * d_x) - r2).min())
    return float(margin)


def reference(frames, **params):
    """frames (Ny, Nx, h, w) -> dict(fourier, complex, phase, amplitude, n_pos, n_neg), complex128 / float64; n_pos and
    n_neg are the pixel counts of the two trotters of every Q"""
    frames = np.asarray(frames)
    ny, nx, h, w = frames.shape
    p = full_params((h, w), **params)
    g = np.fft.fft2(frames.astype(np.float64), axes=(0, 1))
    fourier = np.zeros((ny, nx), np.complex128)
    n_pos = np.zeros((ny, nx), np.int64)
    n_neg = np.zeros((ny, nx), np.int64)
    a = disk((h, w), p)
    assert a.sum() > 0
    for iy in range(ny):
        for ix in range(nx):
            if iy == 0 and ix == 0:
                fourier[0, 0] = g[0, 0][a].sum() / a.sum()
                continue
            pos, neg = masks((h, w), (ny, nx), iy, ix, p)
            n_pos[iy, ix], n_neg[iy, ix] = pos.sum(), neg.sum()
            if pos.sum() >= p['cutoff'] and neg.sum() >= p['cutoff']:
                fourier[iy, ix] = (g[iy, ix][pos].sum() / pos.sum() - g[iy, ix][neg].sum() / neg.sum()) / 2
    cplx = np.fft.ifft2(fourier)
    return dict(fourier=fourier, complex=cplx, phase=np.angle(cplx), amplitude=np.abs(cplx), n_pos=n_pos, n_neg=n_neg)


def masked_sums(spec_half, sig, nav, bf_index, **params):
    """the cutoff rule on half spectra (Ny, Nx // 2 + 1, P) of the listed pixels, completed by
    G[iy, ix] = conj(G[-iy mod Ny, Nx - ix]) -- what ltmi_ssb_trotter computes.  -> fourier complex128 (Ny, Nx)"""
    ny, nx = nav
    p = full_params(sig, **params)
    spec_half = np.asarray(spec_half).astype(np.complex128)
    fourier = np.zeros((ny, nx), np.complex128)
    for iy in range(ny):
        for ix in range(nx):
            g = spec_half[iy, ix] if ix <= nx // 2 else np.conj(spec_half[(-iy) % ny, nx - ix])
            if iy == 0 and ix == 0:
                fourier[0, 0] = g.sum() / len(bf_index)
                continue
            pos, neg = masks(sig, nav, iy, ix, p)
            pos, neg = pos.reshape(-1)[bf_index], neg.reshape(-1)[bf_index]
            if pos.sum() >= p['cutoff'] and neg.sum() >= p['cutoff']:
                fourier[iy, ix] = (g[pos].sum() / pos.sum() - g[neg].sum() / neg.sum()) / 2
    return fourier


def assert_fourier(got, ref, what=''):
    """the issue's tolerance: Q != 0 to rtol 1e-5 and atol 1e-5 max|ref over Q != 0|, DC to rtol 1e-6"""
    got, ref = np.asarray(got).astype(np.complex128), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rest = np.ones(ref.shape, bool)
    rest[0, 0] = False
    scale = np.abs(ref[rest]).max() if rest.any() else 0.
    err = np.abs(got - ref)
    print(f"{what}: Q != 0 max error {err[rest].max() if rest.any() else 0.:.3e} (atol {1e-5 * scale:.3e}), "
          f"DC relative error {err[0, 0] / abs(ref[0, 0]):.3e}")
    assert np.all(err[rest] <= 1e-5 * scale + 1e-5 * np.abs(ref[rest])), \
        (what, float(err[rest].max()), 1e-5 * scale)
    assert err[0, 0] <= 1e-6 * abs(ref[0, 0]), (what, float(err[0, 0]), abs(ref[0, 0]))


def assert_images(got, ref, what=''):
    """`complex`, `phase` and `amplitude` against the restatement.  A fourier within `assert_fourier` moves
    complex = ifft2(fourier) by at most mean_Q |error[Q]| <= tol = 2e-5 max|fourier ref| per pixel (triangle
    inequality; both terms of the tolerance are below 1e-5 max|ref|), the amplitude by as much, and the phase by at
    most asin(tol / |complex|) < 2 tol / min|complex ref| wherever that is small."""
    tol = 2e-5 * np.abs(ref['fourier']).max()
    c = np.asarray(got['complex']).astype(np.complex128)
    assert np.abs(c - ref['complex']).max() <= tol, (what, float(np.abs(c - ref['complex']).max()), tol)
    assert np.abs(np.asarray(got['amplitude'], dtype=np.float64) - ref['amplitude']).max() <= \
        tol + 1e-6 * ref['amplitude'].max(), what
    small = 2 * tol / np.abs(ref['complex']).min()
    assert small < 0.1, (what, small)
    dphi = np.angle(np.exp(1j * (np.asarray(got['phase'], dtype=np.float64) - ref['phase'])))
    assert np.abs(dphi).max() <= small + 1e-6, (what, float(np.abs(dphi).max()), small)


def generic_frames(dtype='uint16'):
    """the seeded generic fixture: Poisson(40) frames (12, 10, 24, 28)"""
    rng = np.random.default_rng(20211)
    return rng.poisson(40., GENERIC_NAV + GENERIC_SIG).astype(dtype)


# ---- the physical fixture: a weak phase object on a periodic 32 x 32 grid ------------------------------------------
PHYS_GRID = 32
PHYS_STEP = 2
PHYS_SEMICONV_PIX = 6.5
PHYS_PIXEL = 0.4e-10            # object pixel size in metres
PHYS_LAMB = 1.9687e-12          # 300 kV


def physical_phase(amplitude=0.1):
    """a band-limited, mean-free phase on the 32 x 32 grid: frequencies up to 3 cycles, peak |phi| = amplitude"""
    rng = np.random.default_rng(77)
    m = PHYS_GRID
    spec = np.zeros((m, m), np.complex128)
    for ky in range(-3, 4):
        for kx in range(-3, 4):
            if (ky, kx) != (0, 0):
                spec[ky % m, kx % m] = rng.normal() + 1j * rng.normal()
    phi = np.fft.ifft2(spec).real
    return phi / np.abs(phi).max() * amplitude


def physical_params():
    """the geometry that goes with `weak_phase_scan(phi, PHYS_STEP, PHYS_SEMICONV_PIX)`: a detector pixel is
    lamb / (grid pixel) radians, so semiconv = semiconv_pix lamb / (32 pixel); the scan step is step pixel"""
    return dict(lamb=PHYS_LAMB, dpix=PHYS_STEP * PHYS_PIXEL,
                semiconv=PHYS_SEMICONV_PIX * PHYS_LAMB / (PHYS_GRID * PHYS_PIXEL), semiconv_pix=PHYS_SEMICONV_PIX,
                cy=PHYS_GRID / 2, cx=PHYS_GRID / 2, cutoff=1)


def phase_agreement(phase, phi):
    """(correlation, scale) of the mean-free reconstructed phase with the truth sampled at the scan positions"""
    truth = phi[::PHYS_STEP, ::PHYS_STEP]
    a = phase - phase.mean()
    b = truth - truth.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())), float((a * b).sum() / (b * b).sum())
