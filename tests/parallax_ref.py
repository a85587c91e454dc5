"""
The fixtures of the parallax tests and an index-by-index float64 restatement of `libertem_amd.udf.parallax` that shares
no code with it: the spectra are direct DFT sums (matrix products with the DFT matrices written out here), the
reference image is the real part of the weighted half-spectrum sum, and the correlation is the explicit real-space
circular sum C_K[t] = sum_r I_K(r + t) ref(r), looped over K, ty and tx.

Fixtures: an object that is a Gaussian-low-passed seeded normal field (sigma 0.18 cycles per pixel) rescaled to
1 +- 0.4; matrix = 0.55 rot(25 deg) [[1, .1], [.1, .9]]; frames of 12 x 14, semiconv_pix 4.3, centre (5.6, 7.2), P = 58;
scans of 12 x 10 (even / even, max_shift up to 4) and 9 x 16 (odd / even).  `frames` are the noise-free float64 frames
at 1000 counts, `counted` the same at 150 counts rounded to integers, which every tested dataset dtype holds exactly.
"""
import functools
import math

import numpy as np

SIG = (12, 14)
SEMICONV_PIX = 4.3
CY, CX = 5.6, 7.2
N_BF = 58
NAVS = ((12, 10), (9, 16))
MAX_SHIFT = 4
ANGLE_DEG = 25.
SEEDS = {(12, 10): 7, (9, 16): 15}
PARAMS = dict(semiconv_pix=SEMICONV_PIX, cy=CY, cx=CX, max_shift=MAX_SHIFT, iterations=2)


def rot(deg):
    """[[c, s], [-s, c]] on (y, x), the convention of corrections.coordinates.rotate_deg"""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, s], [-s, c]])


MATRIX = 0.55 * rot(ANGLE_DEG) @ np.array([[1., .1], [.1, .9]])


def make_obj(nav, seed=None):
    ny, nx = nav
    rng = np.random.default_rng(SEEDS[tuple(nav)] if seed is None else seed)
    field = rng.standard_normal((ny, nx))
    fy, fx = np.fft.fftfreq(ny)[:, None], np.fft.fftfreq(nx)[None, :]
    low = np.fft.ifft2(np.fft.fft2(field) * np.exp(-(fy * fy + fx * fx) / (2 * 0.18 ** 2))).real
    low -= low.mean()
    return 1 + 0.4 * low / np.abs(low).max()


@functools.lru_cache(maxsize=None)
def _frames(nav, counts):
    from libertem_amd.utils.generate import defocused_scan
    out = defocused_scan(make_obj(nav), MATRIX, SIG, SEMICONV_PIX, CY, CX, counts=counts)
    out.setflags(write=False)
    return out


def frames(nav):
    """noise-free float64 frames (Ny, Nx, 12, 14) at 1000 counts (read-only, shared)"""
    return _frames(tuple(nav), 1000.)


@functools.lru_cache(maxsize=None)
def counted(nav):
    """the frames at 150 counts rounded to integers, uint16 (read-only, shared): at most 210, so uint8 holds them"""
    out = np.rint(_frames(tuple(nav), 150.)).astype(np.uint16)
    assert out.max() <= 255
    out.setflags(write=False)
    return out


def pixels(sig=SIG, semiconv_pix=SEMICONV_PIX, cy=CY, cx=CX):
    """the bright-field pixels (y, x), row-major"""
    return [(y, x) for y in range(sig[0]) for x in range(sig[1])
            if (y - cy) * (y - cy) + (x - cx) * (x - cx) < semiconv_pix * semiconv_pix]


def true_shifts():
    return np.array([MATRIX @ np.array([y - CY, x - CX]) for y, x in pixels()])


def signed(i, n):
    return i if i <= (n - 1) // 2 else i - n


def affine_fit(sh, offsets):
    """least squares sh[K] ~ M offsets[K] + b by the normal equations -> M, b, fitted"""
    a = np.array([[oy, ox, 1.] for oy, ox in offsets])
    coeff = np.linalg.solve(a.T @ a, a.T @ sh)
    return coeff[:2].T.copy(), coeff[2].copy(), a @ coeff


def parabola(cm, c0, cp):
    d = cm - 2. * c0 + cp
    if not d < 0:
        return 0.
    return min(max((cm - cp) / (2. * d), -0.5), 0.5)


def reference(data, semiconv_pix=SEMICONV_PIX, cy=CY, cx=CX, max_shift=MAX_SHIFT, iterations=2, regularize=False):
    """data (Ny, Nx, h, w) -> dict of 'shifts', 'matrix', 'offset', 'image', 'bright_field' in float64, and per
    iteration 'margins': for every K (v0 - v2) / v0 with v0 the maximum and v2 the largest candidate of the window that
    is no neighbour of it (Chebyshev distance > 1), and 'adjacent': the same with the largest neighbour"""
    data = np.asarray(data, dtype=np.float64)
    ny, nx = data.shape[:2]
    nxc = nx // 2 + 1
    m = max_shift
    pix = pixels(data.shape[2:], semiconv_pix, cy, cx)
    offsets = [(y - cy, x - cx) for y, x in pix]
    images = [data[:, :, y, x] for y, x in pix]
    n = len(pix)
    dft_y = np.array([[np.exp(-2j * np.pi * iy * ry / ny) for ry in range(ny)] for iy in range(ny)])
    dft_x = np.array([[np.exp(-2j * np.pi * ix * rx / nx) for rx in range(nx)] for ix in range(nxc)])
    spectra = [dft_y @ im @ dft_x.T for im in images]
    weight = [1. if ix == 0 or 2 * ix == nx else 2. for ix in range(nxc)]

    def mean(sh):
        acc = np.zeros((ny, nxc), complex)
        for k in range(n):
            ey = np.array([np.exp(2j * np.pi * signed(iy, ny) * sh[k][0] / ny) for iy in range(ny)])
            ex = np.array([np.exp(2j * np.pi * signed(ix, nx) * sh[k][1] / nx) for ix in range(nxc)])
            acc += spectra[k] * ey[:, None] * ex[None, :]
        return acc / n

    def real_image(half):
        out = np.zeros((ny, nx))
        for iy in range(ny):
            for ix in range(nxc):
                wave = np.outer(np.exp(2j * np.pi * iy * np.arange(ny) / ny), np.exp(2j * np.pi * ix * np.arange(nx) / nx))
                out += weight[ix] * (half[iy, ix] * wave).real
        return out / (ny * nx)

    sh = np.zeros((n, 2))
    margins, adjacent = [], []
    for _ in range(iterations):
        r = mean(sh)
        r[0, 0] = 0
        ref = real_image(r)
        new = np.zeros((n, 2))
        marg, adj = np.zeros(n), np.zeros(n)
        for k in range(n):
            corr = np.zeros((ny, nx))
            for ty in range(ny):
                for tx in range(nx):
                    corr[ty, tx] = (np.roll(images[k], (-ty, -tx), axis=(0, 1)) * ref).sum()
            best = None
            for ty in range(-m, m + 1):
                for tx in range(-m, m + 1):
                    if best is None or corr[ty % ny, tx % nx] > corr[best[0] % ny, best[1] % nx]:
                        best = (ty, tx)
            ty, tx = best
            c0 = corr[ty % ny, tx % nx]
            far = [corr[uy % ny, ux % nx] for uy in range(-m, m + 1) for ux in range(-m, m + 1)
                   if max(abs(uy - ty), abs(ux - tx)) > 1]
            near = [corr[uy % ny, ux % nx] for uy in range(-m, m + 1) for ux in range(-m, m + 1)
                    if max(abs(uy - ty), abs(ux - tx)) == 1]
            marg[k], adj[k] = (c0 - max(far)) / c0, (c0 - max(near)) / c0
            new[k] = (ty + parabola(corr[(ty - 1) % ny, tx % nx], c0, corr[(ty + 1) % ny, tx % nx]),
                      tx + parabola(corr[ty % ny, (tx - 1) % nx], c0, corr[ty % ny, (tx + 1) % nx]))
        margins.append(marg)
        adjacent.append(adj)
        sh = affine_fit(new, offsets)[2] if regularize else new
    matrix, offset, _ = affine_fit(sh, offsets)
    return {'shifts': sh, 'matrix': matrix, 'offset': offset, 'image': real_image(mean(sh)),
            'bright_field': real_image(mean(np.zeros((n, 2)))), 'margins': np.array(margins),
            'adjacent': np.array(adjacent)}


@functools.lru_cache(maxsize=None)
def reference_of(kind, nav, regularize=False, max_shift=MAX_SHIFT):
    """the restatement of a fixture, computed once and shared: kind 'frames' or 'counted'"""
    data = frames(nav) if kind == 'frames' else counted(nav)
    out = reference(data, max_shift=max_shift, regularize=regularize)
    for v in out.values():
        v.setflags(write=False)
    return out


def rotation_deg(matrix):
    """the angle of the rotation part of the polar decomposition, in the convention of `rot`"""
    u, _, vt = np.linalg.svd(matrix)
    r = u @ vt
    return math.degrees(math.atan2(r[0, 1], r[0, 0]))


def errors(res, ref):
    """-> dict of the largest deviations of a result from the restatement: shifts in scan pixels, the matrix in
    absolute terms, the two images relative to the largest reference value"""
    out = {'shifts': float(np.abs(np.asarray(res['shifts'], dtype=np.float64) - ref['shifts']).max()),
           'matrix': float(np.abs(np.asarray(res['matrix'], dtype=np.float64) - ref['matrix']).max()),
           'offset': float(np.abs(np.asarray(res['offset'], dtype=np.float64) - ref['offset']).max())}
    for name in ('image', 'bright_field'):
        out[name] = float(np.abs(np.asarray(res[name], dtype=np.float64) - ref[name]).max() / np.abs(ref[name]).max())
    return out


def same_integer_parts(res, ref):
    """the window candidate of every shift is the restatement's"""
    return np.array_equal(np.rint(np.asarray(res['shifts'])), np.rint(ref['shifts']))
