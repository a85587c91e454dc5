"""Synthetic test frames, under the reference's names (`libertem.utils.generate`).

`hologram_frame` simulates an off-axis electron hologram from an amplitude and a phase image (Lichte & Lehmann,
Rep. Prog. Phys. 71 (2008) 016102): the frames `libertem_amd.udf.holography` reconstructs.
"""
import numpy as np


def hologram_frame(amp, phi, counts=1000., sampling=5., visibility=1., f_angle=30., gaussian_noise=None,
                   poisson_noise=None):
    """
    An off-axis hologram of the object wave amp * exp(i phi) interfering with a plane reference wave:

        holo[y, x] = counts / 2 * (1 + amp^2 + 2 amp visibility cos(2 pi (y cos(a) + x sin(a)) / sampling - phi))

    with a = f_angle in radians.  The carrier has (cos(a), sin(a)) / sampling cycles per pixel in (y, x); its sideband
    at MINUS that frequency carries counts / 2 * amp * visibility * exp(+i phi).

    Parameters
    ----------
    amp, phi : 2D arrays of the same shape
        normalised amplitude and phase of the object wave
    counts : float
        electron counts in vacuum
    sampling : float
        pixels per fringe
    visibility : float
        fringe contrast
    f_angle : float
        angle of the fringes' normal to the y axis, in degrees
    gaussian_noise : float, int or None
        sigma of a Gaussian blur of the hologram (focus spread, detector point spread); needs scipy
    poisson_noise : float, int or None
        shot noise: the hologram becomes s * Poisson(holo / s) with s = poisson_noise * counts, drawn from NumPy's
        global generator (`np.random.seed`); applied before the blur
    """
    amp, phi = np.asarray(amp), np.asarray(phi)
    if amp.shape != phi.shape or phi.ndim != 2:
        raise ValueError(f"amp {amp.shape} and phi {phi.shape} must be 2D arrays of one shape")
    for name, value in (('poisson_noise', poisson_noise), ('gaussian_noise', gaussian_noise)):
        if value and not isinstance(value, (float, int)):
            raise ValueError(f"{name} must be a float, an int or None, not {value!r}")
    h, w = phi.shape
    angle = np.deg2rad(f_angle)
    y = np.arange(h, dtype=np.float64)[:, None]
    x = np.arange(w, dtype=np.float64)[None, :]
    carrier = 2 * np.pi * (y * np.cos(angle) + x * np.sin(angle)) / sampling
    holo = counts / 2 * (1 + amp ** 2 + 2 * visibility * amp * np.cos(carrier - phi))
    if poisson_noise:
        scale = poisson_noise * counts
        holo = scale * np.random.poisson(holo / scale)
    if gaussian_noise:
        from scipy.ndimage import gaussian_filter
        holo = gaussian_filter(holo, gaussian_noise)
    return holo
