"""
HoloReconstructUDF on MI355X: off-axis electron hologram reconstruction by the Fourier method (Lichte & Lehmann,
Rep. Prog. Phys. 71 (2008) 016102), the consumer of `libertem_amd.utils.generate.hologram_frame`.

The operation, for a frame `x` of (h, w) as float32 `y`, an integer `sb_position` (sy, sx)
in the unshifted `fft2` layout, `out_shape` (oh, ow) with oh <= h and ow <= w, a real float32 `aperture` of `out_shape`
in the unshifted layout -- index (0, 0) is the sideband centre -- and an optional complex `reference_wave`, with the
signed frequency s(i, n) = i if i <= (n - 1) // 2 else i - n (NumPy's fftfreq order):

    F       = fft2(y) / (h w)
    G[u, v] = F[(sy + s(u, oh)) mod h, (sx + s(v, ow)) mod w] * aperture[u, v]
    wave    = oh ow ifft2(G)                     the unnormalised inverse DFT: the amplitude depends on neither shape
    wave   /= reference_wave                     where given; a zero there gives Inf / NaN at that pixel only

A frame with a non-finite pixel has an unspecified wave; every other frame is unaffected.  For a hologram
`hologram_frame(amp, phi, counts=c, visibility=V)` whose carrier falls on the integer frequency k, the sideband at -k
reconstructs c / 2 * amp * V * exp(+i phi) sampled at (i h / oh, j w / ow), the one at +k its conjugate phase.

On the device a whole tile goes through two batched hipFFTs and three kernels (`ltmi_holo_reconstruct`,
csrc/ltmi_holo.hip); on a CPU executor NumPy computes the definition in float64 / complex128 and casts at the end.
Not part of this module: line filters (multiply them into `aperture`), averaging over a series, phase unwrapping.
"""
import numpy as np

from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, quiet_floats, runs_on_hip
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES, PlanCache, array_digest, frame_batch, udf_device

# (device, h, w, oh, ow, batch, sy, sx, digest of aperture and reference) -> hip.HoloPlan
_PLANS = PlanCache(8, owned=False)


def signed_frequencies(n):
    """s(i, n) for i in [0, n): 0, 1, ..., (n - 1) // 2, then the negative ones ascending (numpy.fft.fftfreq order)"""
    i = np.arange(int(n))
    return np.where(i <= (int(n) - 1) // 2, i, i - int(n))


def disk_aperture(out_shape, radius, smoothness=0.0):
    """1 where hypot(s(u), s(v)) <= radius, else 0, built in the unshifted layout ((0, 0) is the centre); for
    smoothness > 0 blurred by a Gaussian of that sigma that wraps around, as the layout does (needs scipy).
    -> float32 `out_shape`"""
    oh, ow = (int(s) for s in out_shape)
    r = np.hypot(signed_frequencies(oh)[:, None].astype(np.float64), signed_frequencies(ow)[None, :])
    disk = (r <= float(radius)).astype(np.float64)
    if smoothness > 0:
        from scipy.ndimage import gaussian_filter
        disk = gaussian_filter(disk, sigma=float(smoothness), mode='wrap')
    return disk.astype(np.float32)


def find_sideband(frame, exclude_radius=None, half='upper'):
    """The strongest Fourier component of a hologram away from the centre band, on the host in float64:
    |fft2(frame)| with every index of signed-frequency radius < exclude_radius zeroed (default min(h, w) / 16),
    restricted to s(ky) > 0 or (s(ky) == 0 and s(kx) > 0) for half='upper' and to the mirror half for 'lower'.
    -> (sy, sx) of the first maximum in row-major order, in the unshifted layout: a `sb_position`"""
    frame = np.asarray(frame)
    if frame.ndim != 2:
        raise ValueError(f"find_sideband needs one 2D frame, not shape {frame.shape}")
    if half not in ('upper', 'lower'):
        raise ValueError(f"half must be 'upper' or 'lower', not {half!r}")
    h, w = frame.shape
    if exclude_radius is None:
        exclude_radius = min(h, w) / 16
    fy = signed_frequencies(h)[:, None]
    fx = signed_frequencies(w)[None, :]
    mag = np.abs(np.fft.fft2(frame.astype(np.float64)))
    mag[np.hypot(fy.astype(np.float64), fx) < exclude_radius] = 0
    upper = (fy > 0) | ((fy == 0) & (fx > 0))
    lower = (fy < 0) | ((fy == 0) & (fx < 0))
    first = int(np.argmax(np.where(upper if half == 'upper' else lower, mag, -1.0)))
    return first // w, first % w


def check_params(sig, out_shape, sb_position, aperture, reference_wave):
    """-> (oh, ow), (sy, sx), float32 aperture, complex128 reference or None; ValueError names the value that is off"""
    if len(sig) != 2:
        raise ValueError(f"HoloReconstructUDF needs 2D frames, not {tuple(sig)}")
    h, w = sig
    try:
        oh, ow = (int(s) for s in out_shape)
        sy, sx = (int(s) for s in sb_position)
    except (TypeError, ValueError):
        raise ValueError(f"out_shape {out_shape!r} and sb_position {sb_position!r} must be two integers each")
    if (oh, ow) != tuple(out_shape) or (sy, sx) != tuple(sb_position):
        raise ValueError(f"out_shape {out_shape!r} and sb_position {sb_position!r} must be two integers each")
    if not (1 <= oh <= h and 1 <= ow <= w):
        raise ValueError(f"out_shape {(oh, ow)} must lie between (1, 1) and the frame shape {(h, w)}")
    if not (0 <= sy < h and 0 <= sx < w):
        raise ValueError(f"sb_position {(sy, sx)} lies outside the {(h, w)} frame")
    aperture = np.asarray(aperture)
    if aperture.dtype.kind == 'c':
        raise ValueError(f"aperture must be real, not {aperture.dtype}")
    if aperture.shape != (oh, ow):
        raise ValueError(f"aperture of shape {aperture.shape} for out_shape {(oh, ow)}")
    if reference_wave is not None:
        reference_wave = np.asarray(reference_wave)
        if reference_wave.shape != (oh, ow):
            raise ValueError(f"reference_wave of shape {reference_wave.shape} for out_shape {(oh, ow)}")
        reference_wave = reference_wave.astype(np.complex128)
    return (oh, ow), (sy, sx), np.ascontiguousarray(aperture, dtype=np.float32), reference_wave


def reconstruct_frames(frames, out_shape, sb_position, aperture, reference_wave=None, dtype=np.complex64):
    """The definition in NumPy for frames (n, h, w): float64 / complex128 throughout, cast to `dtype` at the end
    (complex128: no cast).  -> wave (n, oh, ow)"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    (oh, ow), (sy, sx), aperture, reference_wave = check_params((h, w), out_shape, sb_position, aperture,
                                                                reference_wave)
    ky = (sy + signed_frequencies(oh)) % h
    kx = (sx + signed_frequencies(ow)) % w
    with quiet_floats():
        y = frames.astype(np.float32).astype(np.float64)
        spec = np.fft.fft2(y) / (h * w)
        g = spec[:, ky[:, None], kx[None, :]] * aperture.astype(np.float64)[None]
        wave = np.fft.ifft2(g) * (oh * ow)
        if reference_wave is not None:
            wave = wave / reference_wave[None]
        return wave.astype(dtype)


def _plan(device, sig, out_shape, batch, sb, aperture, reference_wave):
    from libertem_amd import hip
    key = (int(device), sig[0], sig[1], out_shape[0], out_shape[1], int(batch), sb[0], sb[1],
           array_digest(aperture, reference_wave))
    return _PLANS.get_or_make(key, lambda: hip.HoloPlan(device, sig[0], sig[1], out_shape[0], out_shape[1], batch,
                                                        sb[0], sb[1], aperture, reference_wave))


def plan_for(udf, sig, out_shape, sb, aperture, reference_wave):
    """the cached plan of a UDF's device, shapes, sideband, aperture, reference and batch: as many frames as the
    workspace budget (the one measured for correlation plans), the tile depth and the partition allow"""
    per_frame = 4 * sig[0] * sig[1] + 8 * sig[0] * (sig[1] // 2 + 1) + 8 * out_shape[0] * out_shape[1]
    batch = frame_batch(udf, per_frame, CORR_WORKSPACE_BYTES)
    return _plan(udf_device(udf), sig, out_shape, batch, sb, aperture, reference_wave)


class HoloReconstructUDF(WholeFrameUDF):
    """
    Parameters
    ----------
    out_shape : (int, int)
        shape of the reconstructed wave, at most the frame shape
    sb_position : (int, int)
        the sideband (sy, sx) in the unshifted `fft2` layout of a frame, e.g. from `find_sideband`
    aperture : array of float, shape `out_shape`, or None
        real aperture in the unshifted layout, (0, 0) the sideband centre; None: `disk_aperture(out_shape, sb_size,
        sb_smoothness)`
    sb_size : float
        radius of the default disk aperture, in pixels of the output's Fourier space
    sb_smoothness : float
        sigma of the Gaussian that softens the default aperture's edge
    reference_wave : array of complex, shape `out_shape`, or None
        the reconstruction of a vacuum hologram: every wave is divided by it

    Result (nav, on the device): 'wave' (complex64, `out_shape`).
    """

    def __init__(self, out_shape, sb_position, aperture=None, sb_size=None, sb_smoothness=0.0, reference_wave=None):
        if aperture is None:
            if sb_size is None:
                raise ValueError("HoloReconstructUDF needs an aperture or the sb_size of a disk aperture: both are None")
            aperture = disk_aperture(out_shape, sb_size, sb_smoothness)
        super().__init__(out_shape=tuple(out_shape), sb_position=tuple(sb_position), aperture=aperture, sb_size=sb_size,
                         sb_smoothness=sb_smoothness, reference_wave=reference_wave)

    def get_result_buffers(self):
        out_shape = tuple(int(s) for s in self.params.out_shape)
        return {'wave': self.buffer(kind='nav', dtype='complex64', extra_shape=out_shape, where='device')}

    def get_dist_merge(self):
        return {'wave': 'disjoint'}

    def get_task_data(self):
        check_whole_frames(self)
        sig = tuple(int(s) for s in self.meta.dataset_shape.sig)
        p = self.params
        out_shape, sb, aperture, reference_wave = check_params(sig, p.out_shape, p.sb_position, p.aperture,
                                                               p.reference_wave)
        td = {'sig': sig, 'out_shape': out_shape, 'sb': sb, 'aperture': aperture, 'reference_wave': reference_wave}
        if runs_on_hip(self):
            td.update(plan=plan_for(self, sig, out_shape, sb, aperture, reference_wave))
        return td

    def _process_tile_numpy(self, tile):
        td = self.task_data
        self.results.wave[:] = reconstruct_frames(np.asarray(tile), td.out_shape, td.sb, td.aperture,
                                                  td.reference_wave)

    def _process_tile_hip(self, tile):
        wave = self.results.wave
        check_device_args(self, tile, wave)
        self.task_data.plan.reconstruct(tile.data_ptr(), tile.dtype, tile.shape[0], tile.ld, wave.data_ptr(), wave.ld,
                                        stream=self.meta.stream_ptr)


def run_holo(ctx, dataset, out_shape, sb_position, aperture=None, sb_size=None, sb_smoothness=0.0,
             reference_wave=None, roi=None):
    """The reconstructed wave of every frame of `dataset`; -> the result buffers by name ('wave')."""
    udf = HoloReconstructUDF(out_shape=out_shape, sb_position=sb_position, aperture=aperture, sb_size=sb_size,
                             sb_smoothness=sb_smoothness, reference_wave=reference_wave)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)
