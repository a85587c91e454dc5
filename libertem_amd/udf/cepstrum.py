"""
CepstrumUDF on MI355X: the exit-wave power cepstrum (EWPC) of every frame of a nanobeam diffraction scan (Padgett et
al., Ultramicroscopy 214 (2020) 112994), the consumer of `libertem_amd.utils.generate.strained_lattice_scan`.

The logarithm of a diffraction pattern turns the product "slowly varying envelope x lattice-periodic part" into a sum;
the magnitude of its Fourier transform has sharp peaks at the real-space lattice vectors, and the envelope collapses
into the centre.  The operation, for a frame `x` of (h, w), `out_shape` (oh, ow) with
1 <= oh <= h and 1 <= ow <= w, `offset` > 0 (rounded to float32), a real float32 `window` of (h, w) and `dc_radius`:

    y         = float32(x)
    z         = log(max(y, 0) + offset)
    t         = z * window
    C         = |fft2(t)| / (h w)                              (h, w), unshifted
    out[u, v] = C[(u - oh // 2) mod h, (v - ow // 2) mod w] * keep[u, v]

The output is centred like `fftshift`: quefrency (0, 0) sits at (oh // 2, ow // 2), and with out_shape equal to the
frame shape the output is fftshift(C), for even and odd sizes.  keep[u, v] is 0 where
hypot(u - oh // 2, v - ow // 2) < dc_radius and 1 elsewhere (dc_radius = 0 keeps everything): with it `find_peaks` on a
mean cepstrum does not return the origin.  Negative pixels count as 0, which is what dark-subtracted data needs.  A frame
with a non-finite pixel has an unspecified result; every other frame is unaffected.

On the device a whole tile goes through one batched hipFFT between two kernels (`ltmi_ceps_transform`,
csrc/ltmi_ceps.hip); on a CPU executor NumPy computes the definition in float64 and casts at the end.
`cepstrum_dataset` keeps the cepstra of a scan in HBM as a dataset that every other UDF of this package runs on: SumUDF
for the mean cepstrum, `find_peaks` on it, `run_correlation` and `run_refine` for strain maps, ApplyMasksUDF for
cepstral virtual detectors, `run_pca`.
Not part of this module: the power cepstrum |F(log |F|^2)|^2, a running mean over frames, peak tracking itself.
"""
import numpy as np

from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, quiet_floats, runs_on_hip
from libertem_amd.udf.plans import CORR_WORKSPACE_BYTES, PlanCache, array_digest, frame_batch, udf_device

# (device, h, w, oh, ow, batch, offset, dc_radius, digest of the window) -> hip.CepstrumPlan
_PLANS = PlanCache(8, owned=False)


def hann_window(sig):
    """The periodic Hann window outer(0.5 - 0.5 cos(2 pi i / h), 0.5 - 0.5 cos(2 pi j / w)), built in float64.
    -> float32 (h, w)"""
    h, w = (int(s) for s in sig)
    wy = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(h, dtype=np.float64) / h)
    wx = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(w, dtype=np.float64) / w)
    return np.outer(wy, wx).astype(np.float32)


def keep_mask(out_shape, dc_radius):
    """0 where hypot(u - oh // 2, v - ow // 2) < dc_radius, 1 elsewhere, decided in float64 -> float64 (oh, ow)"""
    oh, ow = out_shape
    u = np.arange(oh, dtype=np.float64)[:, None] - oh // 2
    v = np.arange(ow, dtype=np.float64)[None, :] - ow // 2
    return np.where(np.hypot(u, v) < float(dc_radius), 0.0, 1.0)


def check_params(sig, out_shape, offset, window, dc_radius):
    """-> (oh, ow), float32 offset, float32 window (h, w), float dc_radius; ValueError names the value that is off"""
    if len(sig) != 2:
        raise ValueError(f"CepstrumUDF needs 2D frames, not {tuple(sig)}")
    h, w = (int(s) for s in sig)
    try:
        oh, ow = (int(s) for s in out_shape)
        whole = (oh, ow) == tuple(out_shape)
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError(f"out_shape {out_shape!r} must be two integers")
    if not (1 <= oh <= h and 1 <= ow <= w):
        raise ValueError(f"out_shape {(oh, ow)} must lie between (1, 1) and the frame shape {(h, w)}")
    try:
        off32 = np.float32(offset)
    except (TypeError, ValueError):
        raise ValueError(f"offset {offset!r} must be a positive finite number")
    if not (np.isfinite(off32) and off32 > 0):
        raise ValueError(f"offset {offset!r} must be a positive finite number (as float32: {off32!r})")
    try:
        dc = float(dc_radius)
    except (TypeError, ValueError):
        raise ValueError(f"dc_radius {dc_radius!r} must be a number that is not negative")
    if not dc >= 0:
        raise ValueError(f"dc_radius {dc_radius!r} must not be negative")
    if window is None:
        window = hann_window((h, w))
    elif isinstance(window, str):
        if window != 'none':
            raise ValueError(f"window {window!r}: None (periodic Hann), 'none' (no window) or an array of {(h, w)}")
        window = np.ones((h, w), np.float32)
    else:
        window = np.asarray(window)
        if window.dtype.kind == 'c':
            raise ValueError(f"window must be real, not {window.dtype}")
        if window.shape != (h, w):
            raise ValueError(f"window of shape {window.shape} for frames of {(h, w)}")
    return (oh, ow), off32, np.ascontiguousarray(window, dtype=np.float32), dc


def cepstrum_frames(frames, out_shape, offset=1.0, window=None, dc_radius=0.0, dtype=np.float32):
    """The definition in NumPy for frames (n, h, w): float64 throughout (after the definition's float32 steps: the
    pixels, the offset, the window), cast to `dtype` at the end.  -> (n, oh, ow)"""
    frames = np.asarray(frames)
    n, h, w = frames.shape
    (oh, ow), off32, window, dc = check_params((h, w), out_shape, offset, window, dc_radius)
    ky = (np.arange(oh) - oh // 2) % h
    kx = (np.arange(ow) - ow // 2) % w
    with quiet_floats():
        y = frames.astype(np.float32).astype(np.float64)
        z = np.log(np.maximum(y, 0.0) + float(off32))
        c = np.abs(np.fft.fft2(z * window.astype(np.float64)[None])) / (h * w)
        out = c[:, ky[:, None], kx[None, :]] * keep_mask((oh, ow), dc)[None]
        return out.astype(dtype)


def _plan(device, sig, out_shape, batch, offset, window, dc_radius):
    from libertem_amd import hip
    key = (int(device), sig[0], sig[1], out_shape[0], out_shape[1], int(batch), float(offset), float(dc_radius),
           array_digest(window))
    return _PLANS.get_or_make(key, lambda: hip.CepstrumPlan(device, sig[0], sig[1], out_shape[0], out_shape[1], batch,
                                                            offset, window, dc_radius))


def plan_for(udf, sig, out_shape, offset, window, dc_radius):
    """the cached plan of a UDF's device, shapes, offset, window, dc_radius and batch: as many frames as the workspace
    budget (the one measured for correlation plans), the tile depth and the partition allow"""
    per_frame = 4 * sig[0] * sig[1] + 8 * sig[0] * (sig[1] // 2 + 1)
    batch = frame_batch(udf, per_frame, CORR_WORKSPACE_BYTES)
    return _plan(udf_device(udf), sig, out_shape, batch, offset, window, dc_radius)


class CepstrumUDF(WholeFrameUDF):
    """
    Parameters
    ----------
    out_shape : (int, int)
        the quefrencies kept around the origin, at most the frame shape; the origin sits at (oh // 2, ow // 2)
    offset : float
        added to the pixels before the logarithm, positive; about the noise floor of the detector
    window : None, 'none' or array of float, shape of the frames
        multiplied onto the logarithm; None: the periodic Hann window (`hann_window`), 'none': no window
    dc_radius : float
        quefrencies closer to the origin than this are set to 0

    Result (nav, on the device): 'cepstrum' (float32, `out_shape`).
    """

    def __init__(self, out_shape, offset=1.0, window=None, dc_radius=0.0):
        super().__init__(out_shape=tuple(out_shape), offset=offset, window=window, dc_radius=dc_radius)

    def get_result_buffers(self):
        out_shape = tuple(int(s) for s in self.params.out_shape)
        return {'cepstrum': self.buffer(kind='nav', dtype='float32', extra_shape=out_shape, where='device')}

    def get_dist_merge(self):
        return {'cepstrum': 'disjoint'}

    def get_task_data(self):
        check_whole_frames(self)
        sig = tuple(int(s) for s in self.meta.dataset_shape.sig)
        p = self.params
        out_shape, offset, window, dc_radius = check_params(sig, p.out_shape, p.offset, p.window, p.dc_radius)
        td = {'sig': sig, 'out_shape': out_shape, 'offset': offset, 'window': window, 'dc_radius': dc_radius}
        if runs_on_hip(self):
            td.update(plan=plan_for(self, sig, out_shape, offset, window, dc_radius))
        return td

    def _process_tile_numpy(self, tile):
        td = self.task_data
        self.results.cepstrum[:] = cepstrum_frames(np.asarray(tile), td.out_shape, td.offset, td.window, td.dc_radius)

    def _process_tile_hip(self, tile):
        ceps = self.results.cepstrum
        check_device_args(self, tile, ceps)
        self.task_data.plan.transform(tile.data_ptr(), tile.dtype, tile.shape[0], tile.ld, ceps.data_ptr(), ceps.ld,
                                      stream=self.meta.stream_ptr)


def run_cepstrum(ctx, dataset, out_shape, offset=1.0, window=None, dc_radius=0.0, roi=None):
    """The cepstrum of every frame of `dataset`; -> the result buffers by name ('cepstrum')."""
    udf = CepstrumUDF(out_shape=out_shape, offset=offset, window=window, dc_radius=dc_radius)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)


def cepstrum_dataset(ctx, dataset, out_shape, offset=1.0, window=None, dc_radius=0.0, num_partitions=None):
    """The cepstra of `dataset` as a dataset of shape nav + out_shape for the other UDFs.  On a HIP executor the run
    leaves its result in HBM (`result_where='device'`) and the MemoryDataSet wraps that HipArray: no copy and no
    download.  On a CPU executor it wraps the NumPy result.  Positions a sync_offset leaves without a frame hold
    zeros."""
    udf = CepstrumUDF(out_shape=out_shape, offset=offset, window=window, dc_radius=dc_radius)
    nav = tuple(int(s) for s in dataset.shape.nav)
    shape = nav + tuple(int(s) for s in out_shape)
    kwargs = {} if num_partitions is None else {'num_partitions': num_partitions}
    if getattr(ctx.executor, 'gpu_id', None) is not None:
        res = ctx.run_udf(dataset=dataset, udf=udf, result_where='device')
        data = res['cepstrum'].device_data
        if data is None:
            raise RuntimeError("the run did not leave 'cepstrum' on the device")
        data = data.reshape(shape)
    else:
        res = ctx.run_udf(dataset=dataset, udf=udf)
        data = np.asarray(res['cepstrum'].data).reshape(shape)
    return ctx.load('memory', data=data, sig_dims=2, **kwargs)
