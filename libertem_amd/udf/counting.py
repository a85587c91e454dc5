"""
Electron counting on MI355X: dense frames of a direct detector at low dose in, a `raw_csr` dataset out.

    ds = ctx.load('k2is', path=...)
    t_bg, t_x = estimate_thresholds(sample_frames, dark=dark)
    count_events(ctx, ds, 'counted.toml', t_bg, t_x, dark=dark)
    counted = ctx.load('raw_csr', path='counted.toml')        # every mask run now reads the events only

What an event is (include/ltmi.h carries the same text).  For a frame of (h, w) pixels with
row-major pixel number p = y w + x, an optional `dark` and `gain` (float32, shape of a frame) and the thresholds
t_bg = background_threshold and t_x = xray_threshold as float32:

    1. v[p] = float32(pixel[p]) as `ndarray.astype(np.float32)` rounds; with `dark`, v = v - dark (one float32
       subtraction); with `gain`, v = v * gain (one float32 multiplication); subtract, then multiply;
    2. u[p] = v[p] if v[p] <= t_x, else 0: an x-ray hit is zeroed and does not count; NaN compares false and becomes
       0; +Inf with t_x = +inf stays and can be an event;
    3. p is an event iff u[p] > t_bg and, for its up to 8 neighbours q inside the frame, u[p] > u[q] where q < p and
       u[p] >= u[q] where q > p: of equal neighbours the first in row-major order wins, no two events are adjacent;
    4. the events of a frame by ascending p; `values='count'` stores uint8(1), `values='intensity'` u[p] as float32;
    5. a scan position that a `sync_offset` leaves without a frame has no events.

Every decision is an exact float32 comparison, so the NumPy branch (`count_frames`) and the kernels
(`ltmi_count_events`, `ltmi_store_events`, csrc/ltmi_count.hip) give the same bytes.

`count_events` runs two UDFs, so the frames are read twice: `EventCountUDF` for the events per position, from which
the row pointer follows, then `EventStoreUDF`, which writes every event to its final place.  For a dataset resident
in HBM that is two passes at memory speed next to one host write of the events; for a dataset streamed from host
memory it doubles the upload.  With `run_udf(corrections=...)` the tiles arrive corrected, as float32, and the UDFs
count them as they are (`dark=None`, `gain=None`).
"""
import os

import numpy as np

from libertem_amd.common.hiparray import HipArray
from libertem_amd.common.math import prod
from libertem_amd.udf.device import WholeFrameUDF, check_device_args, check_whole_frames, runs_on_hip
from libertem_amd.udf.plans import udf_device

#: frame dtypes that are counted (what `ltmi_count_events` takes)
FRAME_DTYPES = tuple(np.dtype(t) for t in ('u1', 'i1', 'u2', 'i2', 'u4', 'i4', 'f4'))
#: widest frame the kernels take (csrc/ltmi_count.hip)
MAX_WIDTH = 4096
VALUES = {'count': np.dtype('u1'), 'intensity': np.dtype('<f4')}


def check_params(sig, background_threshold, xray_threshold=np.inf, dark=None, gain=None, values='count'):
    """-> (t_bg, t_x as np.float32, dark, gain as C-contiguous float32 or None, dtype of the stored values);
    ValueError names the value that is off"""
    sig = tuple(int(s) for s in sig)
    if len(sig) != 2 or min(sig) < 1:
        raise ValueError(f"counting needs 2D frames, not frames of shape {sig}")
    if values not in VALUES:
        raise ValueError(f"values {values!r} must be one of {sorted(VALUES)}")
    with np.errstate(over='ignore'):
        t_bg, t_x = np.float32(background_threshold), np.float32(xray_threshold)
    if t_bg != t_bg:
        raise ValueError(f"background_threshold {background_threshold} is not a number")
    if t_x != t_x:
        raise ValueError(f"xray_threshold {xray_threshold} is not a number")
    out = []
    for name, arr in (('dark', dark), ('gain', gain)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            if arr.shape != sig:
                raise ValueError(f"{name} of shape {arr.shape} for frames of {sig}")
        out.append(arr)
    return t_bg, t_x, out[0], out[1], VALUES[values]


def check_frame_dtype(dtype):
    dtype = np.dtype(dtype)
    if dtype not in FRAME_DTYPES:
        raise ValueError(f"frame dtype {dtype} is not counted: one of {[d.name for d in FRAME_DTYPES]}")
    return dtype


def corrected_frames(frames, dark=None, gain=None):
    """step 1 for frames (n, h, w): float32, dark subtracted, gain multiplied"""
    with np.errstate(all='ignore'):
        v = np.asarray(frames).astype(np.float32)
        if dark is not None:
            v = v - dark[None]
        if gain is not None:
            v = v * gain[None]
    return v


def _event_mask(u, t_bg):
    """step 3 for u (n, h, w) float32 without NaN -> bool (n, h, w)"""
    n, h, w = u.shape
    pad = np.full((n, h + 2, w + 2), -np.inf, dtype=np.float32)
    pad[:, 1:-1, 1:-1] = u
    # a cell outside the frame holds -inf: `>` fails only for u = -inf, which is not above any t_bg; `>=` holds
    ev = u > t_bg
    for dy, dx in ((-1, -1), (-1, 0), (-1, 1), (0, -1)):
        ev &= u > pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        ev &= u >= pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return ev


def count_frames(frames, background_threshold, xray_threshold=np.inf, dark=None, gain=None, values='count'):
    """The definition in vectorised NumPy for host frames (n, h, w) -> (indptr int64 (n + 1,), indices int32, data
    uint8 or float32): the CSR rows of the frames' events.  This is the NumPy branch of both UDFs."""
    frames = np.asarray(frames)
    if frames.ndim != 3:
        raise ValueError(f"frames must have shape (n, h, w), not {frames.shape}")
    check_frame_dtype(frames.dtype)
    n, h, w = frames.shape
    if h * w > 2 ** 31 - 1:
        raise ValueError(f"frames of {h} x {w}: at most 2**31 - 1 pixels each")
    t_bg, t_x, dark, gain, vdtype = check_params((h, w), background_threshold, xray_threshold, dark, gain, values)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indices, data = [], []
    step = max(1, (1 << 22) // (h * w))                       # ~16 MiB of float32 at a time
    for f0 in range(0, n, step):
        with np.errstate(all='ignore'):
            v = corrected_frames(frames[f0:f0 + step], dark, gain)
            u = np.where(v <= t_x, v, np.float32(0))
            ev = _event_mask(u, t_bg).reshape((v.shape[0], -1))
        f, p = np.nonzero(ev)                                 # (row-major: by frame, then ascending p)
        indptr[f0 + 1:f0 + 1 + v.shape[0]] = ev.sum(axis=1)
        indices.append(p.astype(np.int32))
        data.append(np.ones(len(p), dtype=vdtype) if vdtype.kind == 'u' else
                    u.reshape((v.shape[0], -1))[f, p].astype(vdtype))
    np.cumsum(indptr, out=indptr)
    return (indptr, np.concatenate(indices) if indices else np.zeros(0, np.int32),
            np.concatenate(data) if data else np.zeros(0, vdtype))


def estimate_thresholds(frames, dark=None, gain=None, background_sigma=4.0, xray_sigma=10.0):
    """Thresholds from a sample of frames (n, h, w) or (h, w) -- a few hundred, picked with an ROI -- on the host:

        t_x  = mean + xray_sigma * std of all corrected values v;
        t_bg = median + background_sigma * 1.4826 * MAD of the v <= t_x.

    -> (t_bg, t_x) as Python floats.  The x-ray cut assumes that x-ray hits are present and dominate the variance: on
    a sample without any, mean + 10 std can fall below the electron signal, so look at t_x before using it."""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    if frames.ndim != 3 or frames.size == 0:
        raise ValueError(f"frames must have shape (n, h, w) with n, h, w > 0, not {frames.shape}")
    check_frame_dtype(frames.dtype)
    for name, s in (('background_sigma', background_sigma), ('xray_sigma', xray_sigma)):
        if not float(s) >= 0:
            raise ValueError(f"{name} {s} must be at least 0")
    _, _, dark, gain, _ = check_params(frames.shape[1:], 0.0, np.inf, dark, gain)
    v = corrected_frames(frames, dark, gain).astype(np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    if v.size == 0:
        raise ValueError("frames hold no finite value")
    t_x = float(v.mean() + float(xray_sigma) * v.std())
    kept = v[v <= t_x]
    med = float(np.median(kept))
    mad = float(np.median(np.abs(kept - med)))
    return med + float(background_sigma) * 1.4826 * mad, t_x


class _CountingUDF(WholeFrameUDF):
    """what the two UDFs share: the parameter checks and the device copies of dark and gain (positions a sync_offset
    leaves without a frame have no events)"""

    def _counting_task_data(self, values='count'):
        check_whole_frames(self)
        sig = tuple(int(s) for s in self.meta.dataset_shape.sig)
        p = self.params
        t_bg, t_x, dark, gain, vdtype = check_params(sig, p.background_threshold, p.xray_threshold, p.dark, p.gain,
                                                     values)
        check_frame_dtype(self.meta.input_dtype)
        td = {'sig': sig, 't_bg': t_bg, 't_x': t_x, 'dark': dark, 'gain': gain, 'vdtype': vdtype,
              'dark_dev': None, 'gain_dev': None}
        if runs_on_hip(self):
            if sig[1] > MAX_WIDTH:
                raise ValueError(f"frames of {sig[1]} columns: the device counts frames of at most {MAX_WIDTH}")
            device = td['device'] = udf_device(self)
            if dark is not None:
                td['dark_dev'] = HipArray.from_numpy(dark, device)
            if gain is not None:
                td['gain_dev'] = HipArray.from_numpy(gain, device)
        return td

    def _kernel_args(self, tile):
        """the leading arguments of `hip.count_events` / `hip.store_events` for a device tile"""
        td = self.task_data
        check_frame_dtype(tile.dtype)
        return (td.device, tile.data_ptr(), tile.dtype, tile.shape[0], td.sig[0], td.sig[1], tile.ld,
                td.dark_dev.data_ptr() if td.dark_dev is not None else None,
                td.gain_dev.data_ptr() if td.gain_dev is not None else None, float(td.t_bg), float(td.t_x))


class EventCountUDF(_CountingUDF):
    """
    The number of electron events of every frame: the events-per-position map of a scan, and the first pass of
    `count_events`.

    Parameters
    ----------
    background_threshold : float
        t_bg: an event's value exceeds it
    xray_threshold : float
        t_x: values above it are zeroed before the search (default +inf: none)
    dark, gain : array of float, shape of a frame, optional
        subtracted from / multiplied onto the frames, as float32, in this order

    Result (nav, on the device): 'n_events' (int32).
    """

    def __init__(self, background_threshold, xray_threshold=np.inf, dark=None, gain=None):
        super().__init__(background_threshold=background_threshold, xray_threshold=xray_threshold, dark=dark,
                         gain=gain)

    def get_result_buffers(self):
        return {'n_events': self.buffer(kind='nav', dtype='int32', where='device')}

    def get_dist_merge(self):
        return {'n_events': 'disjoint'}

    def get_task_data(self):
        return self._counting_task_data()

    def _process_tile_numpy(self, tile):
        td = self.task_data
        indptr, _, _ = count_frames(np.asarray(tile), td.t_bg, td.t_x, td.dark, td.gain)
        self.results.n_events[:] = np.diff(indptr).astype(np.int32)

    def _process_tile_hip(self, tile):
        from libertem_amd import hip
        check_device_args(self, tile, self.results.n_events)
        hip.count_events(*self._kernel_args(tile), self.results.n_events.data_ptr(), stream=self.meta.stream_ptr)


class EventStoreUDF(_CountingUDF):
    """
    The events of every frame written into the `indices` and `data` files of a CSR triple whose row pointer is
    known: the second pass of `count_events`.

    Same contract as RecordUDF: there are no result buffers; the two files are created by the caller at their exact
    final size (`indptr[-1]` entries of int32 and of the values' dtype), every task maps them again and writes its
    tiles' events at `indptr[first frame of the tile]`.  On the device a tile is one `ltmi_store_events` call into a
    buffer sized from `indptr`, one D2H copy and one assignment per file; a row pointer that does not fit the events
    raises.

    Runs in one process only: with several ranks (`torchrun`) all of them would write one file.

    Parameters
    ----------
    indptr : array of int64, (number of scan positions + 1,)
        concatenate(([0], cumsum(n_events))) of an EventCountUDF run with the same parameters
    indices_file, data_file : str or path-like
        existing files of indptr[-1] * 4 and indptr[-1] * itemsize bytes
    values : 'count' | 'intensity'
        what `data_file` holds: uint8 ones, or the events' corrected values as float32
    background_threshold, xray_threshold, dark, gain
        as for EventCountUDF
    """

    def __init__(self, indptr, indices_file, data_file, values, background_threshold, xray_threshold=np.inf,
                 dark=None, gain=None):
        super().__init__(indptr=indptr, indices_file=indices_file, data_file=data_file, values=values,
                         background_threshold=background_threshold, xray_threshold=xray_threshold, dark=dark,
                         gain=gain)

    def preprocess(self):
        if self.meta.roi is not None:
            raise RuntimeError('Recording with ROI is not supported.')

    def get_result_buffers(self):
        return {}

    def get_task_data(self):
        td = self._counting_task_data(self._kwargs['values'])
        indptr = np.ascontiguousarray(self.params.indptr, dtype=np.int64)
        n_nav = prod(self.meta.dataset_shape.nav)
        if indptr.shape != (n_nav + 1,) or indptr[0] != 0 or np.any(np.diff(indptr) < 0):
            raise ValueError(f"indptr must be a non-decreasing row pointer of {n_nav + 1} entries starting at 0")
        nnz = int(indptr[-1])
        td.update(indptr=indptr, indices=None, data=None, indptr_dev=None)
        for key, fn, dt in (('indices', self.params.indices_file, np.dtype('<i4')),
                            ('data', self.params.data_file, td['vdtype'])):
            if os.path.getsize(fn) != nnz * dt.itemsize:
                raise ValueError(f"{fn} holds {os.path.getsize(fn)} bytes, indptr asks for {nnz * dt.itemsize}")
            if nnz:                                           # (an empty file cannot be mapped)
                td[key] = np.memmap(fn, dtype=dt, mode='r+', shape=(nnz,))
        if runs_on_hip(self):
            td['indptr_dev'] = HipArray.from_numpy(indptr, td['device'])
        return td

    def _span(self, tile):
        """-> the tile's first frame, and where its events begin and end in the two files"""
        first = int(self.meta.slice.origin[0])
        return first, int(self.task_data.indptr[first]), int(self.task_data.indptr[first + tile.shape[0]])

    def _process_tile_numpy(self, tile):
        td = self.task_data
        first, lo, hi = self._span(tile)
        indptr, indices, data = count_frames(np.asarray(tile), td.t_bg, td.t_x, td.dark, td.gain,
                                             self._kwargs['values'])
        if not np.array_equal(indptr + lo, td.indptr[first:first + tile.shape[0] + 1]):
            raise RuntimeError(f"indptr does not fit the events of the frames from {first} on")
        if hi > lo:
            td.indices[lo:hi] = indices
            td.data[lo:hi] = data

    def _process_tile_hip(self, tile):
        import torch
        from libertem_amd import hip
        td = self.task_data
        first, lo, hi = self._span(tile)
        nnz, isz = hi - lo, td.vdtype.itemsize
        # one buffer, one copy: [indices int32 x nnz | values x nnz | padding to 4 bytes | status int32]
        at_values = 4 * nnz
        at_status = (at_values + isz * nnz + 3) // 4 * 4
        buf = torch.empty(at_status + 4, dtype=torch.uint8, device=f'cuda:{td.device}')
        # (the executor's stream is torch's current one: the zeroing, the kernel and the copy are in order)
        buf[at_status:].zero_()
        hip.store_events(*self._kernel_args(tile), td.indptr_dev.data_ptr() + 8 * first, lo, nnz,
                         buf.data_ptr(), buf.data_ptr() + at_values, td.vdtype, buf.data_ptr() + at_status,
                         stream=self.meta.stream_ptr)
        host = buf.cpu().numpy()
        if host[at_status:].view(np.int32)[0] != 0:
            raise RuntimeError(f"indptr does not fit the events of the frames from {first} on")
        if nnz:
            td.indices[lo:hi] = host[:at_values].view('<i4')
            td.data[lo:hi] = host[at_values:at_values + isz * nnz].view(td.vdtype)


def write_sidecar(path, nav_shape, sig_shape, stem, data_dtype):
    """the TOML sidecar of a raw_csr dataset, in the layout RawCSRDataSet's docstring shows"""
    with open(path, 'w') as f:
        f.write('[params]\n'
                'filetype = "raw_csr"\n'
                f'nav_shape = {[int(s) for s in nav_shape]}\n'
                f'sig_shape = {[int(s) for s in sig_shape]}\n'
                '\n'
                '[raw_csr]\n'
                f'indptr_file = "{stem}.indptr"\n'
                'indptr_dtype = "<i8"\n'
                f'indices_file = "{stem}.indices"\n'
                'indices_dtype = "<i4"\n'
                f'data_file = "{stem}.data"\n'
                f'data_dtype = "{np.dtype(data_dtype).str}"\n')


def count_events(ctx, dataset, path, background_threshold, xray_threshold=np.inf, dark=None, gain=None,
                 values='count'):
    """
    Count the electron events of `dataset` and write them as a raw_csr dataset: the TOML sidecar at `path` and, next
    to it, `<stem>.indptr` (int64), `<stem>.indices` (int32) and `<stem>.data` (uint8 ones for values='count',
    float32 for values='intensity'), `<stem>` being the sidecar's name without its extension.
    `ctx.load('raw_csr', path=path)` reads the result.

    Two runs over the frames (EventCountUDF, EventStoreUDF): for data resident in HBM two passes at memory speed; for
    a dataset streamed from host memory the upload happens twice.  One process only, no region of interest.

    -> {'n_events': the int32 events-per-position map (nav shape), 'nnz': their number, 'path': path}
    """
    path = str(path)
    sig = tuple(int(s) for s in dataset.shape.sig)
    nav = tuple(int(s) for s in dataset.shape.nav)
    _, _, _, _, vdtype = check_params(sig, background_threshold, xray_threshold, dark, gain, values)
    params = dict(background_threshold=background_threshold, xray_threshold=xray_threshold, dark=dark, gain=gain)
    res = ctx.run_udf(dataset=dataset, udf=EventCountUDF(**params))
    n_events = np.asarray(res['n_events'].data).astype(np.int32).reshape(nav)
    indptr = np.concatenate(([0], np.cumsum(n_events.reshape(-1), dtype=np.int64))).astype(np.int64)
    nnz = int(indptr[-1])
    folder, name = os.path.split(path)
    stem = os.path.splitext(name)[0]
    files = {key: os.path.join(folder, f'{stem}.{key}') for key in ('indptr', 'indices', 'data')}
    indptr.astype('<i8').tofile(files['indptr'])
    for key, itemsize in (('indices', 4), ('data', vdtype.itemsize)):
        with open(files[key], 'wb') as f:
            f.truncate(nnz * itemsize)
    ctx.run_udf(dataset=dataset, udf=EventStoreUDF(indptr=indptr, indices_file=files['indices'],
                                                   data_file=files['data'], values=values, **params))
    write_sidecar(path, nav, sig, stem, vdtype)
    return {'n_events': n_events, 'nnz': nnz, 'path': path}
