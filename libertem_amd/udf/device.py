"""
What the UDFs that run on the device share.  For the reduction UDFs (SumUDF, SumSigUDF, StdDevUDF, FEMUDF,
LogsumUDF): the backend and argument checks, the scratch buffer of a task, where a tile's sig slice
lies in the full-frame buffer, and the float frames of the NumPy branches -- plain functions and two
small classes; those UDFs derive from `UDF` directly, as the reference's do.  For the UDFs that take
whole frames of every valid position, on the device or in NumPy (correlation, peak search, holography,
cepstrum, orientation matching, event counting, the scan UDFs of `libertem_amd.udf.ssb`): the base
class `WholeFrameUDF`.
"""
import contextlib
import warnings

import numpy as np

from libertem_amd.common.math import prod
from libertem_amd.common.hiparray import HipArray
from libertem_amd.common.exceptions import HipRequiredError
from libertem_amd.udf.base import UDF


def runs_on_hip(udf):
    """True on BACKEND_HIP, False on BACKEND_NUMPY; any other backend is not one these UDFs run on.
    The executor's device class decides, there is no fallback from one to the other."""
    backend = udf.meta.array_backend
    if backend == udf.BACKEND_HIP:
        return True
    if backend != udf.BACKEND_NUMPY:
        raise HipRequiredError(
            f"{type(udf).__name__} needs BACKEND_HIP (an MI355X worker) or BACKEND_NUMPY (a CPU executor)")
    return False


def check_device_args(udf, tile, *buffers, kind=HipArray):
    """the tile is a HipArray and every result buffer a `kind` (HipSigView for sig buffers)"""
    if not isinstance(tile, HipArray) or not all(isinstance(b, kind) for b in buffers):
        raise HipRequiredError(f"{type(udf).__name__}.process_tile expects device tiles and buffers")


def check_whole_frames(udf):
    """for UDFs with WHOLE_FRAME_TILES: a dataset that forces a tileshape cutting the frames is an error"""
    if getattr(udf.meta, 'sig_sliced_tiles', False):
        ds_shape = tuple(udf.meta.dataset_shape)
        ts = udf.meta.tiling_scheme
        shape = tuple(ts.shape) if ts is not None else None
        raise ValueError(
            f"{type(udf).__name__} needs whole frames, but the dataset forces tileshape {shape} that cuts "
            f"the frames of shape {ds_shape[-len(tuple(udf.meta.dataset_shape.sig)):]}")


class WholeFrameUDF(UDF):
    """A UDF of whole frames in their stored dtype, on BACKEND_HIP or BACKEND_NUMPY.  A subclass calls
    `check_whole_frames` and puts the frame shape `sig` into its task data, and processes the tiles,
    none of them empty, in `_process_tile_numpy(tile)` and `_process_tile_hip(tile)`."""

    REUSE_TASK_INSTANCES = True
    #: positions a sync_offset leaves without a frame get no result, on the device as on the host
    VALID_FRAMES_ONLY = True
    WHOLE_FRAME_TILES = True

    def get_preferred_input_dtype(self):
        # the frames as stored: the kernels convert in registers
        return self.USE_NATIVE_DTYPE

    def get_backends(self):
        return (self.BACKEND_HIP, self.BACKEND_NUMPY)

    def process_tile(self, tile):
        if tile.shape[0] == 0:
            return
        if self.meta.array_backend == self.BACKEND_NUMPY:
            self._process_tile_numpy(tile)
            return
        check_device_args(self, tile)
        sig = tuple(self.task_data.sig)
        if tuple(tile.shape[1:]) != sig:
            raise ValueError(
                f"{type(self).__name__} takes whole frames {sig}, got tiles of {tuple(tile.shape[1:])}")
        self._process_tile_hip(tile)


class Workspace:
    """Grow-only scratch buffer on the tile's device.  Kept in the task data, so it lives as long as
    the task instance; reallocated only when a request exceeds what is held."""

    def __init__(self):
        self._buf, self._bytes = None, -1

    def ptr(self, device, nbytes):
        if self._bytes < nbytes:
            import torch
            self._buf = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=f'cuda:{device}')
            self._bytes = nbytes
        return self._buf.data_ptr()


class SigSlice:
    """Where the sig slice of a HipSigView lies in the buffer of the full sig shape."""

    def __init__(self, view, sig_full):
        self.sig_full = tuple(sig_full)
        self.origin = tuple(view.tile_slice.origin[-len(self.sig_full):])
        self.shape = tuple(view.tile_slice.shape.sig)
        self.n_px = prod(self.shape)
        #: the slice is one contiguous run of the buffer (it cuts the outermost sig axis only)
        self.whole_rows = self.shape[1:] == self.sig_full[1:] and all(o == 0 for o in self.origin[1:])
        self.whole_frames = self.whole_rows and self.shape == self.sig_full and self.origin[0] == 0

    def blocks(self):
        """-> (tile_off, n_px, out_off, cols, ld_out) in elements: `n_px` pixels from `tile_off` of
        a frame of the tile are rows of `cols` pixels at stride `ld_out` from `out_off` of the buffer.
        One block for whole rows; for a partial-width slice one block per index of the outer sig
        axes (2D detectors: ONE block)."""
        sig_full, s_origin, s_shape = self.sig_full, self.origin, self.shape
        strides = [prod(sig_full[k + 1:]) for k in range(len(sig_full))]
        if self.whole_rows:
            yield 0, self.n_px, s_origin[0] * strides[0], self.n_px, self.n_px
            return
        rows, cols = s_shape[-2], s_shape[-1]
        for outer in np.ndindex(*s_shape[:-2]):
            off = sum((o + i) * st for o, i, st in zip(s_origin[:-2], outer, strides[:-2]))
            off += s_origin[-2] * strides[-2] + s_origin[-1]
            toff = sum(i * prod(s_shape[k + 1:]) for k, i in enumerate(outer))
            yield toff, rows * cols, off, cols, sig_full[-1]


def float_frames(tile):
    """the tile in the reference's float frame dtype, np.result_type(float32, stored dtype)"""
    tile = np.asarray(tile)
    dtype = np.result_type(np.float32, tile.dtype)
    return tile if tile.dtype == dtype else tile.astype(dtype)


@contextlib.contextmanager
def quiet_floats():
    """NaN / inf / empty-slice arithmetic without NumPy's warnings (the values are the result)"""
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        yield
