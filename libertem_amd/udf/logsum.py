"""
LogsumUDF on MI355X: the sum of log-scaled frames, log(frame - min(frame) + 1).
Drop-in for the reference's libertem.udf.logsum (LogsumUDF, run_logsum; udf/logsum.py:6-83).

Each term is computed in the reference's float frame dtype, np.result_type(float32, stored dtype): the
integer pixels are converted first, so they never wrap.  On the device `ltmi_logsum_frames` folds a tile
of whole frames into the float32 buffer (per-frame min, then float64 sums of the terms per slab of
frames, merged in a fixed order); on a CPU executor NumPy does the same sums.
"""
import numpy as np

from libertem_amd.common.buffers import HipSigView
from libertem_amd.udf.base import UDF
from libertem_amd.udf.device import (
    SigSlice, Workspace, check_device_args, check_whole_frames, float_frames, quiet_floats, runs_on_hip,
)


class LogsumUDF(UDF):
    """
    Sum up log-scaled frames: log(frame - min(frame) + 1) per frame, summed over all frames.

    In comparison to log-scaling the sum, this highlights regions with slightly higher intensity that
    appear in many frames in relation to very high intensity in a few frames.

    Result 'logsum' (sig, float32).  Complex data raises a TypeError, as in the reference.
    """

    REUSE_TASK_INSTANCES = True
    #: positions a sync_offset leaves without a frame add nothing (zero frames would add log(1) = 0
    #: everywhere, but are not delivered either: the same rule as the other frame statistics)
    VALID_FRAMES_ONLY = True
    WHOLE_FRAME_TILES = True

    def __init__(self):
        super().__init__()

    def get_preferred_input_dtype(self):
        # the frames as stored: the kernel converts in registers
        return self.USE_NATIVE_DTYPE

    def get_backends(self):
        return (self.BACKEND_HIP, self.BACKEND_NUMPY)

    def get_result_buffers(self):
        return {'logsum': self.buffer(kind='sig', dtype='float32', where='device')}

    def get_task_data(self):
        dt = np.dtype(self.meta.input_dtype)
        if dt.kind == 'c':
            # the reference cannot cast the complex terms into its float32 buffer (udf/logsum.py:56-59)
            raise TypeError(f"LogsumUDF: complex input ({dt}) cannot be log-summed into a float32 buffer")
        check_whole_frames(self)
        if runs_on_hip(self):
            if dt.kind not in 'fiu' or (dt.kind in 'iu' and dt.itemsize > 4):
                raise NotImplementedError(f"LogsumUDF on MI355X: input dtype {dt} is not supported")
        return {'workspace': Workspace()}

    def process_tile(self, tile):
        if tile.shape[0] == 0:
            return
        if self.meta.array_backend == self.BACKEND_NUMPY:
            self._process_tile_numpy(tile)
        else:
            self._process_tile_hip(tile)

    def _process_tile_numpy(self, tile):
        # np.log(frame - np.min(frame) + 1) per frame (udf/logsum.py:54-59), in the float frame dtype,
        # summed in float64 and added to the float32 buffer
        tile = float_frames(tile)
        if tile.dtype.kind == 'c':
            raise TypeError(f"LogsumUDF: complex input ({tile.dtype}) cannot be log-summed into a float32 buffer")
        n = tile.shape[0]
        flat = tile.reshape((n, -1))
        with quiet_floats():
            mins = np.min(flat, axis=1, keepdims=True)
            terms = np.log(flat - mins + tile.dtype.type(1))
        total = terms.sum(axis=0, dtype=np.float64).reshape(self.results.logsum.shape)
        out = self.results.logsum
        out[:] = out + total

    def _process_tile_hip(self, tile):
        from libertem_amd import hip
        lv = self.results.logsum
        check_device_args(self, tile, lv, kind=HipSigView)
        n = tile.shape[0]
        sl = SigSlice(lv, self.meta.dataset_shape.sig)
        if not sl.whole_frames:
            raise ValueError(f"LogsumUDF needs whole frames, got a tile of sig shape {sl.shape} at {sl.origin}")
        ws = self.task_data.workspace.ptr(tile.device, hip.logsum_workspace(n, sl.n_px, tile.dtype))
        hip.logsum_frames(tile.device, tile.data_ptr(), tile.dtype, n, sl.n_px, tile.ld, lv.array.data_ptr(), ws,
                          stream=self.meta.stream_ptr)

    def merge(self, dest, src):
        dest.logsum[:] += src.logsum[:]

    def merge_all(self, ordered_results):
        # the partitions in order, as `merge` adds them: both give the same numbers
        parts = [b.logsum for b in ordered_results.values()]
        total = np.zeros_like(np.asarray(parts[0]))
        for p in parts:
            total += p
        return {'logsum': total}

    def get_dist_merge(self):
        return {'logsum': 'sum'}


def run_logsum(ctx, dataset, roi=None):
    """
    Sum up log-scaled frames (udf/logsum.py:62-83): sum over frames of log(frame - min(frame) + 1).
    """
    return ctx.run_udf(dataset=dataset, udf=LogsumUDF(), roi=roi)
