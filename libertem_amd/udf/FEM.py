"""
FEMUDF on MI355X: fluctuation electron microscopy, the standard deviation of the pixels of a ring in
every frame.  Drop-in for the reference's libertem.udf.FEM (FEMUDF, run_fem; udf/FEM.py:7-96).

The ring is the reference's exact boolean mask (`_make_circular_mask` of rad_out minus that of rad_in,
pixels where the difference is 1), handed to the device as row spans (row, x0, x1).  On the device
`ltmi_ring_moments` reduces each frame of a tile in one workgroup (float64 sums about the frame's first
ring pixel); on a CPU executor NumPy computes `np.std(frame[mask == 1])` like the reference.
"""
import numpy as np

from libertem_amd.masks import _make_circular_mask
from libertem_amd.udf.base import UDF
from libertem_amd.udf.device import (
    check_device_args, check_whole_frames, float_frames, quiet_floats, runs_on_hip,
)


def ring_mask(center, rad_in, rad_out, sig_shape):
    """the reference's ring (udf/FEM.py:44-63): center[0] is the ROW, center[1] the column"""
    mask_out = 1 * _make_circular_mask(center[1], center[0], sig_shape[1], sig_shape[0], rad_out)
    mask_in = 1 * _make_circular_mask(center[1], center[0], sig_shape[1], sig_shape[0], rad_in)
    return (mask_out - mask_in) == 1


def ring_spans(mask):
    """the True runs of a 2D boolean mask as an (n, 3) int32 array of (row, x0, x1), row-major order"""
    m = np.asarray(mask, dtype=bool)
    padded = np.zeros((m.shape[0], m.shape[1] + 2), dtype=np.int8)
    padded[:, 1:-1] = m
    d = np.diff(padded, axis=1)
    rows, starts = np.nonzero(d == 1)
    _, ends = np.nonzero(d == -1)
    return np.stack([rows, starts, ends], axis=1).astype(np.int32).reshape((-1, 3))


class FEMUDF(UDF):
    '''
    Fluctuation EM: the standard deviation within a ring around the zero order diffraction peak.

    Parameters
    ----------
    center : Tuple[float]
        Center of the ring.  As in the reference's code (its docstring says (x, y)), center[0] is the
        row (y) and center[1] the column (x).
    rad_in : float
        Inner radius of the ring (pixels at this distance are outside the ring).
    rad_out : float
        Outer radius of the ring (pixels at this distance are inside the ring).

    Result 'intensity' (nav, float32): np.std of the ring pixels of each frame, NaN for an empty ring.
    '''

    REUSE_TASK_INSTANCES = True
    #: positions a sync_offset leaves without a frame are not delivered on the device either: a zero
    #: frame there would write a std of 0 where the reference writes nothing
    VALID_FRAMES_ONLY = True
    WHOLE_FRAME_TILES = True

    def __init__(self, center, rad_in, rad_out):
        super().__init__(center=center, rad_in=rad_in, rad_out=rad_out)

    def get_preferred_input_dtype(self):
        # the frames as stored: the kernel converts in registers
        return self.USE_NATIVE_DTYPE

    def get_backends(self):
        return (self.BACKEND_HIP, self.BACKEND_NUMPY)

    def get_result_buffers(self):
        return {'intensity': self.buffer(kind='nav', dtype='float32', where='device')}

    def get_task_data(self):
        check_whole_frames(self)
        sig = tuple(self.meta.dataset_shape.sig)
        if len(sig) != 2:
            raise ValueError(f"FEMUDF needs 2D frames, not {sig}")
        mask = ring_mask(self.params.center, self.params.rad_in, self.params.rad_out, sig)
        if not runs_on_hip(self):
            return {'mask': mask, 'flat': np.flatnonzero(mask.reshape(-1)), 'spans': None}
        spans = ring_spans(mask)
        return {'mask': mask, 'flat': None, 'spans': spans, 'n_ring': int(np.count_nonzero(mask)),
                'device_spans': {}}

    def process_tile(self, tile):
        n = tile.shape[0]
        if n == 0:
            return
        if self.meta.array_backend == self.BACKEND_NUMPY:
            self._process_tile_numpy(tile)
        else:
            self._process_tile_hip(tile)

    def _process_tile_numpy(self, tile):
        # np.std(frame[mask == 1]) per frame (udf/FEM.py:65-66), in the reference's float frame dtype
        tile = float_frames(tile)
        vals = tile.reshape((tile.shape[0], -1))[:, self.task_data.flat]
        with quiet_floats():
            self.results.intensity[:] = np.std(vals, axis=1)

    def _process_tile_hip(self, tile):
        from libertem_amd import hip
        out = self.results.intensity
        check_device_args(self, tile, out)
        td = self.task_data
        spans = td.device_spans.get(tile.device)
        if spans is None:
            # the spans, uploaded once per device (three int32 per span; an empty ring has none)
            import torch
            host = td.spans.reshape(-1) if td.spans.size else np.zeros(3, np.int32)
            spans = td.device_spans[tile.device] = torch.from_numpy(host.copy()).to(f'cuda:{tile.device}')
        width = int(self.meta.dataset_shape.sig[-1])
        hip.ring_moments(tile.device, tile.data_ptr(), tile.dtype, tile.shape[0], width, tile.ld,
                         spans.data_ptr(), len(td.spans), td.n_ring, out.data_ptr(),
                         stream=self.meta.stream_ptr)

    def get_dist_merge(self):
        return {'intensity': 'disjoint'}


def run_fem(ctx, dataset, center, rad_in, rad_out, roi=None):
    """
    The standard deviation of the ring pixels of every frame (udf/FEM.py:69-96); the result's
    'intensity' buffer holds it.
    """
    udf = FEMUDF(center=center, rad_in=rad_in, rad_out=rad_out)
    return ctx.run_udf(dataset=dataset, udf=udf, roi=roi)
