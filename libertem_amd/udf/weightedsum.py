"""
WeightedSumUDF on MI355X: a handful of weighted sums of all frames, wsum[c] = sum_n weights[n, c] * frame[n].

The transposed mask product: ApplyMasksUDF reduces every frame against k masks (frames x mask stack), this
UDF reduces the scan against k weight maps (weights^T x frames).  SumUDF is its one-column case with every
weight 1; soft regions of a scan, the B = Q^T X passes of a randomized PCA (`libertem_amd.udf.pca`) and
the updates of NMF / k-means are others.  Not in the reference.

On the device `ltmi_wsum_frames` folds a tile of whole frames into the float32 buffer: exact float32 FMAs on
the matrix cores per slab of frames, the slabs merged in float64 in a fixed order.  On a CPU executor NumPy
computes the same product in float64.
"""
import numpy as np

from libertem_amd.common.buffers import AuxBufferWrapper
from libertem_amd.common.hiparray import HipArray
from libertem_amd.common.math import prod
from libertem_amd.udf.base import UDF
from libertem_amd.udf.device import Workspace, check_device_args, check_whole_frames, quiet_floats, runs_on_hip


def nav_weights(weights, nav_shape):
    """`weights` of shape nav + (k,), nav (one component), or the same with a flat nav axis -> float32 (N, k)"""
    nav_shape = tuple(int(s) for s in nav_shape)
    n = prod(nav_shape)
    arr = np.asarray(weights)
    if arr.dtype.kind not in 'fiub':
        raise TypeError(f"WeightedSumUDF: weights of dtype {arr.dtype} are not real numbers")
    if arr.shape in (nav_shape, (n,)):
        return np.ascontiguousarray(arr.reshape((n, 1)), dtype=np.float32)
    if arr.ndim >= 1 and arr.shape[:-1] in (nav_shape, (n,)) and arr.shape[-1] >= 1:
        return np.ascontiguousarray(arr.reshape((n, arr.shape[-1])), dtype=np.float32)
    raise ValueError(f"WeightedSumUDF: weights of shape {arr.shape} fit neither the scan {nav_shape} "
                     f"nor {nav_shape + ('k',)}")


class WeightedSumUDF(UDF):
    """
    Weighted sums of all frames: result 'wsum' of shape (k,) + sig (float32),
    wsum[c] = sum over the scan positions n of weights[n, c] * frame[n].

    Parameters
    ----------
    weights : array of shape nav + (k,), or nav for one component, or
        `WeightedSumUDF.aux_data(w, kind='nav', extra_shape=(k,), dtype='float32')`.  The weights are given for
        the whole scan; under a region of interest the rows of the selected positions are used.
    """

    REUSE_TASK_INSTANCES = True
    #: positions a sync_offset leaves without a frame add nothing (the same rule as the other frame statistics)
    VALID_FRAMES_ONLY = True
    WHOLE_FRAME_TILES = True

    def __init__(self, weights):
        super().__init__(weights=weights)

    @classmethod
    def new_for_partition(cls, kwargs, partition, roi):
        # plain arrays become nav aux data here, where the scan's shape is known: sliced per partition and roi as
        # the reference slices aux data (AuxBufferWrapper.new_for_partition)
        w = kwargs['weights']
        if not isinstance(w, AuxBufferWrapper):
            flat = nav_weights(w, partition.meta.shape.nav)
            kwargs = dict(kwargs, weights=cls.aux_data(flat, kind='nav', extra_shape=(flat.shape[1],),
                                                       dtype='float32'))
        return super().new_for_partition(kwargs, partition, roi)

    def get_preferred_input_dtype(self):
        # the frames as stored: the kernel converts in registers
        return self.USE_NATIVE_DTYPE

    def get_backends(self):
        return (self.BACKEND_HIP, self.BACKEND_NUMPY)

    def _n_components(self):
        w = self._kwargs['weights']
        if isinstance(w, AuxBufferWrapper):
            if w.kind != 'nav' or len(w.extra_shape) > 1:
                raise ValueError("WeightedSumUDF: aux weights must be kind='nav' with extra_shape (k,) or ()")
            return int(w.extra_shape[0]) if w.extra_shape else 1
        return nav_weights(w, self.meta.dataset_shape.nav).shape[1]

    def get_result_buffers(self):
        sig = tuple(self.meta.dataset_shape.sig)
        return {'wsum': self.buffer(kind='single', extra_shape=(self._n_components(),) + sig, dtype='float32',
                                    where='device')}

    def get_task_data(self):
        dt = np.dtype(self.meta.input_dtype)
        check_whole_frames(self)
        if runs_on_hip(self):
            if dt.kind not in 'fiub' or dt.itemsize > 4 or (dt.kind == 'f' and dt.itemsize != 4):
                raise NotImplementedError(f"WeightedSumUDF on MI355X: input dtype {dt} is not supported")
        elif dt.kind == 'c':
            raise NotImplementedError(f"WeightedSumUDF: complex input ({dt}) is not supported")
        # 'weights': the partition's weight rows on the device, uploaded with its first tile
        return {'workspace': Workspace(), 'weights': {}}

    def _partition_rows(self):
        """-> (the partition's weight rows (n, k) float32 on the host, first row of the current tile in them)"""
        buf = self.params.get_buffer('weights')
        rows = np.asarray(buf.get_view_for_partition(None))
        rows = rows.reshape((rows.shape[0], -1))
        start = self.meta.slice.origin[0] - self.meta._partition_slice.origin[0]
        return rows, int(start)

    def process_tile(self, tile):
        n = tile.shape[0]
        if n == 0:
            return
        rows, start = self._partition_rows()
        if not 0 <= start <= start + n <= rows.shape[0]:
            raise RuntimeError(f"WeightedSumUDF: tile rows [{start}, {start + n}) outside the partition's "
                               f"{rows.shape[0]} weight rows")
        if self.meta.array_backend == self.BACKEND_NUMPY:
            self._process_tile_numpy(tile, rows[start:start + n])
        else:
            self._process_tile_hip(tile, rows, start)

    def _process_tile_numpy(self, tile, w):
        tile = np.asarray(tile)
        if tile.dtype.kind == 'c':
            raise NotImplementedError(f"WeightedSumUDF: complex input ({tile.dtype}) is not supported")
        flat = tile.reshape((tile.shape[0], -1))
        out = self.results.wsum
        with quiet_floats():
            total = w.T.astype(np.float64) @ flat.astype(np.float64)
            out[:] = out + total.reshape(out.shape)

    def _process_tile_hip(self, tile, rows, start):
        from libertem_amd import hip
        out = self.results.wsum
        check_device_args(self, tile, out)
        n, k = tile.shape[0], rows.shape[1]
        n_px = prod(tile.shape[1:])
        if tuple(out.shape) != (k,) + tuple(tile.shape[1:]) or not out.is_contiguous:
            raise ValueError(f"WeightedSumUDF needs whole frames: tile {tile.shape}, buffer {out.shape}")
        held, buf = self.task_data.weights, self.params.get_buffer('weights')
        if held.get('of') is not buf:
            # once per partition (kept task instances: once per instance, the rows are the same every run)
            held['of'] = buf
            held['dev'] = HipArray.from_numpy(np.ascontiguousarray(rows, dtype=np.float32), tile.device)
        w_dev = held['dev']
        for c0 in range(0, k, hip.WSUM_MAX_K):
            kc = min(hip.WSUM_MAX_K, k - c0)
            ws = self.task_data.workspace.ptr(tile.device, hip.wsum_workspace(n, n_px, kc))
            hip.wsum_frames(tile.device, tile.data_ptr(), tile.dtype, n, n_px, tile.ld,
                            w_dev.data_ptr() + (start * k + c0) * 4, kc, k,
                            out.data_ptr() + c0 * out.ld * 4, out.ld, True, ws, stream=self.meta.stream_ptr)

    def merge(self, dest, src):
        dest.wsum[:] += src.wsum[:]

    def merge_all(self, ordered_results):
        # the partitions in order, as `merge` adds them: both give the same numbers
        parts = [b.wsum for b in ordered_results.values()]
        total = np.zeros_like(np.asarray(parts[0]))
        for p in parts:
            total += p
        return {'wsum': total}

    def get_dist_merge(self):
        return {'wsum': 'sum'}


def run_weighted_sum(ctx, dataset, weights, roi=None):
    """
    Weighted sums of the frames of `dataset`: result 'wsum' (k,) + sig, wsum[c] = sum_n weights[n, c] * frame[n].
    """
    return ctx.run_udf(dataset=dataset, udf=WeightedSumUDF(weights), roi=roi)
