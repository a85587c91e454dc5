"""
StdDevUDF on MI355X: per-pixel sum, variance, standard deviation and mean over all frames.
Drop-in for the reference's libertem.udf.stddev (StdDevUDF, run_stddev, consolidate_result;
udf/stddev.py:198-530).

The moments are merged with the one-pass, numerically stable update of Schubert & Gertz (2018):
for two sets a, b of n_a, n_b frames with sums S and sums of squared deviations V,

    delta = mean_b - mean_a,  mean = mean_a + n_b delta / (n_a + n_b),
    V = V_a + V_b + n_b |delta| |mean_b - mean|,   S = S_a + S_b.

On the device one tile is folded into the running buffers by `ltmi_moments_frames` (float64
moments per slab of frames, slabs merged in a fixed order); on a CPU executor by the same
arithmetic in NumPy.  Partition results are merged on the host with the same update.
"""
from collections import defaultdict

import numpy as np

from libertem_amd.common.buffers import HipSigView
from libertem_amd.udf.base import UDF
from libertem_amd.udf.device import SigSlice, Workspace, check_device_args, runs_on_hip


def _merge_moments(dest_n, dest_sum, dest_varsum, src_n, src_sum, src_varsum):
    """Merge the moments of src into dest in place (arrays of one shape); -> the new frame count
    (udf/stddev.py:66-100, :171-208).  Empty sets (zero frames: ROI, sync offset) merge as the identity."""
    if src_n == 0:
        return dest_n
    if dest_n == 0:
        dest_sum[:] = src_sum
        dest_varsum[:] = src_varsum
        return src_n
    n = dest_n + src_n
    mean_0 = dest_sum / dest_n
    mean_1 = src_sum / src_n
    delta = mean_1 - mean_0
    mean = mean_0 + (src_n * delta) / n
    partial_delta = mean_1 - mean
    dest_sum += src_sum
    dest_varsum += src_varsum + src_n * np.abs(delta) * np.abs(partial_delta)
    return n


def _validate_n(num_frames):
    """the frame count every sig slice of a partition saw (udf/stddev.py:261-268)"""
    if len(num_frames) == 0:
        return 0
    values = tuple(num_frames.values())
    if not all(v == values[0] for v in values):
        raise AssertionError(f"sig slices of a partition saw different frame counts: {num_frames}")
    return values[0]


class StdDevUDF(UDF):
    """
    Sum of frames, sum of squared deviations from the mean, variance, standard deviation and mean
    of every pixel over all frames (one pass; Schubert & Gertz 2018).

    Parameters
    ----------
    dtype : numpy.dtype, optional
        Base dtype of the variance buffers, default float64.  `sum` and `mean` have
        `numpy.result_type(input dtype, dtype)`.
    use_numba : bool
        Accepted for compatibility with the reference; it changes nothing here.

    Results: 'varsum' (variance times number of frames), 'num_frames', 'sum', 'var', 'std', 'mean'.
    """

    REUSE_TASK_INSTANCES = True      # (frame counters restart in preprocess)
    #: positions a sync_offset leaves without a frame are not delivered on the device either: zero
    #: frames there would change the mean, the variance and the frame count
    #: (udf/base.py `_skips_frameless`; under a dark frame that holds for every UDF, flag or not)
    VALID_FRAMES_ONLY = True

    def __init__(self, dtype=None, use_numba=True):
        super().__init__(dtype=dtype, use_numba=use_numba)

    def get_preferred_input_dtype(self):
        # the frames as they are stored: the kernel converts in registers, and sum / mean take
        # result_type(stored dtype, base) -- the same dtypes as the reference's float32 tiles give
        return self.USE_NATIVE_DTYPE

    def get_backends(self):
        # BACKEND_HIP on an MI355X worker, NumPy on a CPU executor (the executor's device class decides)
        return (self.BACKEND_HIP, self.BACKEND_NUMPY)

    def _base_dtype(self):
        return np.dtype(np.float64 if self.params.dtype is None else self.params.dtype)

    def get_result_buffers(self):
        base = self._base_dtype()
        dtype = np.result_type(self.meta.input_dtype, base)
        return {
            'varsum': self.buffer(kind='sig', dtype=base, where='device'),
            'num_frames': self.buffer(kind='single', dtype='int64'),
            'sum': self.buffer(kind='sig', dtype=dtype, where='device'),
            'var': self.buffer(kind='sig', dtype=base, use='result_only'),
            'std': self.buffer(kind='sig', dtype=base, use='result_only'),
            'mean': self.buffer(kind='sig', dtype=dtype, use='result_only'),
        }

    def get_task_data(self):
        if runs_on_hip(self):
            base, idt = self._base_dtype(), np.dtype(self.meta.input_dtype)
            if base.kind != 'f' or idt.kind not in 'fciu' or (idt.kind in 'iu' and idt.itemsize > 4):
                raise NotImplementedError(
                    f"StdDevUDF on MI355X: input dtype {idt} with base dtype {base} is not supported "
                    "(float32 / float64 base; 8- to 32-bit integer, float or complex frames)")
        return {'num_frames': defaultdict(int), 'workspace': Workspace()}

    def preprocess(self):
        # kept task instances run again: the frame counters belong to one run (the instance on
        # the main process that plans the run has no task data)
        if self.task_data is not None:
            self.task_data.num_frames.clear()

    def postprocess(self):
        self.results.num_frames[:] = _validate_n(self.task_data.num_frames)

    # --- tiles ---------------------------------------------------------------------------------------
    def process_tile(self, tile):
        key = self.meta.tiling_scheme_idx
        n_0 = self.task_data.num_frames[key]
        n_1 = tile.shape[0]
        if n_1 == 0:
            return
        if self.meta.array_backend == self.BACKEND_NUMPY:
            self._process_tile_numpy(tile, n_0)
        else:
            self._process_tile_hip(tile, n_0)
        self.task_data.num_frames[key] = n_0 + n_1

    def _process_tile_numpy(self, tile, n_0):
        # the reference's ndarray algorithm (udf/stddev.py:153-168, :425-451), in the sum dtype
        dtype = np.dtype(self.results.sum.dtype)
        tile = np.asarray(tile)
        if tile.dtype != dtype:
            tile = tile.astype(dtype)
        n_1 = tile.shape[0]
        out_sum, out_var = self.results.sum, self.results.varsum
        tsum = tile.sum(axis=0)
        delta = np.abs(tile - tsum / n_1)
        tvar = np.sum(np.multiply(delta, delta), axis=0).real
        tsum, tvar = tsum.reshape(out_sum.shape), tvar.reshape(out_var.shape)
        if n_0 == 0:
            out_sum[:] = tsum
            out_var[:] = tvar
        else:
            _merge_moments(n_0, out_sum, out_var, n_1, tsum, tvar)

    def _process_tile_hip(self, tile, n_0):
        from libertem_amd import hip
        sv, vv = self.results.sum, self.results.varsum
        check_device_args(self, tile, sv, vv, kind=HipSigView)
        s_arr, v_arr = sv.array, vv.array
        n = tile.shape[0]
        device = tile.device
        sz, vz, tz = s_arr.dtype.itemsize, v_arr.dtype.itemsize, np.dtype(tile.dtype).itemsize
        # a partial-width sig slice: the kernel writes the strided sub-rectangle of the buffers
        # directly (rows of `cols` pixels at stride ld_out), one launch per block
        for tile_off, n_px, out_off, cols, ld_out in SigSlice(sv, self.meta.dataset_shape.sig).blocks():
            ws = self.task_data.workspace.ptr(device, hip.moments_workspace(n, n_px, tile.dtype))
            hip.moments_frames(device, tile.data_ptr() + tile_off * tz, tile.dtype, n, n_px, tile.ld, n_0,
                               s_arr.data_ptr() + out_off * sz, s_arr.dtype,
                               v_arr.data_ptr() + out_off * vz, v_arr.dtype, ws,
                               cols=cols, ld_out=ld_out)

    # --- merge ---------------------------------------------------------------------------------------
    def merge(self, dest, src):
        n = _merge_moments(int(dest.num_frames[0]), dest.sum, dest.varsum,
                           int(src.num_frames[0]), src.sum, src.varsum)
        dest.num_frames[:] = n

    def merge_all(self, ordered_results):
        # the partitions in order, with the same update as `merge`: both give the same numbers
        parts = list(ordered_results.values())
        total = np.array(parts[0].sum, copy=True)
        varsum = np.array(parts[0].varsum, copy=True)
        n = int(parts[0].num_frames[0])
        for b in parts[1:]:
            n = _merge_moments(n, total, varsum, int(b.num_frames[0]), b.sum, b.varsum)
        return {'sum': total, 'varsum': varsum, 'num_frames': n}

    def get_results(self):
        num_frames = self.results.num_frames[0]
        var = self.results.varsum / num_frames
        return {
            'var': var,
            'std': np.sqrt(var),
            'mean': self.results.sum / num_frames,
        }


def consolidate_result(udf_result):
    """
    The results of a StdDevUDF run as plain arrays, the frame count as a number
    (udf/stddev.py:470-500): keys 'num_frames', 'varsum', 'sum', 'var', 'std', 'mean'.
    """
    return {
        'num_frames': udf_result['num_frames'].data[0],
        'varsum': udf_result['varsum'].data,
        'sum': udf_result['sum'].data,
        'var': udf_result['var'].data,
        'std': udf_result['std'].data,
        'mean': udf_result['mean'].data,
    }


def run_stddev(ctx, dataset, roi=None, progress=False, use_numba=True):
    """
    Run StdDevUDF on `dataset` and return `consolidate_result` of it (udf/stddev.py:503-530).
    """
    res = ctx.run_udf(dataset=dataset, udf=StdDevUDF(use_numba=use_numba), roi=roi, progress=progress)
    return consolidate_result(res)
