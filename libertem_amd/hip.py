"""
ctypes binding of libltmi.so (include/ltmi.h) -- the only way the product reaches the GPU.

There is deliberately NO CPU fallback anywhere in this module: if the shared library is
missing or a call fails, a `RuntimeError` / `ValueError` is raised.
"""
import ctypes
import enum
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
#: LTMI_LIB selects another build of the same library (the AddressSanitizer host build of
#: `python -m libertem_amd.build --asan`); there is no other implementation to select
LIB_PATH = os.environ.get('LTMI_LIB') or os.path.join(_HERE, '_lib', 'libltmi.so')

_lib = None
_lock = threading.Lock()

# numpy dtype -> enum ltmi_dtype (include/ltmi.h)
_DTYPES = {
    np.dtype('bool'): 0, np.dtype('uint8'): 1, np.dtype('int8'): 2, np.dtype('uint16'): 3,
    np.dtype('int16'): 4, np.dtype('uint32'): 5, np.dtype('int32'): 6, np.dtype('uint64'): 7,
    np.dtype('int64'): 8, np.dtype('float32'): 9, np.dtype('float64'): 10,
    np.dtype('complex64'): 11, np.dtype('complex128'): 12,
}


class Variant(enum.IntEnum):
    """enum ltmi_variant (include/ltmi.h): the kernel-variant codes of `MaskHandle.set_tuning(0, code, ksplit)`"""
    NONE = 0
    DENSE_DEFAULT = 30
    DENSE_NO_DMA = 31
    DENSE_NO_MFMA = 32
    DENSE_PADDED_GROUPS = 33
    DENSE_ONE_TILE = 34
    DENSE_TWO_TILES = 35
    DENSE_SPLIT_BF16 = 36
    DENSE_F32_INSTR = 37
    DENSE_UNFOLDED = 38
    SPARSE_DEFAULT = 40
    SPARSE_SELL = 41
    SPARSE_NO_SCATTER = 42


EXPORTS = (
    'ltmi_version', 'ltmi_last_error', 'ltmi_device_count', 'ltmi_device_info',
    'ltmi_masks_create_dense', 'ltmi_masks_create_csr', 'ltmi_masks_destroy', 'ltmi_masks_kind', 'ltmi_masks_set_sig_shape',
    'ltmi_masks_set_sparse_origin', 'ltmi_masks_set_dense_origin', 'ltmi_masks_create_csr_gather',
    'ltmi_masks_nonfinite_frames',
    'ltmi_apply_masks', 'ltmi_apply_masks_rows', 'ltmi_apply_masks_shifted', 'ltmi_apply_masks_shifted_host', 'ltmi_sum_frames_workspace', 'ltmi_sum_frames', 'ltmi_sum_sig',
    'ltmi_moments_workspace', 'ltmi_moments_frames', 'ltmi_ring_moments', 'ltmi_logsum_workspace',
    'ltmi_logsum_frames', 'ltmi_wsum_workspace', 'ltmi_wsum_frames',
    'ltmi_axpy', 'ltmi_add2d', 'ltmi_gather_rows', 'ltmi_host_device_pointer', 'ltmi_host_copy', 'ltmi_correct', 'ltmi_repair_pixels', 'ltmi_byteswap', 'ltmi_mib_decode', 'ltmi_mib_last_kernel', 'ltmi_k2is_decode', 'ltmi_frms6_decode', 'ltmi_frms6_last_kernel', 'ltmi_records_gather', 'ltmi_records_last_kernel', 'ltmi_transpose2d', 'ltmi_transpose_last_kernel', 'ltmi_com_fields', 'ltmi_fft_plan_create',
    'ltmi_fft_plan_destroy', 'ltmi_crystallinity', 'ltmi_crystallinity_corrected', 'ltmi_fft_plan_last_kernel',
    'ltmi_corr_plan_create', 'ltmi_corr_plan_destroy', 'ltmi_correlate_peaks', 'ltmi_corr_plan_last_kernel',
    'ltmi_lattice_fit', 'ltmi_lattice_last_kernel',
    'ltmi_find_peaks_maps', 'ltmi_find_peaks_last_kernel', 'ltmi_correlate_find',
    'ltmi_count_events', 'ltmi_store_events', 'ltmi_count_strip_rows', 'ltmi_count_last_kernel',
    'ltmi_orient_plan_create', 'ltmi_orient_plan_destroy', 'ltmi_orient_match', 'ltmi_orient_polar',
    'ltmi_orient_plan_last_kernel', 'ltmi_orient_max_polar_words', 'ltmi_orient_score_block',
    'ltmi_holo_plan_create', 'ltmi_holo_plan_destroy', 'ltmi_holo_reconstruct', 'ltmi_holo_plan_last_kernel',
    'ltmi_holo_crop',
    'ltmi_ceps_plan_create', 'ltmi_ceps_plan_destroy', 'ltmi_ceps_transform', 'ltmi_ceps_plan_last_kernel',
    'ltmi_ceps_load', 'ltmi_ceps_store',
    'ltmi_ssb_gather', 'ltmi_ssb_plan_create', 'ltmi_ssb_plan_destroy', 'ltmi_ssb_reconstruct',
    'ltmi_ssb_plan_last_kernel', 'ltmi_ssb_trotter',
    'ltmi_wdd_filter', 'ltmi_wdd_dot', 'ltmi_wdd_finish', 'ltmi_wdd_plan_create', 'ltmi_wdd_plan_destroy',
    'ltmi_wdd_reconstruct', 'ltmi_wdd_plan_last_kernel',
    'ltmi_plx_ramps', 'ltmi_plx_sum', 'ltmi_plx_mul', 'ltmi_plx_peaks', 'ltmi_plx_plan_create', 'ltmi_plx_plan_destroy',
    'ltmi_plx_plan_load', 'ltmi_plx_plan_iterate', 'ltmi_plx_plan_sum', 'ltmi_plx_plan_last_kernel',
    'ltmi_csr_check', 'ltmi_csr_densify', 'ltmi_apply_masks_csr', 'ltmi_csr_max_masks',
    'ltmi_csr_sum_sig', 'ltmi_csr_sum_frames_workspace', 'ltmi_csr_sum_frames', 'ltmi_csr_last_kernel',
    'ltmi_masks_set_tuning',
    'ltmi_masks_last_kernel', 'ltmi_comm_unique_id', 'ltmi_comm_create', 'ltmi_comm_destroy',
    'ltmi_comm_all_gather', 'ltmi_comm_all_reduce_sum', 'ltmi_comm_library_info',
)


class LtmiError(RuntimeError):
    pass


class ReplayMismatch(RuntimeError):
    """a run did not issue the launch that was enqueued ahead for it (LaunchReplay): the caller drops the
    recorded launch, plans afresh and runs again -- nothing of the abandoned run is delivered"""


class ReplayState:
    """the launch-ahead state of ONE executor (`HipJobExecutor.replay`): `expected` = the launches that were
    enqueued ahead for the run in progress (None: none), `recording` = list that collects the launches of the
    task that is running (None: not recording)"""
    __slots__ = ('expected', 'recording')

    def __init__(self):
        self.expected = None
        self.recording = None


class RunInProgressError(RuntimeError):
    """a run was started on an executor whose `run_udf_iter` is suspended between two partial results"""


class RunGate:
    """Serialises the runs of one executor (its delivery targets, launch-ahead state and streams belong to the
    run in progress): re-entrant for the thread that holds it, and -- unlike threading.RLock -- releasable from
    another thread (a generator of partial results that is closed by the garbage collector).

    A `run_udf_iter` holds the gate from its first step to its end, also while it is suspended at a `yield`
    (`suspended` is set then): the executor's per-run state belongs to it.  Another run on the same executor in
    that window -- from the loop body, from the event loop of an `async for`, from any thread -- can neither wait
    (it would wait for ever: the iteration only resumes when its consumer asks for the next part) nor go ahead
    (it would reuse the suspended run's state), so `acquire` raises RunInProgressError instead."""

    def __init__(self):
        self._lock = threading.Lock()
        self._owner = None
        self._depth = 0
        self.suspended = None        # what is suspended (a string for the message) or None

    def _refuse(self):
        raise RunInProgressError(
            f"{self.suspended} of this context is suspended between two partial results and owns the executor: "
            "consume or close() the iterator before starting another run on the same Context "
            "(or run it on a second Context)")

    def acquire(self):
        me = threading.get_ident()
        if self._owner == me:
            if self.suspended:
                self._refuse()
            self._depth += 1
            return
        while not self._lock.acquire(timeout=0.05):
            if self.suspended:
                self._refuse()
        self._owner = me
        self._depth = 1

    def release(self):
        self._depth -= 1
        if self._depth <= 0:
            self._depth = 0
            self._owner = None
            self.suspended = None
            self._lock.release()

    def __enter__(self):
        self.acquire()
        return self

    def __exit__(self, *exc):
        self.release()


class _ReplayMeta(type):
    # `LaunchReplay.expected` / `.recording` are those of the executor whose run is in progress on THIS thread
    # (`LaunchReplay.bound(state)`, entered by Context.run_udf under the executor's gate); outside a run: a state
    # of the thread's own, so that bare handle calls of two threads never see each other's lists
    def _cur(cls):
        st = getattr(cls._tls, 'state', None)
        if st is None:
            st = cls._tls.state = cls._tls.own = ReplayState()
        return st

    @property
    def expected(cls):
        return cls._cur().expected

    @expected.setter
    def expected(cls, v):
        cls._cur().expected = v

    @property
    def recording(cls):
        return cls._cur().recording

    @recording.setter
    def recording(cls, v):
        cls._cur().recording = v


class LaunchReplay(metaclass=_ReplayMeta):
    """
    Launch first, book-keep behind the kernel.  A run of a cached plan (udf/base.py `_plan_for`) whose
    previous run issued exactly ONE `ltmi_apply_masks` launch per task -- same handle, same resident tile,
    result rows written straight into the run's result buffer -- enqueues that launch as soon as the new
    result buffer exists (executor/hip.py `merge_results`), then runs the normal tile loop: the tile loop's
    own call finds itself in `expected` and returns.  A different call raises ReplayMismatch.
    The state (`expected`, `recording`: ReplayState) belongs to the EXECUTOR; a run binds it to its thread
    for its duration, runs of one executor are serialised by the executor's RunGate.
    """
    _tls = threading.local()
    n_ahead = 0          # launches enqueued ahead so far, all executors (tests, bench)

    class bound:
        """context manager: the calling thread's launches are matched against / recorded into `state`"""

        def __init__(self, state):
            self.state = state

        def __enter__(self):
            tls = LaunchReplay._tls
            self.prev = getattr(tls, 'state', None)
            tls.state = self.state
            return self.state

        def __exit__(self, *exc):
            LaunchReplay._tls.state = self.prev

    @staticmethod
    def signature(handle, tile_ptr, tile_dtype, n_frames, ld_tile, out_ptr, ld_out, accumulate, stream):
        return (id(handle), int(tile_ptr), np.dtype(tile_dtype).str, int(n_frames), int(ld_tile), int(out_ptr),
                int(ld_out), bool(accumulate), stream if isinstance(stream, int) else _stream_ptr(stream))


class KernelTimer:
    """
    Optional HIP-event timing of every `ltmi_apply_masks` launch, on the stream the kernel is
    launched on (bench.py's `roofline.achieved`).  Off by default: zero overhead.
    """
    enabled = False
    events = []

    @classmethod
    def start(cls):
        cls.enabled = True
        cls.events = []

    @classmethod
    def stop(cls):
        """-> list of (milliseconds, n_frames, kernel name); synchronises."""
        import torch
        cls.enabled = False
        torch.cuda.synchronize()
        out = [(a.elapsed_time(b), n, k) for a, b, n, k in cls.events]
        cls.events = []
        return out


def dtype_code(dtype):
    try:
        return _DTYPES[np.dtype(dtype)]
    except KeyError:
        raise ValueError(f"dtype {dtype!r} is not supported by libltmi")


def lib():
    """Load libltmi.so once.  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP library has not been built. "
                "Run `python -m libertem_amd.build` (needs hipcc). There is no CPU fallback."
            )
        # torch bundles its own libamdhip64 (soname libamdhip64.so.7, NEEDED by torch under the
        # unversioned name).  It has to be in the process BEFORE libltmi so that libltmi's
        # DT_NEEDED libamdhip64.so.7 binds to the same runtime instance; two HIP runtimes in one
        # process cannot share device pointers (and the second one sees no devices).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        c = ctypes
        vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int
        L.ltmi_version.restype = i32
        L.ltmi_last_error.restype = c.c_char_p
        L.ltmi_device_count.argtypes = [c.POINTER(i32)]
        L.ltmi_device_info.argtypes = [i32, c.c_char_p, c.POINTER(i32), c.POINTER(i64),
                                       c.POINTER(i32)]
        L.ltmi_masks_create_dense.argtypes = [i32, vp, i32, i64, i64, c.POINTER(vp)]
        L.ltmi_masks_create_csr.argtypes = [i32, vp, vp, vp, i32, i64, i64, c.POINTER(vp)]
        L.ltmi_masks_create_csr_gather.argtypes = [i32, vp, vp, vp, i32, i64, i64, c.POINTER(vp)]
        L.ltmi_masks_destroy.argtypes = [vp]
        L.ltmi_apply_masks_rows.argtypes = [vp, vp, i32, vp, i64, i64, vp, i64, i32, vp,
                                            c.POINTER(i32)]
        L.ltmi_masks_kind.argtypes = [vp, c.POINTER(i32)]
        L.ltmi_masks_set_sig_shape.argtypes = [vp, i32, i32]
        L.ltmi_masks_set_sparse_origin.argtypes = [vp, vp]
        L.ltmi_masks_set_dense_origin.argtypes = [vp, vp, vp]
        L.ltmi_masks_nonfinite_frames.argtypes = [vp, vp, c.POINTER(i64)]
        L.ltmi_apply_masks.argtypes = [vp, vp, i32, i64, i64, vp, i64, i32, vp]
        L.ltmi_apply_masks_shifted.argtypes = [vp, vp, i32, i64, i64, i32, i32, vp, vp, i64, i32, vp]
        L.ltmi_apply_masks_shifted_host.argtypes = [vp, vp, i32, i64, i64, i32, i32, vp, vp, i64, i32, vp]
        L.ltmi_sum_frames_workspace.argtypes = [i64, i64, i32]
        L.ltmi_sum_frames_workspace.restype = i64
        L.ltmi_sum_frames.argtypes = [i32, vp, i32, i64, i64, i64, vp, i32, i32, vp, vp]
        L.ltmi_sum_sig.argtypes = [i32, vp, i32, i64, i64, i64, vp, i32, i32, vp]
        L.ltmi_moments_workspace.argtypes = [i64, i64, i32]
        L.ltmi_moments_workspace.restype = i64
        L.ltmi_moments_frames.argtypes = [i32, vp, i32, i64, i64, i64, i64, vp, i32, vp, i32, i64, i64, vp, vp]
        L.ltmi_ring_moments.argtypes = [i32, vp, i32, i64, i64, i64, vp, i32, i64, vp, vp]
        L.ltmi_logsum_workspace.argtypes = [i64, i64, i32]
        L.ltmi_logsum_workspace.restype = i64
        L.ltmi_logsum_frames.argtypes = [i32, vp, i32, i64, i64, i64, vp, i64, i64, vp, vp]
        L.ltmi_wsum_workspace.argtypes = [i64, i64, i32]
        L.ltmi_wsum_workspace.restype = i64
        L.ltmi_wsum_frames.argtypes = [i32, vp, i32, i64, i64, i64, vp, i32, i64, vp, i64, i64, i64, i32, vp, vp]
        L.ltmi_axpy.argtypes = [i32, vp, vp, i32, i64, vp]
        L.ltmi_add2d.argtypes = [i32, vp, i64, vp, i64, i32, i64, i64, i32, vp]
        L.ltmi_gather_rows.argtypes = [i32, vp, i64, vp, i64, i64, vp, vp]
        L.ltmi_host_device_pointer.argtypes = [i32, vp, c.POINTER(vp)]
        L.ltmi_host_copy.argtypes = [vp, vp, i64, i32]
        L.ltmi_correct.argtypes = [i32, vp, i32, i64, i64, i64, vp, vp, vp, i32, i64, vp]
        L.ltmi_repair_pixels.argtypes = [i32, vp, i32, i64, i64, vp, vp, vp, i32, i32, vp]
        L.ltmi_byteswap.argtypes = [i32, vp, vp, i32, i64, vp]
        L.ltmi_mib_decode.argtypes = [i32, vp, i64, i64, i32, i32, i32, i64, i32, i32, vp, i32, vp]
        L.ltmi_mib_last_kernel.argtypes = []
        L.ltmi_k2is_decode.argtypes = [i32, vp, i64, vp, i32, vp]
        L.ltmi_frms6_decode.argtypes = [i32, vp, i64, i64, i32, i32, i32, vp, i32, vp]
        L.ltmi_frms6_last_kernel.argtypes = []
        L.ltmi_frms6_last_kernel.restype = c.c_char_p
        L.ltmi_records_gather.argtypes = [i32, vp, i64, i64, i64, vp, vp]
        L.ltmi_records_last_kernel.argtypes = []
        L.ltmi_records_last_kernel.restype = c.c_char_p
        L.ltmi_transpose2d.argtypes = [i32, vp, i64, i64, i64, i32, vp, i64, vp]
        L.ltmi_transpose_last_kernel.argtypes = []
        L.ltmi_transpose_last_kernel.restype = c.c_char_p
        L.ltmi_mib_last_kernel.restype = c.c_char_p
        L.ltmi_com_fields.argtypes = [i32, vp, i64, i32, i32, ctypes.c_double, ctypes.c_double, vp, vp,
                                      vp, vp, vp, vp, vp]
        L.ltmi_fft_plan_create.argtypes = [i32, i32, i32, i32, c.POINTER(vp)]
        L.ltmi_fft_plan_destroy.argtypes = [vp]
        L.ltmi_crystallinity.argtypes = [vp, vp, i32, i64, i64, vp, vp, i32, i32, i32, vp, i32, vp]
        L.ltmi_crystallinity_corrected.argtypes = [vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, i32, i32,
                                                   vp, vp, i32, i32, i32, vp, i32, vp]
        L.ltmi_csr_check.argtypes = [i32, vp, vp, i64, i64, i64, vp, vp]
        L.ltmi_csr_densify.argtypes = [i32, vp, vp, vp, i32, vp, i64, i64, i64, vp, i64, vp]
        L.ltmi_apply_masks_csr.argtypes = [vp, vp, vp, vp, i32, vp, i64, i64, vp, i64, i32, vp, c.POINTER(i32)]
        L.ltmi_csr_max_masks.argtypes = []
        L.ltmi_csr_sum_sig.argtypes = [i32, vp, vp, vp, i32, vp, i64, i64, i64, vp, i32, i32, vp]
        L.ltmi_csr_sum_frames_workspace.argtypes = [i64]
        L.ltmi_csr_sum_frames_workspace.restype = i64
        L.ltmi_csr_sum_frames.argtypes = [i32, vp, vp, vp, i32, vp, i64, i64, i64, vp, i32, i32, vp, vp]
        L.ltmi_csr_last_kernel.argtypes = []
        L.ltmi_csr_last_kernel.restype = c.c_char_p
        L.ltmi_masks_set_tuning.argtypes = [vp, i32, i32, i32]
        L.ltmi_masks_last_kernel.argtypes = [vp]
        L.ltmi_comm_unique_id.argtypes = [vp]
        L.ltmi_comm_create.argtypes = [i32, i32, i32, vp, c.POINTER(vp)]
        L.ltmi_comm_destroy.argtypes = [vp]
        L.ltmi_comm_all_gather.argtypes = [vp, vp, vp, i64, vp]
        L.ltmi_comm_all_reduce_sum.argtypes = [vp, vp, i32, i64, vp]
        L.ltmi_comm_library_info.argtypes = [ctypes.c_char_p, i64, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.ltmi_masks_last_kernel.restype = c.c_char_p
        L.ltmi_fft_plan_last_kernel.argtypes = [vp]
        L.ltmi_fft_plan_last_kernel.restype = c.c_char_p
        L.ltmi_corr_plan_create.argtypes = [i32, i32, i32, i32, vp, c.POINTER(vp)]
        L.ltmi_corr_plan_destroy.argtypes = [vp]
        L.ltmi_correlate_peaks.argtypes = [vp, vp, i32, i64, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp]
        L.ltmi_corr_plan_last_kernel.argtypes = [vp]
        L.ltmi_corr_plan_last_kernel.restype = c.c_char_p
        L.ltmi_lattice_fit.argtypes = [i32, vp, vp, vp, i64, i32, vp, vp, c.c_double, vp, vp, vp, vp, vp, vp]
        L.ltmi_lattice_last_kernel.argtypes = []
        L.ltmi_lattice_last_kernel.restype = c.c_char_p
        L.ltmi_find_peaks_maps.argtypes = [i32, vp, i64, i32, i32, i64, i32, i32, i32, c.c_float, c.c_float, i32,
                                           vp, vp, vp, vp, vp, vp]
        L.ltmi_find_peaks_last_kernel.argtypes = []
        L.ltmi_find_peaks_last_kernel.restype = c.c_char_p
        L.ltmi_correlate_find.argtypes = [vp, vp, i32, i64, i64, i32, i32, i32, c.c_float, c.c_float, i32,
                                          vp, vp, vp, vp, vp, vp]
        L.ltmi_count_events.argtypes = [i32, vp, i32, i64, i32, i32, i64, vp, vp, c.c_float, c.c_float, vp, vp]
        L.ltmi_store_events.argtypes = [i32, vp, i32, i64, i32, i32, i64, vp, vp, c.c_float, c.c_float, vp, i64, i64,
                                        vp, vp, i32, vp, vp]
        L.ltmi_count_strip_rows.argtypes = [i32, i32]
        L.ltmi_count_last_kernel.argtypes = []
        L.ltmi_count_last_kernel.restype = c.c_char_p
        L.ltmi_orient_plan_create.argtypes = [i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, i32, c.POINTER(vp)]
        L.ltmi_orient_plan_destroy.argtypes = [vp]
        L.ltmi_orient_match.argtypes = [vp, vp, i32, i64, i64, vp, vp, vp, vp, vp]
        L.ltmi_orient_polar.argtypes = [vp, vp, i32, i64, i64, vp, i64, vp]
        L.ltmi_orient_plan_last_kernel.argtypes = [vp]
        L.ltmi_orient_plan_last_kernel.restype = c.c_char_p
        L.ltmi_orient_max_polar_words.argtypes = []
        L.ltmi_orient_score_block.argtypes = []
        L.ltmi_holo_plan_create.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, c.POINTER(vp)]
        L.ltmi_holo_plan_destroy.argtypes = [vp]
        L.ltmi_holo_reconstruct.argtypes = [vp, vp, i32, i64, i64, vp, i64, vp]
        L.ltmi_holo_plan_last_kernel.argtypes = [vp]
        L.ltmi_holo_plan_last_kernel.restype = c.c_char_p
        L.ltmi_holo_crop.argtypes = [i32, vp, i64, i32, i32, i64, i32, i32, i32, i32, vp, vp, i64, vp]
        L.ltmi_ceps_plan_create.argtypes = [i32, i32, i32, i32, i32, i32, c.c_float, vp, c.c_double, c.POINTER(vp)]
        L.ltmi_ceps_plan_destroy.argtypes = [vp]
        L.ltmi_ceps_transform.argtypes = [vp, vp, i32, i64, i64, vp, i64, vp]
        L.ltmi_ceps_plan_last_kernel.argtypes = [vp]
        L.ltmi_ceps_plan_last_kernel.restype = c.c_char_p
        L.ltmi_ceps_load.argtypes = [i32, vp, i32, i64, i64, i64, c.c_float, vp, vp, vp]
        L.ltmi_ceps_store.argtypes = [i32, vp, i64, i32, i32, i64, i32, i32, vp, vp, i64, vp]
        L.ltmi_ssb_gather.argtypes = [i32, vp, i32, i64, i64, i64, vp, i32, vp, i64, vp]
        L.ltmi_ssb_plan_create.argtypes = [i32, i32, i32, i32, vp, i32, i32, vp, i32, c.POINTER(vp)]
        L.ltmi_ssb_plan_destroy.argtypes = [vp]
        L.ltmi_ssb_reconstruct.argtypes = [vp, vp, i64, vp, vp]
        L.ltmi_ssb_plan_last_kernel.argtypes = [vp]
        L.ltmi_ssb_plan_last_kernel.restype = c.c_char_p
        L.ltmi_ssb_trotter.argtypes = [i32, vp, i64, i32, i32, vp, i32, i32, vp, i32, vp, vp]
        L.ltmi_wdd_filter.argtypes = [i32, i32, i32, vp, vp, c.c_double, i64, i64, i32, vp, vp]
        L.ltmi_wdd_dot.argtypes = [i32, vp, i64, i32, i32, vp, i64, i32, i32, vp, i32, vp]
        L.ltmi_wdd_finish.argtypes = [i32, vp, i32, i32, i32, vp, vp]
        L.ltmi_wdd_plan_create.argtypes = [i32, i32, i32, vp, i32, vp, c.c_double, c.POINTER(vp)]
        L.ltmi_wdd_plan_destroy.argtypes = [vp]
        L.ltmi_wdd_reconstruct.argtypes = [vp, vp, i64, vp, vp]
        L.ltmi_wdd_plan_last_kernel.argtypes = [vp]
        L.ltmi_wdd_plan_last_kernel.restype = c.c_char_p
        L.ltmi_plx_ramps.argtypes = [i32, vp, i64, i32, i32, vp, vp, vp]
        L.ltmi_plx_sum.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp, vp]
        L.ltmi_plx_mul.argtypes = [i32, vp, i64, i32, i32, vp, vp, vp]
        L.ltmi_plx_peaks.argtypes = [i32, vp, i64, i32, i32, i32, vp, vp]
        L.ltmi_plx_plan_create.argtypes = [i32, i32, i32, i32, i32, i32, i64, c.POINTER(vp)]
        L.ltmi_plx_plan_destroy.argtypes = [vp]
        L.ltmi_plx_plan_load.argtypes = [vp, vp, i64, vp]
        L.ltmi_plx_plan_iterate.argtypes = [vp, vp, vp]
        L.ltmi_plx_plan_sum.argtypes = [vp, vp, vp, vp]
        L.ltmi_plx_plan_last_kernel.argtypes = [vp]
        L.ltmi_plx_plan_last_kernel.restype = c.c_char_p
        for name in EXPORTS:
            fn = getattr(L, name)
            if fn.restype is c.c_int and name not in ('ltmi_version',):
                fn.restype = i32
        _lib = L
    return _lib


def check(rc, what):
    if rc == 0:
        return
    msg = lib().ltmi_last_error().decode('utf8', 'replace')
    if rc in (-1, -2, -3):
        raise ValueError(f"{what}: {msg} (code {rc})")
    raise LtmiError(f"{what}: {msg} (code {rc})")


def device_count():
    n = ctypes.c_int(0)
    check(lib().ltmi_device_count(ctypes.byref(n)), 'ltmi_device_count')
    return n.value


def device_info(device):
    name = ctypes.create_string_buffer(256)
    cu = ctypes.c_int(0)
    mem = ctypes.c_int64(0)
    arch = ctypes.c_int(0)
    check(lib().ltmi_device_info(device, name, ctypes.byref(cu), ctypes.byref(mem),
                                 ctypes.byref(arch)), 'ltmi_device_info')
    return {'name': name.value.decode(), 'cu_count': cu.value, 'hbm_bytes': mem.value,
            'gfx_arch': hex(arch.value)}


def _stream_ptr(stream):
    """torch.cuda.Stream | int | None -> hipStream_t value"""
    if stream is None:
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


def signed_representative(values):
    """Integer mask values as int64 for an integer product that is truncated to the width of their
    dtype afterwards: unsigned values are read as the signed numbers of the same width (65530 as uint16
    is -6 modulo 2^16) -- the same result, the smallest magnitudes (the float64 route of the sparse
    integer product is exact while the column sums of |values| stay small)."""
    values = np.asarray(values)
    if values.dtype.kind == 'u':
        values = values.view(np.dtype(f'i{values.dtype.itemsize}'))
    return values.astype(np.int64)


class MaskHandle:
    """Owns one `ltmi_masks*` (device image of a sig-sliced, flattened mask stack)."""

    def __init__(self, ptr, device, n_masks, n_px, result_dtype, sparse):
        self._ptr = ptr
        self.device = device
        self.n_masks = n_masks
        self.n_px = n_px
        self.result_dtype = np.dtype(result_dtype)
        self.sparse = sparse
        #: result words per mask the library writes (2: a complex stack held as real column pairs)
        self._out_words = 1

    @classmethod
    def dense(cls, device, masks, result_dtype):
        """
        masks: host array (n_masks, n_px); cast to result_dtype here, like
        `for_backend(m, backend).astype(dtype)` (reference common/container.py:90-91).
        """
        result_dtype = np.dtype(result_dtype)
        m = np.ascontiguousarray(np.asarray(masks).astype(result_dtype, copy=False))
        if m.ndim != 2:
            raise ValueError("dense mask stack must be 2D (n_masks, n_px)")
        out = ctypes.c_void_p()
        check(lib().ltmi_masks_create_dense(
            int(device), m.ctypes.data_as(ctypes.c_void_p), dtype_code(result_dtype),
            m.shape[0], m.shape[1], ctypes.byref(out)), 'ltmi_masks_create_dense')
        return cls(out, device, m.shape[0], m.shape[1], result_dtype, False)

    @classmethod
    def csr(cls, device, csr_px_by_masks, result_dtype, gather_only=False):
        """csr_px_by_masks: scipy.sparse CSR (n_px, n_masks) as built by the reference's
        `_build_sparse` (common/container.py:53-64).  gather_only: just the gather kernel's image (the
        handle a densified stack keeps for frames with non-finite pixels, `set_sparse_origin`)."""
        result_dtype = np.dtype(result_dtype)
        indptr = np.ascontiguousarray(csr_px_by_masks.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(csr_px_by_masks.indices, dtype=np.int64)
        if result_dtype.kind in 'iu':
            # integer results: int64 values (the library keeps them as doubles: exact, see
            # csrc/ltmi_sparse.hip csr_apply); uint64 values beyond 2^63 do not fit
            data = np.ascontiguousarray(signed_representative(
                csr_px_by_masks.data.astype(result_dtype, copy=False)))
        else:
            data = np.ascontiguousarray(csr_px_by_masks.data.astype(result_dtype, copy=False))
        n_px, n_masks = csr_px_by_masks.shape
        out = ctypes.c_void_p()
        create = lib().ltmi_masks_create_csr_gather if gather_only else lib().ltmi_masks_create_csr
        check(create(
            int(device), indptr.ctypes.data_as(ctypes.c_void_p),
            indices.ctypes.data_as(ctypes.c_void_p), data.ctypes.data_as(ctypes.c_void_p),
            dtype_code(result_dtype), n_px, n_masks, ctypes.byref(out)), 'ltmi_masks_create_csr')
        return cls(out, device, n_masks, n_px, result_dtype, True)

    @classmethod
    def csr_complex128(cls, device, csr_px_by_masks, gather_only=False):
        """A complex128 sparse stack for REAL frames, without densifying it: (re, im) of mask k are the
        float64 columns 2k, 2k + 1 of the image (the float64 gather kernel), and the result row of a
        frame -- 2 n_masks doubles -- is its complex128 row.  (complex64 stacks do the same inside the
        library.)"""
        import scipy.sparse as sp
        m = sp.csr_matrix(csr_px_by_masks)
        m.sum_duplicates()
        m.sort_indices()
        n_px, n_masks = m.shape
        vals = np.ascontiguousarray(m.data.astype(np.complex128, copy=False))
        counts = np.diff(m.indptr)
        data = np.empty(2 * vals.size, dtype=np.float64)
        indices = np.empty(2 * vals.size, dtype=np.int64)
        data[0::2], data[1::2] = vals.real, vals.imag
        indices[0::2], indices[1::2] = 2 * m.indices.astype(np.int64), 2 * m.indices.astype(np.int64) + 1
        indptr = np.concatenate([[0], np.cumsum(2 * counts)]).astype(np.int64)
        real = sp.csr_matrix((data, indices, indptr), shape=(n_px, 2 * n_masks))
        h = cls.csr(device, real, np.float64, gather_only=gather_only)
        h.n_masks = n_masks
        h.result_dtype = np.dtype(np.complex128)
        h._out_words = 2
        return h

    def kind(self):
        k = ctypes.c_int(-1)
        check(lib().ltmi_masks_kind(self._ptr, ctypes.byref(k)), 'ltmi_masks_kind')
        return k.value

    def set_sig_shape(self, sig_h, sig_w):
        """the detector shape behind the handle's pixels: lets the library fold a stack that is even / odd under a
        mirror of the detector rows (include/ltmi.h)"""
        check(lib().ltmi_masks_set_sig_shape(self._ptr, int(sig_h), int(sig_w)), 'ltmi_masks_set_sig_shape')

    def set_sparse_origin(self, gather):
        """this DENSE handle holds a stack the reference multiplies sparse (a densified CSR stack): `gather`, the
        MaskHandle.csr / csr_complex128 of the same stack, serves the frames whose results come out non-finite --
        stored entries only, like the reference (include/ltmi.h).  Takes ownership of `gather`."""
        check(lib().ltmi_masks_set_sparse_origin(self._ptr, gather._ptr), 'ltmi_masks_set_sparse_origin')
        gather._ptr = None

    def set_dense_origin(self, csr_px_by_masks):
        """this CSR handle holds the non-zeros of a stack the reference multiplies DENSE: a non-finite pixel then
        reaches every mask, also through the zeros the handle does not store (include/ltmi.h)"""
        indptr = np.ascontiguousarray(csr_px_by_masks.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(csr_px_by_masks.indices, dtype=np.int64)
        check(lib().ltmi_masks_set_dense_origin(
            self._ptr, indptr.ctypes.data_as(ctypes.c_void_p), indices.ctypes.data_as(ctypes.c_void_p)),
            'ltmi_masks_set_dense_origin')

    def nonfinite_frames(self, stream=None):
        """frames of the last product that were listed for the non-finite redo / fix-up (synchronises the stream)"""
        n = ctypes.c_int64(0)
        check(lib().ltmi_masks_nonfinite_frames(self._ptr, stream if isinstance(stream, int) else _stream_ptr(stream),
                                                ctypes.byref(n)), 'ltmi_masks_nonfinite_frames')
        return int(n.value)

    def set_tuning(self, mt=0, waves=0, ksplit=0):
        """(mt, waves, ksplit) of k_dense_mfma, or (0, Variant code, ksplit); plain ints do as well (include/ltmi.h)"""
        check(lib().ltmi_masks_set_tuning(self._ptr, mt, waves, ksplit), 'ltmi_masks_set_tuning')

    def last_kernel(self):
        return lib().ltmi_masks_last_kernel(self._ptr).decode()

    def apply(self, tile_ptr, tile_dtype, n_frames, ld_tile, out_ptr, ld_out, accumulate,
              stream=None):
        if LaunchReplay.expected is not None or LaunchReplay.recording is not None:
            sig = LaunchReplay.signature(self, tile_ptr, tile_dtype, n_frames, ld_tile, out_ptr, ld_out,
                                         accumulate, stream)
            if LaunchReplay.expected is not None:
                if LaunchReplay.expected and LaunchReplay.expected[0] == sig:
                    LaunchReplay.expected.pop(0)              # enqueued ahead of the book-keeping
                    return
                raise ReplayMismatch(f"launch {sig!r} was not the one enqueued ahead")
            LaunchReplay.recording.append((self, sig))
        if KernelTimer.enabled:
            import torch
            st = torch.cuda.current_stream() if stream is None or isinstance(stream, int) \
                else stream
            if isinstance(stream, int) and st.cuda_stream != stream:
                st = torch.cuda.ExternalStream(stream)
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record(st)
        # argtypes are declared: plain ints marshal as pointers
        rc = _lib.ltmi_apply_masks(
            self._ptr, tile_ptr, _DTYPES.get(tile_dtype) or dtype_code(tile_dtype), n_frames, ld_tile, out_ptr,
            ld_out * self._out_words,
            1 if accumulate else 0, stream if isinstance(stream, int) else _stream_ptr(stream))
        if rc:
            check(rc, 'ltmi_apply_masks')
        if KernelTimer.enabled:
            b.record(st)
            KernelTimer.events.append((a, b, n_frames, self.last_kernel()))

    @staticmethod
    def _timer_begin(stream):
        """KernelTimer: the start event of a launch on `stream`, recorded -> (start, stop, stream) | None"""
        if not KernelTimer.enabled:
            return None
        import torch
        st = torch.cuda.current_stream() if stream is None or isinstance(stream, int) else stream
        if isinstance(stream, int) and st.cuda_stream != stream:
            st = torch.cuda.ExternalStream(stream)
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(st)
        return a, b, st

    def _timer_end(self, timing, n_frames):
        if timing is not None:
            a, b, st = timing
            b.record(st)
            KernelTimer.events.append((a, b, n_frames, self.last_kernel()))

    def apply_rows(self, tile_ptr, tile_dtype, rows_ptr, n_rows, ld_tile, out_ptr, ld_out, accumulate,
                   stream=None):
        """out[i] (+)= product of frame rows[i] of the tile (rows: device int32).  Returns False --
        nothing done -- when this handle / tile has no row-list kernel (gather the frames instead)."""
        handled = ctypes.c_int(0)
        timing = self._timer_begin(stream)
        check(lib().ltmi_apply_masks_rows(
            self._ptr, ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), ctypes.c_void_p(rows_ptr),
            int(n_rows), int(ld_tile), ctypes.c_void_p(out_ptr), int(ld_out) * self._out_words,
            1 if accumulate else 0,
            stream if isinstance(stream, int) else _stream_ptr(stream), ctypes.byref(handled)),
            'ltmi_apply_masks_rows')
        if handled.value:
            self._timer_end(timing, n_rows)
        return bool(handled.value)

    def apply_csr(self, indptr_ptr, indices_ptr, data_ptr, data_dtype, rows_ptr, row0, n_frames, out_ptr,
                  ld_out, accumulate, stream=None):
        """out[i] (+)= product of the sparse frame row0 + i (or rows[i]: device int32) of a CSR triple in HBM
        with this dense stack, stored entries only (ltmi_apply_masks_csr).  Returns False -- nothing done --
        when the handle or the data dtype has no such kernel (densify the frames instead)."""
        handled = ctypes.c_int(0)
        timing = self._timer_begin(stream)
        check(lib().ltmi_apply_masks_csr(
            self._ptr, ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(indices_ptr), ctypes.c_void_p(data_ptr),
            dtype_code(data_dtype), ctypes.c_void_p(rows_ptr or None), int(row0), int(n_frames),
            ctypes.c_void_p(out_ptr), int(ld_out), 1 if accumulate else 0,
            stream if isinstance(stream, int) else _stream_ptr(stream), ctypes.byref(handled)),
            'ltmi_apply_masks_csr')
        if handled.value:
            self._timer_end(timing, n_frames)
        return bool(handled.value)

    def apply_shifted(self, tile_ptr, tile_dtype, n_frames, ld_tile, sig_h, sig_w, shifts_ptr,
                      out_ptr, ld_out, accumulate, stream=None):
        check(lib().ltmi_apply_masks_shifted(
            self._ptr, ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), n_frames, ld_tile,
            int(sig_h), int(sig_w), ctypes.c_void_p(shifts_ptr), ctypes.c_void_p(out_ptr), ld_out,
            1 if accumulate else 0, _stream_ptr(stream)), 'ltmi_apply_masks_shifted')

    def apply_shifted_host(self, tile_ptr, tile_dtype, n_frames, ld_tile, sig_h, sig_w, shifts,
                           out_ptr, ld_out, accumulate, stream=None):
        """shifts: host int32 array (n_frames, 2) of (dy, dx), C-contiguous."""
        shifts = np.ascontiguousarray(shifts, dtype=np.int32)
        if shifts.shape != (n_frames, 2):
            raise ValueError(f"shifts must have shape ({n_frames}, 2), got {shifts.shape}")
        check(lib().ltmi_apply_masks_shifted_host(
            self._ptr, ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), n_frames, ld_tile,
            int(sig_h), int(sig_w), shifts.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_void_p(out_ptr), ld_out, 1 if accumulate else 0, _stream_ptr(stream)),
            'ltmi_apply_masks_shifted_host')

    def close(self):
        if self._ptr is not None and self._ptr.value:
            lib().ltmi_masks_destroy(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_max_masks():
    """the largest stack ltmi_apply_masks_csr multiplies with sparse frames"""
    return int(lib().ltmi_csr_max_masks())


def csr_check(device, indptr_ptr, indices_ptr, n_rows, n_px, nnz, stream=None):
    """-> flags of a CSR triple in HBM (synchronises): 0 canonical, bit 0: unusable (index out of range,
    broken indptr), bit 1: rows unsorted or with duplicates"""
    import torch
    flags = torch.zeros(1, dtype=torch.int32, device=f'cuda:{int(device)}')
    check(lib().ltmi_csr_check(int(device), ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(indices_ptr or None),
                               int(n_rows), int(n_px), int(nnz), ctypes.c_void_p(flags.data_ptr()),
                               _stream_ptr(stream)), 'ltmi_csr_check')
    if stream is not None:
        torch.cuda.synchronize(int(device))
    return int(flags.cpu()[0])


def csr_densify(device, indptr_ptr, indices_ptr, data_ptr, data_dtype, rows_ptr, row0, n_frames, n_px,
                out_ptr, ld_out, stream=None):
    """out[i, :n_px] = the dense frame row0 + i (or rows[i]: device int32) of a CSR triple in HBM"""
    check(lib().ltmi_csr_densify(
        int(device), ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(indices_ptr or None),
        ctypes.c_void_p(data_ptr or None), dtype_code(data_dtype), ctypes.c_void_p(rows_ptr or None), int(row0),
        int(n_frames), int(n_px), ctypes.c_void_p(out_ptr), int(ld_out),
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_csr_densify')


def csr_sum_sig(device, indptr_ptr, indices_ptr, data_ptr, data_dtype, rows_ptr, row0, n_frames, n_px, out_ptr,
                out_dtype, accumulate, stream=None):
    """out[i] (+)= sum of the stored entries of the sparse frame row0 + i (or rows[i]: device int32) of a CSR
    triple in HBM; out: float32 / float64 (n_frames,)"""
    check(lib().ltmi_csr_sum_sig(
        int(device), ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(indices_ptr or None),
        ctypes.c_void_p(data_ptr or None), dtype_code(data_dtype), ctypes.c_void_p(rows_ptr or None), int(row0),
        int(n_frames), int(n_px), ctypes.c_void_p(out_ptr), dtype_code(out_dtype), 1 if accumulate else 0,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_csr_sum_sig')


def csr_sum_frames_workspace(n_px):
    """bytes of scratch ltmi_csr_sum_frames needs for frames of n_px pixels"""
    return int(lib().ltmi_csr_sum_frames_workspace(int(n_px)))


def csr_sum_frames(device, indptr_ptr, indices_ptr, data_ptr, data_dtype, rows_ptr, row0, n_frames, n_px, out_ptr,
                   out_dtype, accumulate, workspace_ptr, stream=None):
    """out[p] (+)= sum over the sparse frames row0 + i (or rows[i]: device int32), 0 <= i < n_frames, of their
    entry at pixel p; integer data, out: float32 / float64 (n_px,)"""
    check(lib().ltmi_csr_sum_frames(
        int(device), ctypes.c_void_p(indptr_ptr), ctypes.c_void_p(indices_ptr or None),
        ctypes.c_void_p(data_ptr or None), dtype_code(data_dtype), ctypes.c_void_p(rows_ptr or None), int(row0),
        int(n_frames), int(n_px), ctypes.c_void_p(out_ptr), dtype_code(out_dtype), 1 if accumulate else 0,
        ctypes.c_void_p(workspace_ptr), stream if isinstance(stream, int) else _stream_ptr(stream)),
        'ltmi_csr_sum_frames')


def csr_last_kernel():
    """the kernel the calling thread's last csr_sum_sig / csr_sum_frames launched, e.g. 'k_csr_sum_sig<u16,f32> rows'
    ('' before the first)"""
    return lib().ltmi_csr_last_kernel().decode()


def sum_frames_workspace(n_frames, n_px, out_dtype):
    return int(lib().ltmi_sum_frames_workspace(n_frames, n_px, dtype_code(out_dtype)))


def sum_frames(device, tile_ptr, tile_dtype, n_frames, n_px, ld_tile, out_ptr, out_dtype,
               accumulate, workspace_ptr, stream=None):
    check(lib().ltmi_sum_frames(
        int(device), ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), n_frames, n_px, ld_tile,
        ctypes.c_void_p(out_ptr), dtype_code(out_dtype), 1 if accumulate else 0,
        ctypes.c_void_p(workspace_ptr), _stream_ptr(stream)), 'ltmi_sum_frames')


def moments_workspace(n_frames, n_px, tile_dtype):
    return int(lib().ltmi_moments_workspace(n_frames, n_px, dtype_code(tile_dtype)))


def moments_frames(device, tile_ptr, tile_dtype, n_frames, n_px, ld_tile, n_prev, sum_ptr, sum_dtype,
                   varsum_ptr, varsum_dtype, workspace_ptr, cols=None, ld_out=None, stream=None):
    """fold a tile into running per-pixel (sum, varsum) of `n_prev` frames (StdDevUDF); pixel p of the
    tile is element (p // cols) * ld_out + p % cols of the outputs (default: contiguous)"""
    cols = n_px if cols is None else cols
    ld_out = cols if ld_out is None else ld_out
    check(lib().ltmi_moments_frames(
        int(device), ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), n_frames, n_px, ld_tile,
        int(n_prev), ctypes.c_void_p(sum_ptr), dtype_code(sum_dtype), ctypes.c_void_p(varsum_ptr),
        dtype_code(varsum_dtype), int(cols), int(ld_out), ctypes.c_void_p(workspace_ptr),
        _stream_ptr(stream)), 'ltmi_moments_frames')


def ring_moments(device, tile_ptr, tile_dtype, n_frames, width, ld_tile, spans_ptr, n_spans, n_ring,
                 out_ptr, stream=None):
    """out[f] (float32) = std of the ring pixels of frame f (FEMUDF); `spans_ptr`: device int32 triples
    (row, x0, x1) of the ring, n_ring pixels in all"""
    check(lib().ltmi_ring_moments(
        int(device), ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), int(n_frames), int(width),
        int(ld_tile), ctypes.c_void_p(spans_ptr), int(n_spans), int(n_ring), ctypes.c_void_p(out_ptr),
        _stream_ptr(stream)), 'ltmi_ring_moments')


def logsum_workspace(n_frames, n_px, tile_dtype):
    return int(lib().ltmi_logsum_workspace(n_frames, n_px, dtype_code(tile_dtype)))


def logsum_frames(device, tile_ptr, tile_dtype, n_frames, n_px, ld_tile, out_ptr, workspace_ptr,
                  cols=None, ld_out=None, stream=None):
    """out[p] (float32) += sum over the tile's frames of log(x - min(frame) + 1) (LogsumUDF); pixel p of
    the tile is element (p // cols) * ld_out + p % cols of `out` (default: contiguous)"""
    cols = n_px if cols is None else cols
    ld_out = cols if ld_out is None else ld_out
    check(lib().ltmi_logsum_frames(
        int(device), ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), int(n_frames), int(n_px),
        int(ld_tile), ctypes.c_void_p(out_ptr), int(cols), int(ld_out), ctypes.c_void_p(workspace_ptr),
        _stream_ptr(stream)), 'ltmi_logsum_frames')


#: the most components one ltmi_wsum_frames call takes
WSUM_MAX_K = 64


def wsum_workspace(n_frames, n_px, k):
    return int(lib().ltmi_wsum_workspace(int(n_frames), int(n_px), int(k)))


def wsum_frames(device, tile_ptr, tile_dtype, n_frames, n_px, ld_tile, weights_ptr, k, ld_w, out_ptr,
                comp_stride, accumulate, workspace_ptr, cols=None, ld_out=None, stream=None):
    """out[c, p] (float32) (+)= sum over the tile's frames n of weights[n, c] * frame_n[p] (WeightedSumUDF);
    `weights_ptr`: device float32 (n_frames, k) at leading dimension ld_w, 1 <= k <= WSUM_MAX_K; component c
    of tile pixel p is element c * comp_stride + (p // cols) * ld_out + p % cols of `out` (default:
    contiguous rows)"""
    cols = n_px if cols is None else cols
    ld_out = cols if ld_out is None else ld_out
    check(lib().ltmi_wsum_frames(
        int(device), ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), int(n_frames), int(n_px),
        int(ld_tile), ctypes.c_void_p(weights_ptr), int(k), int(ld_w), ctypes.c_void_p(out_ptr), int(cols),
        int(ld_out), int(comp_stride), 1 if accumulate else 0, ctypes.c_void_p(workspace_ptr),
        _stream_ptr(stream)), 'ltmi_wsum_frames')


def sum_sig(device, tile_ptr, tile_dtype, n_frames, n_px, ld_tile, out_ptr, out_dtype,
            accumulate, stream=None):
    check(lib().ltmi_sum_sig(
        int(device), ctypes.c_void_p(tile_ptr), dtype_code(tile_dtype), n_frames, n_px, ld_tile,
        ctypes.c_void_p(out_ptr), dtype_code(out_dtype), 1 if accumulate else 0,
        _stream_ptr(stream)), 'ltmi_sum_sig')


#: dtypes ltmi_axpy / ltmi_add2d take (every dtype of the enum but bool, whose `+=` is a logical or)
AXPY_DTYPES = frozenset(np.dtype(t) for t in (
    'u1', 'i1', 'u2', 'i2', 'u4', 'i4', 'u8', 'i8', 'f4', 'f8', 'c8', 'c16'))


def axpy(device, dest_ptr, src_ptr, dtype, n, stream=None):
    check(lib().ltmi_axpy(int(device), ctypes.c_void_p(dest_ptr), ctypes.c_void_p(src_ptr),
                          dtype_code(dtype), n, _stream_ptr(stream)), 'ltmi_axpy')


def add2d(device, dest_ptr, ld_dest, src_ptr, ld_src, dtype, rows, cols, negate=False, stream=None):
    """dest[r, c] (+|-)= src[r, c]; leading dimensions in elements, ld_src = 0 broadcasts a row."""
    check(lib().ltmi_add2d(int(device), dest_ptr, int(ld_dest), src_ptr, int(ld_src),
                           dtype_code(dtype), int(rows), int(cols), 1 if negate else 0,
                           _stream_ptr(stream)), 'ltmi_add2d')


def host_device_pointer(device, host_ptr):
    """device address of page-locked host memory (raises if it is not device-accessible)"""
    out = ctypes.c_void_p()
    check(lib().ltmi_host_device_pointer(int(device), host_ptr, ctypes.byref(out)),
          'ltmi_host_device_pointer')
    return int(out.value)


def host_copy(dst, src, threads=0):
    """dst[...] = src for two C-contiguous host arrays of the same byte size, on several threads (the GIL is
    released for the call): the staging copy into page-locked bounce buffers at more than the H2D link's rate"""
    if dst.nbytes != src.nbytes or not dst.flags.c_contiguous or not src.flags.c_contiguous:
        raise ValueError("host_copy: C-contiguous arrays of the same size")
    check(lib().ltmi_host_copy(dst.ctypes.data, src.ctypes.data, int(src.nbytes), int(threads)), 'ltmi_host_copy')


def map_or_upload(device, arr):
    """-> (device pointer, keep-alive object) for a C-contiguous host array: zero-copy if the array
    lives in page-locked, device-mapped memory (the result buffers of a run do), else an H2D copy."""
    import torch
    arr = np.ascontiguousarray(arr)
    try:
        return host_device_pointer(device, arr.ctypes.data), arr
    except Exception:
        t = torch.from_numpy(arr).to(f'cuda:{int(device)}')
        return t.data_ptr(), t


def download_pinned(tensor):
    """Device tensor -> NumPy array in page-locked memory (one D2H at link speed; a pageable
    destination is staged by the runtime at a fraction of it).  The array owns its memory."""
    import torch
    host = torch.empty(tensor.shape, dtype=tensor.dtype, pin_memory=True)
    host.copy_(tensor, non_blocking=True)
    torch.cuda.current_stream(tensor.device).synchronize()
    return host.numpy()


def gather_rows(device, src_ptr, ld_src_bytes, idx_ptr, n_rows, row_bytes, dest_ptr, stream=None):
    """dest[i, :] = src[idx[i], :] inside HBM; idx: device int64."""
    check(lib().ltmi_gather_rows(int(device), src_ptr, int(ld_src_bytes), idx_ptr, int(n_rows),
                                 int(row_bytes), dest_ptr, _stream_ptr(stream)), 'ltmi_gather_rows')


def correct(device, tile_ptr, tile_dtype, n_frames, n_px, ld_tile, dark_ptr, gain_ptr, out_ptr,
            out_dtype, ld_out, stream=None):
    """out = ((double)tile - dark) * gain; dark_ptr / gain_ptr: device float64 arrays or None."""
    check(lib().ltmi_correct(
        int(device), tile_ptr, dtype_code(tile_dtype), n_frames, n_px, ld_tile, dark_ptr or None,
        gain_ptr or None, out_ptr, dtype_code(out_dtype), ld_out,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_correct')


def repair_pixels(device, buf_ptr, dtype, n_frames, ld, excl_ptr, env_ptr, cnt_ptr, n_excl, max_env,
                  stream=None):
    check(lib().ltmi_repair_pixels(
        int(device), buf_ptr, dtype_code(dtype), n_frames, ld, excl_ptr, env_ptr, cnt_ptr,
        int(n_excl), int(max_env), stream if isinstance(stream, int) else _stream_ptr(stream)),
        'ltmi_repair_pixels')


def byteswap(device, src_ptr, dst_ptr, itemsize, n_items, stream=None):
    """Reverse the bytes of every `itemsize`-byte item (device pointers; in place if equal)."""
    check(lib().ltmi_byteswap(
        int(device), src_ptr, dst_ptr, int(itemsize), int(n_items),
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_byteswap')


def mib_decode(device, src_ptr, frame_stride, header_bytes, kind, bits, quad, n_frames, height, width,
               dst_ptr, dst_dtype, stream=None):
    """Frames of a .mib file (device copy of the file bytes) -> (n_frames, height, width) of `dst_dtype`."""
    check(lib().ltmi_mib_decode(
        int(device), src_ptr, int(frame_stride), int(header_bytes), ord(kind), int(bits), int(bool(quad)),
        int(n_frames), int(height), int(width), dst_ptr, dtype_code(dst_dtype),
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_mib_decode')


def mib_last_kernel():
    """Name of the kernel this thread's last `mib_decode` launched, e.g. 'k_mib_decode16<u16>' or
    'k_mib_decode<r12,quad>'; '' before the first decode."""
    return lib().ltmi_mib_last_kernel().decode()


def k2is_decode(device, sector_ptrs, n_frames, dst_ptr, dst_dtype=np.uint16, stream=None):
    """Frames of a K2IS acquisition (device copies of the bytes of the 8 sector files; `sector_ptrs`: the 8
    device addresses of the first block of the first frame) -> (n_frames, 1860, 2048) uint16.  `sector_ptrs`
    None stands for a null array (argument checks)."""
    arr = None
    if sector_ptrs is not None:
        if len(sector_ptrs) != 8:
            raise ValueError(f"a K2IS acquisition has 8 sectors, not {len(sector_ptrs)}")
        arr = (ctypes.c_void_p * 8)(*[int(p) if p else None for p in sector_ptrs])
    check(lib().ltmi_k2is_decode(
        int(device), arr, int(n_frames), dst_ptr, dtype_code(dst_dtype),
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_k2is_decode')


def frms6_decode(device, src_ptr, frame_stride, n_frames, height, width, binning, dst_ptr,
                 dst_dtype=np.uint16, stream=None):
    """Folded frames of a .frms6 file (device copy of the file bytes; `src_ptr`: the first frame's payload,
    the next ones `frame_stride` bytes apart; `height` x `width` raw) -> (n_frames, 2 * height * binning,
    width // 2) uint16."""
    check(lib().ltmi_frms6_decode(
        int(device), src_ptr, int(frame_stride), int(n_frames), int(height), int(width), int(binning),
        dst_ptr, dtype_code(dst_dtype), stream if isinstance(stream, int) else _stream_ptr(stream)),
        'ltmi_frms6_decode')


def frms6_last_kernel():
    """Name of the kernel this thread's last `frms6_decode` launched: 'k_frms6_unfold16' (16-byte loads and
    stores) or 'k_frms6_unfold2' (a pixel per lane); '' before the first."""
    return lib().ltmi_frms6_last_kernel().decode()


def records_gather(device, src_ptr, record_stride, n_frames, payload_bytes, dst_ptr, stream=None):
    """Payloads of fixed-size frame records (device copy of the file bytes; `src_ptr`: the first frame's payload,
    the next ones `record_stride` bytes apart) -> `n_frames * payload_bytes` contiguous bytes at `dst_ptr`; bytes
    are moved, not converted."""
    check(lib().ltmi_records_gather(
        int(device), src_ptr, int(record_stride), int(n_frames), int(payload_bytes), dst_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_records_gather')


def records_last_kernel():
    """Name of the kernel this thread's last `records_gather` launched: 'k_records<16>' ... 'k_records<1>' (the
    bytes a lane moves per access); '' before the first."""
    return lib().ltmi_records_last_kernel().decode()


def transpose2d(device, src_ptr, ld_src, rows, cols, item_bytes, dst_ptr, ld_dst, stream=None):
    """dst[c * ld_dst + r] = src[r * ld_src + c] for r < rows, c < cols, in HBM; elements of `item_bytes` (1, 2, 4,
    8, 16) bytes are moved, not converted, `ld_src` / `ld_dst` in elements.  Nothing outside the cols x rows
    rectangle of dst is written."""
    check(lib().ltmi_transpose2d(
        int(device), src_ptr, int(ld_src), int(rows), int(cols), int(item_bytes), dst_ptr, int(ld_dst),
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_transpose2d')


def transpose_last_kernel():
    """Name of the kernel this thread's last `transpose2d` launched: 'k_transpose<1>' ... 'k_transpose<16>' (the
    item size); '' before the first."""
    return lib().ltmi_transpose_last_kernel().decode()


def com_fields(device, raw_ptr, ld_raw, ny, nx, ref_y, ref_x, transform, out_y, out_x, out_mag=None,
               out_div=None, out_curl=None, stream=None):
    """Shift field + magnitude / divergence / curl of a 2D scan from the raw CoM rows (device
    pointers; `transform`: 2x2 float64, host)."""
    t = np.ascontiguousarray(transform, dtype=np.float64).reshape(4)
    check(lib().ltmi_com_fields(
        int(device), raw_ptr, int(ld_raw), int(ny), int(nx), float(ref_y), float(ref_x),
        t.ctypes.data_as(ctypes.c_void_p), out_y, out_x, out_mag or None, out_div or None,
        out_curl or None, stream if isinstance(stream, int) else _stream_ptr(stream)),
        'ltmi_com_fields')


class _NativePlan:
    """What the owners of a native plan share: `_ptr` (set by the subclass's constructor, None once closed) and the
    library's functions named `_destroy` and `_last_kernel`."""
    _ptr = None
    _destroy = _last_kernel = None

    def last_kernel(self):
        return getattr(lib(), self._last_kernel)(self._ptr).decode()

    def close(self):
        if self._ptr is not None and self._ptr.value:
            getattr(lib(), self._destroy)(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FFTPlan(_NativePlan):
    """Owns one `ltmi_fft_plan*`: batched 2D R2C hipFFT + workspace for frames of (sig_h, sig_w)."""
    _destroy, _last_kernel = 'ltmi_fft_plan_destroy', 'ltmi_fft_plan_last_kernel'

    def __init__(self, device, sig_h, sig_w, max_batch):
        out = ctypes.c_void_p()
        check(lib().ltmi_fft_plan_create(int(device), int(sig_h), int(sig_w), int(max_batch),
                                         ctypes.byref(out)), 'ltmi_fft_plan_create')
        self._ptr = out
        self.device, self.sig, self.max_batch = int(device), (int(sig_h), int(sig_w)), int(max_batch)

    def crystallinity(self, tile_ptr, tile_dtype, n_frames, ld_tile, real_mask_ptr, half_mask_ptr,
                      box, out_ptr, accumulate, stream=None):
        """box = (row_lo, row_hi, n_cols): bounding box of the non-zeros of the half mask."""
        check(lib().ltmi_crystallinity(
            self._ptr, tile_ptr, dtype_code(tile_dtype), n_frames, ld_tile, real_mask_ptr or None,
            half_mask_ptr, int(box[0]), int(box[1]), int(box[2]), out_ptr, 1 if accumulate else 0,
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_crystallinity')

    def crystallinity_corrected(self, tile_ptr, tile_dtype, n_frames, ld_tile, tables,
                                real_mask_ptr, half_mask_ptr, box, out_ptr, accumulate,
                                stream=None):
        """The same on RAW frames; `tables` = CorrectionSet.device_tables(...): dark / gain (float64
        device tensors or None) and the int32 repair tables."""
        def ptr(t):
            return None if t is None else t.data_ptr()
        check(lib().ltmi_crystallinity_corrected(
            self._ptr, tile_ptr, dtype_code(tile_dtype), n_frames, ld_tile, ptr(tables['dark']),
            ptr(tables['gain']), ptr(tables['excl']), ptr(tables['env']), ptr(tables['cnt']),
            int(tables['n_excl']), int(tables['max_env']), real_mask_ptr or None, half_mask_ptr,
            int(box[0]), int(box[1]), int(box[2]), out_ptr, 1 if accumulate else 0,
            stream if isinstance(stream, int) else _stream_ptr(stream)),
            'ltmi_crystallinity_corrected')

    def last_kernel(self):
        """'k_cryst_fused<...>' or 'hipfft_r2c<...>': the route of the last crystallinity call"""
        return super().last_kernel()


class CorrPlan(_NativePlan):
    """Owns one `ltmi_corr_plan*`: batched 2D R2C and C2R hipFFTs + workspace for frames of (sig_h, sig_w), and the
    device spectrum of one template (host float32 (sig_h, sig_w), centred at (sig_h // 2, sig_w // 2))."""
    _destroy, _last_kernel = 'ltmi_corr_plan_destroy', 'ltmi_corr_plan_last_kernel'

    def __init__(self, device, sig_h, sig_w, max_batch, template):
        t = np.ascontiguousarray(template, dtype=np.float32)
        if t.shape != (int(sig_h), int(sig_w)):
            raise ValueError(f"template of shape {t.shape} for frames of {(int(sig_h), int(sig_w))}")
        out = ctypes.c_void_p()
        check(lib().ltmi_corr_plan_create(int(device), int(sig_h), int(sig_w), int(max_batch),
                                          t.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out)),
              'ltmi_corr_plan_create')
        self._ptr = out
        self.device, self.sig, self.max_batch = int(device), (int(sig_h), int(sig_w)), int(max_batch)

    def correlate_peaks(self, tile_ptr, tile_dtype, n_frames, ld_tile, peaks_ptr, n_peaks, crop_radius,
                        refine_radius, centers_ptr, refineds_ptr, peak_values_ptr, peak_elevations_ptr,
                        stream=None):
        """peaks: device int32 (n_peaks, 2) of (py, px); centers int32 / refineds float32 (n_frames, n_peaks, 2),
        peak_values / peak_elevations float32 (n_frames, n_peaks): device pointers (include/ltmi.h)."""
        check(lib().ltmi_correlate_peaks(
            self._ptr, tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), peaks_ptr, int(n_peaks),
            int(crop_radius), int(refine_radius), centers_ptr, refineds_ptr, peak_values_ptr,
            peak_elevations_ptr, stream if isinstance(stream, int) else _stream_ptr(stream)),
            'ltmi_correlate_peaks')

    def find_peaks(self, tile_ptr, tile_dtype, n_frames, ld_tile, num_peaks, min_distance, border, threshold_abs,
                   threshold_rel, refine_radius, n_found_ptr, centers_ptr, refineds_ptr, peak_values_ptr,
                   peak_elevations_ptr, stream=None):
        """The num_peaks strongest local maxima of every frame's correlation map.  n_found
        int32 (n_frames), centers int32 / refineds float32 (n_frames, num_peaks, 2), peak_values / peak_elevations
        float32 (n_frames, num_peaks): device pointers (include/ltmi.h)."""
        check(lib().ltmi_correlate_find(
            self._ptr, tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), int(num_peaks),
            int(min_distance), int(border), float(threshold_abs), float(threshold_rel), int(refine_radius),
            n_found_ptr, centers_ptr, refineds_ptr, peak_values_ptr, peak_elevations_ptr,
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_correlate_find')

    def last_kernel(self):
        """'k_corr_load<...> + hipfft_r2c + k_corr_mul + hipfft_c2r + k_corr_peaks batch=N'; after `find_peaks` the
        search kernels 'k_pf_cells + k_pf_verify + k_pf_select + k_corr_found' stand in place of k_corr_peaks"""
        return super().last_kernel()


def find_peaks_maps(device, maps_ptr, n_frames, h, w, ld_map, num_peaks, min_distance, border, threshold_abs,
                    threshold_rel, refine_radius, n_found_ptr, centers_ptr, refineds_ptr, peak_values_ptr,
                    peak_elevations_ptr, stream=None):
    """`CorrPlan.find_peaks` on float32 maps the caller supplies: map f of (h, w) at maps + f * ld_map elements
    (include/ltmi.h)."""
    check(lib().ltmi_find_peaks_maps(
        int(device), maps_ptr, int(n_frames), int(h), int(w), int(ld_map), int(num_peaks), int(min_distance),
        int(border), float(threshold_abs), float(threshold_rel), int(refine_radius), n_found_ptr, centers_ptr,
        refineds_ptr, peak_values_ptr, peak_elevations_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_find_peaks_maps')


def find_peaks_last_kernel():
    """'k_pf_cells + k_pf_verify + k_pf_select + k_corr_found' after the first launching `find_peaks_maps` call
    on this thread, '' before"""
    return lib().ltmi_find_peaks_last_kernel().decode()


#: frame dtypes ltmi_count_events / ltmi_store_events take
COUNT_DTYPES = frozenset(np.dtype(t) for t in ('u1', 'i1', 'u2', 'i2', 'u4', 'i4', 'f4'))
#: widest frame they take (csrc/ltmi_count.hip)
COUNT_MAX_WIDTH = 4096


def count_events(device, tile_ptr, tile_dtype, n_frames, h, w, ld_tile, dark_ptr, gain_ptr, t_bg, t_x, n_events_ptr,
                 stream=None):
    """n_events[f] = number of electron events of frame f (the definition: include/ltmi.h); `dark_ptr` / `gain_ptr`:
    device float32 (h, w) or None"""
    check(lib().ltmi_count_events(
        int(device), tile_ptr, dtype_code(tile_dtype), int(n_frames), int(h), int(w), int(ld_tile), dark_ptr or None,
        gain_ptr or None, float(t_bg), float(t_x), n_events_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_count_events')


def store_events(device, tile_ptr, tile_dtype, n_frames, h, w, ld_tile, dark_ptr, gain_ptr, t_bg, t_x, indptr_ptr,
                 base, capacity, indices_ptr, values_ptr, values_dtype, status_ptr, stream=None):
    """frame f's events to indices[indptr[f] - base .. indptr[f + 1] - base), ascending, their values (uint8 1 or
    float32 u[p]) to the same places of `values_ptr` (None: indices only); `status_ptr`: device int32, non-zero
    afterwards if `indptr` does not fit the events or the `capacity` elements"""
    check(lib().ltmi_store_events(
        int(device), tile_ptr, dtype_code(tile_dtype), int(n_frames), int(h), int(w), int(ld_tile), dark_ptr or None,
        gain_ptr or None, float(t_bg), float(t_x), indptr_ptr, int(base), int(capacity), indices_ptr,
        values_ptr or None, dtype_code(values_dtype), status_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_store_events')


def count_strip_rows(h, w):
    """rows of a strip of the counting kernels for frames of (h, w); 0 outside their limits"""
    return int(lib().ltmi_count_strip_rows(int(h), int(w)))


def count_last_kernel():
    """'k_count_events' / 'k_store_events' (+ ' vec': 16-byte pixel loads) after this thread's last launching call"""
    return lib().ltmi_count_last_kernel().decode()


#: frame dtypes ltmi_orient_match / ltmi_orient_polar take
ORIENT_DTYPES = COUNT_DTYPES


def orient_max_polar_words():
    """the largest n_r * n_phi an OrientPlan takes: the polar image shares the LDS of a CU with the kernel's scores"""
    return int(lib().ltmi_orient_max_polar_words())


def orient_score_block():
    """templates whose scores the matching kernel selects from at a time (csrc/ltmi_orient.hip)"""
    return int(lib().ltmi_orient_score_block())


class OrientPlan(_NativePlan):
    """Owns one `ltmi_orient_plan*`: the device copies of a polar sampling table (tap_idx int32, tap_w float32, both
    (n_r, n_phi, 4)) for frames of (sig_h, sig_w) and of a template library (indptr (T + 1,), spot_r, spot_phi, spot_w),
    and the number of result slots n_best.  Every index and range is checked by the library (include/ltmi.h)."""
    _destroy, _last_kernel = 'ltmi_orient_plan_destroy', 'ltmi_orient_plan_last_kernel'

    def __init__(self, device, sig_h, sig_w, tap_idx, tap_w, library, n_best):
        tap_idx = np.ascontiguousarray(tap_idx, dtype=np.int32)
        tap_w = np.ascontiguousarray(tap_w, dtype=np.float32)
        if tap_idx.ndim != 3 or tap_idx.shape[2] != 4 or tap_w.shape != tap_idx.shape:
            raise ValueError(f"sampling table of shapes {tap_idx.shape} and {tap_w.shape}, not two of (n_r, n_phi, 4)")
        indptr, spot_r, spot_phi, spot_w = library
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        spot_r = np.ascontiguousarray(spot_r, dtype=np.int32)
        spot_phi = np.ascontiguousarray(spot_phi, dtype=np.int32)
        spot_w = np.ascontiguousarray(spot_w, dtype=np.float32)
        if indptr.ndim != 1 or indptr.size < 1:
            raise ValueError(f"indptr of shape {indptr.shape}, not (T + 1,)")
        n_spots = int(indptr[-1])
        if not (spot_r.shape == spot_phi.shape == spot_w.shape == (max(n_spots, 0),)):
            raise ValueError(f"indptr ends at {n_spots}, the spot arrays have shapes {spot_r.shape}, {spot_phi.shape} "
                             f"and {spot_w.shape}")
        n_r, n_phi = tap_idx.shape[:2]
        out = ctypes.c_void_p()

        def ptr(a):
            return a.ctypes.data_as(ctypes.c_void_p)

        check(lib().ltmi_orient_plan_create(int(device), int(sig_h), int(sig_w), n_r, n_phi, ptr(tap_idx), ptr(tap_w),
                                            indptr.size - 1, ptr(indptr), ptr(spot_r), ptr(spot_phi), ptr(spot_w),
                                            int(n_best), ctypes.byref(out)), 'ltmi_orient_plan_create')
        self._ptr = out
        self.device, self.sig, self.polar_shape = int(device), (int(sig_h), int(sig_w)), (n_r, n_phi)
        self.n_templates, self.n_best = indptr.size - 1, int(n_best)

    def match(self, tile_ptr, tile_dtype, n_frames, ld_tile, template_ptr, rotation_ptr, correlation_ptr, norm_ptr,
              stream=None):
        """the n_best best templates of every frame: template, rotation int32 and correlation float32
        (n_frames, n_best), polar_norm float32 (n_frames): device pointers (include/ltmi.h)"""
        check(lib().ltmi_orient_match(
            self._ptr, tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), template_ptr, rotation_ptr,
            correlation_ptr, norm_ptr, stream if isinstance(stream, int) else _stream_ptr(stream)),
            'ltmi_orient_match')

    def polar(self, tile_ptr, tile_dtype, n_frames, ld_tile, polar_ptr, ld_polar, stream=None):
        """the polar image of frame f, float32 (n_r * n_phi), to polar_ptr + f * ld_polar elements"""
        check(lib().ltmi_orient_polar(
            self._ptr, tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), polar_ptr, int(ld_polar),
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_orient_polar')

    def last_kernel(self):
        """'k_orient_match<dtype,NCH> grid=G lds=B' or 'k_orient_polar<dtype>' after the last launching call"""
        return super().last_kernel()


class HoloPlan(_NativePlan):
    """Owns one `ltmi_holo_plan*`: a batched 2D R2C hipFFT of (sig_h, sig_w), a batched backward C2C hipFFT of
    (out_h, out_w) and their workspace, the sideband position (sb_y, sb_x) in the unshifted fft2 layout, the real
    aperture (host float32 (out_h, out_w), unshifted layout, (0, 0) the sideband centre) and, optionally, a complex
    reference wave of the same shape, inverted here in complex128 and stored as complex64."""
    _destroy, _last_kernel = 'ltmi_holo_plan_destroy', 'ltmi_holo_plan_last_kernel'

    def __init__(self, device, sig_h, sig_w, out_h, out_w, max_batch, sb_y, sb_x, aperture, reference_wave=None):
        out_shape = (int(out_h), int(out_w))
        a = np.ascontiguousarray(aperture, dtype=np.float32)
        if a.shape != out_shape:
            raise ValueError(f"aperture of shape {a.shape} for an output of {out_shape}")
        ref_inv = None
        if reference_wave is not None:
            ref = np.asarray(reference_wave)
            if ref.shape != out_shape:
                raise ValueError(f"reference_wave of shape {ref.shape} for an output of {out_shape}")
            with np.errstate(all='ignore'):
                ref_inv = np.ascontiguousarray((1.0 / ref.astype(np.complex128)).astype(np.complex64))
        out = ctypes.c_void_p()
        check(lib().ltmi_holo_plan_create(
            int(device), int(sig_h), int(sig_w), out_shape[0], out_shape[1], int(max_batch), int(sb_y), int(sb_x),
            a.ctypes.data_as(ctypes.c_void_p),
            None if ref_inv is None else ref_inv.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out)),
            'ltmi_holo_plan_create')
        self._ptr = out
        self.device, self.sig, self.out_shape = int(device), (int(sig_h), int(sig_w)), out_shape
        self.max_batch, self.sb_position = int(max_batch), (int(sb_y), int(sb_x))

    def reconstruct(self, tile_ptr, tile_dtype, n_frames, ld_tile, out_ptr, ld_out, stream=None):
        """tile: device (n_frames, sig_h * sig_w) of tile_dtype, ld_tile elements apart; out: device complex64
        (n_frames, out_h * out_w), rows ld_out elements apart (include/ltmi.h)."""
        check(lib().ltmi_holo_reconstruct(
            self._ptr, tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), out_ptr, int(ld_out),
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_holo_reconstruct')

    def last_kernel(self):
        """'k_corr_load<...> + hipfft_r2c + k_holo_crop + hipfft_c2c + k_holo_store batch=N' after the first launching
        `reconstruct` call, '' before"""
        return super().last_kernel()


def holo_crop(device, spec_ptr, n_frames, h, w, ld_spec, out_h, out_w, sb_y, sb_x, aperture_ptr, g_ptr, ld_g,
              stream=None):
    """The sideband gather of `HoloPlan.reconstruct` on complex64 half spectra the caller supplies: frame f's
    (h, w // 2 + 1) half spectrum at spec + f * ld_spec elements, the float32 aperture (out_h, out_w) on the device,
    used as it is; frame f's (out_h, out_w) result at g + f * ld_g elements (include/ltmi.h)."""
    check(lib().ltmi_holo_crop(
        int(device), spec_ptr, int(n_frames), int(h), int(w), int(ld_spec), int(out_h), int(out_w), int(sb_y),
        int(sb_x), aperture_ptr, g_ptr, int(ld_g), stream if isinstance(stream, int) else _stream_ptr(stream)),
        'ltmi_holo_crop')


class CepstrumPlan(_NativePlan):
    """Owns one `ltmi_ceps_plan*`: a batched 2D R2C hipFFT of (sig_h, sig_w) and its workspace, the offset added before
    the logarithm, the window (host float32 (sig_h, sig_w)) and keep / (sig_h sig_w) for the (out_h, out_w) quefrencies
    around the origin, `keep` clearing those closer to it than dc_radius (include/ltmi.h)."""
    _destroy, _last_kernel = 'ltmi_ceps_plan_destroy', 'ltmi_ceps_plan_last_kernel'

    def __init__(self, device, sig_h, sig_w, out_h, out_w, max_batch, offset, window, dc_radius=0.0):
        sig = (int(sig_h), int(sig_w))
        win = np.ascontiguousarray(window, dtype=np.float32)
        if win.shape != sig:
            raise ValueError(f"window of shape {win.shape} for frames of {sig}")
        out = ctypes.c_void_p()
        check(lib().ltmi_ceps_plan_create(
            int(device), sig[0], sig[1], int(out_h), int(out_w), int(max_batch), float(offset),
            win.ctypes.data_as(ctypes.c_void_p), float(dc_radius), ctypes.byref(out)), 'ltmi_ceps_plan_create')
        self._ptr = out
        self.device, self.sig, self.out_shape = int(device), sig, (int(out_h), int(out_w))
        self.max_batch, self.offset, self.dc_radius = int(max_batch), float(np.float32(offset)), float(dc_radius)

    def transform(self, tile_ptr, tile_dtype, n_frames, ld_tile, out_ptr, ld_out, stream=None):
        """tile: device (n_frames, sig_h * sig_w) of tile_dtype, ld_tile elements apart; out: device float32
        (n_frames, out_h * out_w), rows ld_out elements apart (include/ltmi.h)."""
        check(lib().ltmi_ceps_transform(
            self._ptr, tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), out_ptr, int(ld_out),
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_ceps_transform')

    def last_kernel(self):
        """'k_ceps_load<...> + hipfft_r2c + k_ceps_store batch=N' after the first launching `transform` call, ''
        before"""
        return super().last_kernel()


def ceps_load(device, tile_ptr, tile_dtype, n_frames, ld_tile, n_px, offset, window_ptr, out_ptr, stream=None):
    """The first kernel of `CepstrumPlan.transform` alone: out[f, p] = logf(max(tile[f, p], 0) + offset) * window[p];
    tile: device, frames ld_tile elements apart; window: device float32 (n_px); out: device float32 (n_frames, n_px),
    contiguous (include/ltmi.h)."""
    check(lib().ltmi_ceps_load(
        int(device), tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), int(n_px), float(offset),
        window_ptr, out_ptr, stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_ceps_load')


def ceps_store(device, spec_ptr, n_frames, h, w, ld_spec, out_h, out_w, scale_ptr, out_ptr, ld_out, stream=None):
    """The last kernel of `CepstrumPlan.transform` on complex64 half spectra the caller supplies: frame f's
    (h, w // 2 + 1) half spectrum at spec + f * ld_spec elements, the float32 scale (out_h, out_w) on the device, used
    as it is; frame f's float32 (out_h, out_w) result at out + f * ld_out elements (include/ltmi.h)."""
    check(lib().ltmi_ceps_store(
        int(device), spec_ptr, int(n_frames), int(h), int(w), int(ld_spec), int(out_h), int(out_w), scale_ptr, out_ptr,
        int(ld_out), stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_ceps_store')


def ssb_geometry(lamb, dpix, semiconv, semiconv_pix, cy, cx, transformation):
    """the `geom` array of the ltmi_ssb_* calls (include/ltmi.h): lamb, dy, dx, semiconv, semiconv_pix, cy, cx and the
    2 x 2 transformation row by row, as 11 float64; dpix is (dy, dx)"""
    t = np.asarray(transformation, dtype=np.float64).reshape(2, 2)
    return np.array([lamb, dpix[0], dpix[1], semiconv, semiconv_pix, cy, cx, t[0, 0], t[0, 1], t[1, 0], t[1, 1]],
                    dtype=np.float64)


def ssb_gather(device, tile_ptr, tile_dtype, n_frames, ld_tile, n_px, idx_ptr, n_idx, out_ptr, ld_out, stream=None):
    """The bright-field pixels of every frame of a tile: out[f, k] = float32(tile[f, idx[k]]).  tile: device
    (n_frames, n_px) of tile_dtype, ld_tile elements apart; idx: device int32 (n_idx); out: device float32
    (n_frames, n_idx), rows ld_out elements apart (include/ltmi.h)."""
    check(lib().ltmi_ssb_gather(
        int(device), tile_ptr, dtype_code(tile_dtype), int(n_frames), int(ld_tile), int(n_px), idx_ptr, int(n_idx),
        out_ptr, int(ld_out), stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_ssb_gather')


class SSBPlan(_NativePlan):
    """Owns one `ltmi_ssb_plan*`: the bright-field list (host int32 frame indices), the geometry (`ssb_geometry`), the
    cutoff, a batched 2D R2C hipFFT over the (nav_y, nav_x) scan for min(max_batch, P) bright-field pixels per
    execution and its workspace."""
    _destroy, _last_kernel = 'ltmi_ssb_plan_destroy', 'ltmi_ssb_plan_last_kernel'

    def __init__(self, device, nav_y, nav_x, sig_w, idx, max_batch, geom, cutoff):
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        geom = np.ascontiguousarray(geom, dtype=np.float64).reshape(-1)
        if geom.size != 11:
            raise ValueError(f"the geometry holds 11 values (hip.ssb_geometry), not {geom.size}")
        out = ctypes.c_void_p()
        check(lib().ltmi_ssb_plan_create(
            int(device), int(nav_y), int(nav_x), int(sig_w), idx.ctypes.data_as(ctypes.c_void_p), int(idx.size),
            int(max_batch), geom.ctypes.data_as(ctypes.c_void_p), int(cutoff), ctypes.byref(out)),
            'ltmi_ssb_plan_create')
        self._ptr = out
        self.device, self.nav, self.n_idx = int(device), (int(nav_y), int(nav_x)), int(idx.size)
        self.max_batch = int(max_batch)

    def reconstruct(self, bf_ptr, ld_bf, fourier_ptr, stream=None):
        """bf: device float32 (nav_y * nav_x, P), rows ld_bf elements apart; fourier: device complex64
        (nav_y, nav_x), contiguous (include/ltmi.h)."""
        check(lib().ltmi_ssb_reconstruct(
            self._ptr, bf_ptr, int(ld_bf), fourier_ptr,
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_ssb_reconstruct')

    def last_kernel(self):
        """'k_transpose<4> + hipfft_r2c + k_transpose<8> + k_ssb_trotter batch=N' after the first `reconstruct` call,
        '' before"""
        return super().last_kernel()


def ssb_trotter(device, spec_ptr, ld_spec, nav_y, nav_x, idx_ptr, n_idx, sig_w, geom, cutoff, fourier_ptr,
                stream=None):
    """The trotter sums of `SSBPlan.reconstruct` on complex64 half spectra the caller supplies: element
    [(iy * (nav_x // 2 + 1) + ix) * ld_spec + k] is G[k, iy, ix]; idx: device int32 (n_idx); geom: `ssb_geometry`;
    fourier: device complex64 (nav_y, nav_x) (include/ltmi.h)."""
    geom = np.ascontiguousarray(geom, dtype=np.float64).reshape(-1)
    if geom.size != 11:
        raise ValueError(f"the geometry holds 11 values (hip.ssb_geometry), not {geom.size}")
    check(lib().ltmi_ssb_trotter(
        int(device), spec_ptr, int(ld_spec), int(nav_y), int(nav_x), idx_ptr, int(n_idx), int(sig_w),
        geom.ctypes.data_as(ctypes.c_void_p), int(cutoff), fourier_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_ssb_trotter')


def _wdd_args(window, geom):
    """the window as 4 host int32 (y0, x0, By, Bx) and the geometry as 11 float64"""
    window = np.ascontiguousarray(window, dtype=np.int32).reshape(-1)
    if window.size != 4:
        raise ValueError(f"the window holds 4 values (y0, x0, By, Bx), not {window.size}")
    geom = np.ascontiguousarray(geom, dtype=np.float64).reshape(-1)
    if geom.size != 11:
        raise ValueError(f"the geometry holds 11 values (hip.ssb_geometry), not {geom.size}")
    return window, geom


def wdd_filter(device, nav_y, nav_x, window, geom, epsilon, q0, n_q, q_batch, filter_ptr, stream=None):
    """The Wiener filter F of the Qs [q0, q0 + n_q) of a (nav_y, nav_x) scan -> device complex64 (n_q, By * Bx),
    q_batch Qs per hipFFT execution; window: (y0, x0, By, Bx); geom: `ssb_geometry`.  Returns when the work is done
    (include/ltmi.h)."""
    window, geom = _wdd_args(window, geom)
    check(lib().ltmi_wdd_filter(
        int(device), int(nav_y), int(nav_x), window.ctypes.data_as(ctypes.c_void_p),
        geom.ctypes.data_as(ctypes.c_void_p), float(epsilon), int(q0), int(n_q), int(q_batch), filter_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_wdd_filter')


def wdd_dot(device, spec_ptr, ld_spec, nav_y, nav_x, filter_ptr, ld_filter, k0, n_k, acc_ptr, first=True, stream=None):
    """acc[Q] (+)= sum_j G[j, Q] * F[Q, k0 + j] over n_k window pixels: complex64 half spectra as `ssb_trotter` takes
    them, F device complex64 rows ld_filter apart, acc device float64 (nav_y * nav_x, 2) (include/ltmi.h)."""
    check(lib().ltmi_wdd_dot(
        int(device), spec_ptr, int(ld_spec), int(nav_y), int(nav_x), filter_ptr, int(ld_filter), int(k0), int(n_k),
        acc_ptr, int(bool(first)), stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_wdd_dot')


def wdd_finish(device, acc_ptr, nav_y, nav_x, n_window, fourier_ptr, stream=None):
    """fourier[Q] = conj(S[-Q]) / |S[0, 0]|, S = acc / n_window -> device complex64 (nav_y, nav_x) (include/ltmi.h)"""
    check(lib().ltmi_wdd_finish(
        int(device), acc_ptr, int(nav_y), int(nav_x), int(n_window), fourier_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_wdd_finish')


class WDDPlan(_NativePlan):
    """Owns one `ltmi_wdd_plan*`: the Wiener filter F of every Q of the (nav_y, nav_x) scan for the window
    (y0, x0, By, Bx) -- nav_y * nav_x * By * Bx * 8 bytes, built here --, a batched 2D R2C hipFFT over the scan for
    min(max_batch, By * Bx) window pixels per execution and its workspace.  F that does not fit: LtmiError, code -4."""
    _destroy, _last_kernel = 'ltmi_wdd_plan_destroy', 'ltmi_wdd_plan_last_kernel'

    def __init__(self, device, nav_y, nav_x, window, max_batch, geom, epsilon):
        window, geom = _wdd_args(window, geom)
        out = ctypes.c_void_p()
        check(lib().ltmi_wdd_plan_create(
            int(device), int(nav_y), int(nav_x), window.ctypes.data_as(ctypes.c_void_p), int(max_batch),
            geom.ctypes.data_as(ctypes.c_void_p), float(epsilon), ctypes.byref(out)), 'ltmi_wdd_plan_create')
        self._ptr = out
        self.device, self.nav, self.window = int(device), (int(nav_y), int(nav_x)), tuple(int(v) for v in window)
        self.max_batch = int(max_batch)

    def reconstruct(self, bf_ptr, ld_bf, fourier_ptr, stream=None):
        """bf: device float32 (nav_y * nav_x, By * Bx), rows ld_bf elements apart; fourier: device complex64
        (nav_y, nav_x), contiguous (include/ltmi.h)."""
        check(lib().ltmi_wdd_reconstruct(
            self._ptr, bf_ptr, int(ld_bf), fourier_ptr,
            stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_wdd_reconstruct')

    def last_kernel(self):
        """'k_transpose<4> + hipfft_r2c + k_transpose<8> + k_wdd_dot + k_wdd_finish batch=N' after the first
        `reconstruct` call, '' before"""
        return super().last_kernel()


def _stream_arg(stream):
    return stream if isinstance(stream, int) else _stream_ptr(stream)


def plx_ramps(device, sh_ptr, n, nav_y, nav_x, ey_ptr, ex_ptr, stream=None):
    """The Fourier ramps of n shifts: sh device float64 (n, 2) -> ey device complex128 (n, nav_y), ex device complex128
    (n, nav_x // 2 + 1) (include/ltmi.h)."""
    check(lib().ltmi_plx_ramps(int(device), sh_ptr, int(n), int(nav_y), int(nav_x), ey_ptr, ex_ptr, _stream_arg(stream)),
          'ltmi_plx_ramps')


def plx_sum(device, spec_ptr, n, nav_y, nav_x, ey_ptr, ex_ptr, s_ptr, stream=None):
    """S[Q] = mean over the n pixels of G[K, Q] ey[K, iy] ex[K, ix]: spec device complex64 (n, nav_y, nav_x // 2 + 1),
    pixel-major -> s device complex64 (nav_y, nav_x // 2 + 1) (include/ltmi.h)."""
    check(lib().ltmi_plx_sum(int(device), spec_ptr, int(n), int(nav_y), int(nav_x), ey_ptr, ex_ptr, s_ptr,
                             _stream_arg(stream)), 'ltmi_plx_sum')


def plx_mul(device, spec_ptr, n, nav_y, nav_x, ref_ptr, x_ptr, stream=None):
    """X[K, Q] = G[K, Q] conj(R[Q]) in float32, X[K, 0] = 0: spec, x device complex64 (n, nav_y, nav_x // 2 + 1), ref
    device complex64 (nav_y, nav_x // 2 + 1) (include/ltmi.h)."""
    check(lib().ltmi_plx_mul(int(device), spec_ptr, int(n), int(nav_y), int(nav_x), ref_ptr, x_ptr, _stream_arg(stream)),
          'ltmi_plx_mul')


def plx_peaks(device, maps_ptr, n, nav_y, nav_x, max_shift, shifts_ptr, stream=None):
    """The first maximum within max_shift of the origin of n circular correlation maps, device float32
    (n, nav_y, nav_x), refined by a parabola per axis -> device float64 (n, 2) (include/ltmi.h)."""
    check(lib().ltmi_plx_peaks(int(device), maps_ptr, int(n), int(nav_y), int(nav_x), int(max_shift), shifts_ptr,
                               _stream_arg(stream)), 'ltmi_plx_peaks')


class ParallaxPlan(_NativePlan):
    """Owns one `ltmi_plx_plan*`: the half spectra over the (nav_y, nav_x) scan of n_idx bright-field pixels --
    8 n_idx nav_y (nav_x // 2 + 1) bytes, at most store_limit_bytes --, the ramps, a batched R2C and a batched C2R hipFFT
    for min(max_batch, n_idx) pixels per execution and their workspace.  A store that does not fit: LtmiError, code -4."""
    _destroy, _last_kernel = 'ltmi_plx_plan_destroy', 'ltmi_plx_plan_last_kernel'

    def __init__(self, device, nav_y, nav_x, n_idx, max_batch, max_shift, store_limit_bytes):
        out = ctypes.c_void_p()
        check(lib().ltmi_plx_plan_create(
            int(device), int(nav_y), int(nav_x), int(n_idx), int(max_batch), int(max_shift), int(store_limit_bytes),
            ctypes.byref(out)), 'ltmi_plx_plan_create')
        self._ptr = out
        self.device, self.nav, self.n_idx = int(device), (int(nav_y), int(nav_x)), int(n_idx)
        self.max_batch, self.max_shift = int(max_batch), int(max_shift)

    def load(self, bf_ptr, ld_bf, stream=None):
        """bf: device float32 (nav_y * nav_x, P), rows ld_bf elements apart -> the plan's spectra (include/ltmi.h)"""
        check(lib().ltmi_plx_plan_load(self._ptr, bf_ptr, int(ld_bf), _stream_arg(stream)), 'ltmi_plx_plan_load')

    def iterate(self, shifts_ptr, stream=None):
        """shifts: device float64 (P, 2), the aligning shifts on entry, the measured ones afterwards (include/ltmi.h)"""
        check(lib().ltmi_plx_plan_iterate(self._ptr, shifts_ptr, _stream_arg(stream)), 'ltmi_plx_plan_iterate')

    def sum(self, shifts_ptr, half_ptr, stream=None):
        """the half spectrum of the mean of the scan images aligned by `shifts` -> device complex64
        (nav_y, nav_x // 2 + 1) (include/ltmi.h)"""
        check(lib().ltmi_plx_plan_sum(self._ptr, shifts_ptr, half_ptr, _stream_arg(stream)), 'ltmi_plx_plan_sum')

    def last_kernel(self):
        """what the last of `load`, `iterate` and `sum` launched (include/ltmi.h), '' before the first"""
        return super().last_kernel()


def lattice_fit(device, refineds_ptr, weights_ptr, peak_values_ptr, n_frames, n_peaks, indices_ptr, start, tolerance,
                zero_ptr, a_ptr, b_ptr, selector_ptr, error_ptr, stream=None):
    """The lattice zero + i a + j b that fits the peaks of every frame (include/ltmi.h).  refineds float32
    (n_frames, n_peaks, 2), weights / peak_values float32 (n_frames, n_peaks) or None, indices int32 (n_peaks, 2),
    zero / a / b float32 (n_frames, 2), selector bytes (n_frames, n_peaks), error float32 (n_frames): device
    pointers; start: the six host values zero0, a0, b0 as (y, x) or None."""
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1)
        if start.size != 6:
            raise ValueError(f"start holds zero0, a0, b0 as (y, x): 6 values, not {start.size}")
        start_ptr = start.ctypes.data_as(ctypes.c_void_p)
    else:
        start_ptr = None
    check(lib().ltmi_lattice_fit(
        int(device), refineds_ptr, weights_ptr, peak_values_ptr, int(n_frames), int(n_peaks), indices_ptr,
        start_ptr, float(tolerance), zero_ptr, a_ptr, b_ptr, selector_ptr, error_ptr,
        stream if isinstance(stream, int) else _stream_ptr(stream)), 'ltmi_lattice_fit')


def lattice_last_kernel():
    """'k_lattice_fit' after the first launch of `lattice_fit` on this thread, '' before"""
    return lib().ltmi_lattice_last_kernel().decode()


def clear_last_runtime_error():
    """forget the HIP runtime's sticky 'last error' of this thread (set by a call that failed outside the
    library, e.g. a host registration that was refused) so that the next launch check does not report it"""
    lib().ltmi_device_count(ctypes.byref(ctypes.c_int(0)))


class Comm:
    """RCCL communicator behind the C ABI (`ltmi_comm*`): what a reference-side binding uses to
    gather nav results / reduce sig results across the GPUs of a node without torch.distributed."""

    ID_BYTES = 128

    @staticmethod
    def library_info():
        """-> dict(path, version, was_loaded): the librccl the communicators are bound to (the copy torch has
        mapped when the process runs torch.distributed -- never a second one)"""
        path = ctypes.create_string_buffer(1024)
        ver, was = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().ltmi_comm_library_info(path, 1024, ctypes.byref(ver), ctypes.byref(was)),
              'ltmi_comm_library_info')
        return dict(path=path.value.decode(), version=int(ver.value), was_loaded=bool(was.value))

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(Comm.ID_BYTES)
        check(lib().ltmi_comm_unique_id(buf), 'ltmi_comm_unique_id')
        return buf.raw

    def __init__(self, device, rank, world, unique_id):
        if len(unique_id) != self.ID_BYTES:
            raise ValueError(f"the RCCL unique id has {self.ID_BYTES} bytes")
        out = ctypes.c_void_p()
        check(lib().ltmi_comm_create(int(device), int(rank), int(world),
                                     ctypes.c_char_p(bytes(unique_id)), ctypes.byref(out)),
              'ltmi_comm_create')
        self._ptr = out
        self.rank, self.world = int(rank), int(world)

    def all_gather(self, send_ptr, recv_ptr, bytes_per_rank, stream=None):
        check(lib().ltmi_comm_all_gather(self._ptr, send_ptr, recv_ptr, int(bytes_per_rank),
                                         _stream_ptr(stream)), 'ltmi_comm_all_gather')

    def all_reduce_sum(self, buf_ptr, dtype, n, stream=None):
        check(lib().ltmi_comm_all_reduce_sum(self._ptr, buf_ptr, dtype_code(dtype), int(n),
                                             _stream_ptr(stream)), 'ltmi_comm_all_reduce_sum')

    def close(self):
        if self._ptr is not None and self._ptr.value:
            lib().ltmi_comm_destroy(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
