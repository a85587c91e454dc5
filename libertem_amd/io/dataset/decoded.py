"""
DecodedFileDataSet: what the file formats that are decoded on the GPU share (.mib, K2IS, FRMS6).  `initialize()`
streams the file bytes ONCE through two pinned bounce buffers into HBM, a decode kernel runs behind each copy on
the copy stream, and the dataset is a device-resident `MemoryDataSet` from then on.  A block of the scan that
does not fit is STREAMED instead: each partition decodes its frames from the files into one window of HBM when
its tiles are asked for (`device_frames`), every run re-reads the files.

A format supplies: its host side (which files, which frames, the checks of its parameters), a
`FrameLayout` handed to `_load_frames()`, `_frame_source()` -- the two hooks `fill` (file bytes -> host buffer)
and `decode` (enqueue the kernel) --, its `DataSetMeta`, and the descriptive surface.
"""
from collections import namedtuple

import numpy as np

from libertem_amd.common.math import prod
from libertem_amd.common.hiparray import HipArray
from .base import DataSetException
from .memory import MemoryDataSet

#: nav_shape, sig_shape: of the whole scan, as the dataset reports them; native_shape: of a decoded frame in HBM
#: (as many pixels as sig_shape); storage: dtype of the decoded pixels; stride: file bytes per frame; n_frames:
#: frames present in the files (frame g sits at scan position g - sync_offset)
FrameLayout = namedtuple('FrameLayout', 'nav_shape sig_shape native_shape storage stride n_frames sync_offset')


# --- the arithmetic of blocks, offsets and windows: integers and tuples only ---------------------------------
def shard_block(nav_shape, shard):
    """-> (local_nav, p0, p1): the block of scan positions [p0, p1) of `shard = (rank, world)`, a share of the
    first nav axis, and its nav shape; all of the scan for `shard = None`"""
    nav_shape = tuple(int(n) for n in nav_shape)
    if shard is None:
        return nav_shape, 0, int(prod(nav_shape))
    rank, world = int(shard[0]), int(shard[1])
    if nav_shape[0] % world:
        raise DataSetException(f"first nav axis {nav_shape[0]} does not split over {world} ranks")
    local_nav = (nav_shape[0] // world,) + nav_shape[1:]
    p0 = rank * int(prod(local_nav))
    return local_nav, p0, p0 + int(prod(local_nav))


def source_range(p0, p1, sync_offset, n_frames):
    """-> (g0, g1), g0 <= g1: the frames of the files that land on the scan positions [p0, p1); frame g sits at
    position g - sync_offset"""
    g0 = max(p0 + sync_offset, 0)
    return g0, max(g0, min(p1 + sync_offset, n_frames))


def valid_range(n_nav, n_frames, sync_offset):
    """-> None | (lo, hi): the scan positions that hold a frame of the files; None: all `n_nav` do"""
    lo = min(n_nav, max(0, -sync_offset))
    hi = max(lo, min(n_nav, n_frames - sync_offset))
    return None if (lo, hi) == (0, n_nav) else (lo, hi)


def stream_window(need, frame_bytes, n_local, free_bytes, window_bytes, max_resident, num_partitions):
    """-> (window, n_parts) of a streamed block of `n_local` frames, `need` decoded bytes in all: the bytes of HBM
    a partition's frames may take -- `window_bytes`, a quarter of what is free and `max_resident` (None: no such
    limit) bound it, one frame is the least -- and the partitions that takes, no fewer than asked for"""
    limits = (window_bytes, free_bytes // 4) + (() if max_resident is None else (max_resident,))
    window = int(max(frame_bytes, min(limits)))
    n_parts = max(int(num_partitions or 1), -(-need // window))
    return window, min(n_parts, max(1, n_local))


# --- host side of the pipeline ---------------------------------------------------------------------------------
_BOUNCE = {}


def _bounce_buffers(torch, nbytes):
    """two page-locked host buffers of at least `nbytes`, kept for the next load (page-locking 256 MiB
    costs ~16 ms)"""
    have = _BOUNCE.get('bufs')
    if have is None or have[0].numel() < nbytes:
        _BOUNCE['bufs'] = have = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
    return have


def _host_copy(pool, dst, dst_off, src, src_off, nbytes, piece=16 << 20):
    """file mapping -> pinned buffer on several threads (one memcpy stream reads the page cache at
    ~12 GB/s, a fifth of what the host link takes)"""
    if nbytes <= piece:
        dst[dst_off:dst_off + nbytes] = src[src_off:src_off + nbytes]
        return
    try:
        # the library's copy pool: one thread per L3 domain of the host (csrc/ltmi_capi.cpp)
        from libertem_amd import hip
        hip.host_copy(dst[dst_off:dst_off + nbytes], np.asarray(src[src_off:src_off + nbytes]))
        return
    except Exception:                               # noqa: BLE001  (e.g. a source that is not contiguous)
        pass

    def run(o):
        n = min(piece, nbytes - o)
        dst[dst_off + o:dst_off + o + n] = src[src_off + o:src_off + o + n]
    list(pool.map(run, range(0, nbytes, piece)))


class DecodedFileDataSet(MemoryDataSet):
    CHUNK_BYTES = 256 << 20          # file bytes per copy + decode step (two in flight)
    COPY_THREADS = 8
    #: decoded bytes this process may keep in HBM (None: what is free).  A block of the scan that needs more
    #: is STREAMED: no frame is decoded at load time, every partition decodes its frames from the files
    #: into a window of HBM when its tiles are asked for (partitions of at most STREAM_WINDOW_BYTES).
    MAX_RESIDENT_BYTES = None
    STREAM_WINDOW_BYTES = 4 << 30

    #: what the format calls its files ("this ... is streamed") and the library call that decodes them
    KIND = None
    DECODE_KERNEL = None

    def __init__(self, path, num_partitions, shard, io_backend=None):
        if io_backend is not None:
            raise ValueError("alternative I/O backends are not part of this build")
        self._path = str(path)
        self._num_partitions_arg = num_partitions
        self._shard_arg = shard
        self._layout = None
        self._image_count = None
        self.decode_seconds = None
        self.decode_bytes = None
        self._streamed = None

    def _frame_source(self, device):
        """-> (fill, decode), the format's part of one run of the pipeline:
        `fill(pool, host, g, n_max) -> n` copies the file bytes of `1 <= n <= n_max` frames from frame `g` on to
        the start of the uint8 array `host` (`_host_copy` with `pool`), `n * stride` bytes;
        `decode(src_ptr, n, dst_ptr, stream)` enqueues the decode of these `n` frames, uploaded to `src_ptr`."""
        raise NotImplementedError

    def _gpu_of(self, executor):
        device = getattr(executor, 'gpu_id', None)
        if device is None:
            raise DataSetException(f"{type(self).__name__} decodes the files on the GPU ({self.DECODE_KERNEL}): "
                                   "the executor drives none")
        return device

    def _load_frames(self, executor, device, layout):
        """the common half of `initialize()`: this process's block of the scan resident in HBM, or set up to be
        streamed; leaves `_meta` and `MemoryDataSet.initialize` to the format"""
        import torch
        self._layout = layout
        native, sig_shape, storage = tuple(layout.native_shape), tuple(layout.sig_shape), np.dtype(layout.storage)
        so = layout.sync_offset
        local_nav, p0, p1 = shard_block(layout.nav_shape, self._shard_arg)
        self._streamed = None
        n_local = p1 - p0
        frame_bytes = int(prod(native)) * storage.itemsize
        need = n_local * frame_bytes
        if not self._fits_in_hbm(device, executor, need, layout.stride, n_local):
            # more than the HBM it may take: windows of it, decoded per partition
            free_bytes, _ = torch.cuda.mem_get_info(device)
            _, n_parts = stream_window(need, frame_bytes, n_local, free_bytes, self.STREAM_WINDOW_BYTES,
                                       self.MAX_RESIDENT_BYTES, self._num_partitions_arg)
            self._streamed = dict(device=device, executor=executor, p0=p0, sync_offset=so, key=None,
                                  frames=None)
            self.decode_seconds, self.decode_bytes = 0.0, 0
            placeholder = torch.empty(1, dtype=torch.uint8, device=f'cuda:{device}')
            frames = HipArray(placeholder, (n_local,) + native, storage)
        else:
            n_parts = self._num_partitions_arg
            frames = self._decode_to_device(device, executor, p0, p1, so)
        MemoryDataSet.__init__(self, data=frames.reshape(local_nav + sig_shape), sig_dims=len(sig_shape),
                               num_partitions=n_parts, shard=self._shard_arg)
        self._sync_offset = so
        # scan positions that hold a frame of the files (global positions): the rest are the zero frames decoded
        # above, which UDFs with `VALID_FRAMES_ONLY` -- and, under a dark frame, all UDFs -- are not handed
        # (udf/base.py `_skips_frameless`)
        self._valid_frames = valid_range(int(prod(layout.nav_shape)), layout.n_frames, so)

    def _fits_in_hbm(self, device, executor, need, stride, n_local):
        import torch
        if getattr(executor, '_make_current', None) is not None:
            executor._make_current()
        if self.MAX_RESIDENT_BYTES is not None and need > self.MAX_RESIDENT_BYTES:
            return False
        free_bytes, _ = torch.cuda.mem_get_info(device)
        return need + 2 * min(self.CHUNK_BYTES, max(n_local, 1) * stride) <= free_bytes

    def _upload_and_decode(self, device, source, g0, g1, consume):
        """Frames [g0, g1) of `source = (fill, decode)` (`_frame_source`) -> device, in chunks of whole frames, two
        in flight: file bytes into a pinned bounce buffer, one copy to the device, then, on the copy stream,
        `consume(c0, c1, decode, copy_stream)` with `decode(dst_ptr)` enqueueing the decode of the chunk's frames
        [c0, c1)."""
        import torch
        from concurrent.futures import ThreadPoolExecutor
        fill, decode = source
        stride = self._layout.stride
        chunk = int(max(1, min(g1 - g0, self.CHUNK_BYTES // stride)))
        pinned = _bounce_buffers(torch, chunk * stride)
        raw = [torch.empty(chunk * stride, dtype=torch.uint8, device=f'cuda:{device}') for _ in range(2)]
        free = [None, None]
        copy_stream = torch.cuda.Stream(device=device)
        copy_stream.wait_stream(torch.cuda.current_stream(device))     # (the zero fill)
        pool = ThreadPoolExecutor(self.COPY_THREADS)
        i, g = 0, g0
        while g < g1:
            slot = i & 1
            if free[slot] is not None:
                free[slot].synchronize()
            n = fill(pool, pinned[slot].numpy(), g, min(chunk, g1 - g))
            nb = n * stride
            with torch.cuda.stream(copy_stream):
                raw[slot][:nb].copy_(pinned[slot][:nb], non_blocking=True)

                def decode_chunk(dst_ptr, src_ptr=raw[slot].data_ptr(), n=n):
                    decode(src_ptr, n, dst_ptr, copy_stream.cuda_stream)
                consume(g, g + n, decode_chunk, copy_stream)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
                free[slot] = ev
            g += n
            i += 1
        copy_stream.synchronize()
        pool.shutdown()

    def _decode_to_device(self, device, executor, p0, p1, sync_offset):
        """scan positions [p0, p1) -> HipArray (p1 - p0,) + native frame shape, of the storage dtype"""
        import time
        import torch
        lay = self._layout
        storage = np.dtype(lay.storage)
        n = p1 - p0
        shape = (n,) + tuple(lay.native_shape)
        g0, g1 = source_range(p0, p1, sync_offset, lay.n_frames)
        n_src = g1 - g0
        if getattr(executor, '_make_current', None) is not None:
            executor._make_current()
        need = int(prod(shape)) * storage.itemsize
        free_bytes, _ = torch.cuda.mem_get_info(device)
        if need + 2 * min(self.CHUNK_BYTES, max(n_src, 1) * lay.stride) > free_bytes:
            raise DataSetException(
                f"{n} decoded frames of {shape[1]}x{shape[2]} {storage} need {need / 2**30:.1f} GiB of HBM, "
                f"{free_bytes / 2**30:.1f} GiB are free on GPU {device}: fewer frames per partition "
                "(num_partitions), a part of the scan (nav_shape + sync_offset) or a shard per GPU "
                "(shard=(rank, world))")
        t0 = time.perf_counter()
        out = HipArray.empty(shape, storage, device) if n_src == n else \
            HipArray.zeros(shape, storage, device)              # blank frames stay zero
        if n_src > 0:
            def consume(c0, c1, decode, copy_stream):
                decode(out.rows(c0 - sync_offset - p0, c1 - sync_offset - p0).data_ptr())
            self._upload_and_decode(device, self._frame_source(device), g0, g1, consume)
        torch.cuda.current_stream(device).synchronize()
        if self._streamed is not None:
            self.decode_seconds += time.perf_counter() - t0
            self.decode_bytes += n_src * lay.stride
        else:
            self.decode_seconds = time.perf_counter() - t0
            self.decode_bytes = n_src * lay.stride
        return out

    def device_frames(self, local0, n):
        st = self._streamed
        if st is None:
            return MemoryDataSet.device_frames(self, local0, n)
        if st['key'] != (local0, n):
            st['frames'] = None                     # (one window at a time)
            st['key'] = None
            p = st['p0'] + local0
            st['frames'] = self._decode_to_device(st['device'], st['executor'], p, p + n,
                                                  st['sync_offset'])
            st['key'] = (local0, n)
        return st['frames'], 0

    @property
    def stable_device_tiles(self):
        return self._streamed is None

    @property
    def is_streamed(self):
        """the decoded frames do not stay in HBM: every partition decodes its own from the files"""
        return self._streamed is not None

    @property
    def data(self):
        if self._streamed is not None:
            raise DataSetException(
                f"this {self.KIND} is streamed (larger than the HBM it may take): there is no resident "
                "array of its frames -- run UDFs over it, or load a part (nav_shape + sync_offset)")
        return MemoryDataSet.data.fget(self)

    @property
    def path(self):
        return self._path
