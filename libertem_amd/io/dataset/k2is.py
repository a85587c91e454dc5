"""
K2ISDataSet: raw Gatan K2 IS acquisitions (`ctx.load("k2is", path=...)`, reference io/dataset/k2is.py:727-1062):
8 sector files `*_1.bin` ... `*_8.bin`, each a sequence of blocks of 0x5758 bytes (40-byte big-endian header,
930 rows x 16 pixels packed 12 bit), 32 blocks per frame and sector, frames of 1860 x 2048.  The sectors are
synchronised on the host from their block headers alone, like the reference's K2Syncer (k2is.py:315-469); the
pixels are never touched on the host: where the reference decodes every block of every tile with two nested
numba loops (decode_k2is, k2is.py:104-164), `initialize()` streams the file bytes ONCE through pinned bounce
buffers into HBM, `ltmi_k2is_decode` (csrc/ltmi_k2is.hip) unpacks them behind each copy, and the dataset is a
device-resident uint16 array from then on.  An acquisition that does not fit is STREAMED per partition, as for
.mib files (mib.py).

Scan geometry: the time-series mode of the reference (no scan size known from a .gtg file): `nav_shape`
defaults to (frames with the shutter flag set,), `sync_offset=None` is the files' own offset (whole frames
minus frames with the shutter flag set, k2is.py:834-856), frames are counted from the first block with the
shutter flag set.  A scan position whose frame lies behind the last whole frame of the files is a zero frame.
Reading the scan size out of a .gtg file (a DM file, `ncempy` in the reference) is not part of this build: with
a .gtg beside the data `nav_shape` has to be passed.
"""
import os
import re
import glob

import numpy as np

from libertem_amd.common.math import prod
from libertem_amd.common.hiparray import HipArray
from .base import DataSetException, DataSetMeta
from .memory import MemoryDataSet
from .mib import MIBDataSet, _bounce_buffers

HEADER_SIZE = 40
BLOCK_SIZE = 0x5758
BLOCKS_PER_SECTOR_PER_FRAME = 32
NUM_SECTORS = 8
SECTOR_SIZE = (2 * 930, 256)
SIG_SHAPE = (SECTOR_SIZE[0], NUM_SECTORS * SECTOR_SIZE[1])
FRAME_BYTES_PER_SECTOR = BLOCKS_PER_SECTOR_PER_FRAME * BLOCK_SIZE
SYNC_WORD = 0xFFFF0055
SHUTTER_ACTIVE_MASK = 0x1

# (reference k2is.py:583-598; the padding is skipped)
HEADER_DTYPE = np.dtype({
    'names': ['sync', 'version', 'flags', 'block_count', 'width', 'height', 'frame_id', 'pixel_x_start',
              'pixel_y_start', 'pixel_x_end', 'pixel_y_end', 'block_size'],
    'formats': ['>u4', 'u1', 'u1', '>u4', '>u2', '>u2', '>u4', '>u2', '>u2', '>u2', '>u2', '>u4'],
    'offsets': [0, 8, 9, 16, 20, 22, 24, 28, 30, 32, 34, 36],
    'itemsize': HEADER_SIZE,
})


def _pattern(path):
    """reference k2is.py:239-250"""
    stem, ext = os.path.splitext(path)
    ext = ext.lower()
    if ext == ".gtg":
        return "%s*.bin" % glob.escape(stem)
    if ext == ".bin":
        return "%s*.bin" % glob.escape(re.sub(r'[0-9]+$', '', stem))
    raise DataSetException("unknown extension: %s" % ext)


def get_filenames(path):
    return glob.glob(_pattern(path))


def _get_gtg_path(path):
    stem, ext = os.path.splitext(path)
    if ext.lower() == ".gtg":
        return path
    return "%s.gtg" % re.sub(r'[0-9]+$', '', stem)


class _Sector:
    """the block headers of one sector file, as a strided view into its mapping (nothing is copied, a field of
    block i is read when it is indexed), and the blocks [first, last] that are in use"""

    def __init__(self, path, idx):
        self.path, self.idx = path, idx
        self.n_blocks = os.path.getsize(path) // BLOCK_SIZE
        if self.n_blocks == 0:
            raise DataSetException(f"{path} holds no whole block of {BLOCK_SIZE} bytes")
        self.map = np.memmap(path, dtype=np.uint8, mode='r')
        self.headers = np.ndarray(shape=(self.n_blocks,), dtype=HEADER_DTYPE, buffer=self.map,
                                  strides=(BLOCK_SIZE,))
        self.first, self.last = 0, self.n_blocks - 1

    def is_valid(self, i):
        h = self.headers[i]
        return bool(h['width'] == 256 and h['height'] == 1860 and h['sync'] == SYNC_WORD)

    def field(self, name, lo, hi):
        """`name` of the blocks [lo, hi), clipped to the blocks in use"""
        lo, hi = max(lo, self.first), min(hi, self.last + 1)
        return np.asarray(self.headers[name][lo:hi])

    def find(self, name, predicate, backwards=False):
        """first block in use (last, if `backwards`) whose field `name` satisfies `predicate`; None: no such block"""
        step = 4 * BLOCKS_PER_SECTOR_PER_FRAME
        if not backwards:
            for lo in range(self.first, self.last + 1, step):
                hit = np.flatnonzero(predicate(self.field(name, lo, lo + step)))
                if len(hit):
                    return lo + int(hit[0])
        else:
            for hi in range(self.last + 1, self.first, -step):
                lo = max(hi - step, self.first)
                hit = np.flatnonzero(predicate(self.field(name, lo, hi)))
                if len(hit):
                    return lo + int(hit[-1])
        return None

    def first_shutter_active(self):
        """first block in use with the shutter flag set, by bisection: the flag stays set once it is
        (reference k2is.py:549-576)"""
        flags = self.headers['flags']
        lo, hi = self.first, self.last
        if not int(flags[hi]) & SHUTTER_ACTIVE_MASK:
            return None
        while lo < hi:
            mid = (lo + hi) // 2
            if int(flags[mid]) & SHUTTER_ACTIVE_MASK:
                hi = mid
            else:
                lo = mid + 1
        return lo


def _require(cond, what):
    if not cond:
        raise DataSetException("failed to load dataset: %s" % what)


def _num_frames(sectors):
    s = sectors[0]
    return (s.last - s.first + 1) // BLOCKS_PER_SECTOR_PER_FRAME


def sync_sectors(sectors):
    """whole frames only, the same ones in every sector (reference K2Syncer.sync_sectors, k2is.py:345-420)"""
    n = BLOCKS_PER_SECTOR_PER_FRAME
    for s in sectors:
        _require(s.is_valid(s.first), f"the first block of {s.path} is not valid (sync word, width or height)")
    # a common first block_count
    target = max(int(s.headers[s.first]['block_count']) for s in sectors)
    for s in sectors:
        at = s.find('block_count', lambda v: v == target)
        _require(at is not None and s.is_valid(at), f"{s.path}: no block with block_count {target}")
        s.first = at
    # an incomplete first frame: the next 32 blocks of a sector carry more than one frame_id
    if any(len(np.unique(s.field('frame_id', s.first, s.first + n))) > 1 for s in sectors):
        frame_id = int(sectors[0].headers[sectors[0].first]['frame_id'])
        for s in sectors:
            at = s.find('frame_id', lambda v: v != frame_id)
            _require(at is not None and s.is_valid(at), f"{s.path}: no whole frame")
            s.first = at
    # the same from the end
    for s in sectors:
        _require(s.is_valid(s.last), f"the last block of {s.path} is not valid")
    target = min(int(s.headers[s.last]['block_count']) for s in sectors)
    for s in sectors:
        at = s.find('block_count', lambda v: v == target, backwards=True)
        _require(at is not None and s.is_valid(at), f"{s.path}: no block with block_count {target}")
        s.last = at
    if any(len(np.unique(s.field('frame_id', s.last + 1 - n, s.last + 1))) > 1 for s in sectors):
        frame_id = int(sectors[0].headers[sectors[0].last]['frame_id'])
        for s in sectors:
            at = s.find('frame_id', lambda v: v != frame_id, backwards=True)
            _require(at is not None and s.is_valid(at), f"{s.path}: no whole frame")
            s.last = at


def sync_to_first_frame(sectors):
    """reference K2Syncer.sync_to_first_frame, k2is.py:422-427"""
    for s in sectors:
        at = s.first_shutter_active()
        _require(at is not None, f"{s.path}: no block with the shutter flag set")
        s.first = at


def validate_sync(sectors):
    """first and last frame of every sector whole, with one frame_id (reference k2is.py:429-454)"""
    n = BLOCKS_PER_SECTOR_PER_FRAME
    for name, window in (('first', lambda s: (s.first, s.first + n)), ('last', lambda s: (s.last + 1 - n, s.last + 1))):
        frame_id = None
        for s in sectors:
            ids = s.field('frame_id', *window(s))
            _require(s.is_valid(getattr(s, name)), f"the {name} block of {s.path} is not valid")
            frame_id = int(ids[0]) if frame_id is None else frame_id
            _require(len(ids) == n and bool(np.all(ids == frame_id)),
                     f"the {name} frame of {s.path} is not whole or not frame {frame_id}")


class K2ISDataSet(MemoryDataSet):
    """
    Parameters (reference k2is.py:733-755)
    ----------
    path : str
        one of the 8 .bin files of the acquisition
    nav_shape : tuple of int, optional
        default: (frames with the shutter flag set,)
    sig_shape : tuple of int, optional
        same number of pixels as (1860, 2048)
    sync_offset : int, optional
        > 0: frames to skip at the start; < 0: blank frames inserted at the start; None: the files' own offset
        (whole frames minus frames with the shutter flag set)
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: decode and hold only this rank's block of the first nav axis
    """
    CHUNK_BYTES = MIBDataSet.CHUNK_BYTES         # file bytes per copy + decode step (two in flight)
    COPY_THREADS = MIBDataSet.COPY_THREADS
    #: as for .mib files: decoded bytes this process may keep in HBM (None: what is free); more is streamed
    MAX_RESIDENT_BYTES = None
    STREAM_WINDOW_BYTES = MIBDataSet.STREAM_WINDOW_BYTES

    def __init__(self, path, nav_shape=None, sig_shape=None, sync_offset=None, io_backend=None,
                 num_partitions=None, shard=None):
        if io_backend is not None:
            raise ValueError("alternative I/O backends are not part of this build")
        self._path = str(path)
        self._nav_arg = tuple(nav_shape) if nav_shape else None
        self._sig_arg = tuple(sig_shape) if sig_shape else None
        self._sync_offset_arg = None if sync_offset is None else int(sync_offset)
        self._num_partitions_arg = num_partitions
        self._shard_arg = shard
        self._scan = None
        self._sectors = None
        self._image_count = None
        self.decode_seconds = None
        self.decode_bytes = None
        self._streamed = None

    # --- host side: which files, which blocks -------------------------------------------------------
    def _get_files(self):
        files = get_filenames(self._path)
        if len(files) != NUM_SECTORS:
            raise DataSetException("expected %d files at %s, found %d" % (
                NUM_SECTORS, _pattern(self._path), len(files)))
        return sorted(files)

    def _scan_files(self):
        """Synchronise the 8 sectors from their headers -> dict(files, image_count, num_frames_w_shutter,
        native_sync_offset, sync_offset, nav_shape, first_offsets, last_offsets); `self._sectors` keeps the
        mappings"""
        files = self._get_files()
        if self._nav_arg is None and os.path.exists(_get_gtg_path(self._path)):
            raise DataSetException(
                f"{_get_gtg_path(self._path)}: reading the scan size from a .gtg file is not part of this "
                "build, please pass nav_shape")
        sectors = [_Sector(fn, i) for i, fn in enumerate(files)]
        sync_sectors(sectors)
        image_count = _num_frames(sectors)
        sync_to_first_frame(sectors)
        validate_sync(sectors)
        n_shutter = _num_frames(sectors)
        native = image_count - n_shutter
        # (time series, reference k2is.py:839-856: the user's offset, or the files' own)
        so = native if self._sync_offset_arg is None else self._sync_offset_arg
        if not -image_count < so < image_count:
            raise DataSetException(
                "sync_offset should be in (%s, %s), which is (-image_count, image_count)"
                % (-image_count, image_count))
        self._sectors = sectors
        return dict(files=files, image_count=image_count, num_frames_w_shutter=n_shutter,
                    native_sync_offset=native, sync_offset=so,
                    nav_shape=self._nav_arg if self._nav_arg is not None else (n_shutter,),
                    first_offsets=[s.first * BLOCK_SIZE for s in sectors],
                    last_offsets=[s.last * BLOCK_SIZE for s in sectors])

    def initialize(self, executor):
        device = getattr(executor, 'gpu_id', None)
        if device is None:
            raise DataSetException(
                "K2ISDataSet decodes the files on the GPU (ltmi_k2is_decode): the executor drives none")
        self._scan = scan = self._scan_files()
        nav_shape = tuple(scan['nav_shape'])
        sig_shape = self._sig_arg
        if sig_shape is None:
            sig_shape = SIG_SHAPE
        elif int(prod(sig_shape)) != int(prod(SIG_SHAPE)):
            raise DataSetException("sig_shape must be of size: %s" % int(prod(SIG_SHAPE)))
        n_nav = int(prod(nav_shape))
        self._image_count = scan['image_count']
        so = scan['sync_offset']
        # this process's block of scan positions [p0, p1)
        local_nav = nav_shape
        p0, p1 = 0, n_nav
        if self._shard_arg is not None:
            rank, world = int(self._shard_arg[0]), int(self._shard_arg[1])
            if nav_shape[0] % world:
                raise DataSetException(f"first nav axis {nav_shape[0]} does not split over {world} ranks")
            local_nav = (nav_shape[0] // world,) + tuple(nav_shape[1:])
            p0 = rank * int(prod(local_nav))
            p1 = p0 + int(prod(local_nav))
        self._streamed = None
        n_local = p1 - p0
        storage = np.dtype('uint16')
        frame_bytes = int(prod(SIG_SHAPE)) * storage.itemsize
        need = n_local * frame_bytes
        stride = NUM_SECTORS * FRAME_BYTES_PER_SECTOR
        if not self._fits_in_hbm(device, executor, need, stride, n_local):
            # an acquisition larger than the HBM it may take: windows of it, decoded per partition
            import torch
            free_bytes, _ = torch.cuda.mem_get_info(device)
            window = int(min(self.STREAM_WINDOW_BYTES, max(frame_bytes, free_bytes // 4)))
            if self.MAX_RESIDENT_BYTES is not None:
                window = int(min(window, max(frame_bytes, self.MAX_RESIDENT_BYTES)))
            want = -(-need // window)
            n_parts = max(int(self._num_partitions_arg or 1), int(want))
            self._streamed = dict(device=device, executor=executor, p0=p0, sync_offset=so, key=None,
                                  frames=None)
            self.decode_seconds, self.decode_bytes = 0.0, 0
            placeholder = torch.empty(1, dtype=torch.uint8, device=f'cuda:{device}')
            frames = HipArray(placeholder, (n_local,) + SIG_SHAPE, storage)
            MemoryDataSet.__init__(
                self, data=frames.reshape(local_nav + tuple(sig_shape)), sig_dims=len(sig_shape),
                num_partitions=min(n_parts, max(1, n_local)), shard=self._shard_arg)
        else:
            frames = self._decode_to_device(device, executor, p0, p1, so)
            MemoryDataSet.__init__(
                self, data=frames.reshape(local_nav + tuple(sig_shape)), sig_dims=len(sig_shape),
                num_partitions=self._num_partitions_arg, shard=self._shard_arg)
        self._sync_offset = so
        # scan positions that hold a frame of the files (frame g, counted from the first one with the shutter
        # flag set, sits at g - so): the rest are the zero frames decoded above
        lo = min(n_nav, max(0, -so))
        hi = max(lo, min(n_nav, scan['num_frames_w_shutter'] - so))
        self._valid_frames = None if (lo, hi) == (0, n_nav) else (lo, hi)
        self._meta = DataSetMeta(shape=self._shape, raw_dtype=storage, sync_offset=so,
                                 image_count=self._image_count)
        return MemoryDataSet.initialize(self, executor)

    def _decode_to_device(self, device, executor, p0, p1, sync_offset):
        """scan positions [p0, p1) -> HipArray (p1 - p0, 1860, 2048) uint16"""
        import time
        import torch
        from libertem_amd import hip
        from concurrent.futures import ThreadPoolExecutor
        h, w = SIG_SHAPE
        stride = NUM_SECTORS * FRAME_BYTES_PER_SECTOR           # file bytes of a frame, all sectors
        storage = np.dtype('uint16')
        n = p1 - p0
        g0 = max(p0 + sync_offset, 0)
        g1 = min(p1 + sync_offset, self._scan['num_frames_w_shutter'])
        n_src = max(0, g1 - g0)
        if getattr(executor, '_make_current', None) is not None:
            executor._make_current()
        need = n * h * w * storage.itemsize
        free_bytes, _ = torch.cuda.mem_get_info(device)
        if need + 2 * min(self.CHUNK_BYTES, max(n_src, 1) * stride) > free_bytes:
            raise DataSetException(
                f"{n} decoded frames of {h}x{w} {storage} need {need / 2**30:.1f} GiB of HBM, "
                f"{free_bytes / 2**30:.1f} GiB are free on GPU {device}: fewer frames per partition "
                "(num_partitions), a part of the scan (nav_shape + sync_offset) or a shard per GPU "
                "(shard=(rank, world))")
        t0 = time.perf_counter()
        out = HipArray.empty((n, h, w), storage, device) if n_src == n else \
            HipArray.zeros((n, h, w), storage, device)          # blank frames stay zero
        if n_src > 0:
            chunk = int(max(1, min(n_src, self.CHUNK_BYTES // stride)))
            pinned = _bounce_buffers(torch, chunk * stride)
            raw = [torch.empty(chunk * stride, dtype=torch.uint8, device=f'cuda:{device}')
                   for _ in range(2)]
            free = [None, None]
            copy_stream = torch.cuda.Stream(device=device)
            copy_stream.wait_stream(torch.cuda.current_stream(device))     # (the zero fill)
            pool = ThreadPoolExecutor(self.COPY_THREADS)
            for i, c0 in enumerate(range(g0, g1, chunk)):
                c1 = min(g1, c0 + chunk)
                slot = i & 1
                if free[slot] is not None:
                    free[slot].synchronize()
                host = pinned[slot].numpy()
                # the chunk's 8 byte ranges, sector after sector (each a multiple of 8 bytes long)
                part = (c1 - c0) * FRAME_BYTES_PER_SECTOR
                for s in self._sectors:
                    self._host_copy(pool, host, s.idx * part, s.map,
                                    s.first * BLOCK_SIZE + c0 * FRAME_BYTES_PER_SECTOR, part)
                nb = NUM_SECTORS * part
                with torch.cuda.stream(copy_stream):
                    raw[slot][:nb].copy_(pinned[slot][:nb], non_blocking=True)
                    dst = out.rows(c0 - sync_offset - p0, c1 - sync_offset - p0)
                    base = raw[slot].data_ptr()
                    hip.k2is_decode(device, [base + k * part for k in range(NUM_SECTORS)], c1 - c0,
                                    dst.data_ptr(), storage, stream=copy_stream.cuda_stream)
                    ev = torch.cuda.Event()
                    ev.record(copy_stream)
                    free[slot] = ev
            copy_stream.synchronize()
            pool.shutdown()
        torch.cuda.current_stream(device).synchronize()
        if self._streamed is not None:
            self.decode_seconds += time.perf_counter() - t0
            self.decode_bytes += n_src * stride
        else:
            self.decode_seconds = time.perf_counter() - t0
            self.decode_bytes = n_src * stride
        return out

    # the HBM budget, the window of a streamed partition and the threaded host copy are those of .mib files
    _fits_in_hbm = MIBDataSet._fits_in_hbm
    device_frames = MIBDataSet.device_frames
    _host_copy = staticmethod(MIBDataSet._host_copy)

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
                "this K2IS acquisition is streamed (larger than the HBM it may take): there is no resident "
                "array of its frames -- run UDFs over it, or load a part (nav_shape + sync_offset)")
        return MemoryDataSet.data.fget(self)

    # --- the reference's descriptive surface --------------------------------------------------------
    @property
    def path(self):
        return self._path

    @property
    def storage_dtype(self):
        return np.dtype('uint16')

    def get_diagnostics(self):
        scan = self._scan
        return [{"name": "first block offsets for all sectors",
                 "value": ", ".join(str(o) for o in scan['first_offsets'])},
                {"name": "last block offsets for all sectors",
                 "value": ", ".join(str(o) for o in scan['last_offsets'])},
                {"name": "number of frames before sync (from first sector)",
                 "value": str(scan['image_count'])},
                {"name": "number of frames after sync (from first sector)",
                 "value": str(scan['num_frames_w_shutter'])}]

    @classmethod
    def get_supported_extensions(cls):
        return {"gtg", "bin"}

    @classmethod
    def detect_params(cls, path, executor=None):
        """reference k2is.py:894-929 (without a .gtg: a square scan if the frames make one)"""
        try:
            if len(get_filenames(path)) != NUM_SECTORS or os.path.exists(_get_gtg_path(path)):
                return False
            scan = cls(path=path)._scan_files()
        except (DataSetException, OSError):
            return False
        n = scan['num_frames_w_shutter']
        side = int(np.sqrt(n))
        nav_shape = (side, side) if side * side == n else (n,)
        return {"parameters": {"path": path, "nav_shape": nav_shape, "sig_shape": SIG_SHAPE,
                               "sync_offset": scan['native_sync_offset']},
                "info": {"image_count": scan['image_count'], "native_sig_shape": SIG_SHAPE}}

    def get_cache_key(self):
        return {"gtg_path": _get_gtg_path(self._path), "shape": tuple(self.shape),
                "sync_offset": self._sync_offset}

    def __repr__(self):
        if self._scan is None:
            return f"<K2ISDataSet for pattern={_pattern(self._path)} (not initialized)>"
        return f"<K2ISDataSet for pattern={_pattern(self._path)} nav_shape={tuple(self._scan['nav_shape'])}>"
