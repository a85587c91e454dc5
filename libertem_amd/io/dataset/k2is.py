"""
K2ISDataSet: raw Gatan K2 IS acquisitions (`ctx.load("k2is", path=...)`, reference io/dataset/k2is.py:727-1062):
8 sector files `*_1.bin` ... `*_8.bin`, each a sequence of blocks of 0x5758 bytes (40-byte big-endian header,
930 rows x 16 pixels packed 12 bit), 32 blocks per frame and sector, frames of 1860 x 2048.  The sectors are
synchronised on the host from their block headers alone, like the reference's K2Syncer (k2is.py:315-469); the
pixels are never touched on the host: where the reference decodes every block of every tile with two nested
numba loops (decode_k2is, k2is.py:104-164), `initialize()` streams the file bytes ONCE through pinned bounce
buffers into HBM, `ltmi_k2is_decode` (csrc/ltmi_k2is.hip) unpacks them behind each copy, and the dataset is a
device-resident uint16 array from then on.  An acquisition that does not fit is STREAMED per partition
(decoded.py).

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
from .base import DataSetException, DataSetMeta
from .memory import MemoryDataSet
from .decoded import DecodedFileDataSet, FrameLayout, _host_copy

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


class K2ISDataSet(DecodedFileDataSet):
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
    KIND = "K2IS acquisition"
    DECODE_KERNEL = "ltmi_k2is_decode"

    def __init__(self, path, nav_shape=None, sig_shape=None, sync_offset=None, io_backend=None,
                 num_partitions=None, shard=None):
        DecodedFileDataSet.__init__(self, path, num_partitions, shard, io_backend)
        self._nav_arg = tuple(nav_shape) if nav_shape else None
        self._sig_arg = tuple(sig_shape) if sig_shape else None
        self._sync_offset_arg = None if sync_offset is None else int(sync_offset)
        self._scan = None
        self._sectors = None

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
        device = self._gpu_of(executor)
        self._scan = scan = self._scan_files()
        nav_shape = tuple(scan['nav_shape'])
        sig_shape = self._sig_arg
        if sig_shape is None:
            sig_shape = SIG_SHAPE
        elif int(prod(sig_shape)) != int(prod(SIG_SHAPE)):
            raise DataSetException("sig_shape must be of size: %s" % int(prod(SIG_SHAPE)))
        self._image_count = scan['image_count']
        so = scan['sync_offset']
        storage = np.dtype('uint16')
        # (frames are counted from the first one with the shutter flag set)
        self._load_frames(executor, device, FrameLayout(
            nav_shape=nav_shape, sig_shape=sig_shape, native_shape=SIG_SHAPE, storage=storage,
            stride=NUM_SECTORS * FRAME_BYTES_PER_SECTOR, n_frames=scan['num_frames_w_shutter'], sync_offset=so))
        self._meta = DataSetMeta(shape=self._shape, raw_dtype=storage, sync_offset=so,
                                 image_count=self._image_count)
        return MemoryDataSet.initialize(self, executor)

    def _frame_source(self, device):
        from libertem_amd import hip

        def fill(pool, host, g, n):
            # the chunk's 8 byte ranges, sector after sector (each a multiple of 8 bytes long)
            part = n * FRAME_BYTES_PER_SECTOR
            for s in self._sectors:
                _host_copy(pool, host, s.idx * part, s.map, s.first * BLOCK_SIZE + g * FRAME_BYTES_PER_SECTOR, part)
            return n

        def decode(src_ptr, n, dst_ptr, stream):
            part = n * FRAME_BYTES_PER_SECTOR
            hip.k2is_decode(device, [src_ptr + k * part for k in range(NUM_SECTORS)], n, dst_ptr, np.uint16,
                            stream=stream)
        return fill, decode

    # --- the reference's descriptive surface --------------------------------------------------------
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
