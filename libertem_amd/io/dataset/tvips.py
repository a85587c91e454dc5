"""
TVIPSDataSet: series of TVIPS camera files (`ctx.load("tvips", path=...)`, reference io/dataset/tvips.py).  A camera
writes `name_000.tvips`, `name_001.tvips`, ...; any of them names the set.  `_000` starts with the series header
(256 bytes: thirteen little-endian int32, then padding), and every file is records `[image header | pixels]` of 8-
or 16-bit pixels; the image header has 12 bytes in version 1 and as many as the series header says in version 2.
The frames go to HBM through `RecordFileDataSet`, one segment per file.

Version-2 image headers hold the scan position of their frame; from these `sync_offset` and `nav_shape` are guessed
as the reference guesses them (`detect_shape`).  Two deliberate differences, both where the reference raises
(DESIGN.md 4.11): the series header is always read from the first file of the set, whichever file was named; and
the image header of frame `idx` is read from the file that holds frame `idx`, not at that index in the first file.
"""
import os
import re
from collections import namedtuple
from glob import glob, escape

import numpy as np

from libertem_amd.common.math import make_2D_square
from .base import DataSetException
from .records import RecordFileDataSet, Segment, locate

SERIES_HEADER_SIZE = 256
#: the int32 words of the series header, in the order of the file
SERIES_FIELDS = ('size', 'version', 'xdim', 'ydim', 'bpp', 'xoff', 'yoff', 'xbin', 'ybin', 'pixel_size_nm',
                 'high_tension_kv', 'mag_total', 'frame_header_bytes')
SeriesHeader = namedtuple('SeriesHeader', SERIES_FIELDS)
V1_FRAME_HEADER_BYTES = 12
#: bytes of Scan_x, Scan_y (float32) in a version-2 image header: behind 17 four-byte fields
SCAN_X_OFFSET = 68
MAX_SCAN_IDX = 4096         # the start of the scan is looked for up to this frame


class DetectionError(Exception):
    pass


def read_series_header(path):
    """-> SeriesHeader of the first file of a set (`frame_header_bytes`: 12 for version 1)"""
    try:
        with open(path, 'rb') as f:
            raw = f.read(4 * len(SERIES_FIELDS))
    except OSError as e:
        raise DataSetException("could not open file %s: %s" % (path, e))
    if len(raw) < 4 * len(SERIES_FIELDS):
        raise DataSetException("%s is shorter than a TVIPS series header" % path)
    header = SeriesHeader(*(int(v) for v in np.frombuffer(raw, dtype='<i4')))
    if header.version not in (1, 2):
        raise DataSetException(f"Unknown TVIPS header version: {header.version}")
    if header.size != SERIES_HEADER_SIZE:
        raise DataSetException(f"Invalid header size {header.size}, should be 256. Maybe not a TVIPS file?")
    if header.bpp not in (8, 16):
        raise DataSetException(f"unknown bpp value: {header.bpp} (should be either 8 or 16)")
    if header.version == 1:
        header = header._replace(frame_header_bytes=V1_FRAME_HEADER_BYTES)
    return header


def payload_bytes(header):
    return header.bpp // 8 * header.xdim * header.ydim


def file_suffix(path):
    """the number of a file of a series: its stem ends in an underscore and three digits"""
    stem = os.path.splitext(path)[0]
    try:
        return int(stem[-3:])
    except ValueError:
        raise DataSetException("%s does not end in the three digits of a TVIPS series" % path)


def get_filenames(path):
    """the files of the set that `path` is one of, in the order of their numbers"""
    stem, ext = os.path.splitext(str(path))
    if ext.lower() != '.tvips':
        raise DataSetException("unknown extension")
    files = sorted(glob("%s*.tvips" % re.sub(r'[0-9]+$', '', escape(stem))), key=file_suffix)
    if not files:
        raise DataSetException("no files found for %s" % path)
    return files


def frames_in_file(path, header):
    """-> (bytes in front of the first record, records) of one file of a set"""
    try:
        size = os.stat(path).st_size
    except OSError as e:
        raise DataSetException("could not open file %s: %s" % (path, e))
    file_header = SERIES_HEADER_SIZE if file_suffix(path) == 0 else 0
    stride = header.frame_header_bytes + payload_bytes(header)
    if stride < 1 or payload_bytes(header) < 1 or header.frame_header_bytes < 0:
        raise DataSetException("%s: image headers of %d bytes, images of %d x %d pixels" % (
            path, header.frame_header_bytes, header.ydim, header.xdim))
    count, rest = divmod(max(0, size - file_header), stride)
    if rest or size < file_header:
        raise DataSetException("%s: found a rest of %d bytes behind %d frames of %d bytes, corrupted file?" % (
            path, rest, count, stride))
    return file_header, count


def scan_set(path):
    """-> (SeriesHeader, segments): the series header, from the first file of the set, and one `Segment` per file"""
    files = get_filenames(path)
    header = read_series_header(files[0])
    segments, first = [], 0
    for name in files:
        file_header, count = frames_in_file(name, header)
        segments.append(Segment(name, file_header, first, count))
        first += count
    return header, segments


def detect_shape(header, segments):
    """-> (sync_offset, nav_shape), guessed from Scan_x and Scan_y of the image headers of a version-2 set: the
    scan starts one frame before the first (y, x) = (0, 1) that follows a (0, 0), and a row is as long as x grows
    from there.  DetectionError where that start is not found (reference tvips.py:219-267)"""
    if header.version != 2:
        raise DetectionError("unknown series header version, can only detect shape from v2")
    stride = header.frame_header_bytes + payload_bytes(header)
    count = sum(seg.n_frames for seg in segments)
    limit = min(MAX_SCAN_IDX, count)
    handles = {}

    def scan_of(idx):
        i, offset, _ = locate(idx, 1, segments, stride)
        if i not in handles:
            handles[i] = open(segments[i].path, 'rb')
        handles[i].seek(offset + SCAN_X_OFFSET)
        raw = handles[i].read(8)
        try:
            x, y = (int(v) for v in np.frombuffer(raw, dtype='<f4', count=2))
        except (ValueError, OverflowError) as e:        # (the file ends here; not a number)
            raise DetectionError("no scan position in the image header of frame %d: %s" % (idx, e))
        return y, x

    try:
        idx, sync_offset, seen_zero = 0, None, False            # (`seen_zero` is never cleared, as in the reference)
        while idx < limit:
            scan = scan_of(idx)
            if seen_zero and scan == (0, 1):
                sync_offset = idx - 1
                break
            if scan == (0, 0):
                seen_zero = True
            idx += 1
        if sync_offset is None:
            raise DetectionError("Could not auto-detect sync_offset")
        max_x, found = 0, False
        while idx < limit:
            x = scan_of(idx)[1]
            max_x = max(max_x, x)
            if x < max_x:
                found = True
                break
            idx += 1
    finally:
        for f in handles.values():
            f.close()
    if found:
        return sync_offset, ((count - sync_offset) // (max_x + 1), max_x + 1)
    return sync_offset, (count,)


class TVIPSDataSet(RecordFileDataSet):
    """
    Parameters (reference tvips.py:281-347)
    ----------
    path : str
        any file of the set
    nav_shape : tuple of int, optional
        default: guessed from the image headers of a version-2 set, else (frames,)
    sig_shape : tuple of int, optional
        same number of pixels as (height, width) of the series header
    sync_offset : int, optional
        > 0: frames to skip at the start; < 0: blank frames inserted at the start; default: guessed from the image
        headers of a version-2 set, else 0
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: load and hold only this rank's block of the first nav axis
    """
    KIND = "TVIPS series"

    def __init__(self, path, nav_shape=None, sig_shape=None, sync_offset=None, io_backend=None, num_partitions=None,
                 shard=None):
        RecordFileDataSet.__init__(self, path, nav_shape, sig_shape, 0, io_backend, num_partitions, shard)
        self._sync_offset_given = None if sync_offset is None else int(sync_offset)
        self._header = None

    def _scan_file(self):
        """-> FrameLayout, from the series header, the sizes of the files and, where the caller left `sync_offset`
        or `nav_shape` open, the image headers"""
        header, segments = scan_set(self._path)
        self._header = header
        image_count = sum(seg.n_frames for seg in segments)
        try:
            sync_offset, nav_shape = detect_shape(header, segments)
        except DetectionError:
            sync_offset, nav_shape = 0, (image_count,)
        # what the caller passed wins, each on its own
        self._sync_offset_arg = sync_offset if self._sync_offset_given is None else self._sync_offset_given
        return self._segments_layout(
            segments, frame_header=header.frame_header_bytes, payload_bytes=payload_bytes(header), frame_footer=0,
            storage=np.dtype('u%d' % (header.bpp // 8)), native_shape=(header.ydim, header.xdim),
            nav_shape=self._nav_arg if self._nav_arg is not None else nav_shape)

    def initialize(self, executor):
        self._gpu_of(executor)
        return self._load_records(executor, self._scan_file())

    @property
    def header(self):
        if self._header is None:
            raise RuntimeError("please call initialize() before using the dataset")
        return self._header

    def check_valid(self):
        try:
            if self._records is None:
                self._scan_file()
            for seg in self._records['segments']:
                with open(seg.path, 'rb'):
                    pass
            return True
        except (OSError, ValueError) as e:
            raise DataSetException("invalid dataset: %s" % e)

    def get_diagnostics(self):
        header = self.header
        return [{"name": "Bits per pixel", "value": str(header.bpp)},
                {"name": "High tension (kV)", "value": str(header.high_tension_kv)},
                {"name": "Pixel size (nm)", "value": str(header.pixel_size_nm)},
                {"name": "Binning (x)", "value": str(header.xbin)},
                {"name": "Binning (y)", "value": str(header.ybin)},
                {"name": "File Format Version", "value": str(header.version)}]

    @classmethod
    def get_supported_extensions(cls):
        return {"tvips"}

    @classmethod
    def detect_params(cls, path, executor=None):
        """reference tvips.py:451-474; a .tvips file that is none raises DataSetException"""
        if not str(path).lower().endswith(".tvips"):
            return False
        header, segments = scan_set(path)
        image_count, sig_shape = sum(seg.n_frames for seg in segments), (header.ydim, header.xdim)
        try:
            sync_offset, nav_shape = detect_shape(header, segments)
        except DetectionError:
            sync_offset, nav_shape = 0, make_2D_square((image_count,))
        return {"parameters": {"path": path, "nav_shape": nav_shape, "sig_shape": sig_shape,
                               "sync_offset": sync_offset},
                "info": {"image_count": image_count, "native_sig_shape": sig_shape}}

    def get_cache_key(self):
        return {"path": self._path, "shape": tuple(self.shape), "sync_offset": self._sync_offset}

    def __repr__(self):
        if self._layout is None:
            return f"<TVIPSDataSet for {self._path} (not initialized)>"
        return f"<TVIPSDataSet of {self.dtype} shape={tuple(self.shape)}>"
