"""
RecordFileDataSet: what the formats share that are files of fixed-size frame records (Norpix .seq, EMPAD .raw,
NanoMegas .blo: one file; TVIPS: a series of files): a file header, then per frame
`[frame header | pixels | frame footer]`.

The reference strips headers and footers on the host, per tile and for every run, through numba read ranges
(io/dataset/base/tiling.py, decode.py).  Here the file bytes go up once, whole records at a time, through the
pinned bounce buffers of `DecodedFileDataSet`, and `ltmi_records_gather` (csrc/ltmi_records.hip) moves the payloads
into one contiguous array behind each copy: a device-resident dataset of the file's own pixel type from then on,
or one that is streamed per partition when it does not fit (decoded.py).

A format hands `_record_layout()` (one file) or `_segments_layout()` (a series) what it read from its headers and
gets the `FrameLayout` back, with `stride = frame_header + payload + frame_footer`; `_frame_source()` is implemented
here, once.

The data of a set is an ordered list of `Segment`s `(path, file_header, first_frame, n_frames)`, one per file, that
share the record geometry.  A chunk of the upload never spans two files -- `fill` hands back fewer frames than it
was asked for at the end of a file (`locate`) --, so the bytes of a chunk are records one stride apart and the
kernel's single stride holds.
"""
import os
from bisect import bisect_right
from collections import namedtuple

import numpy as np

from libertem_amd.common.math import prod
from .base import DataSetException, DataSetMeta
from .memory import MemoryDataSet
from .decoded import DecodedFileDataSet, FrameLayout, _host_copy


def check_sync_offset(sync_offset, image_count):
    """(reference io/dataset/base/dataset.py:74)"""
    if not (-max(image_count, 1) < sync_offset < max(image_count, 1)):
        raise DataSetException(
            "offset should be in (%s, %s), which is (-image_count, image_count)" % (-image_count, image_count))


def check_sig_shape(sig_shape, native):
    """-> the sig shape of the dataset: `sig_shape` if given (of as many pixels as a stored frame), else `native`"""
    if sig_shape is None:
        return tuple(native)
    if int(prod(sig_shape)) != int(prod(native)):
        raise DataSetException("sig_shape must be of size: %s" % int(prod(native)))
    return tuple(sig_shape)


#: one file of a set: its path, the bytes in front of its first record, the index of its first frame in the set and
#: the records it holds
Segment = namedtuple('Segment', 'path file_header first_frame n_frames')


def locate(g, n_max, segments, stride):
    """-> (segment index, byte offset, n): the file that holds frame `g` of the set, where its record starts in that
    file, and how many of the `n_max` frames from `g` on that file holds.  `segments`: tuples
    (path, file_header, first_frame, n_frames) in the order of their frames; integers only"""
    if n_max < 1:
        raise ValueError("n_max is %d" % n_max)
    # (of files with the same first frame all but the last are empty: the rightmost is the one to take)
    i = bisect_right([seg[2] for seg in segments], g) - 1
    if i < 0 or not (segments[i][2] <= g < segments[i][2] + segments[i][3]):
        raise IndexError("frame %d is in none of the %d files" % (g, len(segments)))
    _, file_header, first_frame, n_frames = segments[i]
    local = g - first_frame
    return i, file_header + local * stride, min(n_max, n_frames - local)


class RecordFileDataSet(DecodedFileDataSet):
    KIND = "record file"
    DECODE_KERNEL = "ltmi_records_gather"

    def __init__(self, path, nav_shape=None, sig_shape=None, sync_offset=0, io_backend=None, num_partitions=None,
                 shard=None):
        DecodedFileDataSet.__init__(self, path, num_partitions, shard, io_backend)
        self._nav_arg = tuple(nav_shape) if nav_shape else None
        self._sig_arg = tuple(sig_shape) if sig_shape else None
        self._sync_offset_arg = int(sync_offset)
        self._records = None

    def _record_layout(self, data_path, file_header, frame_header, payload_bytes, frame_footer, storage,
                       native_shape, n_frames, nav_shape, image_count=None):
        """the geometry of the file `data_path` -> FrameLayout.  `n_frames`: records the file holds (the last one
        may lack its footer); `image_count`: what the dataset reports (default: `n_frames`), also the bound of
        `sync_offset`"""
        return self._segments_layout(
            [Segment(str(data_path), int(file_header), 0, int(n_frames))], frame_header, payload_bytes, frame_footer,
            storage, native_shape, nav_shape, image_count)

    def _segments_layout(self, segments, frame_header, payload_bytes, frame_footer, storage, native_shape,
                         nav_shape, image_count=None):
        """the geometry of a series of files -> FrameLayout.  `segments`: (path, file_header, first_frame,
        n_frames) per file, in the order of their frames and without gaps; the record geometry is that of all of
        them (the last record of the last file may lack its footer)"""
        segments = [Segment(str(p), int(h), int(f), int(n)) for p, h, f, n in segments]
        n_frames = 0
        for seg in segments:
            if seg.first_frame != n_frames or seg.n_frames < 0:
                raise DataSetException("%s: frames %d to %d do not continue the %d frames before" % (
                    seg.path, seg.first_frame, seg.first_frame + seg.n_frames, n_frames))
            n_frames += seg.n_frames
        if not segments:
            raise DataSetException("a record dataset of no files")
        storage = np.dtype(storage)
        native = tuple(int(s) for s in native_shape)
        if int(prod(native)) * storage.itemsize != payload_bytes:
            raise DataSetException("frames of %s %s are not payloads of %d bytes" % (native, storage, payload_bytes))
        image_count = int(n_frames if image_count is None else image_count)
        sig_shape = check_sig_shape(self._sig_arg, native)
        check_sync_offset(self._sync_offset_arg, image_count)
        self._image_count = image_count
        # (`path` and `file_header`: of the first file -- the whole set for the one-file formats)
        self._records = dict(path=segments[0].path, file_header=segments[0].file_header,
                             frame_header=int(frame_header), payload_bytes=int(payload_bytes),
                             frame_footer=int(frame_footer), segments=tuple(segments))
        return FrameLayout(
            nav_shape=tuple(int(n) for n in nav_shape), sig_shape=sig_shape, native_shape=native, storage=storage,
            stride=int(frame_header) + int(payload_bytes) + int(frame_footer), n_frames=int(n_frames),
            sync_offset=self._sync_offset_arg)

    def _load_records(self, executor, layout, metadata=None):
        """the common end of `initialize()`: frames into HBM (or set up to be streamed), `_meta`"""
        device = self._gpu_of(executor)
        self._load_frames(executor, device, layout)
        self._meta = DataSetMeta(shape=self._shape, raw_dtype=layout.storage, dtype=layout.storage,
                                 metadata=metadata, sync_offset=layout.sync_offset,
                                 image_count=self._image_count)
        return MemoryDataSet.initialize(self, executor)

    def _frame_source(self, device):
        from libertem_amd import hip
        rec = self._records
        stride = self._layout.stride
        segments, frame_header, payload = rec['segments'], rec['frame_header'], rec['payload_bytes']
        # the frames of the layout that follow the last file's first one are that file's, as they always were (a
        # layout may count a last record without its footer, which the whole records of a file size leave out)
        last = segments[-1]
        segments = segments[:-1] + (last._replace(n_frames=self._layout.n_frames - last.first_frame),)
        mappings = {}                                 # one per file, opened when a chunk first needs it

        def fill(pool, host, g, n_max):
            # whole records of ONE file: a chunk ends where its file does.  Of the last record, which may lack
            # its footer, what the file holds (the kernel reads payloads only)
            i, start, n = locate(g, n_max, segments, stride)
            mapped = mappings.get(i)
            if mapped is None:
                mapped = mappings[i] = np.memmap(segments[i].path, dtype=np.uint8, mode='r')
            _host_copy(pool, host, 0, mapped, start, min(n * stride, len(mapped) - start))
            return n

        def decode(src_ptr, n, dst_ptr, stream):
            hip.records_gather(device, src_ptr + frame_header, stride, n, payload, dst_ptr, stream)
        return fill, decode

    @property
    def dtype(self):
        """the pixel type of the file (the corrections a set brings along do not change it, as in the reference)"""
        return self._meta.raw_dtype

    @property
    def storage_dtype(self):
        return np.dtype(self._layout.storage)

    def _file_size(self, path):
        try:
            return os.stat(path).st_size
        except OSError as e:
            raise DataSetException("could not open file %s: %s" % (path, e))
