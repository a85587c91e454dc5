"""
SEQDataSet: Norpix .seq files, as Direct Electron cameras write them (`ctx.load("seq", path=..., nav_shape=...)`,
reference io/dataset/seq.py).  One file: a header (8192 bytes, 1024 for header versions below 5) and per frame
`true_image_size` bytes, of which the first height x width x itemsize are little-endian unsigned pixels and the
rest is a footer (time stamp and padding).  The frames go to HBM through `RecordFileDataSet`.

Corrections a set may bring along, picked up by `Context.run_udf` when no other are passed (the resident frames
stay raw): `<base>.seq.dark.mrc` and `<base>.seq.gain.mrc`, read by the small MRC reader below, and dead pixels
from `<base>.seq.Config.Metadata.xml` when `<base>.seq.metadata` exists too.
"""
import os
import struct
import warnings

import numpy as np

from libertem_amd.common.math import prod, make_2D_square
from .base import DataSetException
from .records import RecordFileDataSet

MAGIC = 0xFEED

# the start of the file header, little-endian: field names, struct codes (name and description are UTF-16)
HEADER_FIELDS = (
    ('magic', 'L'), ('name', '24s'), ('version', 'l'), ('header_size', 'l'), ('description', '512s'),
    ('width', 'L'), ('height', 'L'), ('bit_depth', 'L'), ('bit_depth_real', 'L'), ('image_size_bytes', 'L'),
    ('image_format', 'L'), ('allocated_frames', 'L'), ('origin', 'L'), ('true_image_size', 'L'),
    ('suggested_frame_rate', 'd'), ('description_format', 'l'), ('reference_frame', 'L'), ('fixed_size', 'L'),
    ('flags', 'L'), ('bayer_pattern', 'l'), ('time_offset_us', 'l'), ('extended_header_size', 'l'),
    ('compression_format', 'L'), ('reference_time_s', 'l'), ('reference_time_ms', 'H'), ('reference_time_us', 'H'),
)
# (no padding: the fields are read one after the other, as the reference does)
HEADER_SIZE = sum(struct.calcsize('<' + code) for _, code in HEADER_FIELDS)

#: the values of `<base>.seq.metadata` at byte 282, format 'iiiiiiiiiii?'
METADATA_KEYS = ('DEMetadataSize', 'DEMetadataVersion', 'UnbinnedFrameSizeX', 'UnbinnedFrameSizeY', 'OffsetX',
                 'OffsetY', 'HardwareBinning', 'Bitmode', 'FrameRate', 'RotationMode', 'FlipMode', 'OkraMode')
METADATA_OFFSET = 282
METADATA_FORMAT = 'iiiiiiiiiii?'

#: MRC modes -> little-endian pixel types
MRC_MODES = {0: 'i1', 1: '<i2', 2: '<f4', 6: '<u2'}


def _utf16(raw):
    """a UTF-16 field up to its terminating pair of zero bytes (an all-zero field does not decode, as in the
    reference)"""
    end = raw.find(b'\x00\x00')
    return (raw if end < 0 else raw[:end + 1]).decode('utf16')


def read_header(path):
    """-> dict of `HEADER_FIELDS`"""
    with open(path, 'rb') as f:
        raw = f.read(HEADER_SIZE)
    if len(raw) < HEADER_SIZE:
        raise OSError("%s is shorter than a .seq header of %d bytes" % (path, HEADER_SIZE))
    header, pos = {}, 0
    for name, code in HEADER_FIELDS:
        value, = struct.unpack_from('<' + code, raw, pos)
        header[name] = _utf16(value) if name in ('name', 'description') else value
        pos += struct.calcsize('<' + code)
    return header


def image_offset(header):
    return 8192 if header['version'] >= 5 else 1024


def base_name(path):
    """`x` of `x.seq` and of `x.seq.seq` (both exist in the wild), the path itself for any other extension"""
    name, ext = os.path.splitext(path)
    if ext.lower() != '.seq':
        return path
    name2, ext2 = os.path.splitext(name)
    return name2 if ext2.lower() == '.seq' else name


def read_mrc(path):
    """the data block of an MRC file: 1024-byte header (int32 words: nx, ny, nz, mode; word 23: bytes of extended
    header that follow it), then nz sections of ny rows of nx pixels -> array (nz, ny, nx)"""
    with open(path, 'rb') as f:
        words = np.frombuffer(f.read(1024), dtype='<i4')
        if len(words) < 256:
            raise DataSetException("%s is shorter than an MRC header" % path)
        nx, ny, nz, mode, extended = (int(words[i]) for i in (0, 1, 2, 3, 23))
        if mode not in MRC_MODES:
            raise DataSetException("%s: MRC mode %d is not one of %s" % (path, mode, sorted(MRC_MODES)))
        f.seek(1024 + extended)
        data = np.fromfile(f, dtype=MRC_MODES[mode], count=nx * ny * nz)
    if len(data) != nx * ny * nz:
        raise DataSetException("%s holds fewer than %d x %d x %d pixels" % (path, nz, ny, nx))
    return data.reshape((nz, ny, nx))


def _parse_xml(path):
    try:
        from defusedxml import ElementTree
    except ImportError:                 # (the user's own local side file)
        from xml.etree import ElementTree
    return ElementTree.parse(path).getroot()


def _span(text):
    """'7' -> (7, 8), '3-5' -> (3, 6)"""
    ends = [int(t) for t in text.split('-')]
    return ends[0], ends[-1] + 1


def bad_pixel_map(root, metadata):
    """The dead-pixel mask of `<base>.seq.Config.Metadata.xml` for the acquisition `metadata` describes, as the
    reference builds it (seq.py:133-362).  Of the file's `BadPixelMap` nodes the one is taken whose binning
    matches (`Binning` > 1 for a hardware-binned acquisition, else none or 1), the widest (`Columns`) of those,
    the first of equals.  Its mask has `Columns` entries along the first axis and `Rows` along the second, the
    `Row(s)` of a defect index the first; the crop to the frame (offset and unbinned size of the metadata, halved
    under binning) is applied only where it fits into the map."""
    maps = root.findall('.//BadPixelMap')
    binned = metadata['HardwareBinning'] >= 2
    widths = []
    for node in maps:
        matches = (int(node.attrib.get('Binning', 1)) > 1) == binned
        widths.append(int(node.attrib['Columns']) if matches else 0)
    node = maps[widths.index(max(widths))]
    size = (int(node.attrib['Columns']), int(node.attrib['Rows']))
    mask = np.zeros(size, dtype=bool)
    single = []
    for defect in node.findall('Defect'):
        attrib = defect.attrib
        if len(attrib) != 1:
            single.append((int(attrib['Row']), int(attrib['Column'])))
            continue
        for key in ('Rows', 'Row'):
            if key in attrib:
                lo, hi = _span(attrib[key])
                mask[lo:hi] = True
        for key in ('Columns', 'Column'):
            if key in attrib:
                lo, hi = _span(attrib[key])
                mask[:, lo:hi] = True
    for row, col in single:
        mask[row, col] = True
    want = (metadata['UnbinnedFrameSizeY'], metadata['UnbinnedFrameSizeX'])
    offset = (metadata['OffsetY'], metadata['OffsetX'])
    if metadata['HardwareBinning'] > 1:
        want, offset = tuple(w // 2 for w in want), tuple(o // 2 for o in offset)
    if offset[0] + want[0] <= size[0] and offset[1] + want[1] <= size[1]:
        # (whole pairs of rows and columns about the centre of the wanted window)
        half = (int(want[0]) // 2, int(want[1]) // 2)
        mask = mask[int(offset[0]):int(offset[0]) + 2 * half[0], int(offset[1]):int(offset[1]) + 2 * half[1]]
    return mask


def read_metadata(path):
    with open(path, 'rb') as f:
        raw = f.read()
    return dict(zip(METADATA_KEYS, struct.unpack_from(METADATA_FORMAT, raw, METADATA_OFFSET)))


class SEQDataSet(RecordFileDataSet):
    """
    Parameters (reference seq.py:415-472)
    ----------
    path : str
        the .seq file
    nav_shape : tuple of int
        required: the file does not hold the scan's shape
    sig_shape : tuple of int, optional
        same number of pixels as (height, width) of the header
    sync_offset : int
        > 0: frames to skip at the start; < 0: blank frames inserted at the start
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: load and hold only this rank's block of the first nav axis
    """
    KIND = "SEQ file"

    def __init__(self, path, scan_size=None, nav_shape=None, sig_shape=None, sync_offset=0, io_backend=None,
                 num_partitions=None, shard=None):
        if scan_size is not None:
            warnings.warn("scan_size argument is deprecated. please specify nav_shape instead", FutureWarning)
            if nav_shape is not None:
                raise ValueError("cannot specify both scan_size and nav_shape")
            nav_shape = scan_size
        if not nav_shape:
            raise TypeError("missing 1 required argument: 'nav_shape'")
        RecordFileDataSet.__init__(self, path, nav_shape, sig_shape, sync_offset, io_backend, num_partitions, shard)
        self._basename = base_name(self._path)
        self._header = None
        self._footer_size = None
        self._dark = self._gain = self._excluded_pixels = None

    def _scan_file(self):
        """-> FrameLayout, from the header and the size of the file"""
        self._header = header = read_header(self._path)
        bits = header['bit_depth']
        if bits not in (8, 16, 32):
            raise DataSetException("unsupported bit depth: %s" % bits)
        storage = np.dtype('<u%d' % (bits // 8))
        native = (header['height'], header['width'])
        payload = int(prod(native)) * storage.itemsize
        record = header['true_image_size']
        self._footer_size = record - payload
        if payload < 1 or self._footer_size < 0:
            raise DataSetException("%s: records of %d bytes do not hold frames of %dx%d %s" % (
                self._path, record, native[0], native[1], storage))
        offset = image_offset(header)
        return self._record_layout(
            self._path, file_header=offset, frame_header=0, payload_bytes=payload, frame_footer=self._footer_size,
            storage=storage, native_shape=native, n_frames=max(0, self._file_size(self._path) - offset) // record,
            nav_shape=self._nav_arg)

    def initialize(self, executor):
        self._gpu_of(executor)
        layout = self._scan_file()
        self._load_corrections()
        return self._load_records(executor, layout, metadata=self._header)

    def _load_corrections(self):
        stem = self._basename + '.seq'
        self._dark, self._gain = (
            np.squeeze(read_mrc(p)) if os.path.exists(p) else None for p in (stem + '.dark.mrc', stem + '.gain.mrc'))
        self._excluded_pixels = None
        xml_path, meta_path = stem + '.Config.Metadata.xml', stem + '.metadata'
        if os.path.exists(xml_path) and os.path.exists(meta_path):
            self._excluded_pixels = bad_pixel_map(_parse_xml(xml_path), read_metadata(meta_path))

    def get_correction_data(self):
        from libertem_amd.io.corrections import CorrectionSet
        return CorrectionSet(dark=self._dark, gain=self._gain, excluded_pixels=self._excluded_pixels)

    def check_valid(self):
        header = self._header if self._header is not None else read_header(self._path)
        if header['magic'] != MAGIC:
            raise DataSetException('The format of this .seq file is unrecognized')
        if header['compression_format'] != 0:
            raise DataSetException('Only uncompressed images are supported in .seq files')
        if header['image_format'] != 100:
            raise DataSetException('Non-monochrome images are not supported')
        return True

    def get_diagnostics(self):
        return [{"name": k, "value": str(v)} for k, v in self._header.items()] + [
            {"name": "Footer size", "value": str(self._footer_size)},
            {"name": "Dark frame included", "value": str(self._dark is not None)},
            {"name": "Gain map included", "value": str(self._gain is not None)}]

    @classmethod
    def get_supported_extensions(cls):
        return {"seq"}

    @classmethod
    def detect_params(cls, path, executor=None):
        """reference seq.py:613-644"""
        try:
            header = read_header(path)
            if header['magic'] != MAGIC:
                return False
            image_count = (os.stat(path).st_size - image_offset(header)) // header['true_image_size']
            sig_shape = (header['height'], header['width'])
        except Exception:                               # noqa: BLE001  (anything: not a file of this format)
            return False
        return {"parameters": {"path": path, "nav_shape": make_2D_square((image_count,)), "sig_shape": sig_shape},
                "info": {"image_count": image_count, "native_sig_shape": sig_shape}}

    def get_cache_key(self):
        return {"path": self._path, "shape": tuple(self.shape), "sync_offset": self._sync_offset}

    def __repr__(self):
        if self._layout is None:
            return f"<SEQDataSet for {self._path} (not initialized)>"
        return f"<SEQDataSet of {self.dtype} shape={tuple(self.shape)}>"
