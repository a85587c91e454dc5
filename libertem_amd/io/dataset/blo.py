"""
BloDataSet: NanoMegas ASTAR .blo files (`ctx.load("blo", path=...)`, reference io/dataset/blo.py).  One file: a
header that names the scan (NY x NX positions, DP_SZ x DP_SZ pixels) and two byte offsets -- `Data_offset_1`,
the virtual bright field image, and `Data_offset_2`, the diffraction patterns --, then per pattern a 6-byte frame
header and the pixels: uint8, or uint16 where the text block between byte 240 and `Data_offset_1` (files of magic
259) holds a line "Blo Bit Depth: 16 bits".  The frames go to HBM through `RecordFileDataSet`.

`endianess` reaches the header fields, not the pixels: the reference hands 16-bit pixels of an `endianess='>'`
file on unswapped, read as little-endian, and so does this reader (pinned by a golden case).
"""
import warnings

import numpy as np

from .base import DataSetException
from .records import RecordFileDataSet

MAGIC_EXPECT = (258, 259)
FRAME_HEADER = 6
TEXT_START = 240


def header_dtype(endianess='<'):
    """the file header as a structured dtype; the 22 doubles at its end (centering, distortion) are native"""
    e = endianess
    fields = [
        ('ID', 'S6'), ('MAGIC', e + 'u2'),
        ('Data_offset_1', e + 'u4'),        # the virtual bright field image
        ('Data_offset_2', e + 'u4'),        # the diffraction patterns
        ('UNKNOWN1', e + 'u4'),
        ('DP_SZ', e + 'u2'),                # pixels per side of a pattern
        ('DP_rotation', e + 'u2'),
        ('NX', e + 'u2'), ('NY', e + 'u2'),
        ('Scan_rotation', e + 'u2'),
        ('SX', e + 'f8'), ('SY', e + 'f8'),     # pixel size, nm
        ('Beam_energy', e + 'u4'),              # V
        ('SDP', e + 'u2'),
        ('Camera_length', e + 'u4'),
        ('Acquisition_time', e + 'f8'),
    ]
    fields += [('Centering_N%d' % i, 'f8') for i in range(8)]
    fields += [('Distortion_N%02d' % i, 'f8') for i in range(14)]
    return np.dtype(fields)


def read_header(path, endianess='<'):
    """-> the header fields as Python values"""
    raw = np.fromfile(path, dtype=header_dtype(endianess), count=1)
    if len(raw) != 1:
        raise OSError("%s is shorter than a .blo header" % path)
    return {name: raw[name][0].item() for name in raw.dtype.names}


def read_text_block(path, header):
    """the non-empty lines of the text between byte 240 and `Data_offset_1`, which files of magic 259 hold"""
    if header['MAGIC'] != 259:
        return ()
    with open(path, 'rb') as f:
        f.seek(TEXT_START)
        raw = f.read(max(0, header['Data_offset_1'] - TEXT_START))
    lines = (line.strip() for line in raw.decode(errors='ignore').strip('\x00').splitlines())
    return tuple(line for line in lines if line)


def pixel_dtype(lines):
    """'u2' for a line like "Blo Bit Depth: 16 bits", 'u1' without one (or with one that does not read so)"""
    for line in lines:
        if not line.lower().startswith('blo bit depth:'):
            continue
        for part in line.split(':'):
            part = part.strip().lower()
            if part.endswith(' bits'):
                try:
                    return "u%d" % (int(part.replace(' bits', '')) // 8)
                except ValueError:
                    break
    return "u1"


class BloDataSet(RecordFileDataSet):
    """
    Parameters (reference blo.py:94-158)
    ----------
    path : str
    endianess : '<' or '>'
        of the header fields
    nav_shape : tuple of int, optional
        default: (NY, NX) of the header
    sig_shape : tuple of int, optional
        same number of pixels as (DP_SZ, DP_SZ)
    sync_offset : int
        > 0: frames to skip at the start; < 0: blank frames inserted at the start
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: load and hold only this rank's block of the first nav axis
    """
    KIND = "BLO file"

    def __init__(self, path, tileshape=None, endianess='<', nav_shape=None, sig_shape=None, sync_offset=0,
                 io_backend=None, num_partitions=None, shard=None):
        if tileshape is not None:
            warnings.warn("tileshape argument is ignored and will be removed after 0.6.0", FutureWarning)
        RecordFileDataSet.__init__(self, path, nav_shape, sig_shape, sync_offset, io_backend, num_partitions, shard)
        self._endianess = endianess
        self._header = None

    def _scan_file(self):
        """-> FrameLayout, from the header, the text block and the size of the file"""
        self._header = h = read_header(self._path, self._endianess)
        storage = np.dtype(pixel_dtype(read_text_block(self._path, h)))
        side = h['DP_SZ']
        payload = side * side * storage.itemsize
        image_count = h['NY'] * h['NX']
        stride = FRAME_HEADER + payload
        in_file = max(0, self._file_size(self._path) - h['Data_offset_2']) // stride if payload else 0
        if payload < 1:
            raise DataSetException("%s: patterns of %d x %d pixels" % (self._path, side, side))
        return self._record_layout(
            self._path, file_header=h['Data_offset_2'], frame_header=FRAME_HEADER, payload_bytes=payload,
            frame_footer=0, storage=storage, native_shape=(side, side), n_frames=min(image_count, in_file),
            nav_shape=self._nav_arg if self._nav_arg is not None else (h['NY'], h['NX']), image_count=image_count)

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
            magic = read_header(self._path, self._endianess)['MAGIC']
        except OSError as e:
            raise DataSetException("invalid dataset: %s" % e) from e
        if magic not in MAGIC_EXPECT:
            raise DataSetException(
                f"invalid magic number: {magic:x} not in {tuple(hex(x) for x in MAGIC_EXPECT)}")
        return True

    def get_diagnostics(self):
        return [{"name": str(k), "value": str(v)} for k, v in self.header.items()]

    @classmethod
    def get_supported_extensions(cls):
        return {"blo"}

    @classmethod
    def detect_params(cls, path, executor=None):
        """reference blo.py:188-209"""
        try:
            ds = cls(path, endianess='<')
            layout = ds._scan_file()
            ds.check_valid()
        except Exception:                               # noqa: BLE001  (anything: not a file of this format)
            return False
        nav, sig = tuple(layout.nav_shape), tuple(layout.sig_shape)
        return {"parameters": {"path": path, "nav_shape": nav, "sig_shape": sig, "tileshape": (1, 8) + sig,
                               "endianess": "<"},
                "info": {"image_count": int(np.prod(nav)), "native_sig_shape": sig}}

    def get_cache_key(self):
        return {"path": self._path, "endianess": self._endianess, "shape": tuple(self.shape),
                "sync_offset": self._sync_offset}

    def __repr__(self):
        if self._layout is None:
            return f"<BloDataSet for {self._path} (not initialized)>"
        return f"<BloDataSet of {self.dtype} shape={tuple(self.shape)}>"
