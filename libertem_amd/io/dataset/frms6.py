"""
FRMS6DataSet: PNDetector pnCCD sets (`ctx.load("frms6", path=...)`, reference io/dataset/frms6.py:406-727):
`NAME.hdr` (an INI file: frame counts, scan size, binning) plus `NAME_000.frms6` (dark frames) and
`NAME_001.frms6` ... (signal frames, numbered on across files).  A file is a 1024-byte header and, per frame, a
64-byte frame header + height x width little-endian uint16.  The stored frame is FOLDED: its rows hold the upper
half of the detector in their first half and, reversed, the mirrored row of the lower half in their second
half; binned readouts store one row for `bin` detector rows.

The host reads headers only.  Where the reference builds one read range per detector row and unfolds row by
row under numba for every tile (frms6.py:232-366), `initialize()` streams the frame records ONCE through pinned
bounce buffers into HBM, `ltmi_frms6_decode` (csrc/ltmi_frms6.hip) unfolds them behind each copy, and the
dataset is a device-resident uint16 array from then on.  A scan that does not fit is STREAMED per partition
(decoded.py).

Corrections: the dark frame is the mean of the frames of file 000, decoded by the same kernel and summed on the
device in exact integers (`ltmi_sum_frames`, int64), then converted to float32 and divided once by the frame
count -- the reference's float32 tile sums (frms6.py:585-621) bit for bit while the per-pixel sum stays below
2**24.  With the optional gain map it makes the `CorrectionSet` of `get_correction_data()`, which
`Context.run_udf` applies when no other is passed: folded into mask stacks, or applied to the tiles on the
device; the resident frames stay raw.
"""
import os
import csv
import warnings
import configparser
from glob import glob, escape

import numpy as np

from libertem_amd.common.math import prod
from libertem_amd.common.hiparray import HipArray
from .base import DataSetException, DataSetMeta
from .memory import MemoryDataSet
from .decoded import DecodedFileDataSet, FrameLayout, _host_copy

FILE_HEADER_SIZE = 1024
FRAME_HEADER_SIZE = 64

# the fields of the 1024-byte file header that are read; the bytes between them are skipped
FILE_HEADER_DTYPE = np.dtype({
    'names': ['header_size', 'frame_header_size', 'version', 'width', 'height', 'num_frames'],
    'formats': ['<u2', '<u2', 'u1', '<u2', '<u2', '<u4'],
    'offsets': [0, 2, 7, 88, 90, 1020],
    'itemsize': FILE_HEADER_SIZE,
})

#: `measurementInfo` entries of the .hdr file that are whole numbers
HDR_INT_FIELDS = ('darkframes', 'dwelltimemicroseconds', 'gain', 'signalframes')


def _split_set_path(path):
    """a set is STEM.hdr plus STEM_NNN.frms6 -> (the path without its extension, the extension)"""
    stem, ext = os.path.splitext(path)
    if ext not in ('.hdr', '.frms6'):
        raise DataSetException("unknown extension: %s" % ext)
    return stem, ext


def _get_base_filename(_path):
    """STEM of the set that `_path` (its .hdr or one of its .frms6 files) belongs to"""
    stem, ext = _split_set_path(_path)
    if ext == '.frms6':
        head, sep, number = stem.rpartition('_')
        if sep and number.isascii() and number.isdigit():
            stem = head
    return stem


def _pattern(path):
    """the glob pattern of the set's .frms6 files: from a .frms6 file, every file that differs from it in the
    trailing number only"""
    stem, ext = _split_set_path(path)
    if ext == '.hdr':
        return escape(stem) + '_*.frms6'
    return escape(stem.rstrip('0123456789')) + '*.frms6'


def get_filenames(path, disable_glob=False):
    return [path] if disable_glob else sorted(glob(_pattern(path)))


def _number(text):
    text = text.strip()
    if not (text.isascii() and text.isdigit()):
        raise ValueError(text)
    return int(text)


def _parse_readoutmode(text):
    """`"bin: B, windowing: I x J"`, the quotes included -> dict(bin=B, win_i=I, win_j=J)"""
    try:
        if len(text) < 2 or text[0] != '"' or text[-1] != '"':
            raise ValueError(text)
        binning, windowing = text[1:-1].split(',')
        bin_key, bin_value = binning.split(':')
        win_key, win_value = windowing.split(':')
        if bin_key != 'bin' or win_key.strip() != 'windowing':
            raise ValueError(text)
        win_i, win_j = win_value.split('x')
        return {'bin': _number(bin_value), 'win_i': _number(win_i), 'win_j': _number(win_j)}
    except ValueError:
        raise DataSetException("could not parse readout mode") from None


def _read_dataset_hdr(fname):
    """the `measurementInfo` section of the set's .hdr file (an INI file) as a dict: the counts as int,
    `stemimagesize = AxB` as (A, B), `readoutmode` as `_parse_readoutmode` gives it"""
    config = configparser.ConfigParser()
    if not os.path.exists(fname) or not config.read(fname):
        raise DataSetException("Could not find .hdr file {}".format(fname))
    if not config.has_section('measurementInfo'):
        raise DataSetException(
            "measurementInfo missing from .hdr file {}, have: {}".format(fname, repr(config.sections())))
    info = dict(config['measurementInfo'])
    for key in HDR_INT_FIELDS:
        if key in info:
            info[key] = int(info[key])
    info['stemimagesize'] = tuple(int(n) for n in info['stemimagesize'].split('x'))
    info['readoutmode'] = _parse_readoutmode(info['readoutmode'])
    return info


def _read_file_header(path):
    """the fields of `FILE_HEADER_DTYPE` as Python ints (no uint16 overflow in later products), plus
    `filesize` and `path`"""
    raw = np.fromfile(path, dtype=FILE_HEADER_DTYPE, count=1)
    if len(raw) != 1:
        raise DataSetException("%s is shorter than a file header of %d bytes" % (path, FILE_HEADER_SIZE))
    header = {name: int(raw[name][0]) for name in FILE_HEADER_DTYPE.names}
    header['filesize'] = os.stat(path).st_size
    header['path'] = path
    return header


def _header_valid(header):
    return (header['header_size'] == FILE_HEADER_SIZE and header['frame_header_size'] == FRAME_HEADER_SIZE
            and header['version'] == 6)


def _num_frames(header):
    """frames in a file: the header's count, or for older files, which hold 0 there, what the file size gives"""
    count = header['num_frames']
    if count == 0:
        record = FRAME_HEADER_SIZE + 2 * header['height'] * header['width']
        count, rest = divmod(header['filesize'] - FILE_HEADER_SIZE, record)
        if rest:
            raise DataSetException("could not determine number of frames")
    return count


def _get_sig_shape(path, bin_factor):
    header = _read_file_header(get_filenames(path)[0])
    return (2 * header['height'] * bin_factor, header['width'] // 2)


def _read_gain_map(path):
    """a .mat file with a variable `GainMap`; or a .csv file, `;`-separated, empty cells dropped, holding the
    transposed map (what the reference reads, frms6.py:623-635); None without a path or for any other extension"""
    ext = '' if path is None else os.path.splitext(path)[1].lower()
    if ext == '.mat':
        from scipy.io import loadmat
        return loadmat(path)['GainMap']
    if ext == '.csv':
        with open(path, newline='') as f:
            lines = [[float(cell) for cell in line if cell != ''] for line in csv.reader(f, delimiter=';')]
        return np.array(lines).T
    return None


class FRMS6DataSet(DecodedFileDataSet):
    """
    Parameters (reference frms6.py:412-440)
    ----------
    path : str
        the .hdr file or one of the .frms6 files of the set
    enable_offset_correction : bool
        subtract the mean of the dark frames (file 000): `dtype` is float32 then
    gain_map_path : str, optional
        a gain map to apply (.mat with a variable `GainMap`, or `;`-separated .csv holding the transposed map)
    nav_shape : tuple of int, optional
        default: `stemimagesize` of the .hdr file
    sig_shape : tuple of int, optional
        same number of pixels as the unfolded frame (2 * height * bin, width / 2)
    sync_offset : int
        > 0: frames to skip at the start; < 0: blank frames inserted at the start
    num_partitions : int, optional
    shard : (rank, world), optional
        one process per GPU: decode and hold only this rank's block of the first nav axis
    """
    KIND = "FRMS6 set"
    DECODE_KERNEL = "ltmi_frms6_decode"

    def __init__(self, path, enable_offset_correction=True, gain_map_path=None, dest_dtype=None,
                 nav_shape=None, sig_shape=None, sync_offset=0, io_backend=None, num_partitions=None,
                 shard=None):
        DecodedFileDataSet.__init__(self, path, num_partitions, shard, io_backend)
        if dest_dtype is not None:
            warnings.warn("dest_dtype is now handled per `get_tiles` call, and ignored here",
                          DeprecationWarning)
        self._enable_offset_correction = bool(enable_offset_correction)
        self._gain_map_path = None if gain_map_path is None else str(gain_map_path)
        self._nav_arg = tuple(nav_shape) if nav_shape else None
        self._sig_arg = tuple(sig_shape) if sig_shape else None
        self._sync_offset_arg = int(sync_offset)
        self._scan = None
        self._hdr_info = None
        self._headers = None
        self._dark_frame = None
        self._gain_map = None

    # --- host side: which files, which frames -------------------------------------------------------
    def _scan_files(self):
        """-> dict(hdr, headers (all files, 000 first), height, width, binning, native_sig_shape, image_count,
        sig_shape, nav_shape, sync_offset, counts (frames per signal file), starts (first frame of each signal
        file))"""
        filenames = get_filenames(self._path)
        hdr = _read_dataset_hdr("%s.hdr" % _get_base_filename(self._path))
        if len(filenames) < 2:
            raise DataSetException(
                "expected a file of dark frames and at least one of signal frames at %s, found %d files"
                % (_pattern(self._path), len(filenames)))
        headers = [_read_file_header(fn) for fn in filenames]
        first = headers[0]
        for h in headers:
            if (h['height'], h['width']) != (first['height'], first['width']):
                raise DataSetException("%s: frames of %dx%d differ from the first file's %dx%d" % (
                    h['path'], h['height'], h['width'], first['height'], first['width']))
        if first['width'] % 2 != 0:
            raise DataSetException("%s: a folded frame has an even width, not %d" % (
                first['path'], first['width']))
        binning = hdr['readoutmode']['bin']
        if binning not in (1, 2, 4):
            raise DataSetException("binning is 1, 2 or 4, not %d" % binning)
        image_count = int(hdr['signalframes'])
        so = self._sync_offset_arg
        # (reference io/dataset/base/dataset.py:74)
        if not (-max(image_count, 1) < so < max(image_count, 1)):
            raise DataSetException(
                "offset should be in (%s, %s), which is (-image_count, image_count)" % (-image_count, image_count))
        counts = [_num_frames(h) for h in headers[1:]]
        native = (2 * first['height'] * binning, first['width'] // 2)
        sig_shape = self._sig_arg
        if sig_shape is None:
            sig_shape = native
        elif int(prod(sig_shape)) != int(prod(native)):
            raise DataSetException("sig_shape must be of size: %s" % int(prod(native)))
        return dict(hdr=hdr, headers=headers, height=first['height'], width=first['width'], binning=binning,
                    native_sig_shape=native, sig_shape=tuple(sig_shape),
                    image_count=image_count, sync_offset=so,
                    nav_shape=self._nav_arg if self._nav_arg is not None else tuple(hdr['stemimagesize']),
                    counts=counts, starts=np.cumsum([0] + counts))

    def initialize(self, executor):
        device = self._gpu_of(executor)
        self._scan = scan = self._scan_files()
        self._hdr_info, self._headers = scan['hdr'], scan['headers']
        native = scan['native_sig_shape']
        nav_shape = tuple(scan['nav_shape'])
        sig_shape = scan['sig_shape']
        self._image_count = scan['image_count']
        so = scan['sync_offset']
        storage = np.dtype('uint16')
        self._load_frames(executor, device, FrameLayout(
            nav_shape=nav_shape, sig_shape=sig_shape, native_shape=native, storage=storage,
            stride=FRAME_HEADER_SIZE + scan['height'] * scan['width'] * 2, n_frames=int(scan['starts'][-1]),
            sync_offset=so))
        self._dark_frame = None
        if self._enable_offset_correction:
            self._dark_frame = self._get_dark_frame(device, executor).reshape(tuple(sig_shape))
        # like the dark frame, the gain map is stored in the unfolded frame's own shape and follows a `sig_shape`
        gain = _read_gain_map(self._gain_map_path)
        if gain is not None:
            if tuple(gain.shape) not in (tuple(native), tuple(sig_shape)):
                raise DataSetException("the gain map %s is of shape %s, the frames are of %s" % (
                    self._gain_map_path, tuple(gain.shape), tuple(native)))
            gain = gain.reshape(tuple(sig_shape))
        self._gain_map = gain
        self._meta = DataSetMeta(
            shape=self._shape, raw_dtype=storage,
            dtype=np.dtype('float32') if self._enable_offset_correction else storage,
            metadata={'raw_frame_size': (scan['height'], scan['width'])}, sync_offset=so,
            image_count=self._image_count)
        return MemoryDataSet.initialize(self, executor)

    def _frame_source(self, device, headers=None, starts=None):
        """the signal files; or the files `headers`, frame numbers running on across them (`starts`: first frame
        of each)"""
        from libertem_amd import hip
        scan = self._scan
        if headers is None:
            headers, starts = scan['headers'][1:], scan['starts']
        h, w, binning = scan['height'], scan['width'], scan['binning']
        stride = FRAME_HEADER_SIZE + h * w * 2
        mapped = {}

        def fill(pool, host, g, n):
            # whole frame records of ONE file: a chunk never spans two files
            fi = int(np.searchsorted(starts, g, side='right') - 1)
            if fi not in mapped:
                mapped.clear()                                              # one mapping at a time
                mapped[fi] = np.memmap(headers[fi]['path'], dtype=np.uint8, mode='r')
            a = g - int(starts[fi])                                     # first frame of the chunk in its file
            n = min(n, int(starts[fi + 1]) - g)
            _host_copy(pool, host, 0, mapped[fi], FILE_HEADER_SIZE + a * stride, n * stride)
            return n

        def decode(src_ptr, n, dst_ptr, stream):
            hip.frms6_decode(device, src_ptr + FRAME_HEADER_SIZE, stride, n, h, w, binning, dst_ptr, np.uint16,
                             stream=stream)
        return fill, decode

    def _get_dark_frame(self, device, executor):
        """float32 mean of the frames of file 000 (native sig shape): unfolded by `ltmi_frms6_decode`, summed
        per pixel in int64 on the device, divided once"""
        import torch
        from libertem_amd import hip
        scan = self._scan
        header = scan['headers'][0]
        num_frames = _num_frames(header)
        sig = scan['native_sig_shape']
        n_px = int(prod(sig))
        if num_frames == 0:
            raise DataSetException("%s holds no dark frame: pass enable_offset_correction=False" % header['path'])
        if getattr(executor, '_make_current', None) is not None:
            executor._make_current()
        chunk = int(max(1, min(num_frames, self.CHUNK_BYTES // self._layout.stride)))
        total = HipArray.zeros((n_px,), np.int64, device)
        decoded = [HipArray.empty((chunk,) + sig, np.uint16, device) for _ in range(2)]
        ws_bytes = hip.sum_frames_workspace(chunk, n_px, np.int64)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=f'cuda:{device}')
        state = {'i': 0}

        def consume(c0, c1, decode, copy_stream):
            # (chunk i + 2 is decoded into the buffer of chunk i: same stream, after its sum)
            buf = decoded[state['i'] & 1]
            state['i'] += 1
            decode(buf.data_ptr())
            hip.sum_frames(device, buf.data_ptr(), np.uint16, c1 - c0, n_px, n_px, total.data_ptr(), np.int64,
                           True, ws.data_ptr(), stream=copy_stream)
        self._upload_and_decode(device, self._frame_source(device, [header], np.array([0, num_frames])), 0,
                                num_frames, consume)
        torch.cuda.current_stream(device).synchronize()
        return total.cpu().astype(np.float32).reshape(sig) / num_frames

    # --- the reference's descriptive surface --------------------------------------------------------
    @property
    def dtype(self):
        """float32 with offset correction (what the corrected tiles are), uint16 without (frms6.py:515-516)"""
        return self._meta.dtype

    @property
    def storage_dtype(self):
        return np.dtype('uint16')

    def get_correction_data(self):
        from libertem_amd.io.corrections import CorrectionSet
        return CorrectionSet(dark=self._dark_frame, gain=self._gain_map)

    def check_valid(self):
        try:
            for header in self._headers if self._headers is not None else self._scan_files()['headers']:
                if not _header_valid(header):
                    raise DataSetException("error while checking validity of %s" % header['path'])
            return True
        except OSError as e:
            raise DataSetException("invalid dataset: %s" % e)

    def get_diagnostics(self):
        return [{"name": "Offset correction available and enabled", "value": str(self._dark_frame is not None)}] \
            + [{"name": str(k), "value": str(v)} for k, v in self._hdr_info.items()]

    @classmethod
    def get_supported_extensions(cls):
        return {"frms6", "hdr"}

    @classmethod
    def detect_params(cls, path, executor=None):
        """reference frms6.py:536-557"""
        try:
            hdr = _read_dataset_hdr("%s.hdr" % _get_base_filename(path))
            nav_shape = tuple(hdr['stemimagesize'])
            sig_shape = _get_sig_shape(path, hdr['readoutmode']['bin'])
        except Exception:                               # noqa: BLE001  (anything: not a set of this format)
            return False
        return {"parameters": {"path": path, "nav_shape": nav_shape, "sig_shape": sig_shape},
                "info": {"image_count": int(prod(nav_shape)), "native_sig_shape": sig_shape}}

    def get_cache_key(self):
        return {"path": self._path, "enable_offset_correction": self._enable_offset_correction,
                "gain_map_path": self._gain_map_path, "shape": tuple(self.shape),
                "sync_offset": self._sync_offset}

    def __repr__(self):
        if self._scan is None:
            return f"<FRMS6DataSet for pattern={_pattern(self._path)} (not initialized)>"
        return f"<FRMS6DataSet for pattern={_pattern(self._path)} nav_shape={tuple(self._scan['nav_shape'])}>"
