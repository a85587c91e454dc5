"""
Synthetic PNDetector FRMS6 sets for the tests (a helper, not a test): a writer of the `.hdr`, `.frms6`, `.mat`
and `.csv` files of a set, and a plain NumPy decoder of `.frms6` files -- the CPU yardstick of the FRMS6 tests,
which tests/test_frms6_cpu.py pins to the reference's decoder through tests/golden/frms6.npz.

The format (see DESIGN.md "FRMS6"): `NAME.hdr` is an INI file whose section `measurementInfo` holds
signalframes, darkframes, stemimagesize = AxB and readoutmode = "bin: B, windowing: I x J"; `NAME_000.frms6`
holds the dark frames, `NAME_001.frms6` ... the signal frames.  A file is a 1024-byte header (`<u2` 1024 at 0,
`<u2` 64 at 2, `u1` 6 at 7, `<u2` width at 88, `<u2` height at 90, `<u4` num_frames at 1020; 0 in old files) and
per frame a 64-byte frame header + height x width little-endian uint16.  The stored frame is folded: with
x = width / 2 the frame is (2 height binning, x); output row y, yb = y // binning, is raw row yb, columns [0, x),
for yb < height and raw row 2 height - 1 - yb, columns [x, 2 x), reversed otherwise.
"""
import os

import numpy as np

FILE_HEADER = 1024
FRAME_HEADER = 64

FILE_HEADER_DTYPE = np.dtype({
    'names': ['header_size', 'frame_header_size', 'version', 'width', 'height', 'num_frames'],
    'formats': ['<u2', '<u2', 'u1', '<u2', '<u2', '<u4'],
    'offsets': [0, 2, 7, 88, 90, 1020],
    'itemsize': FILE_HEADER,
})


def random_raw(n, height, width, seed, high=4096):
    """(n, height, width) uint16 raw (folded) frames with values < `high` from a seed"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, high, (n, height, width), dtype=np.uint16)


def unfold(raw, binning=1):
    """raw (n, height, width) -> frames (n, 2 height binning, width / 2): the yardstick decoder, written from
    the description of the format above"""
    raw = np.asarray(raw)
    n, h, w = raw.shape
    x = w // 2
    out = np.empty((n, 2 * h * binning, x), dtype=raw.dtype)
    for y in range(2 * h * binning):
        yb = y // binning
        if yb < h:
            out[:, y] = raw[:, yb, :x]
        else:
            out[:, y] = raw[:, 2 * h - 1 - yb, x:][:, ::-1]
    return out


def frame_record_offset(i, height, width):
    """byte offset of the payload of frame i of a file"""
    return FILE_HEADER + FRAME_HEADER * (i + 1) + i * width * height * 2


def file_bytes(raw, num_frames_field=None, fill=0):
    """the bytes of a .frms6 file holding the raw frames (n, height, width); `fill`: every header byte that
    is not one of the fields read; `num_frames_field`: what the header says (default: n; 0: an old file)"""
    raw = np.asarray(raw, dtype='<u2')
    n, h, w = raw.shape
    head = np.full(FILE_HEADER, fill, dtype=np.uint8)
    fields = head.view(FILE_HEADER_DTYPE)
    fields['header_size'], fields['frame_header_size'], fields['version'] = FILE_HEADER, FRAME_HEADER, 6
    fields['width'], fields['height'] = w, h
    fields['num_frames'] = n if num_frames_field is None else num_frames_field
    records = np.full((n, FRAME_HEADER + h * w * 2), fill, dtype=np.uint8)
    records[:, FRAME_HEADER:] = raw.reshape(n, -1).view(np.uint8)
    return np.concatenate([head, records.reshape(-1)])


def write_frms6(path, raw, num_frames_field=None, fill=0):
    file_bytes(raw, num_frames_field, fill).tofile(path)
    return path


def write_hdr(path, signalframes, darkframes, stemimagesize, binning, sig_shape):
    with open(path, 'w') as f:
        f.write("[measurementInfo]\n"
                f"signalframes = {signalframes}\n"
                f"darkframes = {darkframes}\n"
                f"stemimagesize = {'x'.join(str(s) for s in stemimagesize)}\n"
                f"readoutmode = \"bin: {binning}, windowing: {sig_shape[0]} x {sig_shape[1]}\"\n"
                "dwelltimemicroseconds = 100\n"
                "gain = 1\n"
                "comment = synthetic\n")
    return path


def write_set(dirpath, name, dark_raw, signal_raw_files, stemimagesize, binning, num_frames_field=None, fill=0):
    """NAME.hdr, NAME_000.frms6 (dark frames) and NAME_001.frms6 ... (one per entry of `signal_raw_files`)
    -> path of the .hdr"""
    h, w = dark_raw.shape[1:]
    sig_shape = (2 * h * binning, w // 2)
    write_frms6(os.path.join(dirpath, f"{name}_000.frms6"), dark_raw, num_frames_field, fill)
    for i, raw in enumerate(signal_raw_files):
        write_frms6(os.path.join(dirpath, f"{name}_{i + 1:03d}.frms6"), raw, num_frames_field, fill)
    return write_hdr(os.path.join(dirpath, f"{name}.hdr"), sum(len(r) for r in signal_raw_files), len(dark_raw),
                     stemimagesize, binning, sig_shape)


def read_file(path):
    """plain NumPy reader of a .frms6 file -> raw frames (n, height, width)"""
    data = np.fromfile(path, dtype=np.uint8)
    fields = data[:FILE_HEADER].view(FILE_HEADER_DTYPE)[0]
    h, w = int(fields['height']), int(fields['width'])
    n = int(fields['num_frames']) or (len(data) - FILE_HEADER) // (FRAME_HEADER + h * w * 2)
    records = data[FILE_HEADER:FILE_HEADER + n * (FRAME_HEADER + h * w * 2)].reshape(n, -1)
    return np.ascontiguousarray(records[:, FRAME_HEADER:]).view('<u2').reshape(n, h, w)


def decode_set(hdr_path, binning):
    """-> (dark frames, signal frames across the files 001 ...), unfolded"""
    import glob
    files = sorted(glob.glob(glob.escape(os.path.splitext(hdr_path)[0]) + '_*.frms6'))
    dark = unfold(read_file(files[0]), binning)
    signal = np.concatenate([unfold(read_file(f), binning) for f in files[1:]])
    return dark, signal


def dark_frame(dark_frames):
    """float32 mean of the dark frames, summed as exact integers (sums < 2**24: what float32 sums give)"""
    total = dark_frames.astype(np.int64).sum(axis=0)
    assert total.max() < 2 ** 24
    return total.astype(np.float32) / np.float32(len(dark_frames))


def random_gain(sig_shape, seed):
    """float64 gain map with values in [0.5, 2]"""
    return np.random.default_rng(seed).uniform(0.5, 2.0, sig_shape)


def write_gain_mat(path, gain):
    import scipy.io
    scipy.io.savemat(path, {'GainMap': np.asarray(gain, dtype=np.float64)})
    return path


def write_gain_csv(path, gain):
    """the file holds the transposed map, `;`-separated, with a trailing `;` on every line (an empty cell)"""
    with open(path, 'w') as f:
        for col in np.asarray(gain).T:
            f.write(';'.join(repr(float(v)) for v in col) + ';\n')
    return path


def positioned(frames, n_nav, sync_offset):
    """frame g at scan position g - sync_offset, zero frames elsewhere -> (n_nav,) + frame shape"""
    out = np.zeros((n_nav,) + frames.shape[1:], dtype=frames.dtype)
    for p in range(n_nav):
        if 0 <= p + sync_offset < len(frames):
            out[p] = frames[p + sync_offset]
    return out
