"""
Seeded inputs of the TVIPS golden vectors (tests/golden/tvips.npz): which synthetic series are written
(tests/tvips_synth.py) and how each is loaded.  Imported by generate_tvips_golden.py (which loads the files with the
reference's TVIPSDataSet) and by the tests (which load the same files with this package); only small results and
checksums are stored.

Pixel values are <= 4095 (<= 255 in 8-bit files): every sum is a whole number below 2**24.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tvips_synth as synth  # noqa: E402
from records_recipes import ROI, N_MASKS  # noqa: E402,F401

# the series: format version, pixel type, frame shape, image header bytes, frames per file, (y, x) of the image
# headers (version 2).  Strides: t16 208 (gathered 16 bytes wide), t16v1 84 (4), t8v1 37 (1), tline 132 (4),
# tnoscan 150 (2)
FILESETS = {
    # two (0, 0), then rows of four: the scan starts at frame 1; 11 frames from there make 2 whole rows
    't16': dict(version=2, dtype='u2', shape=(6, 8), header=112, files=(7, 3, 2), seed=101,
                scan=((0, 0), (0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1),
                      (2, 2))),
    't16v1': dict(version=1, dtype='u2', shape=(6, 6), header=12, files=(6,), seed=102, scan=None),
    't8v1': dict(version=1, dtype='u1', shape=(5, 5), header=12, files=(4, 3), seed=103, scan=None),
    # x never falls: a start, but no row length
    'tline': dict(version=2, dtype='u1', shape=(4, 6), header=108, files=(6,), seed=104,
                  scan=((0, 0), (0, 0), (0, 1), (0, 2), (0, 3), (0, 4))),
    # no (0, 1): no start (one file: the reference looks for the image headers of all frames in the first)
    'tnoscan': dict(version=2, dtype='u2', shape=(3, 5), header=120, files=(5,), seed=105, scan=((0, 0),) * 5),
}

# the loads.  kwargs: what the caller passes besides the path; nav, sync_offset: what the dataset reports then
# (the generator checks that the reference reports the same)
CASES = [
    dict(name='TV_bare', fileset='t16', kwargs={}, nav=(2, 4), sync_offset=1, roi=None),
    dict(name='TV_nav', fileset='t16', kwargs=dict(nav_shape=(2, 4)), nav=(2, 4), sync_offset=1, roi=None),
    dict(name='TV_p2', fileset='t16', kwargs=dict(sync_offset=2), nav=(2, 4), sync_offset=2, roi=ROI),
    dict(name='TV_m2', fileset='t16', kwargs=dict(sync_offset=-2), nav=(2, 4), sync_offset=-2, roi=ROI),
    dict(name='TV_sig', fileset='t16', kwargs=dict(sig_shape=(8, 6)), nav=(2, 4), sync_offset=1, roi=None),
    dict(name='TV_v1_16', fileset='t16v1', kwargs={}, nav=(6,), sync_offset=0, roi=None),
    dict(name='TV_v1_8', fileset='t8v1', kwargs={}, nav=(7,), sync_offset=0, roi=None),
    dict(name='TV_line', fileset='tline', kwargs={}, nav=(6,), sync_offset=1, roi=None),
    dict(name='TV_noscan', fileset='tnoscan', kwargs={}, nav=(5,), sync_offset=0, roi=None),
]

# what `detect_params` says of each series: (nav_shape, sync_offset); where no start is found, a square or a line
DETECTED = {'t16': ((2, 4), 1), 't16v1': ((6,), 0), 't8v1': ((7,), 0), 'tline': ((6,), 1), 'tnoscan': ((5,), 0)}


def case(name):
    return next(c for c in CASES if c['name'] == name)


def native_shape(fileset):
    return tuple(FILESETS[fileset]['shape'])


def sig_shape(case):
    return tuple(case['kwargs'].get('sig_shape', native_shape(case['fileset'])))


def stored_dtype(fileset):
    return np.dtype('<' + FILESETS[fileset]['dtype'])


def n_frames(fileset):
    return sum(FILESETS[fileset]['files'])


def stride(fileset):
    fs = FILESETS[fileset]
    return fs['header'] + int(np.prod(fs['shape'])) * stored_dtype(fileset).itemsize


def make_frames(fileset):
    """the frames as the camera counted them, (n,) + frame shape"""
    fs = FILESETS[fileset]
    rng = np.random.default_rng(fs['seed'])
    high = 256 if stored_dtype(fileset).itemsize == 1 else 4096
    return rng.integers(0, high, (n_frames(fileset),) + tuple(fs['shape'])).astype(fs['dtype'])


def crop(fileset):
    """-> f(frame): the rows next to the framing (the first two and the last two), at most 16 columns"""
    return lambda frame: frame[np.r_[0:2, frame.shape[0] - 2:frame.shape[0]]][:, :16]


def write_fileset(fileset, dirpath):
    """-> dict(path: the first file; paths: all of them; frames: what a reader hands out)"""
    fs = FILESETS[fileset]
    frames = make_frames(fileset)
    paths = synth.write_series(dirpath, fileset, frames, fs['version'], fs['header'], fs['files'], fs['scan'],
                               seed=fs['seed'] + 1000)
    return dict(path=paths[0], paths=paths, frames=frames)


def load_kwargs(case, paths):
    """keyword arguments of TVIPSDataSet for a case (the reference's and this package's alike)"""
    return dict(case['kwargs'], path=paths['path'])


def make_masks(case):
    """3 float32 masks over the frame as the case shapes it: random weights, a ramp, a sparse one"""
    rng = np.random.default_rng(7)
    h, w = sig_shape(case)
    masks = np.zeros((N_MASKS, h, w), dtype=np.float32)
    masks[0] = rng.random((h, w), dtype=np.float32) - 0.25
    masks[1] = (np.arange(w, dtype=np.float32) / w)[None, :] * (np.arange(h, dtype=np.float32) / h)[:, None]
    masks[2, h // 2 - 1:h // 2 + 1, 1:w - 1] = 1
    masks[2, ::3, ::2] = 2
    return masks
