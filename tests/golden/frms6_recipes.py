"""
Seeded inputs of the FRMS6 golden vectors (tests/golden/frms6.npz): which synthetic sets are written
(tests/frms6_synth.py) and how each is loaded.  Imported by generate_frms6_golden.py (which loads the files with
the reference's FRMS6DataSet) and by the tests (which load the same files with this package); only small results
and checksums are stored.

Pixel values are <= 4095 (dark frames < 256), dark files hold <= 64 frames (every dark sum < 2**18: float32
sums of them are exact, the dark frame compares bit-equal), gain values lie in [0.5, 2].
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import frms6_synth  # noqa: E402

# the file sets: raw (folded) frame height x width, binning, frames per signal file, dark frames, stemimagesize
FILESETS = {
    'a': dict(height=4, width=16, binning=1, files=(5, 3), dark=3, nav=(2, 4), seed=81),
    'b': dict(height=3, width=24, binning=2, files=(6,), dark=4, nav=(6,), seed=82),
    'c': dict(height=2, width=10, binning=4, files=(2, 3), dark=2, nav=(5,), seed=83),
    # old files: num_frames = 0 in every file header, the count comes from the file size
    'f': dict(height=4, width=16, binning=1, files=(5, 3), dark=3, nav=(2, 4), seed=84, num_frames_field=0),
}

ROI_D = np.array([[True, False, True, True], [False, True, True, False]])

# the loads
CASES = [
    dict(name='A', fileset='a', offset=True, gain=None, sync_offset=0, roi=None),
    dict(name='B', fileset='b', offset=True, gain='mat', sync_offset=0, roi=None),
    dict(name='C', fileset='c', offset=False, gain='csv', sync_offset=0, roi=None),
    dict(name='D_p2', fileset='a', offset=True, gain=None, sync_offset=2, roi=ROI_D),
    dict(name='D_m2', fileset='a', offset=True, gain=None, sync_offset=-2, roi=ROI_D),
    dict(name='E', fileset='a', offset=False, gain=None, sync_offset=0, roi=None),
    dict(name='F', fileset='f', offset=True, gain=None, sync_offset=0, roi=None),
]

N_MASKS = 3


def sig_shape(fileset):
    fs = FILESETS[fileset]
    return (2 * fs['height'] * fs['binning'], fs['width'] // 2)


def crop(fileset):
    """rows around the fold (the last straight row and the first reversed one), all columns"""
    fs = FILESETS[fileset]
    mid = fs['height'] * fs['binning']
    return (slice(mid - 2, mid + 2), slice(None))


def make_raw(fileset):
    """-> (raw dark frames, [raw signal frames of file 001, 002, ...])"""
    fs = FILESETS[fileset]
    dark = frms6_synth.random_raw(fs['dark'], fs['height'], fs['width'], fs['seed'], high=256)
    signal = [frms6_synth.random_raw(n, fs['height'], fs['width'], fs['seed'] * 100 + i)
              for i, n in enumerate(fs['files'])]
    return dark, signal


def make_gain(fileset):
    return frms6_synth.random_gain(sig_shape(fileset), FILESETS[fileset]['seed'] + 1000)


def write_fileset(fileset, dirpath):
    """-> dict(hdr, mat, csv: paths; dark, signal: the unfolded frames; gain)"""
    fs = FILESETS[fileset]
    dark, signal = make_raw(fileset)
    hdr = frms6_synth.write_set(dirpath, fileset, dark, signal, fs['nav'], fs['binning'],
                                num_frames_field=fs.get('num_frames_field'))
    gain = make_gain(fileset)
    return dict(
        hdr=hdr, gain=gain,
        mat=frms6_synth.write_gain_mat(os.path.join(dirpath, f"{fileset}_gain.mat"), gain),
        csv=frms6_synth.write_gain_csv(os.path.join(dirpath, f"{fileset}_gain.csv"), gain),
        dark=frms6_synth.unfold(dark, fs['binning']),
        signal=np.concatenate([frms6_synth.unfold(r, fs['binning']) for r in signal]))


def load_kwargs(case, paths):
    """keyword arguments of FRMS6DataSet for a case (the reference's and this package's alike)"""
    kw = dict(path=paths['hdr'], enable_offset_correction=case['offset'], sync_offset=case['sync_offset'])
    if case['gain'] is not None:
        kw['gain_map_path'] = paths[case['gain']]
    return kw


def make_masks(fileset):
    """3 float32 masks over the frame: random weights, a ramp across the fold, a sparse one"""
    rng = np.random.default_rng(7)
    h, w = sig_shape(fileset)
    masks = np.zeros((N_MASKS, h, w), dtype=np.float32)
    masks[0] = rng.random((h, w), dtype=np.float32) - 0.25
    masks[1] = (np.arange(w, dtype=np.float32) / w)[None, :] * (np.arange(h, dtype=np.float32) / h)[:, None]
    masks[2, h // 2 - 1:h // 2 + 1, 1:w - 1] = 1
    masks[2, ::3, ::2] = 2
    return masks


def make_int_masks(fileset):
    """2 int64 masks (set E: integer frames x integer masks stay exact integers)"""
    rng = np.random.default_rng(8)
    h, w = sig_shape(fileset)
    return rng.integers(-3, 4, (2, h, w)).astype(np.int64)
