"""
Seeded inputs of the K2IS golden vectors (tests/golden/k2is.npz): which synthetic 8-file sets are written
(tests/k2is_synth.py) and how each is loaded.  Imported by generate_k2is_golden.py (which loads the files with
the reference's K2ISDataSet) and by the tests (which load the same files with this package); only small
results and checksums are stored.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import k2is_synth  # noqa: E402

# the file sets: frames (all of them, leading shutter-off frames included), how the sectors start and end
FILESETS = {
    # an unsynchronised start (sectors begin with 0 ... 5 blocks of the frame before), one frame before the
    # shutter opens, a truncated last frame in two sectors
    'lead': dict(n=4, seed=71, lead=1, extra=(0, 3, 0, 5, 0, 0, 2, 0), trailing=(0, 0, 7, 0, 0, 0, 0, 1)),
    'plain': dict(n=4, seed=72, lead=0, extra=None, trailing=None),
}

# the loads: sync_offset None = the native offset of the files
CASES = [
    dict(name='lead_unsync', fileset='lead', sync_offset=None),
    dict(name='sync_p1', fileset='plain', sync_offset=1),
    dict(name='sync_m2', fileset='plain', sync_offset=-2),
]

CROP = (slice(926, 934), slice(248, 264))       # a block-row edge (row 930) and a sector edge (column 256)
N_MASKS = 3


def make_frames(fileset):
    fs = FILESETS[fileset]
    return k2is_synth.random_frames(fs['n'], fs['seed'])


def write_fileset(fileset, dirpath):
    """-> (path of the first sector file, all frames of the set)"""
    fs = FILESETS[fileset]
    frames = make_frames(fileset)
    paths = k2is_synth.write_k2is(dirpath, frames, name=fileset, lead=fs['lead'], extra=fs['extra'],
                                  trailing=fs['trailing'])
    return paths[0], frames


def make_masks():
    """3 float32 masks over the frame: random weights, a ramp across the sector edges, a sparse one"""
    rng = np.random.default_rng(7)
    h, w = k2is_synth.FRAME_SHAPE
    masks = np.zeros((N_MASKS, h, w), dtype=np.float32)
    masks[0] = rng.random((h, w), dtype=np.float32) - 0.25
    masks[1] = (np.arange(w, dtype=np.float32) / w)[None, :] * (np.arange(h, dtype=np.float32) / h)[:, None]
    masks[2, 925:935, 250:262] = 1
    masks[2, ::97, ::101] = 2
    return masks
