"""
Seeded inputs of the record-file golden vectors (tests/golden/records.npz): which synthetic SEQ, EMPAD and BLO
files are written (tests/records_synth.py) and how each is loaded.  Imported by generate_records_golden.py (which
loads the files with the reference's SEQDataSet, EMPADDataSet and BloDataSet) and by the tests (which load the same
files with this package); only small results and checksums are stored.

Pixel values are <= 4095 (whole numbers in EMPAD's float32 too), dark values < 256, gain values lie in [0.5, 2].
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import records_synth as synth  # noqa: E402

# the files.  seq: frame height x width, pixel type, header version (< 5: the frames start at byte 1024), footer
# bytes, frames, side files; empad: frames, what the .xml says; blo: DP_SZ, pixel type, (NY, NX), endianess, magic,
# the bit depth line, bytes between the virtual bright field image and the patterns
FILESETS = {
    's16': dict(kind='seq', shape=(6, 8), dtype='u2', version=5, footer=8, n=8, side_files=True, seed=91),
    's8': dict(kind='seq', shape=(5, 5), dtype='u1', version=3, footer=3, n=6, side_files=False, seed=92),
    'e_acq': dict(kind='empad', n=8, acquire=(2, 4), search=(1, 2), seed=93),
    'e_search': dict(kind='empad', n=6, acquire=(4, 4), search=(2, 3), seed=94),
    'e_series': dict(kind='empad', n=5, series=5, seed=95),
    'b8': dict(kind='blo', side=5, dtype='u1', nav=(2, 3), endianess='<', magic=259, line=None, gap=1, seed=96),
    'b16le': dict(kind='blo', side=6, dtype='u2', nav=(2, 2), endianess='<', magic=259,
                  line='Blo Bit Depth: 16 bits', gap=3, seed=97),
    'b16be': dict(kind='blo', side=6, dtype='u2', nav=(2, 2), endianess='>', magic=259,
                  line='Blo Bit Depth: 16 bits', gap=3, seed=98),
    'b258': dict(kind='blo', side=5, dtype='u1', nav=(3, 2), endianess='<', magic=258, line=None, gap=2, seed=99),
}

# the bad-pixel maps of s16's XML file.  The frame is 6 x 8, its window starts at (OffsetY, OffsetX) = (1, 1).
# The reference builds a map's mask with `Columns` entries along the first axis and `Rows` along the second and
# crops only where offset + frame size fits into both: 8 "columns" x 10 "rows" takes the 6 x 8 window [1:7, 1:9].
# Of the three maps the second is taken: not binned, and wider than the first.
SEQ_OFFSET_YX = (1, 1)
SEQ_MAPS = [
    dict(columns=6, rows=10, binning=1, defects=[{'Row': '1'}]),
    dict(columns=8, rows=10, binning=None, defects=[
        {'Rows': '0-0'}, {'Row': '3'}, {'Column': '5'}, {'Column': '2', 'Row': '5'}, {'Columns': '9-9'}]),
    dict(columns=12, rows=12, binning=2, defects=[{'Columns': '2-7'}]),
]

ROI = np.array([[True, False, True, True], [False, True, True, False]])

# the loads
CASES = [
    dict(name='SEQ_A', fileset='s16', nav=(2, 4), sync_offset=0, roi=None),
    dict(name='SEQ_B', fileset='s8', nav=(6,), sync_offset=0, roi=None),
    dict(name='SEQ_p2', fileset='s16', nav=(2, 4), sync_offset=2, roi=ROI),
    dict(name='SEQ_m2', fileset='s16', nav=(2, 4), sync_offset=-2, roi=ROI),
    dict(name='EMPAD_acquire', fileset='e_acq', nav=(2, 4), via='xml', sync_offset=0, roi=None),
    dict(name='EMPAD_search', fileset='e_search', nav=(2, 3), via='xml', sync_offset=0, roi=None),
    dict(name='EMPAD_raw', fileset='e_acq', nav=(4, 2), via='raw', sync_offset=0, roi=None),
    dict(name='EMPAD_series', fileset='e_series', nav=(5,), via='xml', sync_offset=0, roi=None),
    dict(name='BLO_u8', fileset='b8', nav=(2, 3), sync_offset=0, roi=None),
    dict(name='BLO_u16le', fileset='b16le', nav=(2, 2), sync_offset=0, roi=None),
    dict(name='BLO_u16be', fileset='b16be', nav=(2, 2), sync_offset=0, roi=None),
    dict(name='BLO_258', fileset='b258', nav=(3, 2), sync_offset=0, roi=None),
]

N_MASKS = 3


def case(name):
    return next(c for c in CASES if c['name'] == name)


def sig_shape(fileset):
    fs = FILESETS[fileset]
    if fs['kind'] == 'seq':
        return fs['shape']
    return synth.EMPAD_SIZE if fs['kind'] == 'empad' else (fs['side'], fs['side'])


def stored_dtype(fileset):
    """the pixel type a reader hands out: '<f4' for EMPAD, little-endian unsigned for the others -- whatever
    `endianess` says (the byte-order pin)"""
    fs = FILESETS[fileset]
    return np.dtype('<f4') if fs['kind'] == 'empad' else np.dtype('<' + fs['dtype'])


def n_frames(fileset):
    fs = FILESETS[fileset]
    return fs['n'] if 'n' in fs else int(np.prod(fs['nav']))


def make_frames(fileset):
    """the frames as the detector counted them, (n,) + sig shape"""
    fs = FILESETS[fileset]
    rng = np.random.default_rng(fs['seed'])
    high = 256 if stored_dtype(fileset).itemsize == 1 else 4096
    values = rng.integers(0, high, (n_frames(fileset),) + tuple(sig_shape(fileset)))
    return values.astype(np.float32 if fs['kind'] == 'empad' else fs['dtype'])


def make_dark(fileset):
    return np.random.default_rng(FILESETS[fileset]['seed'] + 1000).integers(
        0, 256, sig_shape(fileset)).astype(np.float32)


def make_gain(fileset):
    return np.random.default_rng(FILESETS[fileset]['seed'] + 2000).uniform(
        0.5, 2.0, sig_shape(fileset)).astype(np.float32)


def seq_excluded():
    """the dead pixels of s16 as a (6, 8) mask, by hand from SEQ_MAPS[1]: 'Row(s)' index the mask's first axis,
    then the window [1:7, 1:9]"""
    mask = np.zeros((8, 10), dtype=bool)
    mask[0] = True
    mask[3] = True
    mask[:, 5] = True
    mask[5, 2] = True
    mask[:, 9] = True
    return mask[1:7, 1:9]


def crop(fileset):
    """-> f(frame): the rows next to the framing (the first two and the last two), at most 16 columns"""
    return lambda frame: frame[np.r_[0:2, frame.shape[0] - 2:frame.shape[0]]][:, :16]


def write_fileset(fileset, dirpath):
    """-> dict(path: what `load_kwargs` needs; frames: what a reader hands out, (n,) + sig shape of `stored_dtype`;
    kind-specific entries)"""
    fs = FILESETS[fileset]
    frames = make_frames(fileset)
    out = dict(kind=fs['kind'])
    if fs['kind'] == 'seq':
        path = synth.write_seq(os.path.join(dirpath, fileset + '.seq'), frames, fs['footer'], fs['version'])
        out.update(path=path, frames=frames, dark=None, gain=None, excluded=None)
        if fs['side_files']:
            dark, gain = make_dark(fileset), make_gain(fileset)
            synth.write_mrc(path + '.dark.mrc', dark[None], extended=64)
            synth.write_mrc(path + '.gain.mrc', gain[None])
            synth.write_seq_xml(path + '.Config.Metadata.xml', SEQ_MAPS)
            synth.write_seq_metadata(path + '.metadata', fs['shape'], SEQ_OFFSET_YX)
            out.update(dark=dark, gain=gain, excluded=seq_excluded())
    elif fs['kind'] == 'empad':
        raw = synth.write_empad_raw(os.path.join(dirpath, fileset + '.raw'), frames)
        xml = synth.write_empad_xml(os.path.join(dirpath, fileset + '.xml'), fileset + '.raw',
                                    fs.get('acquire'), fs.get('search'), fs.get('series'))
        out.update(path=xml, raw=raw, frames=frames)
    else:
        path, offset_2 = synth.write_blo(os.path.join(dirpath, fileset + '.blo'), frames, fs['nav'],
                                         fs['endianess'], fs['magic'], fs['line'], fs['gap'])
        # 16-bit pixels of an endianess='>' file come out unswapped: their bytes, read as little-endian
        stored = frames.byteswap() if (fs['endianess'] == '>' and frames.dtype.itemsize > 1) else frames
        out.update(path=path, frames=stored, data_offset=offset_2)
    return out


def load_kwargs(case, paths):
    """keyword arguments of the dataset class for a case (the reference's and this package's alike)"""
    fs = FILESETS[case['fileset']]
    kw = dict(path=paths['path'], sync_offset=case['sync_offset'])
    if fs['kind'] == 'seq':
        kw['nav_shape'] = case['nav']
    elif fs['kind'] == 'empad':
        if case['via'] == 'raw':
            kw.update(path=paths['raw'], nav_shape=case['nav'])
    else:
        kw['endianess'] = fs['endianess']
    return kw


def make_masks(fileset):
    """3 float32 masks over the frame: random weights, a ramp, a sparse one"""
    rng = np.random.default_rng(7)
    h, w = sig_shape(fileset)
    masks = np.zeros((N_MASKS, h, w), dtype=np.float32)
    masks[0] = rng.random((h, w), dtype=np.float32) - 0.25
    masks[1] = (np.arange(w, dtype=np.float32) / w)[None, :] * (np.arange(h, dtype=np.float32) / h)[:, None]
    masks[2, h // 2 - 1:h // 2 + 1, 1:w - 1] = 1
    masks[2, ::3, ::2] = 2
    return masks
