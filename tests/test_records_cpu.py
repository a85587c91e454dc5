"""
SEQDataSet, EMPADDataSet and BloDataSet without a GPU: the NumPy decoder of tests/records_synth.py (the yardstick
of the GPU tests) against the frames the REAL reference's readers read from the same synthetic files
(tests/golden/records.npz), the host-side parsing (headers, footers, frame counts, both nav-shape routes of EMPAD,
the bit depth and byte order of BLO, the MRC and XML side files of SEQ) against what the reference made of it,
the errors and warnings, and `Context.run_udf` picking up the corrections a SEQ set brings along.
"""
import os
import sys
import hashlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)

import records_recipes as recipes  # noqa: E402
import records_synth as synth  # noqa: E402

from libertem_amd.io.dataset.base import DataSetException  # noqa: E402
from libertem_amd.io import dataset  # noqa: E402
from libertem_amd.io.dataset import seq, blo, empad  # noqa: E402
from libertem_amd.io.dataset.seq import SEQDataSet  # noqa: E402
from libertem_amd.io.dataset.empad import EMPADDataSet  # noqa: E402
from libertem_amd.io.dataset.blo import BloDataSet  # noqa: E402
from libertem_amd.io.dataset.records import RecordFileDataSet  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'records.npz'))
CLASSES = {'seq': SEQDataSet, 'empad': EMPADDataSet, 'blo': BloDataSet}


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    d = tmp_path_factory.mktemp('records')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def make(case, filesets):
    kind = recipes.FILESETS[case['fileset']]['kind']
    return CLASSES[kind](**recipes.load_kwargs(case, filesets[case['fileset']]))


def expected_frames(case, frames):
    """the raw frames at the scan positions a case picks (all of them, or its ROI)"""
    at_positions = synth.positioned(frames, int(np.prod(case['nav'])), case['sync_offset'])
    return at_positions if case['roi'] is None else at_positions[case['roi'].reshape(-1)]


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_host_side_and_numpy_decoder_like_the_reference(filesets, case):
    name, fileset = case['name'], case['fileset']
    fs, rec = filesets[fileset], recipes.FILESETS[fileset]
    ds = make(case, filesets)
    layout = ds._scan_file()
    r = ds._records
    # the geometry
    assert tuple(layout.nav_shape) + tuple(layout.sig_shape) == tuple(GOLDEN[name + '__shape'])
    assert tuple(layout.nav_shape) == tuple(case['nav']) and layout.sig_shape == recipes.sig_shape(fileset)
    assert ds._image_count == int(GOLDEN[name + '__image_count']) == layout.n_frames == recipes.n_frames(fileset)
    assert layout.storage == np.dtype(str(GOLDEN[name + '__raw_dtype'])) == recipes.stored_dtype(fileset)
    assert str(GOLDEN[name + '__dtype']) == str(GOLDEN[name + '__raw_dtype'])     # (ds.dtype stays the raw dtype)
    assert layout.stride == r['frame_header'] + r['payload_bytes'] + r['frame_footer']
    assert layout.sync_offset == case['sync_offset']
    if rec['kind'] == 'seq':
        assert r['frame_footer'] == int(GOLDEN[name + '__footer']) == rec['footer'] == ds._footer_size
        assert (r['file_header'], r['frame_header']) == (8192 if rec['version'] >= 5 else 1024, 0)
    elif rec['kind'] == 'empad':
        assert (r['file_header'], r['frame_header'], r['payload_bytes'], r['frame_footer']) == (0, 0, 65536, 1024)
        assert r['path'] == fs['raw']
    else:
        assert (r['file_header'], r['frame_header'], r['frame_footer']) == (fs['data_offset'], 6, 0)
    # the decoder: strips the framing of the file as the reference's reader did
    data = np.fromfile(r['path'], dtype=np.uint8)
    frames = synth.strip(data, r['file_header'], r['frame_header'], r['payload_bytes'], r['frame_footer'],
                         layout.n_frames, layout.storage, layout.native_shape)
    assert np.array_equal(frames, fs['frames']) and frames.dtype == fs['frames'].dtype.newbyteorder('<')
    want = expected_frames(case, frames)
    assert len(want) == len(GOLDEN[name + '__sha_frames'])
    for p, frame in enumerate(want):
        assert np.array_equal(sha(frame), GOLDEN[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(recipes.crop(fileset)(frame), GOLDEN[name + '__crops'][p]), (name, p)
    assert ds.check_valid() is True


def test_geometries_of_the_recipes(filesets):
    """the cases the formats differ in: an odd pattern offset, a footer that is no multiple of 2, the offsets of
    both header versions, the byte-order pin"""
    assert filesets['b8']['data_offset'] % 2 == 1
    assert recipes.FILESETS['s8']['footer'] % 2 == 1 and recipes.FILESETS['s8']['version'] < 5
    assert recipes.FILESETS['s16']['footer'] == 8
    # 16-bit pixels of an endianess='>' file: the reference handed the words on unswapped (read as little-endian)
    counted = recipes.make_frames('b16be')
    assert np.array_equal(filesets['b16be']['frames'], counted.byteswap())
    assert np.array_equal(sha(counted.byteswap()[0]), GOLDEN['BLO_u16be__sha_frames'][0])
    assert not np.array_equal(sha(counted[0]), GOLDEN['BLO_u16be__sha_frames'][0])
    assert np.array_equal(sha(recipes.make_frames('b16le')[0]), GOLDEN['BLO_u16le__sha_frames'][0])


def test_strip_by_hand():
    """file header 3, frame header 2, payload 4, footer 1; the last record without its footer"""
    data = np.array([9, 9, 9, 8, 8, 1, 2, 3, 4, 7, 8, 8, 5, 6, 7, 8], dtype=np.uint8)
    assert np.array_equal(synth.strip(data, 3, 2, 4, 1, 2, np.uint8, (2, 2)), [[[1, 2], [3, 4]], [[5, 6], [7, 8]]])
    assert np.array_equal(synth.strip(data, 3, 2, 4, 1, 2, '<u2', (2,)), [[0x0201, 0x0403], [0x0605, 0x0807]])
    rec = synth.records(np.arange(8, dtype=np.uint8).reshape(2, 4), 2, 3, last_footer=False)
    assert rec.tolist() == [255, 255, 0, 1, 2, 3, 238, 238, 238, 255, 255, 4, 5, 6, 7]


# --- SEQ --------------------------------------------------------------------------------------------------------
def test_seq_header_and_base_name(filesets):
    h = seq.read_header(filesets['s16']['path'])
    assert seq.HEADER_SIZE == 632          # (4 + 24 + 4 + 4 + 512 + 9 x 4 + 8 + 9 x 4 + 2 + 2)
    assert (h['magic'], h['version'], h['width'], h['height'], h['bit_depth']) == (0xFEED, 5, 8, 6, 16)
    assert h['name'] == 'Norpix seq' and h['description'] == 'synthetic frames'
    assert h['true_image_size'] == 6 * 8 * 2 + 8 and h['image_format'] == 100 and h['compression_format'] == 0
    assert h['suggested_frame_rate'] == 30.0
    assert seq.image_offset(h) == 8192 and seq.image_offset(dict(version=4)) == 1024
    assert seq.base_name('/d/x.seq') == seq.base_name('/d/x.seq.seq') == seq.base_name('/d/x.SEQ') == '/d/x'
    assert seq.base_name('/d/x.bin') == '/d/x.bin' and seq.base_name('/d/x.mrc.seq') == '/d/x.mrc'


def test_seq_corrections_like_the_reference(filesets):
    fs = filesets['s16']
    ds = make(recipes.case('SEQ_A'), filesets)
    ds._scan_file()
    ds._load_corrections()
    corr = ds.get_correction_data()
    dark, gain, excluded = corr.get_dark_frame(), corr.get_gain_map(), corr.get_excluded_pixels()
    assert dark.dtype == gain.dtype == np.float32 and dark.shape == gain.shape == (6, 8)
    assert np.array_equal(dark, GOLDEN['SEQ_A__dark']) and np.array_equal(gain, GOLDEN['SEQ_A__gain'])
    assert np.array_equal(dark, fs['dark']) and np.array_equal(gain, fs['gain'])
    assert excluded.shape == (6, 8)
    got = set(zip(*excluded.coords.tolist()))
    assert got == set(zip(*GOLDEN['SEQ_A__excluded'].tolist())) and len(got) == GOLDEN['SEQ_A__excluded'].shape[1]
    assert np.array_equal(excluded.todense(), fs['excluded'])
    diag = {x['name']: x['value'] for x in ds.get_diagnostics()}
    assert diag['Footer size'] == '8' and diag['Dark frame included'] == diag['Gain map included'] == 'True'
    assert diag['width'] == '8' and diag['name'] == 'Norpix seq'
    # no side files: an empty set; the XML alone (no .metadata) is not read
    plain = make(recipes.case('SEQ_B'), filesets)
    plain._scan_file()
    plain._load_corrections()
    assert not plain.get_correction_data().have_corrections()
    synth.write_seq_xml(filesets['s8']['path'] + '.Config.Metadata.xml', recipes.SEQ_MAPS)
    try:
        plain._load_corrections()
        assert plain.get_correction_data().get_excluded_pixels() is None
    finally:
        os.remove(filesets['s8']['path'] + '.Config.Metadata.xml')


def test_both_mrc_readers_against_what_the_writer_wrote(tmp_path):
    """the package's reader and the generator's stand-in for ncempy are both ours: each against the array in the
    file, every mode, with and without an extended header"""
    sys.path.insert(0, os.path.join(HERE, 'golden', 'refshim'))
    try:
        from ncempy.io.mrc import mrcReader
    finally:
        sys.path.remove(os.path.join(HERE, 'golden', 'refshim'))
        for mod in [m for m in sys.modules if m == 'ncempy' or m.startswith('ncempy.')]:
            del sys.modules[mod]
    rng = np.random.default_rng(3)
    for dtype, extended, shape in ((np.int8, 0, (1, 3, 5)), (np.int16, 128, (2, 3, 5)), (np.float32, 64, (1, 6, 8)),
                                   (np.uint16, 0, (1, 1, 7))):
        data = (rng.integers(0, 100, shape) - (0 if dtype == np.uint16 else 50)).astype(dtype)
        path = synth.write_mrc(str(tmp_path / 'x.mrc'), data, extended)
        for got in (seq.read_mrc(path), mrcReader(path)['data'], synth.read_mrc(path)):
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, data)
    words = np.zeros(256, dtype='<i4')
    words[:4] = 2, 2, 1, 4
    words.tofile(str(tmp_path / 'complex.mrc'))
    with pytest.raises(DataSetException, match='MRC mode 4'):
        seq.read_mrc(str(tmp_path / 'complex.mrc'))
    synth.write_mrc(str(tmp_path / 'cut.mrc'), np.zeros((1, 4, 4), np.float32))
    os.truncate(str(tmp_path / 'cut.mrc'), 1024 + 60)
    with pytest.raises(DataSetException, match='fewer than 1 x 4 x 4'):
        seq.read_mrc(str(tmp_path / 'cut.mrc'))


def test_bad_pixel_map_choice_and_crop(tmp_path):
    from xml.etree import ElementTree
    path = synth.write_seq_xml(str(tmp_path / 'm.xml'), recipes.SEQ_MAPS)
    root = ElementTree.parse(path).getroot()
    meta = dict(UnbinnedFrameSizeY=6, UnbinnedFrameSizeX=8, OffsetY=1, OffsetX=1, HardwareBinning=1)
    assert np.array_equal(seq.bad_pixel_map(root, meta), recipes.seq_excluded())
    # a window that does not fit into the map: the map comes back whole (as the reference leaves it)
    whole = seq.bad_pixel_map(root, dict(meta, OffsetX=3))
    assert whole.shape == (8, 10) and whole[0].all() and whole[:, 9].all() and whole[5, 2]
    # a hardware-binned acquisition takes the binned map, sizes and offsets halved: 12 x 12 -> [1:5, 2:8]
    binned = seq.bad_pixel_map(root, dict(UnbinnedFrameSizeY=8, UnbinnedFrameSizeX=12, OffsetY=2, OffsetX=4,
                                          HardwareBinning=2))
    assert binned.shape == (4, 6) and np.array_equal(binned, np.ones((4, 6), dtype=bool))
    m = synth.write_seq_metadata(str(tmp_path / 'm.metadata'), (6, 8), (1, 2), binning=2)
    got = seq.read_metadata(m)
    assert (got['UnbinnedFrameSizeY'], got['UnbinnedFrameSizeX'], got['OffsetY'], got['OffsetX']) == (6, 8, 1, 2)
    assert got['HardwareBinning'] == 2 and got['OkraMode'] is False and len(got) == 12


def test_seq_errors_and_warnings(filesets, tmp_path):
    path = filesets['s16']['path']
    with pytest.raises(TypeError, match="missing 1 required argument: 'nav_shape'"):
        SEQDataSet(path=path)
    with pytest.warns(FutureWarning, match='scan_size argument is deprecated'):
        ds = SEQDataSet(path=path, scan_size=(4, 2))
    assert ds._scan_file().nav_shape == (4, 2)
    with pytest.warns(FutureWarning), pytest.raises(ValueError, match='cannot specify both scan_size and nav_shape'):
        SEQDataSet(path=path, scan_size=(4, 2), nav_shape=(4, 2))
    with pytest.raises(ValueError, match='I/O backends'):
        SEQDataSet(path=path, nav_shape=(8,), io_backend=object())
    with pytest.raises(DataSetException, match='sig_shape must be of size: 48'):
        SEQDataSet(path=path, nav_shape=(8,), sig_shape=(7, 7))._scan_file()
    assert SEQDataSet(path=path, nav_shape=(8,), sig_shape=(48,))._scan_file().sig_shape == (48,)
    for so in (8, -8):
        with pytest.raises(DataSetException, match=r'offset should be in \(-8, 8\), which is \(-image_count'):
            SEQDataSet(path=path, nav_shape=(8,), sync_offset=so)._scan_file()
    frames = recipes.make_frames('s8')
    for override, message in ((dict(magic=0xBEEF), 'The format of this .seq file is unrecognized'),
                              (dict(compression_format=1), 'Only uncompressed images are supported'),
                              (dict(image_format=200), 'Non-monochrome images are not supported')):
        bad = synth.write_seq(str(tmp_path / 'bad.seq'), frames, 3, **override)
        ds = SEQDataSet(path=bad, nav_shape=(6,))
        ds._scan_file()
        with pytest.raises(DataSetException, match=message):
            ds.check_valid()
    bad = synth.write_seq(str(tmp_path / 'bad.seq'), frames, 3, bit_depth=12)
    with pytest.raises(DataSetException, match='unsupported bit depth: 12'):
        SEQDataSet(path=bad, nav_shape=(6,))._scan_file()
    # a last record without its footer still counts only whole records (the reference's rule)
    cut = synth.write_seq(str(tmp_path / 'cut.seq'), frames, 3, last_footer=False)
    assert SEQDataSet(path=cut, nav_shape=(5,))._scan_file().n_frames == 5


# --- EMPAD ------------------------------------------------------------------------------------------------------
def test_empad_nav_shape_routes_and_errors(filesets, tmp_path):
    raw, xml = filesets['e_acq']['raw'], filesets['e_acq']['path']
    assert empad.get_params_from_xml(xml) == (raw, (2, 4))
    assert empad.get_params_from_xml(xml, 'search') == (raw, (1, 2))
    assert empad.get_params_from_xml(filesets['e_series']['path'])[1] == (5,)
    # the file size matches the "search" shape only
    ds = EMPADDataSet(path=filesets['e_search']['path'])
    assert ds._scan_file().nav_shape == (2, 3) and ds._image_count == 6
    # a nav_shape of the caller's wins over the file's; image_count stays what the XML says
    ds = EMPADDataSet(path=xml, nav_shape=(3,))
    assert ds._scan_file().nav_shape == (3,) and ds._image_count == 8
    # neither shape matches
    synth.write_empad_raw(str(tmp_path / 'odd.raw'), np.zeros((3, 128, 128), np.float32))
    odd = synth.write_empad_xml(str(tmp_path / 'odd.xml'), 'odd.raw', acquire=(2, 2), search=(1, 2))
    with pytest.raises(ValueError, match=r'RAW data file size mismatch; filesize=199680 vs expected size 266240 '
                                         r'for nav \(2, 2\) or alternate 133120 for nav \(1, 2\)'):
        EMPADDataSet(path=odd)._scan_file()
    with pytest.raises(DataSetException, match='need to set or detect nav_shape!'):
        EMPADDataSet(path=raw)._scan_file()
    with pytest.raises(DataSetException, match='path should either be .xml or .raw'):
        EMPADDataSet(path=str(tmp_path / 'x.bin'))._scan_file()
    (tmp_path / 'broken.xml').write_text('<root><type>tomography</type><raw_file filename="x.raw"/></root>')
    with pytest.raises(DataSetException, match='could not initialize EMPAD file; error: unknown type: tomography'):
        EMPADDataSet(path=str(tmp_path / 'broken.xml'))._scan_file()
    with pytest.raises(DataSetException, match='could not open file .*gone.raw'):
        EMPADDataSet(path=str(tmp_path / 'gone.raw'), nav_shape=(2,))._scan_file()
    with pytest.raises(DataSetException, match='sig_shape must be of size: 16384'):
        EMPADDataSet(path=xml, sig_shape=(128, 127))._scan_file()
    with pytest.warns(FutureWarning, match='scan_size argument is deprecated'):
        assert EMPADDataSet(path=raw, scan_size=(8,))._scan_file().nav_shape == (8,)
    # a .raw file whose last record lacks its footer rows: 7 whole records
    synth.write_empad_raw(str(tmp_path / 'cut.raw'), recipes.make_frames('e_acq'), last_footer=False)
    assert EMPADDataSet(path=str(tmp_path / 'cut.raw'), nav_shape=(7,))._scan_file().n_frames == 7


# --- BLO --------------------------------------------------------------------------------------------------------
def test_blo_header_text_block_and_errors(filesets, tmp_path):
    for name, endianess in (('b16le', '<'), ('b16be', '>')):
        h = blo.read_header(filesets[name]['path'], endianess)
        assert (h['MAGIC'], h['DP_SZ'], h['NY'], h['NX'], h['ID']) == (259, 6, 2, 2, b'IMGBLO')
        assert h['Data_offset_2'] == filesets[name]['data_offset'] == h['Data_offset_1'] + 4 + 3
        assert h['SX'] == 1.5 and h['Beam_energy'] == 200000
        lines = blo.read_text_block(filesets[name]['path'], h)
        assert lines == ('Astar blockfile', 'Camera: synthetic', 'Blo Bit Depth: 16 bits', 'end')
        assert blo.pixel_dtype(lines) == 'u2'
    assert blo.header_dtype('<').itemsize == blo.TEXT_START == 240        # (the text block starts behind it)
    h = blo.read_header(filesets['b258']['path'])
    assert h['MAGIC'] == 258 and blo.read_text_block(filesets['b258']['path'], h) == ()
    assert blo.pixel_dtype(()) == 'u1' and blo.pixel_dtype(('blo bit depth: 8 bits',)) == 'u1'
    assert blo.pixel_dtype(('Blo Bit Depth: sixteen bits',)) == 'u1' and blo.pixel_dtype(('Bit Depth: 16 bits',)) == 'u1'
    assert blo.pixel_dtype(('x', 'BLO BIT DEPTH:  32 bits ')) == 'u4'
    # the wrong endianess: a magic that is none
    ds = BloDataSet(path=filesets['b16be']['path'])
    with pytest.raises(DataSetException, match=r"invalid magic number: 301 not in \('0x102', '0x103'\)"):
        ds.check_valid()
    with pytest.raises(DataSetException, match='invalid dataset'):
        BloDataSet(path=str(tmp_path / 'gone.blo')).check_valid()
    path = filesets['b8']['path']
    with pytest.warns(FutureWarning, match='tileshape argument is ignored'):
        BloDataSet(path=path, tileshape=(1, 8, 5, 5))
    with pytest.raises(DataSetException, match='sig_shape must be of size: 25'):
        BloDataSet(path=path, sig_shape=(5, 6))._scan_file()
    assert BloDataSet(path=path, nav_shape=(3, 2), sig_shape=(25,))._scan_file()[:2] == ((3, 2), (25,))
    for so in (6, -6):
        with pytest.raises(DataSetException, match=r'offset should be in \(-6, 6\), which is \(-image_count'):
            BloDataSet(path=path, sync_offset=so)._scan_file()
    with pytest.raises(RuntimeError, match='initialize'):
        BloDataSet(path=path).header


# --- the public surface -----------------------------------------------------------------------------------------
def test_load_is_available_under_both_spellings(filesets):
    # (fails without the feature: "dataset type 'seq' is not available")
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    kwargs = {'seq': dict(path=filesets['s16']['path'], nav_shape=(2, 4)),
              'empad': dict(path=filesets['e_acq']['path']), 'blo': dict(path=filesets['b8']['path'])}
    for key, cls in CLASSES.items():
        assert cls.__name__ in dataset.__all__ and issubclass(cls, RecordFileDataSet)
        assert cls.DECODE_KERNEL == 'ltmi_records_gather' and key.upper() in cls.KIND
        for spelling in (key, key.upper()):
            ds = dataset.load(spelling, **kwargs[key])
            assert type(ds) is cls and 'not initialized' in repr(ds) and ds.path == kwargs[key]['path']
        assert f"'{key}'" in str(pytest.raises(DataSetException, dataset.load, 'nothing_like_it').value)
    assert all(word in dataset.load.__doc__ for word in ('SEQ', 'EMPAD', 'BLO'))
    # the files are gathered on the GPU: an executor that drives none is told so, not handed host frames
    ctx = Context(executor=InlineJobExecutor())
    try:
        for key in CLASSES:
            with pytest.raises(DataSetException, match=r'decodes the files on the GPU \(ltmi_records_gather\)'):
                ctx.load(key, **kwargs[key])
    finally:
        ctx.close()


def test_detect_params_and_extensions(filesets, tmp_path):
    assert SEQDataSet.get_supported_extensions() == {'seq'}
    assert EMPADDataSet.get_supported_extensions() == {'xml', 'raw'}
    assert BloDataSet.get_supported_extensions() == {'blo'}
    path = filesets['s16']['path']
    assert SEQDataSet.detect_params(path) == {
        'parameters': {'path': path, 'nav_shape': (8,), 'sig_shape': (6, 8)},
        'info': {'image_count': 8, 'native_sig_shape': (6, 8)}}
    path = filesets['e_search']['path']
    assert EMPADDataSet.detect_params(path) == {
        'parameters': {'path': path, 'nav_shape': (2, 3), 'sig_shape': (128, 128)},
        'info': {'image_count': 6, 'native_sig_shape': (128, 128)}}
    path = filesets['b258']['path']
    assert BloDataSet.detect_params(path) == {
        'parameters': {'path': path, 'nav_shape': (3, 2), 'sig_shape': (5, 5), 'tileshape': (1, 8, 5, 5),
                       'endianess': '<'},
        'info': {'image_count': 6, 'native_sig_shape': (5, 5)}}
    garbage = tmp_path / 'garbage.bin'
    garbage.write_bytes(bytes(range(256)) * 40)
    for cls in CLASSES.values():
        assert cls.detect_params(str(garbage)) is False
        assert cls.detect_params(__file__) is False
        assert cls.detect_params(str(tmp_path / 'absent')) is False
    assert EMPADDataSet.detect_params(filesets['e_acq']['raw']) is False     # (a .raw alone names no scan)
    assert BloDataSet.detect_params(filesets['b16be']['path']) is False      # (detection reads little-endian)


def test_compat_alias():
    import importlib
    import libertem_amd.compat as compat
    had = 'libertem' in sys.modules
    compat.install()
    try:
        assert importlib.import_module('libertem.io.dataset.seq').SEQDataSet is SEQDataSet
        assert importlib.import_module('libertem.io.dataset.empad').EMPADDataSet is EMPADDataSet
        assert importlib.import_module('libertem.io.dataset.blo').BloDataSet is BloDataSet
    finally:
        if not had:
            compat.uninstall()


def test_context_applies_a_seq_sets_own_corrections(filesets):
    """`run_udf` with `corrections=None` takes what `get_correction_data()` of the dataset returns -- here the
    CorrectionSet a SEQDataSet built from its side files, carried by a host-side stand-in for the resident frames
    (the stand-in of tests/test_frms6_cpu.py)"""
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.io.dataset.memory import MemoryDataSet
    from libertem_amd.udf.sumsigudf import SumSigUDF
    fs = filesets['s16']
    seq_ds = make(recipes.case('SEQ_A'), filesets)
    seq_ds._scan_file()
    seq_ds._load_corrections()

    class Stub(MemoryDataSet):
        def get_correction_data(self):
            return seq_ds.get_correction_data()
    ctx = Context(executor=InlineJobExecutor())
    try:
        ds = Stub(data=fs['frames'].reshape(2, 4, 6, 8), sig_dims=2, num_partitions=2).initialize(ctx.executor)
        got = ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data
        ref = GOLDEN['SEQ_A__sumsig']
        assert got.shape == ref.shape and np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
        assert np.allclose(got.reshape(-1), GOLDEN['SEQ_A__picked_sumsig'], rtol=1e-5)
        plain = ctx.run_udf(dataset=ds, udf=SumSigUDF(), corrections=CorrectionSet())['intensity'].data
        assert np.array_equal(plain.reshape(-1), fs['frames'].reshape(8, -1).sum(axis=1, dtype=np.float64))
    finally:
        ctx.close()
