"""
TVIPSDataSet, the segments of RecordFileDataSet and `load('auto')` without a GPU: the by-hand decoder of
tests/tvips_synth.py (the yardstick of the GPU tests) against the frames the REAL reference's reader read from the
same synthetic series (tests/golden/tvips.npz); the host-side parsing (series header, frames per file, the guessed
sync_offset and nav_shape) against what the reference made of it; the arithmetic that keeps a chunk inside one
file against a brute-force loop; file ordering, the errors, the two places where this package deliberately does
not raise where the reference does; and the registry: `detect()`, `load('auto')`, `get_extensions()`.

Before the feature `load('tvips')` and `load('auto')` answered "dataset type ... is not available".
"""
import os
import sys
import hashlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)

import tvips_recipes as recipes  # noqa: E402
import tvips_synth as synth  # noqa: E402
import records_synth  # noqa: E402

from libertem_amd.io.dataset.base import DataSetException  # noqa: E402
from libertem_amd.io import dataset  # noqa: E402
from libertem_amd.io.dataset import tvips  # noqa: E402
from libertem_amd.io.dataset.tvips import TVIPSDataSet  # noqa: E402
from libertem_amd.io.dataset.records import RecordFileDataSet, Segment, locate  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'tvips.npz'))


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    d = tmp_path_factory.mktemp('tvips')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def expected_frames(case, frames):
    """the raw frames at the scan positions a case picks (all of them, or its ROI), shaped as the case shapes them"""
    at_positions = records_synth.positioned(frames, int(np.prod(case['nav'])), case['sync_offset'])
    at_positions = at_positions.reshape((len(at_positions),) + recipes.sig_shape(case))
    return at_positions if case['roi'] is None else at_positions[case['roi'].reshape(-1)]


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_host_side_and_by_hand_decoder_like_the_reference(filesets, case):
    name, fileset = case['name'], case['fileset']
    fs, rec = filesets[fileset], recipes.FILESETS[fileset]
    ds = TVIPSDataSet(**recipes.load_kwargs(case, fs))
    layout = ds._scan_file()
    r = ds._records
    # the geometry, the guessed parameters
    assert tuple(layout.nav_shape) + tuple(layout.sig_shape) == tuple(GOLDEN[name + '__shape'])
    assert tuple(layout.nav_shape) == tuple(case['nav']) and layout.sig_shape == recipes.sig_shape(case)
    assert layout.native_shape == recipes.native_shape(fileset)
    assert layout.sync_offset == int(GOLDEN[name + '__sync_offset']) == case['sync_offset']
    assert ds._image_count == int(GOLDEN[name + '__image_count']) == layout.n_frames == recipes.n_frames(fileset)
    assert layout.storage == np.dtype(str(GOLDEN[name + '__raw_dtype'])) == recipes.stored_dtype(fileset)
    assert str(GOLDEN[name + '__dtype']) == str(GOLDEN[name + '__raw_dtype'])
    assert layout.stride == recipes.stride(fileset) == r['frame_header'] + r['payload_bytes']
    assert (r['path'], r['file_header'], r['frame_header'], r['frame_footer']) == (fs['path'], 256, rec['header'], 0)
    # one segment per file
    firsts = np.concatenate([[0], np.cumsum(rec['files'])[:-1]])
    assert r['segments'] == tuple(Segment(p, 256 if i == 0 else 0, int(firsts[i]), n)
                                  for i, (p, n) in enumerate(zip(fs['paths'], rec['files'])))
    # the decoder: strips the framing of the files as the reference's reader did
    frames = synth.strip_series(fs['paths'], rec['files'], rec['header'], layout.storage, layout.native_shape)
    assert np.array_equal(frames, fs['frames']) and frames.dtype == recipes.stored_dtype(fileset)
    assert frames.max() <= (255 if frames.dtype.itemsize == 1 else 4095)
    want = expected_frames(case, frames)
    assert len(want) == len(GOLDEN[name + '__sha_frames'])
    for p, frame in enumerate(want):
        assert np.array_equal(sha(frame), GOLDEN[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(recipes.crop(fileset)(frame), GOLDEN[name + '__crops'][p]), (name, p)
    assert ds.check_valid() is True
    assert ds.header.version == rec['version'] and ds.header.frame_header_bytes == rec['header']


def test_image_header_offsets_are_the_references():
    """Scan_x and Scan_y: float32 behind 17 four-byte fields; the writer, the package and the recipe agree, and the
    golden sync_offset of t16 (1: read from these bytes) says the reference does too"""
    assert (synth.SCAN_X_AT, synth.SCAN_Y_AT) == (tvips.SCAN_X_OFFSET, tvips.SCAN_X_OFFSET + 4) == (68, 72)
    assert int(GOLDEN['TV_bare__sync_offset']) == 1 and tuple(GOLDEN['TV_bare__shape'][:2]) == (2, 4)
    assert int(GOLDEN['TV_line__sync_offset']) == 1 and int(GOLDEN['TV_noscan__sync_offset']) == 0
    assert tvips.SERIES_FIELDS == synth.SERIES_WORDS and tvips.SERIES_HEADER_SIZE == 256


# --- the segments ------------------------------------------------------------------------------------------------
def test_locate_against_a_brute_force_loop(filesets):
    """every (g, n_max) of t16: the file of frame g, its byte offset there, and no frame of the next file"""
    ds = TVIPSDataSet(path=filesets['t16']['path'])
    stride = ds._scan_file().stride
    segments = ds._records['segments']
    assert [s[1:] for s in segments] == [(256, 0, 7), (0, 7, 3), (0, 10, 2)] and stride == 208
    owner = []                                  # frame -> (file, index in the file), by counting
    for i, seg in enumerate(segments):
        owner += [(i, k) for k in range(seg.n_frames)]
    assert len(owner) == 12
    for g in range(12):
        for n_max in range(1, 14):
            i, k = owner[g]
            n = 0
            while n < n_max and g + n < 12 and owner[g + n][0] == i:
                n += 1
            assert locate(g, n_max, segments, stride) == (i, segments[i].file_header + k * stride, n), (g, n_max)
    for g in (-1, 12, 13):
        with pytest.raises(IndexError, match='is in none of the 3 files'):
            locate(g, 1, segments, stride)
    with pytest.raises(ValueError, match='n_max is 0'):
        locate(0, 0, segments, stride)
    # files without frames are stepped over
    gappy = [('a', 5, 0, 0), ('b', 0, 0, 2), ('c', 9, 2, 0), ('d', 1, 2, 3), ('e', 0, 5, 0)]
    assert [locate(g, 9, gappy, 10) for g in range(5)] == [(1, 0, 2), (1, 10, 1), (3, 1, 3), (3, 11, 2), (3, 21, 1)]
    with pytest.raises(IndexError):
        locate(5, 1, gappy, 10)


def test_one_file_formats_are_one_segment(tmp_path):
    """`_record_layout` keeps its signature and its `_records` keys; a series must continue frame by frame"""
    ds = RecordFileDataSet('x.bin')
    layout = ds._record_layout('x.bin', file_header=7, frame_header=2, payload_bytes=12, frame_footer=1,
                               storage='<u2', native_shape=(2, 3), n_frames=5, nav_shape=(5,))
    assert layout.stride == 15 and layout.n_frames == 5
    assert ds._records == dict(path='x.bin', file_header=7, frame_header=2, payload_bytes=12, frame_footer=1,
                               segments=(Segment('x.bin', 7, 0, 5),))
    layout = ds._segments_layout([('a', 7, 0, 2), ('b', 0, 2, 3)], 2, 12, 1, '<u2', (2, 3), (5,))
    assert layout.n_frames == 5 and ds._image_count == 5 and ds._records['path'] == 'a'
    with pytest.raises(DataSetException, match='b: frames 3 to 6 do not continue the 2 frames before'):
        ds._segments_layout([('a', 7, 0, 2), ('b', 0, 3, 3)], 2, 12, 1, '<u2', (2, 3), (5,))
    with pytest.raises(DataSetException, match='no files'):
        ds._segments_layout([], 2, 12, 1, '<u2', (2, 3), (5,))


# --- the files of a set ------------------------------------------------------------------------------------------
def test_file_ordering(tmp_path):
    frames = recipes.make_frames('t8v1')[:3]
    d = str(tmp_path)
    # _010 sorts behind _002 (by number, not by name: '_010' < '_002' is false, but 'x_10' < 'x_2' would be true)
    paths = synth.write_series(d, 'scan', np.concatenate([frames] * 4), 1, 12, (3, 3, 3, 3), numbers=(0, 1, 2, 10))
    # another set in the same directory, and a stem that ends in digits
    other = synth.write_series(d, 'scanner', frames, 1, 12, (2, 1))
    digits = synth.write_series(d, 'run42', frames, 1, 12, (1, 2))
    for given in paths:
        assert tvips.get_filenames(given) == paths
    assert [tvips.file_suffix(p) for p in paths] == [0, 1, 2, 10]
    assert tvips.get_filenames(other[1]) == other
    # 'run42_000': only the digits at the very end of the stem are stripped
    assert tvips.get_filenames(digits[0]) == digits
    layout = TVIPSDataSet(path=paths[3])._scan_file()
    assert layout.n_frames == 12 and layout.nav_shape == (12,)
    # brackets in the directory name are no pattern
    odd = tmp_path / 'a[1]'
    odd.mkdir()
    inside = synth.write_series(str(odd), 's', frames, 1, 12, (2, 1))
    assert tvips.get_filenames(inside[1]) == inside
    assert tvips.get_filenames(inside[0].replace('.tvips', '.TVIPS')) == inside     # (the extension in any case)
    with pytest.raises(DataSetException, match='unknown extension'):
        tvips.get_filenames(str(tmp_path / 'scan_000.tif'))
    with pytest.raises(DataSetException, match='unknown extension'):
        TVIPSDataSet(path=str(tmp_path / 'scan_000.raw'))._scan_file()
    with pytest.raises(DataSetException, match='no files found'):
        tvips.get_filenames(str(tmp_path / 'absent_000.tvips'))
    (tmp_path / 'lone.tvips').write_bytes(b'\x00' * 300)
    with pytest.raises(DataSetException, match='three digits'):
        tvips.get_filenames(str(tmp_path / 'lone.tvips'))


def test_errors(filesets, tmp_path):
    frames = recipes.make_frames('t8v1')
    d = str(tmp_path)
    for k, (override, message) in enumerate((
            (dict(version=3), 'Unknown TVIPS header version: 3'),
            (dict(version=0), 'Unknown TVIPS header version: 0'),
            (dict(size=512), r'Invalid header size 512, should be 256. Maybe not a TVIPS file\?'),
            (dict(bpp=12), r'unknown bpp value: 12 \(should be either 8 or 16\)'),
            (dict(bpp=32), r'unknown bpp value: 32 \(should be either 8 or 16\)'))):
        bad = synth.write_series(d, 'bad%d' % k, frames, 1, 12, (7,), override=override)[0]
        with pytest.raises(DataSetException, match=message):
            TVIPSDataSet(path=bad)._scan_file()
        with pytest.raises(DataSetException, match=message):
            TVIPSDataSet.detect_params(bad)
    (tmp_path / 'short_000.tvips').write_bytes(b'\x00\x01' * 20)
    with pytest.raises(DataSetException, match='shorter than a TVIPS series header'):
        TVIPSDataSet(path=str(tmp_path / 'short_000.tvips'))._scan_file()
    # a file that is no whole number of records (the reference asserts here)
    cut = synth.write_series(d, 'cut', frames, 1, 12, (4, 3))
    with open(cut[1], 'ab') as f:
        f.write(b'\x07' * 5)
    with pytest.raises(DataSetException, match=r'cut_001.tvips: found a rest of 5 bytes behind 3 frames of 37 bytes'):
        TVIPSDataSet(path=cut[0])._scan_file()
    os.truncate(cut[1], 3 * 37)
    os.truncate(cut[0], 256 + 4 * 37 - 1)
    with pytest.raises(DataSetException, match=r'cut_000.tvips: found a rest of 36 bytes behind 3 frames'):
        TVIPSDataSet(path=cut[1])._scan_file()
    # the checks of every record format
    path = filesets['t16']['path']
    with pytest.raises(DataSetException, match='sig_shape must be of size: 48'):
        TVIPSDataSet(path=path, sig_shape=(7, 7))._scan_file()
    assert TVIPSDataSet(path=path, sig_shape=(48,))._scan_file().sig_shape == (48,)
    for so in (12, -12):
        with pytest.raises(DataSetException, match=r'offset should be in \(-12, 12\), which is \(-image_count'):
            TVIPSDataSet(path=path, sync_offset=so)._scan_file()
    with pytest.raises(ValueError, match='I/O backends'):
        TVIPSDataSet(path=path, io_backend=object())
    with pytest.raises(RuntimeError, match='initialize'):
        TVIPSDataSet(path=path).header
    gone = TVIPSDataSet(path=cut[0])
    os.truncate(cut[0], 256 + 4 * 37)
    gone._scan_file()
    os.remove(cut[1])
    with pytest.raises(DataSetException, match='invalid dataset'):
        gone.check_valid()


def test_arguments_win_each_on_its_own(filesets):
    path = filesets['t16']['path']
    layout = TVIPSDataSet(path=path, sync_offset=0)._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (0, (2, 4))           # (a 0 that was passed is not "none")
    layout = TVIPSDataSet(path=path, nav_shape=(3, 3))._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (1, (3, 3))
    layout = TVIPSDataSet(path=path, nav_shape=(12,), sync_offset=-3)._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (-3, (12,))
    # version 1 and failed detection: offset 0, a line of all frames; the arguments still hold
    layout = TVIPSDataSet(path=filesets['t8v1']['path'], sync_offset=2)._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (2, (7,))
    layout = TVIPSDataSet(path=filesets['tnoscan']['path'], nav_shape=(5, 1))._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (0, (5, 1))


def test_the_flag_of_the_first_loop_is_never_cleared(tmp_path):
    """(0, 0), (3, 3), (0, 1): the reference takes the (0, 1) at frame 2 for the start although the frame before
    is no (0, 0) -- kept"""
    frames = recipes.make_frames('tline')
    scan = ((0, 0), (3, 3), (0, 1), (0, 2), (0, 0), (0, 1))
    path = synth.write_series(str(tmp_path), 'flag', frames, 2, 108, (6,), scan)[0]
    layout = TVIPSDataSet(path=path)._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (1, (1, 3))            # ((6 - 1) // 3, 3)


# --- the two deliberate differences from the reference -----------------------------------------------------------
def test_any_file_of_a_version_2_set_names_it(filesets):
    """the series header comes from the first file of the set (the reference reads the file it was given and raises
    "Unknown TVIPS header version" for all but `_000`)"""
    fs = filesets['t16']
    first = TVIPSDataSet(path=fs['paths'][0])
    want = first._scan_file()
    for path in fs['paths'][1:]:
        ds = TVIPSDataSet(path=path)
        assert ds._scan_file() == want and ds._records == first._records and ds.header == first.header
        got = TVIPSDataSet.detect_params(path)
        assert got == dict(TVIPSDataSet.detect_params(fs['path']),
                           parameters=dict(got['parameters'], path=path))
        assert got['parameters']['nav_shape'] == (2, 4) and got['parameters']['sync_offset'] == 1


def test_detection_reads_each_image_header_from_its_own_file(tmp_path):
    """4 + 4 frames of a 2 x 4 scan: the row ends in the second file (the reference looks for frame 4 in the first
    file and dies with IndexError)"""
    frames = recipes.make_frames('t16')[:8]
    scan = tuple((y, x) for y in range(2) for x in range(4))
    paths = synth.write_series(str(tmp_path), 'two', frames, 2, 112, (4, 4), scan, seed=5)
    for path in paths:
        layout = TVIPSDataSet(path=path)._scan_file()
        assert (layout.sync_offset, layout.nav_shape, layout.n_frames) == (0, (2, 4), 8)
    # and a start that lies in the second file
    scan = ((5, 5),) * 4 + ((0, 0), (0, 1), (1, 0), (1, 1))
    paths = synth.write_series(str(tmp_path), 'late', frames, 2, 112, (4, 4), scan, seed=6)
    layout = TVIPSDataSet(path=paths[0])._scan_file()
    assert (layout.sync_offset, layout.nav_shape) == (4, (2, 2))


# --- the public surface ------------------------------------------------------------------------------------------
def test_detect_params_like_the_reference(filesets, tmp_path):
    assert TVIPSDataSet.get_supported_extensions() == {'tvips'}
    for fileset, fs in filesets.items():
        got = TVIPSDataSet.detect_params(fs['path'])
        nav, so = recipes.DETECTED[fileset]
        sig = recipes.native_shape(fileset)
        assert got == {'parameters': {'path': fs['path'], 'nav_shape': nav, 'sig_shape': sig, 'sync_offset': so},
                       'info': {'image_count': recipes.n_frames(fileset), 'native_sig_shape': sig}}
        assert tuple(GOLDEN[fileset + '__detect_nav']) == nav and int(GOLDEN[fileset + '__detect_sync_offset']) == so
        assert tuple(GOLDEN[fileset + '__detect_sig']) == tuple(GOLDEN[fileset + '__detect_native_sig']) == sig
        assert int(GOLDEN[fileset + '__detect_image_count']) == recipes.n_frames(fileset)
    # failed detection: a square where the frames make one
    frames = np.concatenate([recipes.make_frames('t8v1'), recipes.make_frames('t8v1')[:2]])
    square = synth.write_series(str(tmp_path), 'sq', frames, 1, 12, (5, 4))[0]
    assert TVIPSDataSet.detect_params(square)['parameters']['nav_shape'] == (3, 3)
    assert TVIPSDataSet.detect_params(__file__) is False
    assert TVIPSDataSet.detect_params(str(tmp_path / 'x.bin')) is False


def test_load_is_available_under_both_spellings(filesets):
    # (fails without the feature: "dataset type 'tvips' is not available")
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    path = filesets['t16']['path']
    assert 'TVIPSDataSet' in dataset.__all__ and issubclass(TVIPSDataSet, RecordFileDataSet)
    assert TVIPSDataSet.DECODE_KERNEL == 'ltmi_records_gather' and 'TVIPS' in TVIPSDataSet.KIND
    for spelling in ('tvips', 'TVIPS'):
        ds = dataset.load(spelling, path=path)
        assert type(ds) is TVIPSDataSet and 'not initialized' in repr(ds) and ds.path == path
    assert "'tvips'" in str(pytest.raises(DataSetException, dataset.load, 'nothing_like_it').value)
    assert 'TVIPS' in dataset.load.__doc__ and "'auto'" in dataset.load.__doc__
    # the files are gathered on the GPU: an executor that drives none is told so, not handed host frames
    ctx = Context(executor=InlineJobExecutor())
    try:
        for spelling in ('tvips', 'auto'):
            with pytest.raises(DataSetException, match=r'decodes the files on the GPU \(ltmi_records_gather\)'):
                ctx.load(spelling, path=path)
    finally:
        ctx.close()


def test_registry_and_extensions():
    # this build's types in the reference's order of registration, its own 'stream' behind them
    assert list(dataset.filetypes) == ['raw', 'raw_csr', 'mib', 'blo', 'k2is', 'frms6', 'empad', 'seq', 'tvips',
                                       'npy', 'memory', 'stream']
    assert dataset.filetypes['tvips'] is TVIPSDataSet
    assert dataset.get_extensions() == {'toml', 'mib', 'hdr', 'blo', 'gtg', 'bin', 'frms6', 'xml', 'raw', 'seq',
                                        'tvips', 'npy'}
    for key in ('memory', 'raw', 'stream'):
        assert dataset.filetypes[key].detect_params('x.bin') is False
        assert dataset.filetypes[key].get_supported_extensions() == set()
    plain = list(dataset.filetypes)
    assert dataset.get_search_order('x.unknown') == plain and dataset.get_search_order(None) == plain
    assert dataset.get_search_order('/d/x_000.TVIPS')[:2] == ['tvips', 'raw']
    assert dataset.get_search_order('x.hdr')[:3] == ['mib', 'frms6', 'raw']         # (in their own order)
    assert dataset.get_search_order('x.npy')[0] == 'npy' and sorted(dataset.get_search_order('x.npy')) == sorted(plain)


def test_detect_and_auto_load_find_every_format(filesets, tmp_path):
    """one synthetic file of every format the suite writes: each is found as its own type, and `load('auto')` hands
    the caller's own arguments to that type"""
    import records_recipes
    import k2is_recipes
    import frms6_recipes
    d = str(tmp_path)
    seq = records_recipes.write_fileset('s8', d)['path']
    blo = records_recipes.write_fileset('b8', d)['path']
    empad = records_recipes.write_fileset('e_series', d)
    frms6 = frms6_recipes.write_fileset('c', d)['hdr']
    k2is_dir = tmp_path / 'k2'
    k2is_dir.mkdir()
    k2is = k2is_recipes.write_fileset('plain', str(k2is_dir))[0]
    npy = str(tmp_path / 'a.npy')
    np.save(npy, np.zeros((2, 3, 4, 5), dtype=np.uint16))
    tv = filesets['t16']
    found = {'seq': seq, 'blo': blo, 'empad': empad['path'], 'frms6': frms6, 'k2is': k2is, 'npy': npy,
             'tvips': tv['paths'][1]}
    for key, path in found.items():
        got = dataset.detect(path)
        assert got['type'] == key and got['parameters']['path'] == path, (key, got)
        assert got == dict(dataset.filetypes[key].detect_params(path), type=key)
        more = dict(nav_shape=(6,)) if key == 'seq' else {}         # (what SEQDataSet requires of its caller)
        assert type(dataset.load('auto', path, **more)) is dataset.filetypes[key]
        assert type(dataset.load('auto', path=path, **more)) is dataset.filetypes[key]
    assert dataset.detect(tv['path']) == {
        'parameters': {'path': tv['path'], 'nav_shape': (2, 4), 'sig_shape': (6, 8), 'sync_offset': 1},
        'info': {'image_count': 12, 'native_sig_shape': (6, 8)}, 'type': 'tvips'}
    # the caller's arguments go to the detected type; what detection found is not merged in
    ds = dataset.load('auto', tv['path'], nav_shape=(3, 2), sync_offset=4)
    assert (ds._nav_arg, ds._sync_offset_given) == ((3, 2), 4)
    ds = dataset.load('auto', path=seq, nav_shape=(3, 2))
    assert ds._nav_arg == (3, 2)
    with pytest.raises(TypeError, match="missing 1 required argument: 'nav_shape'"):
        dataset.load('auto', seq)                           # (detected (6,), but not passed on)
    # a file nothing knows, a .tvips file that is none, an EMPAD .raw alone; no path
    garbage = tmp_path / 'garbage.bin'
    garbage.write_bytes(bytes(range(256)) * 40)
    fake = tmp_path / 'fake_000.tvips'
    fake.write_bytes(bytes(range(256)) * 2)
    for path in (str(garbage), str(fake), empad['raw'], str(tmp_path / 'absent.seq')):
        assert dataset.detect(path) == {}
        with pytest.raises(DataSetException, match="could not determine DataSet type for file '%s'" % path):
            dataset.load('auto', path)
    for call in (lambda: dataset.load('auto'), lambda: dataset.load('auto', path=None),
                 lambda: dataset.load('auto', nav_shape=(2, 2))):
        with pytest.raises(DataSetException, match='please specify the `path` argument to allow auto detection'):
            call()


def test_context_loads_auto(tmp_path):
    """`Context.load('auto', ...)` on a type a CPU executor can hold"""
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    from libertem_amd.io.dataset import NPYDataSet
    data = np.arange(2 * 3 * 4 * 5, dtype=np.uint16).reshape(2, 3, 4, 5)
    path = str(tmp_path / 'a.npy')
    np.save(path, data)
    ctx = Context(executor=InlineJobExecutor())
    try:
        for ds in (ctx.load('auto', path), ctx.load('auto', path=path)):
            assert type(ds) is NPYDataSet and tuple(ds.shape) == (2, 3, 4, 5)
        with pytest.raises(DataSetException, match='could not determine DataSet type'):
            ctx.load('auto', path=str(tmp_path / 'absent.bin'))
        with pytest.raises(DataSetException, match='please specify the `path` argument'):
            ctx.load('auto')
    finally:
        ctx.close()


def test_compat_alias():
    import importlib
    import libertem_amd.compat as compat
    had = 'libertem' in sys.modules
    compat.install()
    try:
        assert importlib.import_module('libertem.io.dataset.tvips').TVIPSDataSet is TVIPSDataSet
        assert importlib.import_module('libertem.io.dataset').detect is dataset.detect
    finally:
        if not had:
            compat.uninstall()
