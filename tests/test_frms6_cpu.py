"""
FRMS6DataSet without a GPU: the NumPy decoder of tests/frms6_synth.py (the yardstick of the GPU tests) against
the frames the REAL reference's FRMS6DataSet read from the same synthetic files (tests/golden/frms6.npz), the
host-side helpers (file discovery, file and .hdr headers, frame counts of old files, both gain map readers)
against what the reference made of them, the errors, and `Context.run_udf` picking up the corrections a dataset
brings along.
"""
import os
import sys
import hashlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)

import frms6_recipes as recipes  # noqa: E402
import frms6_synth as synth  # noqa: E402

from libertem_amd.io.dataset.base import DataSetException  # noqa: E402
from libertem_amd.io.dataset import frms6  # noqa: E402
from libertem_amd.io.dataset.frms6 import FRMS6DataSet  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'frms6.npz'))


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    """{name: dict(hdr, mat, csv, gain, dark, signal)}, written once"""
    d = tmp_path_factory.mktemp('frms6')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def expected_frames(case, signal):
    """the raw frames at the scan positions a case picks (all of them, or its ROI): frame g at g - sync_offset,
    zero frames where the files hold none"""
    nav = recipes.FILESETS[case['fileset']]['nav']
    at_positions = synth.positioned(signal, int(np.prod(nav)), case['sync_offset'])
    return at_positions if case['roi'] is None else at_positions[case['roi'].reshape(-1)]


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_numpy_decoder_is_the_reference_decoder(filesets, case):
    fs = filesets[case['fileset']]
    binning = recipes.FILESETS[case['fileset']]['binning']
    dark, signal = synth.decode_set(fs['hdr'], binning)
    assert np.array_equal(dark, fs['dark']) and np.array_equal(signal, fs['signal'])    # (the writer round-trips)
    name = case['name']
    want = expected_frames(case, signal)
    assert want.dtype == np.uint16 and want.max() <= 4095
    assert len(want) == len(GOLDEN[name + '__sha_frames'])
    for p, frame in enumerate(want):
        assert np.array_equal(sha(frame), GOLDEN[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(frame[recipes.crop(case['fileset'])], GOLDEN[name + '__crops'][p]), (name, p)
    assert tuple(GOLDEN[name + '__shape'][-2:]) == recipes.sig_shape(case['fileset']) == want.shape[1:]
    # the dark frame: the mean of the unfolded dark frames, bit for bit
    if case['offset']:
        assert len(dark) <= 64
        assert np.array_equal(synth.dark_frame(dark), GOLDEN[name + '__dark'])
        assert GOLDEN[name + '__dark'].dtype == np.float32 and str(GOLDEN[name + '__dtype']) == '<f4'
    else:
        assert name + '__dark' not in GOLDEN.files and str(GOLDEN[name + '__dtype']) == '<u2'
    assert str(GOLDEN[name + '__raw_dtype']) == '<u2'


def test_unfold_by_hand():
    """2 x 6 raw, binning 2: rows 0, 1 straight (each twice), then rows 1, 0 of the right half reversed"""
    raw = np.arange(12, dtype=np.uint16).reshape(1, 2, 6)
    want = [[0, 1, 2]] * 2 + [[6, 7, 8]] * 2 + [[11, 10, 9]] * 2 + [[5, 4, 3]] * 2
    assert np.array_equal(synth.unfold(raw, 2)[0], want)


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_host_side_scan_like_the_reference(filesets, case):
    fs, rec = filesets[case['fileset']], recipes.FILESETS[case['fileset']]
    name = case['name']
    scan = FRMS6DataSet(**recipes.load_kwargs(case, fs))._scan_files()
    assert scan['image_count'] == int(GOLDEN[name + '__image_count']) == sum(rec['files'])
    assert tuple(scan['nav_shape']) + tuple(scan['sig_shape']) == tuple(GOLDEN[name + '__shape'])
    assert scan['sig_shape'] == scan['native_sig_shape'] == recipes.sig_shape(case['fileset'])
    assert (scan['height'], scan['width'], scan['binning']) == (rec['height'], rec['width'], rec['binning'])
    assert scan['counts'] == list(rec['files']) and scan['starts'].tolist() == np.cumsum((0,) + rec['files']).tolist()
    assert scan['sync_offset'] == case['sync_offset']
    assert [os.path.basename(h['path']) for h in scan['headers']] == \
        [f"{case['fileset']}_{i:03d}.frms6" for i in range(len(rec['files']) + 1)]


def test_file_discovery(filesets):
    hdr = filesets['a']['hdr']
    stem = hdr[:-len('.hdr')]
    files = [f"{stem}_{i:03d}.frms6" for i in range(3)]
    assert frms6.get_filenames(hdr) == files
    for f in files:
        assert frms6.get_filenames(f) == files                      # any .frms6 names the set
        assert frms6._get_base_filename(f) == stem
    assert frms6._get_base_filename(hdr) == stem
    assert frms6.get_filenames(files[1], disable_glob=True) == [files[1]]
    assert frms6._pattern(hdr).endswith('a_*.frms6') and frms6._pattern(files[2]).endswith('a_*.frms6')
    # ... and loads like the .hdr
    a, b = (FRMS6DataSet(path=p)._scan_files() for p in (hdr, files[2]))
    assert [h['path'] for h in a['headers']] == [h['path'] for h in b['headers']] and a['hdr'] == b['hdr']


def test_headers(filesets, tmp_path):
    rec = recipes.FILESETS['b']
    hdr = frms6._read_dataset_hdr(filesets['b']['hdr'])
    assert hdr['signalframes'] == 6 and hdr['darkframes'] == rec['dark'] and hdr['stemimagesize'] == (6,)
    assert hdr['readoutmode'] == {'bin': 2, 'win_i': 12, 'win_j': 12}
    assert hdr['dwelltimemicroseconds'] == 100 and hdr['gain'] == 1 and hdr['comment'] == 'synthetic'
    assert frms6._read_dataset_hdr(filesets['a']['hdr'])['stemimagesize'] == (2, 4)
    # the fields of a file header, whatever the bytes around them are
    raw = synth.random_raw(3, 5, 14, 1)
    path = synth.write_frms6(str(tmp_path / 'x_001.frms6'), raw, fill=0xFF)
    h = frms6._read_file_header(path)
    assert h == dict(header_size=1024, frame_header_size=64, version=6, width=14, height=5, num_frames=3,
                     filesize=1024 + 3 * (64 + 5 * 14 * 2), path=path)
    assert frms6._header_valid(h) and frms6._num_frames(h) == 3
    for field, value in (('header_size', 1000), ('frame_header_size', 32), ('version', 5)):
        assert not frms6._header_valid(dict(h, **{field: value}))
    assert np.array_equal(synth.read_file(path), raw)
    assert synth.frame_record_offset(2, 5, 14) == 1024 + 3 * 64 + 2 * 140


def test_frame_count_of_old_files(filesets, tmp_path):
    # set F: num_frames = 0 in every header
    scan = FRMS6DataSet(path=filesets['f']['hdr'])._scan_files()
    assert all(h['num_frames'] == 0 for h in scan['headers'])
    assert scan['counts'] == [5, 3] and frms6._num_frames(scan['headers'][0]) == 3
    # a file that ends inside a frame
    raw = synth.random_raw(2, 4, 16, 2)
    data = synth.file_bytes(raw, num_frames_field=0)
    path = str(tmp_path / 'cut_001.frms6')
    data[:-10].tofile(path)
    with pytest.raises(DataSetException, match='could not determine number of frames'):
        frms6._num_frames(frms6._read_file_header(path))
    # a header that holds the count is believed
    synth.file_bytes(raw, num_frames_field=2)[:-10].tofile(path)
    assert frms6._num_frames(frms6._read_file_header(path)) == 2


@pytest.mark.parametrize('case', [c for c in recipes.CASES if c['gain']], ids=lambda c: c['name'])
def test_gain_readers(filesets, case):
    fs = filesets[case['fileset']]
    got = frms6._read_gain_map(fs[case['gain']])
    assert got.dtype == np.float64 and got.shape == recipes.sig_shape(case['fileset'])
    assert np.array_equal(got, GOLDEN[case['name'] + '__gain'])      # what the reference read from the file
    assert np.array_equal(got, fs['gain']) and got.min() >= 0.5 and got.max() <= 2
    assert frms6._read_gain_map(None) is None
    if case['gain'] == 'csv':
        with open(fs['csv']) as f:
            line = f.readline()
        assert line.endswith(';\n') and line.count(';') == got.shape[0]      # transposed, with an empty cell


def test_errors(filesets, tmp_path):
    hdr = filesets['a']['hdr']
    with pytest.raises(ValueError, match='I/O backends'):
        FRMS6DataSet(path=hdr, io_backend=object())
    with pytest.warns(DeprecationWarning, match='dest_dtype'):
        FRMS6DataSet(path=hdr, dest_dtype=np.float32)
    with pytest.raises(DataSetException, match='unknown extension: .raw'):
        FRMS6DataSet(path=str(tmp_path / 'x.raw'))._scan_files()
    with pytest.raises(DataSetException, match='unknown extension'):
        frms6._get_base_filename(str(tmp_path / 'x.bin'))
    # a .frms6 without its .hdr
    lone = synth.write_frms6(str(tmp_path / 'lone_001.frms6'), synth.random_raw(1, 2, 4, 3))
    with pytest.raises(DataSetException, match='Could not find .hdr file .*lone.hdr'):
        FRMS6DataSet(path=lone)._scan_files()
    (tmp_path / 'lone.hdr').write_text("[other]\nx = 1\n")
    with pytest.raises(DataSetException, match=r"measurementInfo missing from .hdr file .*, have: \['other'\]"):
        FRMS6DataSet(path=lone)._scan_files()
    (tmp_path / 'lone.hdr').write_text(
        "[measurementInfo]\nsignalframes = 1\ndarkframes = 0\nstemimagesize = 1x1\nreadoutmode = \"binning 2\"\n")
    with pytest.raises(DataSetException, match='could not parse readout mode'):
        FRMS6DataSet(path=lone)._scan_files()
    # one file only: nothing but dark frames
    synth.write_hdr(str(tmp_path / 'lone.hdr'), 1, 0, (1,), 1, (4, 2))
    with pytest.raises(DataSetException, match='found 1 files'):
        FRMS6DataSet(path=lone)._scan_files()
    with pytest.raises(DataSetException, match='sig_shape must be of size: 64'):
        FRMS6DataSet(path=hdr, sig_shape=(8, 9))._scan_files()
    assert FRMS6DataSet(path=hdr, sig_shape=(4, 16))._scan_files()['sig_shape'] == (4, 16)
    for so in (8, -8):
        with pytest.raises(DataSetException, match=r'offset should be in \(-8, 8\), which is \(-image_count'):
            FRMS6DataSet(path=hdr, sync_offset=so)._scan_files()
    # an old file cut short: the count cannot be told
    d = tmp_path / 'cut'
    d.mkdir()
    dark, signal = recipes.make_raw('f')
    cut = synth.write_set(str(d), 'cut', dark, signal, (2, 4), 1, num_frames_field=0)
    with open(str(d / 'cut_002.frms6'), 'r+b') as f:
        f.truncate(os.path.getsize(str(d / 'cut_002.frms6')) - 2)
    with pytest.raises(DataSetException, match='could not determine number of frames'):
        FRMS6DataSet(path=cut)._scan_files()
    # a bad version byte: check_valid says which file
    with open(str(d / 'cut_001.frms6'), 'r+b') as f:
        f.seek(7)
        f.write(b'\x05')
    ds = FRMS6DataSet(path=str(d / 'cut_000.frms6'))
    with pytest.raises(DataSetException, match='error while checking validity of .*cut_001.frms6'):
        ds._headers = [frms6._read_file_header(p) for p in frms6.get_filenames(cut)]
        ds.check_valid()
    assert FRMS6DataSet(path=hdr).check_valid() is True


def test_load_frms6_is_available(filesets):
    # (fails without the feature: "dataset type 'frms6' is not available")
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    from libertem_amd.io import dataset
    assert 'FRMS6DataSet' in dataset.__all__
    for key in ('frms6', 'FRMS6'):
        ds = dataset.load(key, path=filesets['a']['hdr'])
        assert isinstance(ds, FRMS6DataSet) and 'not initialized' in repr(ds) and 'a_*.frms6' in repr(ds)
    with pytest.raises(DataSetException, match="'frms6'.*in scope"):
        dataset.load('nothing_like_it')
    assert 'FRMS6' in dataset.load.__doc__
    # the files are decoded on the GPU: an executor that drives none is told so, not handed host frames
    ctx = Context(executor=InlineJobExecutor())
    try:
        with pytest.raises(DataSetException, match='decodes the files on the GPU'):
            ctx.load('frms6', path=filesets['a']['hdr'])
    finally:
        ctx.close()


def test_interface(filesets):
    assert FRMS6DataSet.get_supported_extensions() == {'frms6', 'hdr'}
    hdr = filesets['b']['hdr']
    for path in (hdr, hdr[:-4] + '_001.frms6'):
        d = FRMS6DataSet.detect_params(path)
        assert d['parameters'] == {'path': path, 'nav_shape': (6,), 'sig_shape': (12, 12)}
        assert d['info'] == {'image_count': 6, 'native_sig_shape': (12, 12)}
    assert FRMS6DataSet.detect_params(filesets['a']['hdr'])['parameters']['nav_shape'] == (2, 4)
    assert FRMS6DataSet.detect_params(__file__) is False
    assert FRMS6DataSet.detect_params(filesets['b']['mat']) is False
    ds = FRMS6DataSet(path=hdr)
    assert ds.path == hdr and ds.storage_dtype == np.uint16


def _stub(data, corr):
    """a MemoryDataSet that brings a CorrectionSet along, like FRMS6DataSet does"""
    from libertem_amd.io.dataset.memory import MemoryDataSet

    class Stub(MemoryDataSet):
        def get_correction_data(self):
            return corr
    return Stub(data=data, sig_dims=2, num_partitions=2)


def test_context_applies_the_datasets_own_corrections():
    """`corrections=None` picks up `dataset.get_correction_data()` on every entry point; an explicit set wins,
    an empty one included (reference api.py: run_udf, run_udf_iter, map)"""
    import asyncio
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf.sumsigudf import SumSigUDF
    rng = np.random.default_rng(5)
    data = rng.integers(0, 4096, (6, 4, 4)).astype(np.uint16)
    dark = rng.integers(0, 256, (4, 4)).astype(np.float32)
    other = np.full((4, 4), 2.0, dtype=np.float32)
    plain = data.reshape(6, -1).sum(axis=1, dtype=np.float64)
    own, explicit = plain - dark.sum(dtype=np.float64), plain - 32.0
    ctx = Context(executor=InlineJobExecutor())
    try:
        ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=2)
        assert ds.get_correction_data() is None
        assert np.allclose(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data, plain)
        ds = _stub(data, CorrectionSet(dark=dark)).initialize(ctx.executor)
        assert np.allclose(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data, own)
        assert np.allclose(ctx.run_udf(dataset=ds, udf=SumSigUDF(), corrections=CorrectionSet(dark=other))
                           ['intensity'].data, explicit)
        assert np.allclose(ctx.run_udf(dataset=ds, udf=SumSigUDF(), corrections=CorrectionSet())
                           ['intensity'].data, plain)
        # run_udf_iter, map, and the async twins
        last = None
        for last in ctx.run_udf_iter(dataset=ds, udf=SumSigUDF()):
            pass
        assert np.allclose(last.buffers[0]['intensity'].data, own)
        for last in ctx.run_udf_iter(dataset=ds, udf=SumSigUDF(), corrections=CorrectionSet(dark=other)):
            pass
        assert np.allclose(last.buffers[0]['intensity'].data, explicit)
        assert np.allclose(ctx.map(dataset=ds, f=np.sum).data, own)
        assert np.allclose(ctx.map(dataset=ds, f=np.sum, corrections=CorrectionSet(dark=other)).data, explicit)

        async def twins():
            res = await ctx.run_udf(dataset=ds, udf=SumSigUDF(), sync=False)
            parts = [p async for p in ctx.run_udf_iter(dataset=ds, udf=SumSigUDF(), sync=False)]
            return res['intensity'].data, parts[-1].buffers[0]['intensity'].data
        for got in asyncio.run(twins()):
            assert np.allclose(got, own)
        # a run nested in an iteration (the sibling context resolves the dataset's corrections itself)
        for _ in ctx.run_udf_iter(dataset=ds, udf=SumSigUDF()):
            assert np.allclose(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data, own)
            break
        # an analysis through ctx.run
        res = ctx.run(ctx.create_sum_analysis(dataset=ds))
        assert np.allclose(res['intensity'].raw_data, data.sum(axis=0, dtype=np.float64) - 6 * dark)
    finally:
        ctx.close()


def test_compat_alias():
    import importlib
    import libertem_amd.compat as compat
    had = 'libertem' in sys.modules
    compat.install()
    try:
        mod = importlib.import_module('libertem.io.dataset.frms6')
        assert mod.FRMS6DataSet is FRMS6DataSet
    finally:
        if not had:
            compat.uninstall()


def test_readoutmode_and_set_names(tmp_path):
    """`readoutmode = "bin: B, windowing: I x J"`, with or without the blanks; STEM.hdr + STEM_NNN.frms6"""
    parse = frms6._parse_readoutmode
    assert parse('"bin: 2, windowing: 132 x 264"') == {'bin': 2, 'win_i': 132, 'win_j': 264}
    assert parse('"bin:1,windowing:4x8 "') == {'bin': 1, 'win_i': 4, 'win_j': 8}
    for bad in ('', '"', 'bin: 1, windowing: 4 x 8', '"bin: 1"', '"bin: 1, windowing: 4"', '"bin: a, windowing: 4 x 8"',
                '"bin: 1, window: 4 x 8"', '"bins: 1, windowing: 4 x 8"', '"bin: -1, windowing: 4 x 8"',
                '"bin: 1, windowing: 4 x 8 x 2"', '"bin: 1, windowing: 4 x 8, more: 1"', '"bin: 1.5, windowing: 4 x 8"'):
        with pytest.raises(DataSetException, match='could not parse readout mode'):
            parse(bad)
    base, pattern = frms6._get_base_filename, frms6._pattern
    assert base('/d/scan_2_017.frms6') == base('/d/scan_2.hdr') == '/d/scan_2'
    assert base('/d/scan_x.frms6') == '/d/scan_x' and base('/d/scan017.frms6') == '/d/scan017'
    assert pattern('/d/scan_2_017.frms6') == pattern('/d/scan_2.hdr') == '/d/scan_2_*.frms6'
    assert pattern('/d/sc[1]_000.frms6') == '/d/sc[[]1]_*.frms6'            # (a literal bracket, not a glob class)
    # a set whose stem ends in digits is not mixed up with its neighbour's files
    for name in ('s1_000.frms6', 's1_001.frms6', 's11_000.frms6', 's1.hdr'):
        (tmp_path / name).write_bytes(b'')
    assert [os.path.basename(f) for f in frms6.get_filenames(str(tmp_path / 's1_001.frms6'))] == \
        ['s1_000.frms6', 's1_001.frms6']
