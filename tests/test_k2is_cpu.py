"""
K2ISDataSet without a GPU: the NumPy decoder of tests/k2is_synth.py (the yardstick of the GPU tests) against
the frames the REAL reference's K2ISDataSet decoded from the same synthetic files (tests/golden/k2is.npz), the
host-side synchronisation of the sectors against the reference's, and the errors.

Where the golden vectors stop: a scan position whose frame lies behind the last whole frame of the files
(position p with p + sync_offset >= frames with the shutter flag set; the last position of `lead_unsync`) is
read by the reference past the end of the synchronised blocks -- its result there is whatever those bytes
are; this package gives a zero frame.  Such positions are left out of the comparison (`in_files`).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
sys.path.insert(0, HERE)

import k2is_recipes as recipes  # noqa: E402
import k2is_synth as synth  # noqa: E402

from libertem_amd.io.dataset.base import DataSetException  # noqa: E402
from libertem_amd.io.dataset.k2is import K2ISDataSet  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'k2is.npz'))


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    """{name: (path of the first sector file, frames)}, written once"""
    d = tmp_path_factory.mktemp('k2is')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


def expected_frames(case, frames):
    """(frames at their scan positions by the yardstick's rules, which positions hold a frame of the files or
    lie before the first one)"""
    lead = recipes.FILESETS[case['fileset']]['lead']
    shutter = frames[lead:]
    so = lead if case['sync_offset'] is None else case['sync_offset']
    n_nav = len(shutter)
    in_files = np.arange(n_nav) + so < len(shutter)
    return synth.positioned(shutter, n_nav, so), in_files, so


def sha(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_numpy_decoder_is_the_reference_decoder(filesets, case):
    path, frames = filesets[case['fileset']]
    files = [path.replace('_1.bin', f'_{s + 1}.bin') for s in range(8)]
    decoded, shutter, _ = synth.decode_files(files)
    lead = recipes.FILESETS[case['fileset']]['lead']
    assert np.array_equal(decoded, frames)                  # (and the writer round-trips)
    assert np.array_equal(shutter, np.arange(len(frames)) >= lead)
    want, in_files, so = expected_frames(case, decoded)
    name = case['name']
    assert int(GOLDEN[name + '__sync_offset']) == so
    assert in_files.sum() >= 2
    for p in np.flatnonzero(in_files):
        assert np.array_equal(sha(want[p]), GOLDEN[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(want[p][recipes.CROP], GOLDEN[name + '__crops'][p]), (name, p)
    # the crop does cover a block-row edge and a sector edge
    rows, cols = recipes.CROP
    assert rows.start < 930 < rows.stop and cols.start < 256 < cols.stop


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_host_side_scan_like_the_reference(filesets, case):
    path, frames = filesets[case['fileset']]
    name = case['name']
    scan = K2ISDataSet(path=path, sync_offset=case['sync_offset'])._scan_files()
    assert scan['image_count'] == int(GOLDEN[name + '__image_count'])
    assert scan['sync_offset'] == int(GOLDEN[name + '__sync_offset'])
    assert tuple(scan['nav_shape']) + (1860, 2048) == tuple(GOLDEN[name + '__shape'])
    assert scan['first_offsets'] == GOLDEN[name + '__first_offsets'].tolist()
    assert scan['last_offsets'] == GOLDEN[name + '__last_offsets'].tolist()
    lead = recipes.FILESETS[case['fileset']]['lead']
    assert scan['native_sync_offset'] == lead and scan['num_frames_w_shutter'] == len(frames) - lead
    # any of the 8 files names the set
    other = K2ISDataSet(path=path.replace('_1.bin', '_5.bin'), sync_offset=case['sync_offset'])._scan_files()
    assert other['first_offsets'] == scan['first_offsets'] and other['files'] == scan['files']


def test_unsynchronised_start_and_truncated_end(filesets):
    """the offsets by the writer's own bookkeeping: extra leading blocks and the frame before the shutter opens
    are skipped, a truncated last frame is left out"""
    fs = recipes.FILESETS['lead']
    scan = K2ISDataSet(path=filesets['lead'][0])._scan_files()
    assert scan['first_offsets'] == [(e + 32 * fs['lead']) * synth.BLOCK_SIZE for e in fs['extra']]
    assert scan['last_offsets'] == [(e + 32 * fs['n'] - 1) * synth.BLOCK_SIZE for e in fs['extra']]
    fs = recipes.FILESETS['plain']
    scan = K2ISDataSet(path=filesets['plain'][0])._scan_files()
    assert scan['first_offsets'] == [0] * 8
    assert scan['last_offsets'] == [(32 * fs['n'] - 1) * synth.BLOCK_SIZE] * 8
    assert scan['image_count'] == fs['n'] and scan['native_sync_offset'] == 0


def _small_set(dirpath, name='s', n=1):
    """headers only matter here: zero frames"""
    return synth.write_k2is(str(dirpath), np.zeros((n,) + synth.FRAME_SHAPE, dtype=np.uint16), name=name)


def test_errors(tmp_path, filesets):
    paths = _small_set(tmp_path)
    with pytest.raises(ValueError, match='I/O backends'):
        K2ISDataSet(path=paths[0], io_backend=object())
    with pytest.raises(DataSetException, match=r'sync_offset should be in \(-1, 1\), which is \(-image_count'):
        K2ISDataSet(path=paths[0], sync_offset=1)._scan_files()
    with pytest.raises(DataSetException, match=r'sync_offset should be in \(-4, 4\)'):
        K2ISDataSet(path=filesets['plain'][0], sync_offset=-4)._scan_files()
    with pytest.raises(DataSetException, match='unknown extension'):
        K2ISDataSet(path=str(tmp_path / 's.raw'))._scan_files()
    # a .gtg beside the data: its scan size cannot be read here
    (tmp_path / 's_.gtg').write_bytes(b'\0' * 16)
    with pytest.raises(DataSetException, match='gtg.*nav_shape'):
        K2ISDataSet(path=paths[0])._scan_files()
    assert K2ISDataSet(path=paths[0], nav_shape=(1,))._scan_files()['nav_shape'] == (1,)
    assert K2ISDataSet.detect_params(paths[0]) is False
    os.remove(tmp_path / 's_.gtg')
    # a bad sync word in a first block
    with open(paths[3], 'r+b') as f:
        f.write(b'\xff\xff\x00\x56')
    with pytest.raises(DataSetException, match='first block of .*s_4.bin is not valid'):
        K2ISDataSet(path=paths[0])._scan_files()
    # 7 files
    os.remove(paths[3])
    with pytest.raises(DataSetException, match='expected 8 files at .*, found 7'):
        K2ISDataSet(path=paths[0])._scan_files()
    assert K2ISDataSet.detect_params(paths[0]) is False


def test_load_k2is_is_available(filesets):
    # (fails without the feature: "dataset type 'k2is' is not available")
    from libertem_amd.api import Context
    from libertem_amd.executor.inline import InlineJobExecutor
    from libertem_amd.io import dataset
    assert 'K2ISDataSet' in dataset.__all__
    for key in ('k2is', 'K2IS'):
        ds = dataset.load(key, path=filesets['plain'][0])
        assert isinstance(ds, K2ISDataSet) and 'not initialized' in repr(ds)
    with pytest.raises(DataSetException, match="'k2is'.*in scope"):
        dataset.load('nothing_like_it')
    # the files are decoded on the GPU: an executor that drives none is told so, not handed host frames
    ctx = Context(executor=InlineJobExecutor())
    try:
        with pytest.raises(DataSetException, match='decodes the files on the GPU'):
            ctx.load('k2is', path=filesets['plain'][0])
    finally:
        ctx.close()


def test_interface(filesets):
    assert K2ISDataSet.get_supported_extensions() == {'bin', 'gtg'}
    d = K2ISDataSet.detect_params(filesets['lead'][0])
    assert d['parameters'] == {'path': filesets['lead'][0], 'nav_shape': (3,), 'sig_shape': (1860, 2048),
                               'sync_offset': 1}
    assert d['info'] == {'image_count': 4, 'native_sig_shape': (1860, 2048)}
    assert K2ISDataSet.detect_params(filesets['plain'][0])['parameters']['nav_shape'] == (2, 2)
    assert K2ISDataSet.detect_params(__file__) is False


def test_compat_alias():
    import importlib
    import libertem_amd.compat as compat
    had = 'libertem' in sys.modules
    compat.install()
    try:
        mod = importlib.import_module('libertem.io.dataset.k2is')
        assert mod.K2ISDataSet is K2ISDataSet
    finally:
        if not had:
            compat.uninstall()
