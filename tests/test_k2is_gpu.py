"""
K2ISDataSet on the GPU (-m gpu): `ctx.load('k2is', ...)` on the synthetic 8-file sets of
tests/golden/k2is_recipes.py against the NumPy decoder of tests/k2is_synth.py and against what the REAL
reference's K2ISDataSet gave for the same files (tests/golden/k2is.npz): decoded frames bit-equal, SumSigUDF
and ApplyMasksUDF with the tolerances of tests/test_mib_gpu.py.  Then sync offsets, a reshaped scan, streamed
mode, shards and a region of interest.

A scan position whose frame lies behind the last whole frame of the files is a zero frame here; the reference
reads past the end of the synchronised blocks there, so the golden vectors are compared on the other positions
only (tests/test_k2is_cpu.py, `expected_frames`).
"""
import os
import hashlib

import numpy as np
import pytest

import k2is_recipes as recipes
import k2is_synth as synth
from test_k2is_cpu import expected_frames

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG = synth.FRAME_SHAPE


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    d = tmp_path_factory.mktemp('k2is')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


@pytest.fixture(scope='module')
def masks():
    return recipes.make_masks()


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def mask_udf(masks):
    from libertem_amd.udf.masks import ApplyMasksUDF
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_dataset_vs_reference(ctx, filesets, masks, golden_dir, case):
    from libertem_amd.udf.sumsigudf import SumSigUDF
    from libertem_amd.udf.raw import PickUDF
    g = np.load(os.path.join(golden_dir, 'k2is.npz'))
    name = case['name']
    path, frames = filesets[case['fileset']]
    want, in_files, so = expected_frames(case, frames)
    ds = ctx.load('k2is', path=path, sync_offset=case['sync_offset'])
    assert tuple(ds.shape) == tuple(g[name + '__shape']) and ds.dtype == np.uint16
    assert ds.storage_dtype == np.uint16 and ds.meta.raw_dtype == np.uint16
    assert ds.meta.image_count == int(g[name + '__image_count'])
    assert ds.meta.sync_offset == int(g[name + '__sync_offset']) == so
    assert ds.is_device_resident and not ds.is_streamed
    n_nav = len(want)
    n_src = int(np.sum((np.arange(n_nav) + so >= 0) & in_files))
    assert ds.decode_bytes == n_src * 8 * 32 * synth.BLOCK_SIZE and ds.decode_seconds > 0
    # blank positions are zero frames and not valid; with none, every frame is valid
    held = np.flatnonzero((np.arange(n_nav) + so >= 0) & in_files)
    assert ds._valid_frames == (None if len(held) == n_nav else (held[0], held[-1] + 1))
    picked = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=np.ones(n_nav, dtype=bool))['intensity'].data
    picked = np.asarray(picked).reshape((n_nav,) + SIG)
    assert picked.dtype == np.uint16
    assert np.array_equal(picked, want)
    assert np.array_equal(ds.data.cpu().reshape(want.shape), want)
    for p in np.flatnonzero(in_files):
        assert np.array_equal(sha(picked[p]), g[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(picked[p][recipes.CROP], g[name + '__crops'][p])
    sums = ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data
    ref_s = g[name + '__sumsig']
    assert sums.dtype == ref_s.dtype and np.allclose(sums[in_files], ref_s[in_files], rtol=1e-6)
    assert np.all(sums[~in_files] == 0)
    res = ctx.run_udf(dataset=ds, udf=mask_udf(masks))['intensity'].data
    ref_m = g[name + '__masks']
    assert res.dtype == ref_m.dtype, (res.dtype, ref_m.dtype)
    tol = 1e-5 if ref_m.dtype == np.float32 else 1e-12
    assert np.allclose(res[in_files], ref_m[in_files], rtol=tol, atol=tol * np.abs(ref_m[in_files]).max())
    assert np.all(res[~in_files] == 0)
    diag = {x['name']: x['value'] for x in ds.get_diagnostics()}
    assert diag['first block offsets for all sectors'] == ', '.join(str(o) for o in g[name + '__first_offsets'])
    assert diag['last block offsets for all sectors'] == ', '.join(str(o) for o in g[name + '__last_offsets'])
    assert diag['number of frames before sync (from first sector)'] == str(int(g[name + '__image_count']))
    assert ds.get_cache_key()['sync_offset'] == so and 'nav_shape=' in repr(ds)


def test_reshaped_scan_roi_and_shards(ctx, filesets):
    from libertem_amd.udf.raw import PickUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    path, frames = filesets['plain']
    ds = ctx.load('k2is', path=path, nav_shape=(2, 2))
    assert tuple(ds.shape) == (2, 2) + SIG and ds._valid_frames is None
    assert np.array_equal(ds.data.cpu().reshape(frames.shape), frames)
    # 2 of 4 frames
    roi = np.array([[False, True], [True, False]])
    picked = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=roi)['intensity'].data
    assert np.array_equal(np.asarray(picked).reshape((2,) + SIG), frames[1:3])
    sums = ctx.run_udf(dataset=ds, udf=SumSigUDF(), roi=roi)['intensity'].raw_data
    assert np.allclose(sums, frames[1:3].reshape(2, -1).sum(axis=1, dtype=np.int64), rtol=1e-6)
    # two ranks: each decodes its block of the first nav axis, together the unsharded frames
    halves = []
    for rank in (0, 1):
        part = ctx.load('k2is', path=path, nav_shape=(2, 2), shard=(rank, 2))
        assert tuple(part.shape) == (2, 2) + SIG and part.shard == (rank, 2)
        assert part.decode_bytes == 2 * 8 * 32 * synth.BLOCK_SIZE
        halves.append(part.data.cpu().reshape((2,) + SIG))
    assert np.array_equal(np.concatenate(halves), frames)
    # more scan positions than frames, and a sig_shape of the same size
    ds = ctx.load('k2is', path=path, nav_shape=(5,), sig_shape=(2048, 1860))
    assert tuple(ds.shape) == (5, 2048, 1860) and ds._valid_frames == (0, 4)
    got = ds.data.cpu().reshape((5,) + SIG)
    assert np.array_equal(got[:4], frames) and not got[4].any()
    from libertem_amd.io.dataset.base import DataSetException
    with pytest.raises(DataSetException, match='sig_shape must be of size'):
        ctx.load('k2is', path=path, sig_shape=(2048, 1861))


@pytest.mark.parametrize('sync_offset', (1, -2))
def test_streamed_like_resident(ctx, filesets, masks, monkeypatch, sync_offset):
    """decoded frames that may not stay in HBM: every partition decodes its own from the files"""
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.io.dataset.k2is import K2ISDataSet
    from libertem_amd.udf.sumsigudf import SumSigUDF
    path, frames = filesets['plain']
    resident = ctx.load('k2is', path=path, sync_offset=sync_offset)
    monkeypatch.setattr(K2ISDataSet, 'MAX_RESIDENT_BYTES', SIG[0] * SIG[1] * 2)
    ds = ctx.load('k2is', path=path, sync_offset=sync_offset)
    monkeypatch.setattr(K2ISDataSet, 'MAX_RESIDENT_BYTES', None)
    assert ds.is_streamed and not resident.is_streamed and not ds.stable_device_tiles
    assert tuple(ds.shape) == tuple(resident.shape) and ds._valid_frames == resident._valid_frames
    assert ds.get_num_partitions() == 4 and ds.decode_bytes == 0
    with pytest.raises(DataSetException, match='streamed'):
        ds.data
    want = synth.positioned(frames, 4, sync_offset)
    want_sum = ctx.run_udf(dataset=resident, udf=SumSigUDF())['intensity'].data
    # (SumSigUDF accumulates in float32: the tolerance of tests/test_mib_gpu.py for it)
    assert np.allclose(want_sum, want.reshape(4, -1).sum(axis=1, dtype=np.int64), rtol=1e-6)
    want_masks = ctx.run_udf(dataset=resident, udf=mask_udf(masks))['intensity'].data
    assert np.array_equal(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data, want_sum)
    assert np.array_equal(ctx.run_udf(dataset=ds, udf=mask_udf(masks))['intensity'].data, want_masks)
    assert ds.decode_bytes > 0
    for p in ds.get_partitions():
        arr, row0 = ds.device_frames(p._local0, p._num_frames)
        assert np.array_equal(arr.rows(row0, row0 + p._num_frames).cpu().reshape((-1,) + SIG),
                              want[p._start_frame:p._start_frame + p._num_frames])


def test_four_chunks_in_one_decode(ctx, filesets):
    """a frame per copy + decode step: four chunks, each bounce buffer used twice, every chunk after the first at
    an offset into the sector files and into the decoded array"""
    from libertem_amd.io.dataset.k2is import K2ISDataSet
    path, frames = filesets['plain']
    assert len(frames) == 4
    want_bytes = ctx.load('k2is', path=path).decode_bytes
    old = K2ISDataSet.CHUNK_BYTES
    K2ISDataSet.CHUNK_BYTES = 8 * 32 * synth.BLOCK_SIZE
    try:
        ds = ctx.load('k2is', path=path)
    finally:
        K2ISDataSet.CHUNK_BYTES = old
    assert not ds.is_streamed
    assert np.array_equal(ds.data.cpu().reshape(frames.shape), frames)
    assert ds.decode_bytes == want_bytes == 4 * 8 * 32 * synth.BLOCK_SIZE
