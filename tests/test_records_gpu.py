"""
SEQDataSet, EMPADDataSet and BloDataSet on the GPU (-m gpu): `ctx.load('seq' | 'empad' | 'blo', ...)` on the
synthetic files of tests/golden/records_recipes.py against the NumPy decoder of tests/records_synth.py and against
what the REAL reference's readers gave for the same files (tests/golden/records.npz).

Bit-equal: the resident frames and the uncorrected picks, with the sha256 of every picked frame.  UDF results,
with a SEQ set's own dark frame, gain map and dead pixels picked up by `run_udf`: the comparison and tolerance of
tests/test_frms6_gpu.py::test_dataset_vs_reference, rtol = 1e-5 and atol = 1e-5 max|reference|.

Then a reshaped frame, shards, a streamed load and what `decode_bytes` counts.
"""
import os
import hashlib

import numpy as np
import pytest

import records_recipes as recipes
import records_synth as synth
from test_records_cpu import expected_frames

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F32_TOL = 1e-5


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    d = tmp_path_factory.mktemp('records')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'records.npz'))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def close(a, b, tol=F32_TOL):
    scale = max(np.abs(b).max(), 1e-30)
    return np.allclose(a, b, rtol=tol, atol=tol * scale)


def mask_udf(masks):
    from libertem_amd.udf.masks import ApplyMasksUDF
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


def kind_of(fileset):
    return recipes.FILESETS[fileset]['kind']


def load(ctx, case, filesets, **more):
    fileset = case['fileset']
    return ctx.load(kind_of(fileset), **dict(recipes.load_kwargs(case, filesets[fileset]), **more))


def record_bytes(ds):
    r = ds._records
    return r['frame_header'] + r['payload_bytes'] + r['frame_footer']


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_dataset_vs_reference(ctx, filesets, golden, case):
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    from libertem_amd.udf.raw import PickUDF
    g = golden
    name, fileset = case['name'], case['fileset']
    fs, kind = filesets[fileset], kind_of(fileset)
    sig = tuple(recipes.sig_shape(fileset))
    so, roi, nav = case['sync_offset'], case['roi'], tuple(case['nav'])
    ds = load(ctx, case, filesets)
    assert tuple(ds.shape) == tuple(g[name + '__shape']) == nav + sig
    assert ds.dtype == np.dtype(str(g[name + '__dtype'])) == recipes.stored_dtype(fileset)
    assert ds.storage_dtype == ds.dtype and ds.meta.raw_dtype == np.dtype(str(g[name + '__raw_dtype']))
    assert ds.meta.image_count == int(g[name + '__image_count']) and ds.meta.sync_offset == so
    assert ds.is_device_resident and not ds.is_streamed
    n_nav = int(np.prod(nav))
    n_src = n_nav - abs(so)
    # whole records went up and were gathered
    assert ds.decode_bytes == n_src * record_bytes(ds) and ds.decode_seconds > 0
    assert ds._valid_frames == (None if so == 0 else (max(0, -so), min(n_nav, n_nav - so)))
    # the resident frames: raw, at their scan positions
    at_positions = synth.positioned(fs['frames'], n_nav, so)
    resident = ds.data.cpu().reshape((n_nav,) + sig)
    assert resident.dtype == ds.dtype and np.array_equal(resident, at_positions)
    # the corrections a SEQ set brings along
    has_corr = kind == 'seq' and fs['dark'] is not None
    if kind == 'seq':
        corr = ds.get_correction_data()
        assert corr.have_corrections() == has_corr
        if has_corr:
            assert np.array_equal(corr.get_dark_frame(), g[name + '__dark'])
            assert np.array_equal(corr.get_gain_map(), g[name + '__gain'])
            assert set(zip(*corr.get_excluded_pixels().coords.tolist())) == set(zip(*g[name + '__excluded'].tolist()))
    else:
        assert ds.get_correction_data() is None
    # uncorrected picks: an explicit (empty) set wins over the dataset's own
    pick_roi = roi if roi is not None else np.ones(nav, dtype=bool)
    want = expected_frames(case, fs['frames'])
    raw = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=pick_roi, corrections=CorrectionSet())['intensity'].data
    raw = np.asarray(raw).reshape((-1,) + sig)
    assert raw.dtype == ds.dtype and np.array_equal(raw, want)
    for p, frame in enumerate(raw):
        assert np.array_equal(sha(frame), g[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(recipes.crop(fileset)(frame), g[name + '__crops'][p])
    # with the dataset's own corrections (corrections=None)
    picked = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=pick_roi)['intensity'].data
    picked = np.asarray(picked).reshape((-1,) + sig)
    assert picked.dtype == np.dtype(str(g[name + '__picked_dtype']))
    if has_corr:
        assert close(picked, g[name + '__picked'])
    else:
        assert np.array_equal(picked, want)
    assert close(picked.reshape(len(picked), -1).sum(axis=1, dtype=np.float64), g[name + '__picked_sumsig'])
    masks = recipes.make_masks(fileset)
    for key, udf in (('sum', SumUDF()), ('sumsig', SumSigUDF()), ('masks', mask_udf(masks))):
        got = ctx.run_udf(dataset=ds, udf=udf, roi=roi)['intensity'].data
        ref = g[f"{name}__{key}"]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (key, got.dtype, ref.dtype)
        same = np.isnan(ref) == np.isnan(got)               # (nav results outside a ROI)
        assert same.all(), key
        got, ref = np.nan_to_num(got), np.nan_to_num(ref)
        print(name, key, 'max |got - ref| =', np.abs(got - ref).max(), 'max |ref| =', np.abs(ref).max())
        assert close(got, ref), (key, np.abs(got - ref).max(), np.abs(ref).max())
        if not has_corr and key != 'masks' and (kind != 'empad' or key == 'sum'):
            # whole numbers, sums below 2**24 in float32 (not a frame sum of EMPAD: 16384 pixels of up to 4095)
            assert np.array_equal(got, ref), key
    # the descriptive surface
    assert ds.check_valid() is True and f"shape={tuple(ds.shape)}" in repr(ds)
    key = ds.get_cache_key()
    assert key['shape'] == tuple(ds.shape) and key['sync_offset'] == so
    diag = {x['name']: x['value'] for x in ds.get_diagnostics()}
    if kind == 'seq':
        assert diag['Footer size'] == str(int(g[name + '__footer'])) and key['path'] == fs['path']
        assert diag['Dark frame included'] == diag['Gain map included'] == str(has_corr)
    elif kind == 'empad':
        assert key['path_raw'] == fs['raw'] and diag['Frames'] == str(n_nav)
    else:
        assert key['endianess'] == recipes.FILESETS[fileset]['endianess'] and diag['DP_SZ'] == str(sig[0])


def test_reshaped_frames_and_shards(ctx, filesets):
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.udf.sumsigudf import SumSigUDF
    fs = filesets['s16']
    frames = fs['frames']
    # a sig_shape of the same size, another scan shape
    ds = ctx.load('seq', path=fs['path'], nav_shape=(4, 2), sig_shape=(4, 12))
    assert tuple(ds.shape) == (4, 2, 4, 12) and ds._valid_frames is None
    assert np.array_equal(ds.data.cpu().reshape(frames.shape), frames)
    with pytest.raises(DataSetException, match='sig_shape must be of size: 48'):
        ctx.load('seq', path=fs['path'], nav_shape=(4, 2), sig_shape=(7, 7))
    # two ranks: each loads its half of the first nav axis
    for kind, name, kw, n in (('seq', 's16', dict(nav_shape=(2, 4)), 8), ('empad', 'e_acq', {}, 8),
                              ('blo', 'b16le', {}, 4)):
        halves = []
        for rank in (0, 1):
            part = ctx.load(kind, path=filesets[name]['path'], shard=(rank, 2), **kw)
            assert part.shard == (rank, 2) and tuple(part.shape)[1:] == tuple(part._layout.nav_shape)[1:] + tuple(part._layout.sig_shape)
            assert part.local_frame_range == (n // 2 * rank, n // 2 * rank + n // 2)
            assert part.decode_bytes == n // 2 * record_bytes(part)
            halves.append(part.data.cpu().reshape((n // 2,) + filesets[name]['frames'].shape[1:]))
        assert np.array_equal(np.concatenate(halves), filesets[name]['frames'])
    with pytest.raises(DataSetException, match='does not split over 3 ranks'):
        ctx.load('empad', path=filesets['e_acq']['path'], shard=(0, 3))
    # more scan positions than frames: zero frames behind the last one
    ds = ctx.load('blo', path=filesets['b8']['path'], nav_shape=(8,))
    assert tuple(ds.shape) == (8, 5, 5) and ds._valid_frames == (0, 6)
    got = ds.data.cpu().reshape((8, 5, 5))
    assert np.array_equal(got[:6], filesets['b8']['frames']) and not got[6:].any()
    sums = ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data
    assert np.array_equal(sums[:6], filesets['b8']['frames'].reshape(6, -1).sum(axis=1)) and np.all(sums[6:] == 0)


def test_a_last_record_without_its_footer_loads(ctx, filesets, tmp_path):
    """an EMPAD file cut behind the last image row: the caller counts 8 frames by hand, all 8 load (the upload copies
    what the file holds, the kernel reads payloads only)"""
    from libertem_amd.io.dataset.empad import EMPADDataSet
    frames = recipes.make_frames('e_acq')
    path = synth.write_empad_raw(str(tmp_path / 'cut.raw'), frames, last_footer=False)
    ds = EMPADDataSet(path=path, nav_shape=(8,))
    layout = ds._scan_file()
    assert layout.n_frames == 7
    # (the file's own count stays the reference's rule: whole records; the 8th is reached through the layout)
    ds._scan_file = lambda: layout._replace(n_frames=8)
    ds.initialize(ctx.executor)
    assert np.array_equal(ds.data.cpu().reshape(frames.shape), frames)


@pytest.mark.parametrize('name', ('SEQ_A', 'SEQ_p2', 'SEQ_m2', 'EMPAD_acquire', 'BLO_u16le'))
def test_streamed_like_resident(ctx, filesets, monkeypatch, name):
    """frames that may not stay in HBM: every partition gathers its own from the file"""
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.io.dataset.records import RecordFileDataSet
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    case = recipes.case(name)
    fs = filesets[case['fileset']]
    masks = recipes.make_masks(case['fileset'])
    resident = load(ctx, case, filesets)
    frame_bytes = resident._records['payload_bytes']
    monkeypatch.setattr(RecordFileDataSet, 'MAX_RESIDENT_BYTES', frame_bytes - 1)       # below one frame
    ds = load(ctx, case, filesets)
    monkeypatch.setattr(RecordFileDataSet, 'MAX_RESIDENT_BYTES', None)
    n_nav = int(np.prod(case['nav']))
    assert ds.is_streamed and not resident.is_streamed and not ds.stable_device_tiles
    assert tuple(ds.shape) == tuple(resident.shape) and ds._valid_frames == resident._valid_frames
    assert ds.get_num_partitions() == n_nav and ds.decode_bytes == 0
    with pytest.raises(DataSetException, match=f"this {ds.KIND} is streamed"):
        ds.data
    for udf in (SumSigUDF, lambda: mask_udf(masks)):
        want = ctx.run_udf(dataset=resident, udf=udf())['intensity'].data
        assert np.array_equal(ctx.run_udf(dataset=ds, udf=udf())['intensity'].data, want)
    # (a sum over all frames: one partition there, one per frame here -- float32 sums in another order)
    want = ctx.run_udf(dataset=resident, udf=SumUDF())['intensity'].data
    assert close(ctx.run_udf(dataset=ds, udf=SumUDF())['intensity'].data, want)
    assert ds.decode_bytes > 0 and ds.decode_bytes % record_bytes(ds) == 0
    at_positions = synth.positioned(fs['frames'], n_nav, case['sync_offset'])
    for p in ds.get_partitions():
        arr, row0 = ds.device_frames(p._local0, p._num_frames)
        assert np.array_equal(arr.rows(row0, row0 + p._num_frames).cpu().reshape((-1,) + at_positions.shape[1:]),
                              at_positions[p._start_frame:p._start_frame + p._num_frames])


def test_chunks_of_whole_records(ctx, filesets, monkeypatch):
    """two records per copy: 6 BLO patterns go up as 2 + 2 + 2 records, each gathered behind its copy; the source
    pointer is the chunk's first payload, 6 bytes into the upload"""
    from libertem_amd import hip
    from libertem_amd.io.dataset.blo import BloDataSet
    fs = filesets['b8']
    calls = []
    real = hip.records_gather

    def spy(device, src, stride, n, payload, dst, stream=None):
        calls.append((src % 2, stride, n, payload))
        return real(device, src, stride, n, payload, dst, stream)
    monkeypatch.setattr(hip, 'records_gather', spy)
    monkeypatch.setattr(BloDataSet, 'CHUNK_BYTES', 2 * 31)
    ds = ctx.load('blo', path=fs['path'])
    assert calls == [(0, 31, 2, 25)] * 3
    assert hip.records_last_kernel() == 'k_records<1>'
    assert np.array_equal(ds.data.cpu().reshape(fs['frames'].shape), fs['frames'])
    assert ds.decode_bytes == 6 * 31
