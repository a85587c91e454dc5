"""
TVIPSDataSet on the GPU (-m gpu): `ctx.load('tvips', ...)` on the synthetic series of
tests/golden/tvips_recipes.py against the by-hand decoder of tests/tvips_synth.py and against what the REAL
reference's reader gave for the same files (tests/golden/tvips.npz).

Bit-equal: the resident frames and the picks, with the sha256 of every picked frame, and the sums (whole numbers
below 2**24).  Mask results: the comparison and tolerance of tests/test_records_gpu.py::test_dataset_vs_reference,
rtol = 1e-5 and atol = 1e-5 max|reference|.

Then what a series adds to the record path: chunks that end where a file ends, the width of `k_records<W>` each
series is gathered with (16, 4, 1, 4, 2), a streamed load, shards, and `ctx.load('auto', ...)`.
"""
import os
import hashlib

import numpy as np
import pytest

import tvips_recipes as recipes
import records_synth
from test_tvips_cpu import expected_frames

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F32_TOL = 1e-5
#: W of k_records<W>: the largest of 16, 8, 4, 2, 1 that divides image header, stride and payload (the uploads and
#: the destination start at multiples of 16)
WIDTHS = {'t16': 16, 't16v1': 4, 't8v1': 1, 'tline': 4, 'tnoscan': 2}


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def filesets(tmp_path_factory):
    d = tmp_path_factory.mktemp('tvips')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'tvips.npz'))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def close(a, b, tol=F32_TOL):
    scale = max(np.abs(b).max(), 1e-30)
    return np.allclose(a, b, rtol=tol, atol=tol * scale)


def mask_udf(masks):
    from libertem_amd.udf.masks import ApplyMasksUDF
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


def load(ctx, case, filesets, **more):
    return ctx.load('tvips', **dict(recipes.load_kwargs(case, filesets[case['fileset']]), **more))


def at_positions(case, frames):
    """all scan positions of a case, (n_nav,) + its sig shape: frame g at g - sync_offset, zero frames elsewhere"""
    n_nav = int(np.prod(case['nav']))
    return records_synth.positioned(frames, n_nav, case['sync_offset']).reshape((n_nav,) + recipes.sig_shape(case))


def frames_with_a_position(case):
    """how many frames of the files land on a scan position, and which positions hold one"""
    n_nav, so, n = int(np.prod(case['nav'])), case['sync_offset'], recipes.n_frames(case['fileset'])
    held = [p for p in range(n_nav) if 0 <= p + so < n]
    return len(held), (None if len(held) == n_nav else (held[0], held[-1] + 1))


def spy_on_gather(monkeypatch):
    """-> list that collects (n, W by the rule of include/ltmi.h) of every `records_gather` call"""
    from libertem_amd import hip
    calls = []
    real = hip.records_gather

    def spy(device, src, stride, n, payload, dst, stream=None):
        w = next(w for w in (16, 8, 4, 2, 1) if all(v % w == 0 for v in (src, stride, payload, dst)))
        calls.append((n, w))
        return real(device, src, stride, n, payload, dst, stream)
    monkeypatch.setattr(hip, 'records_gather', spy)
    return calls


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_dataset_vs_reference(ctx, filesets, golden, case):
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    from libertem_amd.udf.raw import PickUDF
    g = golden
    name, fileset = case['name'], case['fileset']
    fs = filesets[fileset]
    sig = recipes.sig_shape(case)
    so, roi, nav = case['sync_offset'], case['roi'], tuple(case['nav'])
    ds = load(ctx, case, filesets)
    assert tuple(ds.shape) == tuple(g[name + '__shape']) == nav + sig
    assert ds.dtype == np.dtype(str(g[name + '__dtype'])) == recipes.stored_dtype(fileset)
    assert ds.storage_dtype == ds.dtype and ds.meta.raw_dtype == np.dtype(str(g[name + '__raw_dtype']))
    assert ds.meta.image_count == int(g[name + '__image_count']) == recipes.n_frames(fileset)
    assert ds.meta.sync_offset == int(g[name + '__sync_offset']) == so
    assert ds.is_device_resident and not ds.is_streamed
    n_nav = int(np.prod(nav))
    n_src, valid = frames_with_a_position(case)
    # whole records went up and were gathered
    assert ds.decode_bytes == n_src * recipes.stride(fileset) and ds.decode_seconds > 0
    assert ds._valid_frames == valid
    # the resident frames: raw, at their scan positions
    want_all = at_positions(case, fs['frames'])
    resident = ds.data.cpu().reshape((n_nav,) + sig)
    assert resident.dtype == ds.dtype and np.array_equal(resident, want_all)
    assert ds.get_correction_data() is None
    # picks
    pick_roi = roi if roi is not None else np.ones(nav, dtype=bool)
    want = expected_frames(case, fs['frames'])
    for corrections in (CorrectionSet(), None):
        raw = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=pick_roi, corrections=corrections)['intensity'].data
        raw = np.asarray(raw).reshape((-1,) + sig)
        assert raw.dtype == ds.dtype == np.dtype(str(g[name + '__picked_dtype'])) and np.array_equal(raw, want)
    for p, frame in enumerate(raw):
        assert np.array_equal(sha(frame), g[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(recipes.crop(fileset)(frame), g[name + '__crops'][p])
    assert np.array_equal(raw.reshape(len(raw), -1).sum(axis=1, dtype=np.float64), g[name + '__picked_sumsig'])
    masks = recipes.make_masks(case)
    for key, udf in (('sum', SumUDF()), ('sumsig', SumSigUDF()), ('masks', mask_udf(masks))):
        got = ctx.run_udf(dataset=ds, udf=udf, roi=roi)['intensity'].data
        ref = g[f"{name}__{key}"]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (key, got.dtype, ref.dtype)
        same = np.isnan(ref) == np.isnan(got)               # (nav results outside a ROI)
        assert same.all(), key
        got, ref = np.nan_to_num(got), np.nan_to_num(ref)
        print(name, key, 'max |got - ref| =', np.abs(got - ref).max(), 'max |ref| =', np.abs(ref).max())
        assert close(got, ref), (key, np.abs(got - ref).max(), np.abs(ref).max())
        if key != 'masks':
            assert np.array_equal(got, ref), key            # (whole numbers, sums below 2**24 in float32)
    # the descriptive surface
    assert ds.check_valid() is True and f"shape={tuple(ds.shape)}" in repr(ds)
    assert ds.get_cache_key() == {'path': fs['path'], 'shape': tuple(ds.shape), 'sync_offset': so}
    rec = recipes.FILESETS[fileset]
    assert ds.get_diagnostics() == [
        {'name': 'Bits per pixel', 'value': str(8 * ds.dtype.itemsize)}, {'name': 'High tension (kV)', 'value': '300'},
        {'name': 'Pixel size (nm)', 'value': '7'}, {'name': 'Binning (x)', 'value': '2'},
        {'name': 'Binning (y)', 'value': '4'}, {'name': 'File Format Version', 'value': str(rec['version'])}]
    assert ds.header.xdim == recipes.native_shape(fileset)[1] and len(ds.diagnostics) == 6 + 6


def test_chunks_end_where_a_file_ends(ctx, filesets, monkeypatch):
    """two records per copy on 7 + 3 + 2 frames: the chunks are 2 2 2 1 | 2 1 | 2 frames, each gathered behind its
    copy with one stride, and the frames are those of a load in one chunk per file"""
    from libertem_amd import hip
    from libertem_amd.io.dataset.tvips import TVIPSDataSet
    fs = filesets['t16']
    calls = spy_on_gather(monkeypatch)
    whole = ctx.load('tvips', path=fs['path'], nav_shape=(12,), sync_offset=0)
    assert calls == [(7, 16), (3, 16), (2, 16)]             # (the default chunk: a file at a time)
    del calls[:]
    monkeypatch.setattr(TVIPSDataSet, 'CHUNK_BYTES', 2 * 208)
    ds = ctx.load('tvips', path=fs['path'], nav_shape=(12,), sync_offset=0)
    assert calls == [(n, 16) for n in (2, 2, 2, 1, 2, 1, 2)]
    assert hip.records_last_kernel() == 'k_records<16>'
    assert ds.decode_bytes == whole.decode_bytes == 12 * 208
    assert np.array_equal(ds.data.cpu(), whole.data.cpu())
    assert np.array_equal(ds.data.cpu().reshape(fs['frames'].shape), fs['frames'])
    # the detected scan starts at frame 1: 2 2 2 | 2 frames
    del calls[:]
    ds = ctx.load('tvips', path=fs['path'])
    assert calls == [(2, 16)] * 4 and tuple(ds.shape) == (2, 4, 6, 8)
    assert np.array_equal(ds.data.cpu().reshape((8, 6, 8)), fs['frames'][1:9])


@pytest.mark.parametrize('fileset', sorted(WIDTHS))
def test_width_of_the_gather_per_series(ctx, filesets, monkeypatch, fileset):
    """image headers of 112, 12 and 12, 108 and 120 bytes in front of payloads of 96, 72, 25, 24 and 30: the kernel
    that ran is the one the placement allows, with chunks of two records and of a file at a time alike"""
    from libertem_amd import hip
    from libertem_amd.io.dataset.tvips import TVIPSDataSet
    fs, rec = filesets[fileset], recipes.FILESETS[fileset]
    stride, n = recipes.stride(fileset), recipes.n_frames(fileset)
    assert WIDTHS[fileset] == next(w for w in (16, 8, 4, 2, 1)
                                   if all(v % w == 0 for v in (rec['header'], stride, stride - rec['header'])))
    calls = spy_on_gather(monkeypatch)
    for chunk_bytes in (2 * stride, TVIPSDataSet.CHUNK_BYTES):
        del calls[:]
        monkeypatch.setattr(TVIPSDataSet, 'CHUNK_BYTES', chunk_bytes)
        ds = ctx.load('tvips', path=fs['path'], nav_shape=(n,), sync_offset=0)
        assert calls and all(w == WIDTHS[fileset] for _, w in calls) and sum(k for k, _ in calls) == n
        assert hip.records_last_kernel() == f"k_records<{WIDTHS[fileset]}>"
        assert np.array_equal(ds.data.cpu().reshape(fs['frames'].shape), fs['frames'])


@pytest.mark.parametrize('name', ('TV_bare', 'TV_p2', 'TV_m2', 'TV_v1_8'))
def test_streamed_like_resident(ctx, filesets, monkeypatch, name):
    """frames that may not stay in HBM: every partition gathers its own from the file that holds it"""
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.io.dataset.records import RecordFileDataSet
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    case = recipes.case(name)
    fs = filesets[case['fileset']]
    masks = recipes.make_masks(case)
    resident = load(ctx, case, filesets)
    frame_bytes = resident._records['payload_bytes']
    monkeypatch.setattr(RecordFileDataSet, 'MAX_RESIDENT_BYTES', frame_bytes - 1)       # below one frame
    ds = load(ctx, case, filesets)
    monkeypatch.setattr(RecordFileDataSet, 'MAX_RESIDENT_BYTES', None)
    n_nav = int(np.prod(case['nav']))
    assert ds.is_streamed and not resident.is_streamed and not ds.stable_device_tiles
    assert tuple(ds.shape) == tuple(resident.shape) and ds._valid_frames == resident._valid_frames
    assert ds.meta.sync_offset == resident.meta.sync_offset == case['sync_offset']
    assert ds.get_num_partitions() == n_nav and ds.decode_bytes == 0
    with pytest.raises(DataSetException, match=f"this {ds.KIND} is streamed"):
        ds.data
    for udf in (SumSigUDF, lambda: mask_udf(masks)):
        want = ctx.run_udf(dataset=resident, udf=udf())['intensity'].data
        assert np.array_equal(ctx.run_udf(dataset=ds, udf=udf())['intensity'].data, want)
    # (whole numbers below 2**24: the order of the partitions does not show)
    want = ctx.run_udf(dataset=resident, udf=SumUDF())['intensity'].data
    assert np.array_equal(ctx.run_udf(dataset=ds, udf=SumUDF())['intensity'].data, want)
    assert ds.decode_bytes > 0 and ds.decode_bytes % recipes.stride(case['fileset']) == 0
    want_all = at_positions(case, fs['frames'])
    for p in ds.get_partitions():
        arr, row0 = ds.device_frames(p._local0, p._num_frames)
        assert np.array_equal(arr.rows(row0, row0 + p._num_frames).cpu().reshape((-1,) + want_all.shape[1:]),
                              want_all[p._start_frame:p._start_frame + p._num_frames])


def test_shards_and_auto(ctx, filesets):
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.io.dataset.tvips import TVIPSDataSet
    fs = filesets['t16']
    # two ranks: each loads its row of the scan (frames 1 - 4 and 5 - 8, the second from two files)
    halves = []
    for rank in (0, 1):
        part = ctx.load('tvips', path=fs['path'], shard=(rank, 2))
        assert part.shard == (rank, 2) and tuple(part.shape) == (2, 4, 6, 8)        # (the shape of the whole scan)
        assert part.local_frame_range == (4 * rank, 4 * rank + 4) and part.meta.sync_offset == 1
        assert part.decode_bytes == 4 * 208
        halves.append(part.data.cpu().reshape((4, 6, 8)))
    assert np.array_equal(np.concatenate(halves), fs['frames'][1:9])
    with pytest.raises(DataSetException, match='does not split over 3 ranks'):
        ctx.load('tvips', path=fs['path'], shard=(0, 3))
    # 'auto': the type is detected, the arguments are the caller's
    for kwargs in ({}, dict(nav_shape=(3, 4), sync_offset=0), dict(sig_shape=(48,))):
        named = ctx.load('tvips', path=fs['path'], **kwargs)
        for auto in (ctx.load('auto', path=fs['paths'][2], **kwargs), ctx.load('auto', fs['path'], **kwargs)):
            assert type(auto) is TVIPSDataSet and tuple(auto.shape) == tuple(named.shape)
            assert auto.meta.sync_offset == named.meta.sync_offset and auto.dtype == named.dtype
            assert np.array_equal(auto.data.cpu(), named.data.cpu())
    with pytest.raises(DataSetException, match='could not determine DataSet type'):
        ctx.load('auto', path=__file__)
