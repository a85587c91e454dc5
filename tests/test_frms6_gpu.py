"""
FRMS6DataSet on the GPU (-m gpu): `ctx.load('frms6', ...)` on the synthetic sets A-F of
tests/golden/frms6_recipes.py against the NumPy decoder of tests/frms6_synth.py and against what the REAL
reference's FRMS6DataSet gave for the same files (tests/golden/frms6.npz).

Bit-equal: the resident frames and the uncorrected picks (an explicit empty CorrectionSet), everything of set E
(no corrections: uint16 frames, integer masks), the dark frame.  Corrected float32 results (the dataset's own
dark frame and gain map, picked up by `run_udf`): the tolerance of the comparisons against
tests/golden/corrections.npz in tests/test_udf_gpu.py, rtol = 1e-5 and atol = 1e-5 max|reference|.

Then a streamed load, shards, a reshaped scan and the descriptive surface.
"""
import os
import hashlib

import numpy as np
import pytest

import frms6_recipes as recipes
import frms6_synth as synth
from test_frms6_cpu import expected_frames

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
    d = tmp_path_factory.mktemp('frms6')
    return {name: recipes.write_fileset(name, str(d)) for name in recipes.FILESETS}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def close(a, b, tol=F32_TOL):
    scale = max(np.abs(b).max(), 1e-30)
    return np.allclose(a, b, rtol=tol, atol=tol * scale)


def mask_udf(masks):
    from libertem_amd.udf.masks import ApplyMasksUDF
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


def record_bytes(fileset):
    rec = recipes.FILESETS[fileset]
    return synth.FRAME_HEADER + rec['height'] * rec['width'] * 2


@pytest.mark.parametrize('case', recipes.CASES, ids=lambda c: c['name'])
def test_dataset_vs_reference(ctx, filesets, golden_dir, case):
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    from libertem_amd.udf.raw import PickUDF
    g = np.load(os.path.join(golden_dir, 'frms6.npz'))
    name, fileset = case['name'], case['fileset']
    fs, rec = filesets[fileset], recipes.FILESETS[fileset]
    sig = recipes.sig_shape(fileset)
    so, roi = case['sync_offset'], case['roi']
    ds = ctx.load('frms6', **recipes.load_kwargs(case, fs))
    assert tuple(ds.shape) == tuple(g[name + '__shape']) and tuple(ds.shape.sig) == sig
    assert ds.dtype == np.dtype(str(g[name + '__dtype'])) == (np.float32 if case['offset'] else np.uint16)
    assert ds.storage_dtype == np.uint16 and ds.meta.raw_dtype == np.dtype(str(g[name + '__raw_dtype']))
    assert ds.meta.image_count == int(g[name + '__image_count']) and ds.meta.sync_offset == so
    assert ds.is_device_resident and not ds.is_streamed
    n_nav = int(np.prod(rec['nav']))
    n_src = n_nav - abs(so)
    assert ds.decode_bytes == n_src * record_bytes(fileset) and ds.decode_seconds > 0
    assert ds._valid_frames == (None if so == 0 else (max(0, -so), min(n_nav, n_nav - so)))
    # the resident frames: raw, at their scan positions
    at_positions = synth.positioned(fs['signal'], n_nav, so)
    resident = ds.data.cpu().reshape((n_nav,) + sig)
    assert resident.dtype == np.uint16 and np.array_equal(resident, at_positions)
    # the corrections the set brings along
    corr = ds.get_correction_data()
    if case['offset']:
        dark = corr.get_dark_frame()
        assert dark.dtype == np.float32 and np.array_equal(dark, g[name + '__dark'])
        assert np.array_equal(dark, synth.dark_frame(fs['dark']))
    else:
        assert corr.get_dark_frame() is None
    if case['gain']:
        assert np.array_equal(corr.get_gain_map(), g[name + '__gain'])
    else:
        assert corr.get_gain_map() is None
    assert corr.have_corrections() == (name != 'E')
    # uncorrected picks: an explicit (empty) set wins over the dataset's own
    pick_roi = roi if roi is not None else np.ones(rec['nav'], dtype=bool)
    want = expected_frames(case, fs['signal'])
    raw = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=pick_roi, corrections=CorrectionSet())['intensity'].data
    raw = np.asarray(raw).reshape((-1,) + sig)
    assert np.array_equal(raw, want)
    for p, frame in enumerate(raw.astype(np.uint16)):
        assert np.array_equal(sha(frame), g[name + '__sha_frames'][p]), (name, p)
        assert np.array_equal(frame[recipes.crop(fileset)], g[name + '__crops'][p])
    # with the dataset's own corrections (corrections=None)
    exact = name == 'E'
    picked = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=pick_roi)['intensity'].data
    picked = np.asarray(picked).reshape((-1,) + sig)
    ref = g[name + '__picked']
    assert picked.dtype == ref.dtype, (picked.dtype, ref.dtype)
    assert np.array_equal(picked, ref) if exact else close(picked, ref)
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
        if exact and key != 'masks':
            assert np.array_equal(got, ref), key            # integer sums below 2**24 in float32
    if exact:
        int_masks = recipes.make_int_masks(fileset)
        got = ctx.run_udf(dataset=ds, udf=mask_udf(int_masks), roi=roi)['intensity'].data
        assert np.array_equal(got, g[name + '__int_masks'])
        assert np.array_equal(got, np.tensordot(at_positions.astype(np.int64), int_masks,
                                                ([1, 2], [1, 2])).reshape(got.shape))
    # the descriptive surface
    diag = {x['name']: x['value'] for x in ds.get_diagnostics()}
    assert diag['Offset correction available and enabled'] == str(case['offset'])
    assert diag['signalframes'] == str(n_nav) and diag['darkframes'] == str(rec['dark'])
    assert diag['stemimagesize'] == str(tuple(rec['nav']))
    assert diag['readoutmode'] == str({'bin': rec['binning'], 'win_i': sig[0], 'win_j': sig[1]})
    key = ds.get_cache_key()
    assert key == {'path': fs['hdr'], 'enable_offset_correction': case['offset'],
                   'gain_map_path': fs[case['gain']] if case['gain'] else None, 'shape': tuple(ds.shape),
                   'sync_offset': so}
    assert ds.check_valid() is True and f"nav_shape={tuple(rec['nav'])}" in repr(ds)


def test_reshaped_scan_and_shards(ctx, filesets):
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.udf.sumsigudf import SumSigUDF
    fs = filesets['a']
    frames, dark = fs['signal'], synth.dark_frame(fs['dark'])
    want_sums = (frames.astype(np.float64) - dark).reshape(8, -1).sum(axis=1)
    # loaded through one of the .frms6 files, another scan shape, a sig_shape of the same size
    ds = ctx.load('frms6', path=fs['hdr'][:-4] + '_002.frms6', nav_shape=(4, 2), sig_shape=(4, 16))
    assert tuple(ds.shape) == (4, 2, 4, 16) and ds._valid_frames is None
    assert np.array_equal(ds.data.cpu().reshape(frames.shape), frames)
    assert ds.get_correction_data().get_dark_frame().shape == (4, 16)
    assert close(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data.reshape(-1), want_sums)
    # two ranks: each decodes its block of the first nav axis (ranks 0 and 1 start in files 001 and 002)
    halves = []
    for rank in (0, 1):
        part = ctx.load('frms6', path=fs['hdr'], shard=(rank, 2))
        assert tuple(part.shape) == (2, 4, 8, 8) and part.shard == (rank, 2)
        assert part.local_frame_range == (4 * rank, 4 * rank + 4)
        assert part.decode_bytes == 4 * record_bytes('a')
        halves.append(part.data.cpu().reshape((4, 8, 8)))
        assert np.array_equal(part.get_correction_data().get_dark_frame(), dark)
    assert np.array_equal(np.concatenate(halves), frames)
    # more scan positions than frames: zero frames behind the last one, left out of corrected results
    ds = ctx.load('frms6', path=fs['hdr'], nav_shape=(10,))
    assert tuple(ds.shape) == (10, 8, 8) and ds._valid_frames == (0, 8)
    got = ds.data.cpu().reshape((10, 8, 8))
    assert np.array_equal(got[:8], frames) and not got[8:].any()
    sums = ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data
    assert close(sums[:8], want_sums) and np.all(sums[8:] == 0)
    with pytest.raises(DataSetException, match='sig_shape must be of size: 64'):
        ctx.load('frms6', path=fs['hdr'], sig_shape=(8, 9))
    with pytest.raises(DataSetException, match='does not split over 3 ranks'):
        ctx.load('frms6', path=fs['hdr'], shard=(0, 3))


@pytest.mark.parametrize('sync_offset', (0, 2, -2))
def test_streamed_like_resident(ctx, filesets, monkeypatch, sync_offset):
    """decoded frames that may not stay in HBM: every partition decodes its own from the files"""
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.io.dataset.frms6 import FRMS6DataSet
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    fs = filesets['a']
    masks = recipes.make_masks('a')
    resident = ctx.load('frms6', path=fs['hdr'], sync_offset=sync_offset)
    monkeypatch.setattr(FRMS6DataSet, 'MAX_RESIDENT_BYTES', 3 * 8 * 8 * 2)       # three frames
    ds = ctx.load('frms6', path=fs['hdr'], sync_offset=sync_offset)
    monkeypatch.setattr(FRMS6DataSet, 'MAX_RESIDENT_BYTES', None)
    assert ds.is_streamed and not resident.is_streamed and not ds.stable_device_tiles
    assert tuple(ds.shape) == tuple(resident.shape) and ds._valid_frames == resident._valid_frames
    assert ds.get_num_partitions() == 3 and ds.decode_bytes == 0
    assert np.array_equal(ds.get_correction_data().get_dark_frame(),
                          resident.get_correction_data().get_dark_frame())
    with pytest.raises(DataSetException, match='streamed'):
        ds.data
    for udf in (SumSigUDF, lambda: mask_udf(masks)):
        want = ctx.run_udf(dataset=resident, udf=udf())['intensity'].data
        assert np.array_equal(ctx.run_udf(dataset=ds, udf=udf())['intensity'].data, want)
    # (a sum over all frames: one partition there, three here -- float32 sums in another order)
    want = ctx.run_udf(dataset=resident, udf=SumUDF())['intensity'].data
    assert close(ctx.run_udf(dataset=ds, udf=SumUDF())['intensity'].data, want)
    assert ds.decode_bytes > 0
    at_positions = synth.positioned(fs['signal'], 8, sync_offset)
    for p in ds.get_partitions():
        arr, row0 = ds.device_frames(p._local0, p._num_frames)
        assert np.array_equal(arr.rows(row0, row0 + p._num_frames).cpu().reshape((-1, 8, 8)),
                              at_positions[p._start_frame:p._start_frame + p._num_frames])


def test_a_chunk_never_spans_two_files(ctx, filesets, monkeypatch):
    """two records per copy: files of 5 + 3 frames go up as 2 + 2 + 1 and 2 + 1 records"""
    from libertem_amd import hip
    from libertem_amd.io.dataset.frms6 import FRMS6DataSet
    fs = filesets['a']
    calls = []
    real = hip.frms6_decode

    def spy(device, src, stride, n, *args, **kw):
        calls.append(n)
        return real(device, src, stride, n, *args, **kw)
    monkeypatch.setattr(hip, 'frms6_decode', spy)
    monkeypatch.setattr(FRMS6DataSet, 'CHUNK_BYTES', 2 * record_bytes('a'))
    ds = ctx.load('frms6', path=fs['hdr'])
    assert calls == [2, 2, 1, 2, 1, 2, 1]                   # the signal files, then the dark file (3 frames)
    assert np.array_equal(ds.data.cpu().reshape(fs['signal'].shape), fs['signal'])
    assert np.array_equal(ds.get_correction_data().get_dark_frame(), synth.dark_frame(fs['dark']))


@pytest.mark.parametrize('name', ('D_p2', 'D_m2'))
def test_frameless_positions_next_to_a_non_folding_udf(ctx, filesets, golden_dir, name):
    """Runs in which the corrections are NOT folded into the masks (a PickUDF in the same run, shifted masks): the
    frames are corrected on the device, SumSigUDF and ApplyMasksUDF would take write-once buffers -- but with a dark
    frame the scan positions the sync_offset left without a frame are not handed to them, so their rows keep the
    zero fill, as in the reference.  (A run on set A with the same ROI goes first: it leaves non-zero rows of the
    same size behind in the result memory that is reused.)"""
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    from libertem_amd.udf.raw import PickUDF
    g = np.load(os.path.join(golden_dir, 'frms6.npz'))
    case = next(c for c in recipes.CASES if c['name'] == name)
    fs, so, roi = filesets[case['fileset']], case['sync_offset'], case['roi']
    masks = recipes.make_masks(case['fileset'])

    def shifted():
        return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                             mask_dtype=masks.dtype, shifts=(0, 0))
    runs = (('sumsig', lambda: [SumSigUDF(), PickUDF()]), ('masks', lambda: [mask_udf(masks), PickUDF()]),
            ('masks', lambda: [shifted()]))
    full = ctx.load('frms6', **recipes.load_kwargs(dict(case, sync_offset=0), fs))
    for key, udfs in runs:
        assert np.any(ctx.run_udf(dataset=full, udf=udfs(), roi=roi)[0]['intensity'].data[roi] != 0)
    ds = ctx.load('frms6', **recipes.load_kwargs(case, fs))
    lo, hi = ds._valid_frames
    frameless = roi.reshape(-1) & ~((np.arange(roi.size) >= lo) & (np.arange(roi.size) < hi))
    assert frameless.sum() == 1                                 # (position 6 for +2, position 0 for -2)
    for key, udfs in runs:
        got = ctx.run_udf(dataset=ds, udf=udfs(), roi=roi)[0]['intensity'].data
        ref = g[f"{name}__{key}"]
        assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), key
        flat = got.reshape((roi.size, -1))
        assert np.all(flat[frameless] == 0), (key, flat[frameless])
        assert close(np.nan_to_num(got), np.nan_to_num(ref)), (key, got, ref)


def test_gain_map_follows_sig_shape(ctx, filesets, tmp_path):
    """the gain map is stored in the unfolded frame's shape: like the dark frame it is reshaped to a `sig_shape`;
    one of another size is refused"""
    from libertem_amd.io.dataset.base import DataSetException
    from libertem_amd.udf.sumsigudf import SumSigUDF
    fs = filesets['b']
    ds = ctx.load('frms6', path=fs['hdr'], gain_map_path=fs['mat'], sig_shape=(6, 24))
    corr = ds.get_correction_data()
    assert tuple(ds.shape) == (6, 6, 24)
    assert corr.get_dark_frame().shape == corr.get_gain_map().shape == (6, 24)
    assert np.array_equal(corr.get_gain_map(), fs['gain'].reshape(6, 24))
    want = ((fs['signal'].astype(np.float64) - synth.dark_frame(fs['dark'])) * fs['gain']).reshape(6, -1).sum(axis=1)
    assert close(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data, want)
    small = synth.write_gain_csv(str(tmp_path / 'small.csv'), fs['gain'][:, :11])
    with pytest.raises(DataSetException, match=r'gain map .*small.csv is of shape \(12, 11\), the frames are of'):
        ctx.load('frms6', path=fs['hdr'], gain_map_path=small)
