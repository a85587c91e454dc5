"""
CPU half of electron counting (libertem_amd/udf/counting.py): `count_frames`, the vectorised definition and NumPy
branch of both UDFs, against the pixel-by-pixel loop of tests/count_ref.py on every input of its table, both kinds of
stored values; the planted events of `electron_frames` recovered exactly; `count_events` on the inline executor
writing the three files and the sidecar that `ctx.load('raw_csr')` reads back; `estimate_thresholds`; the argument
errors; the entries of the header against their bindings.  Everything is compared for equality: no tolerance.

Before counting existed this file failed with an ImportError (no libertem_amd.udf.counting, no electron_frames).
"""
import os
import re

import numpy as np
import pytest

import count_ref as cr

from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.counting import (EventCountUDF, EventStoreUDF, count_events, count_frames,
                                       estimate_thresholds)
from libertem_amd.utils.generate import electron_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'ltmi_count_events': 13, 'ltmi_store_events': 19, 'ltmi_count_strip_rows': 2, 'ltmi_count_last_kernel': 0}


@pytest.fixture(scope='module')
def ctx():
    ctx = Context(executor=InlineJobExecutor())
    yield ctx
    ctx.close()


def same(got, want):
    assert len(got) == len(want) == 3
    for g, w, name in zip(got, want, ('indptr', 'indices', 'data')):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), name


@pytest.mark.parametrize('values', ('count', 'intensity'))
@pytest.mark.parametrize('name', sorted(cr.CASES))
def test_count_frames_is_the_definition(name, values):
    frames, t_bg, t_x, dark, gain = cr.case(name)
    want = cr.reference(name, values)
    if name in ('lattice', 'special', 'special-inf') or name.startswith('ties'):
        assert want[0][-1] > 0                               # (the case is about events that exist)
    same(count_frames(frames, t_bg, t_x, dark=dark, gain=gain, values=values), want)


def test_the_special_values_are_decided_as_stated():
    frames, t_bg, t_x, _, _ = cr.case('special')
    indptr, indices, data = count_frames(frames, t_bg, t_x, values='intensity')
    first = set(indices[indptr[0]:indptr[1]].tolist())
    at = lambda y, x: y * 9 + x
    assert at(2, 2) not in first                             # v == t_bg
    assert at(2, 6) in first                                 # v == t_x
    assert at(6, 2) not in first and at(6, 3) in first       # v > t_x
    assert at(6, 6) not in first and at(5, 6) in first       # NaN
    second = set(indices[indptr[1]:indptr[2]].tolist())
    assert at(1, 1) not in second and at(1, 2) in second     # +Inf above t_x
    assert at(4, 5) in second
    assert at(7, 7) in second and at(7, 8) not in second and at(8, 7) not in second
    assert indptr[3] == indptr[2]                            # all NaN
    frames, t_bg, t_x, _, _ = cr.case('special-inf')
    indptr, indices, data = count_frames(frames, t_bg, t_x, values='intensity')
    first = indices[indptr[0]:indptr[1]].tolist()
    assert at(3, 3) in first and at(3, 4) not in first and at(4, 2) not in first and at(8, 8) not in first
    assert np.isposinf(data[first.index(at(3, 3))])
    assert indices[indptr[1]:indptr[2]].tolist() == [at(4, 4)] and data[indptr[1]] == 0


def test_no_two_events_are_adjacent():
    frames, t_bg, t_x, _, _ = cr.case('ties-33x35')
    indptr, indices, _ = count_frames(frames, t_bg, t_x)
    y, x = np.divmod(indices[indptr[0]:indptr[1]].astype(np.int64), 35)
    apart = np.maximum(np.abs(y[:, None] - y[None]), np.abs(x[:, None] - x[None])) + 2 * np.eye(len(y), dtype=np.int64)
    assert len(y) > 20 and apart.min() >= 2


@pytest.mark.parametrize('seed', (1, 2))
def test_planted_events_are_recovered(seed):
    frames, dark, (indptr, indices) = electron_frames(6, (64, 66), 0.05, seed, xrays=3)
    assert frames.dtype == np.uint16 and dark.dtype == np.float32 and (frames == 60000).sum() == 18
    assert indptr[-1] > 20
    got = count_frames(frames, 10, 1000, dark=dark)
    same(got, (indptr, indices, np.ones(len(indices), np.uint8)))
    # without the x-ray threshold the hits count too
    assert count_frames(frames, 10, dark=dark)[0][-1] == indptr[-1] + 18


def test_estimate_thresholds_make_counting_exact():
    frames, dark, (indptr, indices) = electron_frames(40, (64, 64), 0.05, 5, xrays=3)
    t_bg, t_x = estimate_thresholds(frames, dark=dark)
    assert isinstance(t_bg, float) and isinstance(t_x, float)
    # noise is at most 3.75 and must stay below, a centre is at least 39.75 and must lie above; a centre is at most
    # 20 + 4 + 15 + 40 - 20.25 = 58.75 and must be kept, an x-ray hit is 60000 - 20.25 and must go
    assert 3.75 <= t_bg < 39.75
    assert 58.75 <= t_x < 60000 - 20.25
    same(count_frames(frames, t_bg, t_x, dark=dark), (indptr, indices, np.ones(len(indices), np.uint8)))
    with pytest.raises(ValueError, match='background_sigma'):
        estimate_thresholds(frames, background_sigma=-1)
    with pytest.raises(ValueError, match='dark'):
        estimate_thresholds(frames, dark=dark[:5])
    with pytest.raises(ValueError, match='float64'):
        estimate_thresholds(frames.astype(np.float64))
    with pytest.raises(ValueError, match='shape'):
        estimate_thresholds(np.zeros((0, 4, 4), np.uint8))


def test_argument_errors_name_the_value():
    frames = np.zeros((2, 4, 5), np.uint16)
    with pytest.raises(ValueError, match=r'dark of shape \(4, 4\)'):
        count_frames(frames, 1, dark=np.zeros((4, 4)))
    with pytest.raises(ValueError, match=r'gain of shape \(5, 4\)'):
        count_frames(frames, 1, gain=np.zeros((5, 4)))
    with pytest.raises(ValueError, match='background_threshold nan'):
        count_frames(frames, np.nan)
    with pytest.raises(ValueError, match='xray_threshold nan'):
        count_frames(frames, 1, np.nan)
    with pytest.raises(ValueError, match="values 'sum'"):
        count_frames(frames, 1, values='sum')
    with pytest.raises(ValueError, match=r'\(2, 4, 5, 1\)'):
        count_frames(frames[..., None], 1)
    with pytest.raises(ValueError, match='float64'):
        count_frames(frames.astype(np.float64), 1)
    with pytest.raises(ValueError, match='uint64'):
        count_frames(frames.astype(np.uint64), 1)
    assert count_frames(frames[:0], 1)[0].tolist() == [0]


# ---- the UDFs and count_events on the inline executor ---------------------------------------------------------------
NAV, SIG, OFFSET = (5, 4), (24, 28), 3


@pytest.fixture(scope='module')
def scan():
    frames, dark, _ = electron_frames(20, SIG, 0.2, 11, xrays=2)
    return frames, dark


def expected_triple(frames, dark, values, offset=OFFSET):
    """count_frames of the whole array, the rows moved by the sync offset: position i holds frame i + offset"""
    n = len(frames)
    indptr, indices, data = count_frames(frames, 10, 1000, dark=dark, values=values)
    counts = np.zeros(n, np.int64)
    src = np.arange(n) + offset
    ok = (src >= 0) & (src < n)
    counts[ok] = np.diff(indptr)[src[ok]]
    lo, hi = indptr[src[ok][0]], indptr[src[ok][-1] + 1]
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64), indices[lo:hi], data[lo:hi]


@pytest.mark.parametrize('values', ('count', 'intensity'))
def test_count_events_writes_a_raw_csr_dataset(ctx, scan, tmp_path, values):
    from libertem_amd.udf.raw import PickUDF
    from libertem_amd.udf.sum import SumUDF
    frames, dark = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=3, sig_dims=2, sync_offset=OFFSET)
    path = str(tmp_path / 'counted.toml')
    res = count_events(ctx, ds, path, 10, 1000, dark=dark, values=values)
    indptr, indices, data = expected_triple(frames, dark, values)
    assert res['path'] == path and res['nnz'] == indptr[-1] > 0
    assert res['n_events'].dtype == np.int32 and res['n_events'].shape == NAV
    assert np.array_equal(res['n_events'].reshape(-1), np.diff(indptr))
    assert np.all(res['n_events'].reshape(-1)[-OFFSET:] == 0)            # positions without a frame
    for key, want in (('indptr', indptr.astype('<i8')), ('indices', indices.astype('<i4')), ('data', data)):
        with open(str(tmp_path / f'counted.{key}'), 'rb') as f:
            assert f.read() == want.tobytes(), key
    assert data.dtype == (np.uint8 if values == 'count' else np.float32)
    with open(path) as f:
        text = f.read()
    assert text == ('[params]\nfiletype = "raw_csr"\nnav_shape = [5, 4]\nsig_shape = [24, 28]\n\n[raw_csr]\n'
                    'indptr_file = "counted.indptr"\nindptr_dtype = "<i8"\nindices_file = "counted.indices"\n'
                    'indices_dtype = "<i4"\ndata_file = "counted.data"\n'
                    'data_dtype = "%s"\n' % ('|u1' if values == 'count' else '<f4'))
    counted = ctx.load('raw_csr', path=path)
    assert tuple(counted.shape) == NAV + SIG and counted.dtype == data.dtype
    images = cr.dense_event_images(indptr, indices, data, SIG)
    picked = ctx.run_udf(dataset=counted, udf=PickUDF(), roi=np.ones(NAV, dtype=bool))['intensity'].data
    assert np.array_equal(np.asarray(picked).reshape(images.shape), images)
    total = np.asarray(ctx.run_udf(dataset=counted, udf=SumUDF())['intensity'].data)
    # (integers, or a few float32 values below 2**7 with two fractional bits: the sums are exact in any order)
    assert np.array_equal(total.astype(np.float64), images.astype(np.float64).sum(axis=0))


def test_event_count_udf_alone(ctx, scan):
    frames, dark = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=3, sig_dims=2)
    got = ctx.run_udf(dataset=ds, udf=EventCountUDF(10, 1000, dark=dark))['n_events'].data
    assert got.dtype == np.int32 and got.shape == NAV
    assert np.array_equal(got.reshape(-1), np.diff(count_frames(frames, 10, 1000, dark=dark)[0]))
    roi = np.zeros(NAV, bool)
    roi[1, 1:3] = True
    part = ctx.run_udf(dataset=ds, udf=EventCountUDF(10, 1000, dark=dark), roi=roi)['n_events'].raw_data
    assert np.array_equal(np.asarray(part), got[roi])


def test_udf_errors(ctx, scan, tmp_path):
    frames, dark = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='dark of shape'):
        ctx.run_udf(dataset=ds, udf=EventCountUDF(10, dark=dark[:3]))
    with pytest.raises(ValueError, match='background_threshold'):
        ctx.run_udf(dataset=ds, udf=EventCountUDF(np.nan))
    with pytest.raises(ValueError, match="values 'both'"):
        count_events(ctx, ds, str(tmp_path / 'x.toml'), 10, values='both')
    ds64 = ctx.load('memory', data=frames.reshape(NAV + SIG).astype(np.float64), num_partitions=2, sig_dims=2)
    with pytest.raises(ValueError, match='float64'):
        ctx.run_udf(dataset=ds64, udf=EventCountUDF(10))
    ds3 = ctx.load('memory', data=frames.reshape((20, 2, 12, 28)), num_partitions=2, sig_dims=3)
    with pytest.raises(ValueError, match='2D frames'):
        ctx.run_udf(dataset=ds3, udf=EventCountUDF(10))


def test_store_refuses_a_roi_and_a_wrong_row_pointer(ctx, scan, tmp_path):
    frames, dark = scan
    ds = ctx.load('memory', data=frames.reshape(NAV + SIG), num_partitions=2, sig_dims=2)
    indptr, indices, data = count_frames(frames, 10, 1000, dark=dark)
    files = [str(tmp_path / 'a.indices'), str(tmp_path / 'a.data')]
    np.zeros(len(indices), '<i4').tofile(files[0])
    np.zeros(len(indices), 'u1').tofile(files[1])
    roi = np.zeros(NAV, bool)
    roi[2, 1:] = True
    with pytest.raises(RuntimeError, match='Recording with ROI is not supported.'):
        ctx.run_udf(dataset=ds, udf=EventStoreUDF(indptr, files[0], files[1], 'count', 10, 1000, dark=dark), roi=roi)
    ctx.run_udf(dataset=ds, udf=EventStoreUDF(indptr, files[0], files[1], 'count', 10, 1000, dark=dark))
    assert np.array_equal(np.fromfile(files[0], '<i4'), indices)
    wrong = indptr.copy()
    wrong[7] += 1
    with pytest.raises(RuntimeError, match='indptr does not fit'):
        ctx.run_udf(dataset=ds, udf=EventStoreUDF(wrong, files[0], files[1], 'count', 10, 1000, dark=dark))
    with pytest.raises(ValueError, match='indptr must be'):
        ctx.run_udf(dataset=ds, udf=EventStoreUDF(indptr[:-1], files[0], files[1], 'count', 10, 1000, dark=dark))
    with pytest.raises(ValueError, match='bytes'):
        ctx.run_udf(dataset=ds, udf=EventStoreUDF(indptr, files[0], files[0], 'count', 10, 1000, dark=dark))


# ---- header and binding ---------------------------------------------------------------------------------------------
def _declared_arguments(name):
    hdr = open(os.path.join(ROOT, 'include', 'ltmi.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, hdr)
    assert m, f"{name} is not declared in include/ltmi.h"
    args = m.group(1).strip()
    return 0 if args in ('', 'void') else len(args.split(','))


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_and_binding_agree(name):
    from libertem_amd import hip
    assert _declared_arguments(name) == ENTRIES[name]
    assert name in hip.EXPORTS
    assert len(getattr(hip.lib(), name).argtypes) == ENTRIES[name]


def test_strip_rows():
    from libertem_amd import hip
    assert hip.count_strip_rows(256, 256) == 30
    assert hip.count_strip_rows(5, 515) == 5
    assert hip.count_strip_rows(4096, 4096) == 1
    assert hip.count_strip_rows(100, 1000) == 3 * 4104 // 1008 - 2
    assert hip.count_strip_rows(10, 4097) == 0 and hip.count_strip_rows(0, 5) == 0
    assert hip.COUNT_MAX_WIDTH == 4096
