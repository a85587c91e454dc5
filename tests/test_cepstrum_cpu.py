"""
The cepstrum without a GPU: the NumPy branch (`cepstrum_frames`) against the index-by-index float64 restatement of the
definition (tests/cepstrum_ref.py) on every case of the kernel table, with and without a window and a cleared centre; a
frame whose cepstrum is known in closed form; `strained_lattice_scan` -- the cepstral peaks of 600 strained frames lie
at their lattice vectors --; CepstrumUDF on the inline executor with a region of interest and a sync offset;
`cepstrum_dataset` feeding SumUDF; the parameter errors; the names the feature adds.

The closed form: log(exp(2 + 0.5 cos(phi)) + 1e-30) = 2 + 0.5 cos(phi) to 1e-31, and the DFT of 2 + 0.5 cos(2 pi (3 i /
16 + 5 j / 20)) divided by h w is 2 at the origin and 0.25 at +-(3, 5).  The frame is float32: its rounding (6e-8
relative, on values up to 12.2) moves the logarithm by 6e-8 per pixel, white, so every quefrency by about 6e-8 /
sqrt(320): the bound of 1e-6 is 300 of those.
"""
import inspect

import numpy as np
import pytest

import cepstrum_ref as cr
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf import CepstrumUDF, cepstrum_dataset, cepstrum_frames, hann_window, run_cepstrum
from libertem_amd.udf.cepstrum import check_params, keep_mask
from libertem_amd.udf.sum import SumUDF
from libertem_amd.utils.generate import strained_lattice_scan


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


@pytest.mark.parametrize('dc_radius', [0.0, 2.5])
@pytest.mark.parametrize('windowed', [False, True], ids=['hann', 'window'])
@pytest.mark.parametrize('case', cr.CASES, ids=cr.case_id)
def test_numpy_branch_equals_restatement(case, windowed, dc_radius):
    sig, out_shape = case
    window = cr.window_for(case) if windowed else None
    for dtype in ('float32', 'int16'):
        frames = cr.noise_frames(sig, 3, dtype)
        ref = cr.reference(frames, out_shape, 0.75, window, dc_radius)
        got = cepstrum_frames(frames, out_shape, 0.75, window, dc_radius, dtype=np.float64)
        assert got.dtype == np.float64 and got.shape == (3,) + out_shape
        for f in range(3):
            assert np.abs(got[f] - ref[f]).max() <= 1e-12 * np.abs(ref[f]).max() or np.abs(ref[f]).max() == 0, f
        # the UDF's dtype: the same values, rounded once
        assert np.array_equal(cepstrum_frames(frames, out_shape, 0.75, window, dc_radius), got.astype(np.float32))
    # the cleared centre is exactly 0 and nothing else is
    k = cr.keep(out_shape, dc_radius)
    assert np.array_equal(keep_mask(out_shape, dc_radius), k)
    assert np.all(got[:, k == 0] == 0) and (dc_radius == 0 or k[out_shape[0] // 2, out_shape[1] // 2] == 0)


@pytest.mark.parametrize('sig', [(16, 12), (15, 17), (8, 9), (9, 8)])
def test_full_size_output_is_fftshift(sig):
    frames = cr.noise_frames(sig, 2, 'uint16')
    window = cr.window_for((sig, sig))
    z = np.log(frames.astype(np.float64) + 1.0) * window.astype(np.float64)
    expected = np.fft.fftshift(np.abs(np.fft.fft2(z)), axes=(1, 2)) / (sig[0] * sig[1])
    got = cepstrum_frames(frames, sig, 1.0, window, dtype=np.float64)
    assert np.allclose(got, expected, rtol=1e-12, atol=1e-12 * expected.max())


def test_exact_delta_frame():
    frame = cr.delta_frame()
    got = cepstrum_frames(frame[None], (16, 20), offset=1e-30, window='none', dtype=np.float64)[0]
    expected = np.zeros((16, 20))
    expected[8, 10] = 2.0
    expected[8 + 3, 10 + 5] = expected[8 - 3, 10 - 5] = 0.25
    assert np.abs(got - expected).max() < 1e-6
    # ... and the restatement says the same
    assert np.abs(cr.reference(frame[None], (16, 20), 1e-30, np.ones((16, 20), np.float32))[0] - expected).max() < 1e-6


def test_negative_pixels_count_as_zero():
    frames = cr.noise_frames((16, 16), 2, 'int16')
    assert (frames < 0).any()
    clipped = np.maximum(frames, 0)
    assert np.array_equal(cepstrum_frames(frames, (8, 8), 0.5), cepstrum_frames(clipped, (8, 8), 0.5))


def test_hann_window():
    for sig in ((16, 16), (15, 17), (1, 4)):
        win = hann_window(sig)
        assert win.dtype == np.float32 and win.shape == sig
        assert np.array_equal(win, cr.hann(sig))
        assert np.all(win[0] == 0) and np.all(win[:, 0] == 0)
    assert hann_window((8, 8))[4, 4] == 1.0


# ---- the lattice -------------------------------------------------------------------------------------------------------
def two_strongest(ceps, min_distance=3.0):
    """the two strongest elements of the upper half plane (qy > 0, or qy == 0 and qx > 0) that are at least
    `min_distance` apart -> [(qy, qx), (qy, qx)]"""
    oh, ow = ceps.shape
    qy = (np.arange(oh) - oh // 2)[:, None] + np.zeros((1, ow), int)
    qx = (np.arange(ow) - ow // 2)[None, :] + np.zeros((oh, 1), int)
    upper = (qy > 0) | ((qy == 0) & (qx > 0))
    order = np.argsort(np.where(upper, ceps, -1.0).reshape(-1))[::-1]
    first = order[0]
    y0, x0 = qy.reshape(-1)[first], qx.reshape(-1)[first]
    for cand in order[1:]:
        y1, x1 = qy.reshape(-1)[cand], qx.reshape(-1)[cand]
        if np.hypot(y1 - y0, x1 - x0) >= min_distance:
            return [(int(y0), int(x0)), (int(y1), int(x1))]
    raise AssertionError("no second maximum")


def into_upper(vec):
    y, x = int(vec[0]), int(vec[1])
    return (y, x) if (y > 0 or (y == 0 and x > 0)) else (-y, -x)


@pytest.mark.parametrize('sig,out_shape', [((64, 64), (32, 32)), ((48, 64), (24, 40)), ((33, 40), (21, 20))])
def test_strained_lattice_peaks(sig, out_shape):
    rng = np.random.default_rng(2020)
    strain = rng.uniform(-0.05, 0.05, (200, 2, 2))
    frames, a_n, b_n = strained_lattice_scan((200,), sig, a=(6, 1.5), b=(-1, 7), strain=strain)
    assert frames.shape == (200,) + sig and frames.dtype == np.uint16
    assert np.allclose(a_n, np.array([6, 1.5]) + strain @ np.array([6, 1.5]))
    assert np.allclose(b_n, np.array([-1, 7]) + strain @ np.array([-1, 7]))
    ceps = cepstrum_frames(frames, out_shape, dc_radius=3.5)
    coords = np.concatenate([a_n, b_n], axis=1)
    near = np.all(np.abs(coords - np.rint(coords)) <= 0.35, axis=1)
    assert near.sum() >= 10, near.sum()
    failed = []
    for f in np.flatnonzero(near):
        want = {into_upper(np.rint(a_n[f])), into_upper(np.rint(b_n[f]))}
        if set(two_strongest(ceps[f])) != want:
            failed.append(int(f))
    print(f"{sig} -> {out_shape}: {near.sum()} frames near integer peaks, {len(failed)} failed")
    assert not failed, failed


def test_strained_lattice_scan_values_and_errors():
    frames, a_n, b_n = strained_lattice_scan((2, 3), (8, 10), (2, 0), (0, 3), dtype='float64', counts=10.,
                                             modulation=0.25, envelope=0.5)
    assert frames.shape == (2, 3, 8, 10) and a_n.shape == b_n.shape == (2, 3, 2)
    assert np.all(a_n == (2, 0)) and np.all(b_n == (0, 3))
    i, j = 5, 7
    ry, rx = (i - 4) / 8, (j - 5) / 10
    expected = 10. * np.exp(-((ry / 0.5) ** 2 + (rx / 0.5) ** 2) / 2) \
        * np.exp(0.25 * (np.cos(2 * np.pi * 2 * ry) + np.cos(2 * np.pi * 3 * rx)))
    assert np.allclose(frames[:, :, i, j], expected, rtol=1e-14)
    as_int = strained_lattice_scan((2, 3), (8, 10), (2, 0), (0, 3), dtype='uint8', counts=10., modulation=0.25,
                                   envelope=0.5)[0]
    assert as_int.dtype == np.uint8 and np.array_equal(as_int, np.rint(frames))
    with pytest.raises(ValueError, match='strain of shape'):
        strained_lattice_scan((2, 3), (8, 10), (2, 0), (0, 3), strain=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='does not fit'):
        strained_lattice_scan((1,), (8, 8), (2, 0), (0, 3), counts=1000., dtype='uint8')
    with pytest.raises(ValueError, match='two vectors'):
        strained_lattice_scan((1,), (8, 8), (2, 0, 1), (0, 3))


# ---- the UDF -----------------------------------------------------------------------------------------------------------
SIG, NAV, OUT = (32, 20), (3, 4), (6, 9)


@pytest.fixture(scope='module')
def scan():
    frames = strained_lattice_scan(NAV, SIG, (5, 1), (-1, 4))[0]
    return frames, cepstrum_frames(frames.reshape((12,) + SIG), OUT, 2.0, None, 1.5)


def test_udf_equals_cepstrum_frames_roi_three_partitions(ctx, scan):
    frames, expected = scan
    ds = ctx.load('memory', data=frames, num_partitions=3, sig_dims=2)
    res = run_cepstrum(ctx, ds, OUT, offset=2.0, dc_radius=1.5)
    assert res['cepstrum'].data.shape == NAV + OUT and res['cepstrum'].data.dtype == np.float32
    assert np.array_equal(np.asarray(res['cepstrum'].data).reshape((12,) + OUT), expected)
    roi = np.zeros(NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[1, 3] = roi[2, 2] = roi[2, 3] = True
    part = run_cepstrum(ctx, ds, OUT, offset=2.0, dc_radius=1.5, roi=roi)
    got = np.asarray(part['cepstrum'].raw_data)
    assert got.shape == (5,) + OUT
    for i, r in enumerate(np.flatnonzero(roi.reshape(-1))):
        assert np.array_equal(got[i], expected[r]), (i, r)
    # a window of one's own, and none
    window = cr.window_for((SIG, OUT))
    res = ctx.run_udf(dataset=ds, udf=CepstrumUDF(OUT, window=window))
    assert np.array_equal(np.asarray(res['cepstrum'].data).reshape((12,) + OUT),
                          cepstrum_frames(frames.reshape((12,) + SIG), OUT, 1.0, window))
    res = ctx.run_udf(dataset=ds, udf=CepstrumUDF(OUT, window='none'))
    assert np.array_equal(np.asarray(res['cepstrum'].data).reshape((12,) + OUT),
                          cepstrum_frames(frames.reshape((12,) + SIG), OUT, 1.0, np.ones(SIG)))


@pytest.mark.parametrize('sync_offset', [2, -2])
def test_sync_offset(ctx, scan, sync_offset):
    frames, expected = scan
    ds = ctx.load('memory', data=frames, num_partitions=2, sig_dims=2, sync_offset=sync_offset)
    got = np.asarray(run_cepstrum(ctx, ds, OUT, offset=2.0, dc_radius=1.5)['cepstrum'].data).reshape((12,) + OUT)
    src = np.arange(12) + sync_offset
    valid = (src >= 0) & (src < 12)
    assert np.array_equal(got[valid], expected[src[valid]])
    assert np.all(got[~valid] == 0)                              # no frame, no result
    # ... and the dataset made of it holds zeros there
    cds = cepstrum_dataset(ctx, ds, OUT, offset=2.0, dc_radius=1.5)
    total = np.asarray(ctx.run_udf(dataset=cds, udf=SumUDF())['intensity'].data)
    assert np.allclose(total, expected[src[valid]].astype(np.float64).sum(axis=0), rtol=1e-6)


def test_cepstrum_dataset_feeds_sum_udf(ctx, scan):
    frames, expected = scan
    ds = ctx.load('memory', data=frames, num_partitions=3, sig_dims=2)
    cds = cepstrum_dataset(ctx, ds, OUT, offset=2.0, dc_radius=1.5)
    assert tuple(cds.shape) == NAV + OUT and tuple(cds.shape.sig) == OUT and cds.dtype == np.float32
    total = np.asarray(ctx.run_udf(dataset=cds, udf=SumUDF())['intensity'].data)
    assert total.shape == OUT
    assert np.allclose(total, expected.astype(np.float64).sum(axis=0), rtol=1e-6)
    assert total[OUT[0] // 2, OUT[1] // 2] == 0                  # (the cleared centre)


def test_value_errors(ctx):
    sig = (16, 12)
    ds = ctx.load('memory', data=np.ones((2, 2) + sig, np.float32), num_partitions=1, sig_dims=2)
    for out_shape in ((17, 6), (8, 13), (0, 6)):
        with pytest.raises(ValueError, match=r'out_shape \(%d, %d\)' % out_shape):
            run_cepstrum(ctx, ds, out_shape)
    with pytest.raises(ValueError, match='two integers'):
        run_cepstrum(ctx, ds, (3.5, 1))
    for offset in (0.0, -1.0, np.inf, np.nan, 1e-60):            # (1e-60 rounds to 0 as float32)
        with pytest.raises(ValueError, match='offset'):
            run_cepstrum(ctx, ds, (8, 6), offset=offset)
    with pytest.raises(ValueError, match=r'offset -1\.0'):
        run_cepstrum(ctx, ds, (8, 6), offset=-1.0)
    with pytest.raises(ValueError, match=r'window of shape \(16, 11\)'):
        run_cepstrum(ctx, ds, (8, 6), window=np.ones((16, 11), np.float32))
    with pytest.raises(ValueError, match='window must be real'):
        run_cepstrum(ctx, ds, (8, 6), window=np.ones(sig, np.complex64))
    with pytest.raises(ValueError, match="window 'hamming'"):
        run_cepstrum(ctx, ds, (8, 6), window='hamming')
    with pytest.raises(ValueError, match=r'dc_radius -0\.5'):
        run_cepstrum(ctx, ds, (8, 6), dc_radius=-0.5)
    with pytest.raises(ValueError, match='dc_radius'):
        run_cepstrum(ctx, ds, (8, 6), dc_radius=np.nan)
    ds3 = ctx.load('memory', data=np.zeros((3, 4, 8, 8), np.float32), num_partitions=1, sig_dims=3)
    with pytest.raises(ValueError, match='2D'):
        run_cepstrum(ctx, ds3, (4, 4))
    out_shape, offset, window, dc = check_params(sig, (8, 6), 0.1, None, 2)
    assert out_shape == (8, 6) and offset == np.float32(0.1) and isinstance(offset, np.float32) and dc == 2.0
    assert window.dtype == np.float32 and np.array_equal(window, hann_window(sig))


def test_udf_declarations():
    udf = CepstrumUDF((6, 9))
    assert udf.get_backends() == (udf.BACKEND_HIP, udf.BACKEND_NUMPY)
    assert udf.WHOLE_FRAME_TILES and udf.VALID_FRAMES_ONLY and udf.REUSE_TASK_INSTANCES
    assert udf.get_preferred_input_dtype() is udf.USE_NATIVE_DTYPE
    assert udf.get_dist_merge() == {'cepstrum': 'disjoint'}
    bufs = udf.get_result_buffers()
    assert {k: (b.kind, np.dtype(b.dtype), b.extra_shape) for k, b in bufs.items()} == {
        'cepstrum': ('nav', np.dtype('float32'), (6, 9))}
    assert udf.params.offset == 1.0 and udf.params.window is None and udf.params.dc_radius == 0.0


NEW_EXPORTS = ('ltmi_ceps_plan_create', 'ltmi_ceps_plan_destroy', 'ltmi_ceps_plan_last_kernel', 'ltmi_ceps_transform',
               'ltmi_ceps_load', 'ltmi_ceps_store')


def test_names():
    from libertem_amd import hip, udf
    from libertem_amd.build import SOURCES, header_exports
    assert 'ltmi_ceps.hip' in SOURCES
    declared = header_exports()
    for name in NEW_EXPORTS:
        assert name in hip.EXPORTS and name in declared
    assert sorted(n for n in hip.EXPORTS if n.startswith('ltmi_ceps')) == sorted(NEW_EXPORTS) == \
        sorted(n for n in declared if n.startswith('ltmi_ceps'))
    for name in ('CepstrumUDF', 'run_cepstrum', 'cepstrum_dataset', 'cepstrum_frames', 'hann_window'):
        assert name in udf.__all__ and hasattr(udf, name)
    assert list(inspect.signature(hip.CepstrumPlan.__init__).parameters) == [
        'self', 'device', 'sig_h', 'sig_w', 'out_h', 'out_w', 'max_batch', 'offset', 'window', 'dc_radius']
    assert list(inspect.signature(hip.CepstrumPlan.transform).parameters) == [
        'self', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'out_ptr', 'ld_out', 'stream']
    assert list(inspect.signature(hip.ceps_load).parameters) == [
        'device', 'tile_ptr', 'tile_dtype', 'n_frames', 'ld_tile', 'n_px', 'offset', 'window_ptr', 'out_ptr', 'stream']
    assert list(inspect.signature(hip.ceps_store).parameters) == [
        'device', 'spec_ptr', 'n_frames', 'h', 'w', 'ld_spec', 'out_h', 'out_w', 'scale_ptr', 'out_ptr', 'ld_out',
        'stream']
    assert list(inspect.signature(strained_lattice_scan).parameters) == [
        'nav_shape', 'sig_shape', 'a', 'b', 'strain', 'modulation', 'counts', 'envelope', 'dtype']


def test_store_rule_of_the_kernel_tests_against_the_restatement():
    # cepstrum_ref.store (the bit-exact model of k_ceps_store) applied to NumPy's half spectra gives the definition
    for case in cr.CASES:
        sig, out_shape = case
        frames = cr.noise_frames(sig, 2, 'uint16')
        window = cr.window_for(case)
        t = (cr.log_frames(frames, 1.0) * window.astype(np.float64)).astype(np.float32)
        spec = np.fft.rfft2(t.astype(np.float64)).astype(np.complex64)
        scale = (cr.keep(out_shape, 1.5) / (sig[0] * sig[1])).astype(np.float32)
        got = cr.store(spec, sig, out_shape, scale)
        cr.compare(got, cr.reference(frames, out_shape, 1.0, window, 1.5), frames, 1.0, window, what=cr.case_id(case))
