"""
The routes behind `hip.CorrPlan`, `hip.find_peaks_maps` and `hip.HoloPlan` at frame counts beyond the first step of
everything in them that depends on the frame count:

    a  CorrPlan.correlate_peaks  70 000 x (8, 8) uint8, one batch         k_corr_load: more frames than grid rows
    b  CorrPlan.correlate_peaks  524 300 x (8, 8) uint8, one batch        k_corr_mul: more groups of 8 than grid rows
    c  find_peaks_maps           70 000 x (8, 8), d = 1, N = 3            chunks of 32 768 maps: three, the last partial
    d  find_peaks_maps           16 400 x (64, 64), d = 1, N = 7          chunks of 2^24 / 1024 cells = 16 384 maps: two
    e  CorrPlan.find_peaks       the tile of (a), one batch               k_corr_load, then three search chunks
    f  holo_crop                 70 000 half spectra (8, 5) -> (4, 4)     second round of k_holo_crop's frame loop
    g  HoloPlan.reconstruct      70 000 x (8, 8) uint8 -> (4, 4)          k_corr_load, both k_holo_store<REF>

The float64 restatements are per-frame Python loops, so every tile is drawn from a pool of 61 distinct members
(correlation_ref.pool_index: seeded, 61 is prime; the first and the last frame, the frames on both sides of grid row
65 535 and those on both sides of each chunk boundary hold a member that differs from both neighbours').  The
restatement runs on the pool once, and frame f is held to what it gives for member idx[f] -- EVERY frame, with the
per-member bounds sent through idx: a skipped, repeated or shifted frame index shows, and a frame that no kernel wrote
keeps the poison of its guarded.Region.  Each case runs twice and gives the same bytes.

(c), (d) and (f) are exact.  (a), (b), (e) and (g) use the bounds their routes have (correlation_ref.compare and
holo_ref.compare with C = 8, peakfind_ref.REFINED_TOL / ELEVATION_RTOL), and no (frame, peak) pair is left out: the
pool is decided by the reference alone (tests/test_correlation_cpu.py, tests/test_peakfind_cpu.py).
"""
import time

import numpy as np
import pytest

import correlation_ref as cr
import holo_ref as hr
import peakfind_ref as pr
from test_correlation_kernels_gpu import NAMES as CORR_NAMES, Call as CorrCall
from test_holo_kernels_gpu import Call as HoloCall, Crop
from test_peakfind_kernels_gpu import KERNELS, NAMES as FIND_NAMES, MapCall, PlanCall, check_exact

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N = 70000                                # more than 65 535 grid rows, more than two search chunks of 32 768
N_MUL = 524300                           # more than 65 535 groups of 8 frames: 524 280 + two full groups + 4 frames
N_CELLS = 16400                          # 64 x 64, d = 1: 1024 cells a map, chunks of 2^24 / 1024 = 16 384 maps
CHUNK_EDGES = (32767, 32768, 65535, 65536)


def same_bytes(first, again, names):
    for name in names:
        assert first[name].tobytes() == again[name].tobytes(), name


@pytest.fixture(scope='module')
def corr_pool():
    """the 8 x 8 pool, its template and what the restatements give for it, computed once"""
    frames, tmpl, search = pr.pool_case()
    maps64 = np.stack([cr.correlation(f, tmpl) for f in frames])
    return dict(frames=frames, template=tmpl, bound=cr.value_bound(frames, tmpl),
                peaks=cr.reference(frames, tmpl, cr.POOL_PEAKS, cr.POOL_R, cr.POOL_Q),
                search=search, found=pr.reference(maps64, **search))


def correlate(corr_pool, n, extra, pad):
    t0 = time.perf_counter()
    idx = cr.pool_index(n, extra)
    call = CorrCall(corr_pool['frames'][idx], corr_pool['template'], cr.POOL_PEAKS, n, pad)
    got = call.run(cr.POOL_R, cr.POOL_Q)
    stats = cr.compare(got, cr.through(corr_pool['peaks'], idx), None, None, cr.POOL_Q, bound=corr_pool['bound'][idx],
                       max_skipped=0.0)
    assert stats['skipped'] == 0
    kern = call.plan.last_kernel()
    for name in ('k_corr_load<uint8>', 'hipfft_r2c', 'k_corr_mul', 'hipfft_c2r', 'k_corr_peaks', f'batch={n}'):
        assert name in kern, kern
    same_bytes(got, call.run(cr.POOL_R, cr.POOL_Q), CORR_NAMES)
    print(f"correlate_peaks {n} frames, ld_tile {call.tile.ld}: {stats}, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize('pad', [3, 0], ids=['scalar-loads', 'vector-loads'])
def test_a_correlate_peaks_more_frames_than_grid_rows(corr_pool, pad):
    correlate(corr_pool, N, (), pad)


def test_b_correlate_peaks_more_multiply_groups_than_grid_rows(corr_pool):
    # groups 65 535, 65 536 and 65 537 (the last one of 4 frames) are the second round of grid rows 0, 1 and 2
    correlate(corr_pool, N_MUL, (8 * cr.GRID_ROWS - 1, 8 * cr.GRID_ROWS, 8 * cr.GRID_ROWS + 8, N_MUL - 5, N_MUL - 4), 0)


# (threshold_abs 4.5 on the values -2 .. 6 of the 8 x 8 maps: 0, 1, 2 and 3 peaks found, about a quarter of the maps each)
@pytest.mark.parametrize('sig,seed,n,num_peaks,threshold_abs,pad,extra',
                         [pr.POOL_MAPS[0] + (N, 3, 4.5, 5, CHUNK_EDGES),
                          pr.POOL_MAPS[1] + (N_CELLS, 7, -5.0, 0, (16383, 16384))],
                         ids=['c-8x8-chunks-of-32768', 'd-64x64-chunks-of-16384'])
def test_cd_find_peaks_maps_in_chunks(sig, seed, n, num_peaks, threshold_abs, pad, extra):
    from libertem_amd import hip
    t0 = time.perf_counter()
    pool = pr.pool_maps(sig, seed)
    p = pr.params(num_peaks, 1, threshold_abs=threshold_abs)
    ref = pr.reference(pool, **p)
    assert ref['n_found'][7] == int(1.5 > threshold_abs) and ref['n_found'][23] == 0
    assert ref['n_found'].max() == num_peaks
    t1 = time.perf_counter()
    idx = cr.pool_index(n, extra)
    maps = pool[idx]
    call = MapCall(maps, num_peaks, pad)
    got = call.run(p)
    check_exact(got, cr.through(ref, idx), maps)
    for name in KERNELS:
        assert name in hip.find_peaks_last_kernel()
    same_bytes(got, call.run(p), FIND_NAMES)
    print(f"find_peaks_maps {n} maps of {sig}: reference of the pool {t1 - t0:.2f} s, "
          f"device and checks {time.perf_counter() - t1:.2f} s")


def test_e_find_peaks_three_search_chunks_in_one_batch(corr_pool):
    t0 = time.perf_counter()
    p = corr_pool['search']
    k = p['num_peaks']
    idx = cr.pool_index(N, CHUNK_EDGES)
    call = PlanCall(corr_pool['frames'][idx], corr_pool['template'], k, N, 3)
    got = call.find(p)
    ref = cr.through(corr_pool['found'], idx)
    assert np.array_equal(got['n_found'], ref['n_found'])
    assert np.array_equal(got['centers'], ref['centers'])
    found = np.arange(k)[None] < got['n_found'][:, None]
    assert found.any(axis=1).all()
    bound = corr_pool['bound'][idx][:, None] * np.ones((1, k))
    err = np.abs(got['peak_values'].astype(np.float64) - ref['peak_values'])
    ratio = (err[found] / bound[found]).max()
    print(f"find_peaks {N} frames: largest |device - float64| / B for peak_values = {ratio:.4f}")
    assert ratio <= 1.0, ratio
    assert np.abs(got['refineds'].astype(np.float64) - ref['refineds'])[found].max() <= pr.REFINED_TOL
    e_el = np.abs(got['peak_elevations'].astype(np.float64) - ref['peak_elevations'])[found]
    assert np.all(e_el <= pr.ELEVATION_RTOL * np.abs(ref['peak_elevations'][found]))
    assert np.all(got['centers'][~found] == -1) and np.all(np.isnan(got['peak_values'][~found]))
    assert np.all(np.isnan(got['refineds'][~found])) and np.all(np.isnan(got['peak_elevations'][~found]))
    kern = call.plan.last_kernel()
    for name in ('k_corr_load<uint8>', 'hipfft_r2c', 'k_corr_mul', 'hipfft_c2r', f'batch={N}') + KERNELS:
        assert name in kern, kern
    same_bytes(got, call.find(p), FIND_NAMES)
    print(f"find_peaks {N} frames: {time.perf_counter() - t0:.2f} s")


def test_f_holo_crop_second_round_of_the_frame_loop():
    t0 = time.perf_counter()
    sig, out_shape, sb = case = hr.POOL_CASE
    pool = hr.pool_spectra()
    idx = cr.pool_index(N)
    call = Crop(case, N, 3, 2, spec_host=pool[idx])
    got = call.run()
    ref = hr.gather(pool, sig, out_shape, sb, call.aperture_host)[idx]
    assert got.dtype == np.complex64
    assert got.tobytes() == ref.tobytes(), np.argwhere(got.view(np.uint64) != ref.view(np.uint64))[:4]
    assert call.run().tobytes() == got.tobytes()
    print(f"holo_crop {N} spectra: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize('with_reference,pad_tile', [(False, 0), (True, 3)], ids=['plain-vector-loads', 'ref-scalar-loads'])
def test_g_reconstruct_more_frames_than_grid_rows(with_reference, pad_tile):
    t0 = time.perf_counter()
    sig, out_shape, sb = case = hr.POOL_CASE
    pool = hr.pool_frames()
    idx = cr.pool_index(N)
    frames = pool[idx]
    call = HoloCall(case, frames, N, pad_tile, 2, with_reference)
    got = call.run()
    ref = hr.reference(pool, out_shape, sb, call.aperture, call.reference_wave)[idx]
    ratio = hr.compare(got, ref, frames, call.aperture, call.reference_wave, what=f"{N} frames")
    assert call.plan.last_kernel() == \
        f'k_corr_load<uint8> + hipfft_r2c + k_holo_crop + hipfft_c2c + k_holo_store batch={N}'
    assert call.run().tobytes() == got.tobytes()
    print(f"reconstruct {N} frames, reference wave {with_reference}: ratio {ratio:.4f}, "
          f"{time.perf_counter() - t0:.2f} s")

