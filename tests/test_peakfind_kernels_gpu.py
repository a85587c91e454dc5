"""
`ltmi_find_peaks_maps` and `ltmi_correlate_find` on the MI355X against the brute-force restatement of the definition
(tests/peakfind_ref.py).

The search alone runs on float32 maps the test supplies, so every decision of steps 1 - 3 is exact: n_found and centers
must EQUAL the restatement's, peak_values the map's bits; refineds within 0.02 px and peak_elevations within 1e-3
relative (tests/correlation_ref.py).  Maps: constant, maxima in the four corners, on every edge and inside the border
strip, equal values next to each other, d and d + 1 apart across the boundaries of the kernel's (d+1)^2 cells and of
its runs of cell rows, a relative threshold exactly on a value, a plateau, a NaN and an Inf between finite frames,
quantised noise full of ties; 32 x 32, 33 x 35 and 48 x 40 (edges that are no multiple of d + 1, of 64 or of 4);
d = 1, 2, 5 and beyond the frame; 1 and 7 frames; padded ld_map; N = 1, 7, more than found, 130; more passing
candidates than the selection ranks in one go.  Guard bytes around the maps and all five results, bitwise repeats, no
frames, error codes.

Through `CorrPlan.find_peaks`: the stored dtypes, three batches with a partial last one, padded tile rows; on the
seeded frames (all decided: tests/test_peakfind_cpu.py) n_found and centers equal the float64 restatement's and
peak_values lie within correlation_ref's bound; `correlate_peaks` at a frame's found centres with crop_radius = d gives
the same centres and bit-equal peak_values, refineds and peak_elevations.
"""
import numpy as np
import pytest

import correlation_ref as cr
import guarded
import peakfind_ref as pr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NAMES = pr.NAMES
KERNELS = ('k_pf_cells', 'k_pf_verify', 'k_pf_select', 'k_corr_found')


def result_regions(n, k):
    return {'n_found': guarded.Region(n, 1, 1, np.int32), 'centers': guarded.Region(n, 2 * k, 2 * k, np.int32),
            'refineds': guarded.Region(n, 2 * k, 2 * k, np.float32), 'peak_values': guarded.Region(n, k, k, np.float32),
            'peak_elevations': guarded.Region(n, k, k, np.float32)}


def read_results(out, n, k):
    got = {}
    for name in NAMES:
        guarded.unchanged_outside(out[name], name)
        a = out[name].result()
        got[name] = a.reshape(n) if name == 'n_found' else \
            a.reshape((n, k, 2)) if name in ('centers', 'refineds') else a
    return got


class MapCall:
    """guarded float32 maps and five guarded result buffers for one num_peaks"""

    def __init__(self, maps, num_peaks, pad=0):
        n, h, w = maps.shape
        self.n, self.h, self.w, self.k = n, h, w, num_peaks
        self.maps = guarded.Region(n, h * w, h * w + pad, np.float32, init=maps.reshape((n, h * w)), fill='nan')
        self.out = result_regions(n, num_peaks)

    def run(self, p, **kw):
        from libertem_amd import hip
        assert p['num_peaks'] == self.k
        args = dict(device=0, maps_ptr=self.maps.ptr, n_frames=self.n, h=self.h, w=self.w, ld_map=self.maps.ld,
                    n_found_ptr=self.out['n_found'].ptr, centers_ptr=self.out['centers'].ptr,
                    refineds_ptr=self.out['refineds'].ptr, peak_values_ptr=self.out['peak_values'].ptr,
                    peak_elevations_ptr=self.out['peak_elevations'].ptr, **p)
        args.update(kw)
        hip.find_peaks_maps(**args)
        torch.cuda.synchronize()
        got = read_results(self.out, self.n, self.k)
        guarded.unchanged(self.maps, 'maps')
        return got


def check_exact(got, ref, maps):
    """decisions equal, values the map's bits, statistics within correlation_ref's tolerances, empty slots empty"""
    assert np.array_equal(got['n_found'], ref['n_found']), (got['n_found'], ref['n_found'])
    assert np.array_equal(got['centers'], ref['centers'])
    n, k = got['peak_values'].shape
    found = np.arange(k)[None] < got['n_found'][:, None]
    f, s = np.nonzero(found)
    at = maps[f, got['centers'][f, s, 0], got['centers'][f, s, 1]]
    assert got['peak_values'][f, s].tobytes() == at.astype(np.float32).tobytes()
    assert np.all(np.isnan(got['peak_values'][~found])) and np.all(np.isnan(got['peak_elevations'][~found]))
    assert np.all(np.isnan(got['refineds'][~found])) and np.all(got['centers'][~found] == -1)
    e_ref = np.abs(got['refineds'][f, s].astype(np.float64) - ref['refineds'][f, s])
    assert e_ref.size == 0 or e_ref.max() <= pr.REFINED_TOL, e_ref.max()
    e_el = np.abs(got['peak_elevations'][f, s].astype(np.float64) - ref['peak_elevations'][f, s])
    assert np.all(e_el <= pr.ELEVATION_RTOL * np.abs(ref['peak_elevations'][f, s])), e_el.max()


def run_and_check(maps, p, pad=0):
    call = MapCall(maps, p['num_peaks'], pad)
    got = call.run(p)
    check_exact(got, pr.reference(maps, **p), maps)
    again = call.run(p)                                      # no atomics: a second call gives the same bytes
    for name in NAMES:
        assert got[name].tobytes() == again[name].tobytes(), name
    return got


@pytest.mark.parametrize('d', [1, 2, 5])
@pytest.mark.parametrize('sig', pr.MAP_SIGS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_special_maps(sig, d):
    from libertem_amd import hip
    maps = pr.special_maps(sig, d)
    got = run_and_check(maps, pr.params(20, d, threshold_abs=-1.0))
    assert got['n_found'][0] == 1 and tuple(got['centers'][0, 0]) == (0, 0)       # the constant map
    assert got['n_found'][1] == 10 and got['n_found'][5] == 10                     # corners, edges, strip, middle
    assert got['n_found'][4] == 0 and got['n_found'][6] == 0                       # NaN, Inf
    for name in KERNELS:
        assert name in hip.find_peaks_last_kernel()
    run_and_check(maps, pr.params(7, d, border=3), pad=5)
    run_and_check(maps, pr.params(1, d, refine_radius=2), pad=1)
    rel = run_and_check(maps, pr.params(20, d, threshold_rel=0.5, refine_radius=3))
    kept = list(rel['peak_values'][3, :rel['n_found'][3]])
    assert 4.0 in kept and 2.0 not in kept                                         # 4 is not below 0.5 * 8
    run_and_check(maps[2:3], pr.params(20, d), pad=3)                              # one frame


@pytest.mark.parametrize('d', [1, 2, 5])
@pytest.mark.parametrize('sig', pr.MAP_SIGS, ids=lambda s: f'{s[0]}x{s[1]}')
def test_quantised_maps(sig, d):
    maps = pr.quantised_maps(sig, 7, seed=10 * sig[0] + d)
    got = run_and_check(maps, pr.params(130, d, threshold_abs=-5.0), pad=7)
    assert np.all(got['n_found'] >= 1)
    run_and_check(maps[:1], pr.params(7, d, border=3, threshold_abs=1.0, threshold_rel=0.75))


def test_130_peaks_and_distances_beyond_the_frame():
    rng = np.random.default_rng(8)
    maps = rng.normal(size=(2, 48, 40)).astype(np.float32)
    got = run_and_check(maps, pr.params(130, 1, threshold_abs=-10.0))
    assert np.all(got['n_found'] == 130)                     # more than a wave, fewer than there are candidates
    special = pr.special_maps((48, 40), 40)
    for d in (40, 47, 48, 5000):                             # two cells, one cell, the clamp
        far = run_and_check(special, pr.params(3, d, threshold_abs=-1.0))
        assert list(far['n_found']) == [1, 1, 1, 1, 0, 1, 0]


def test_more_candidates_than_one_ranking_takes():
    # 7225 peaks pass: the selection first finds the 130th largest key by bisection
    maps = pr.comb_map()
    got = run_and_check(maps, pr.params(130, 1))
    assert got['n_found'][0] == 130
    assert np.array_equal(got['peak_values'][0], np.arange(7225, 7225 - 130, -1, dtype=np.float32))


def test_no_frames_and_error_codes():
    maps = pr.special_maps((32, 32), 2)
    empty = MapCall(maps[:0], 5)
    got = empty.run(pr.params(5, 2))
    assert got['centers'].shape == (0, 5, 2)
    call = MapCall(maps, 5)
    p = pr.params(5, 2)
    for kw in (dict(num_peaks=0), dict(num_peaks=1025), dict(min_distance=0), dict(refine_radius=0), dict(border=-1),
               dict(border=16), dict(threshold_rel=1.5), dict(threshold_rel=-0.5), dict(threshold_rel=np.nan),
               dict(threshold_abs=np.nan), dict(ld_map=32 * 32 - 1), dict(n_frames=-1), dict(h=0), dict(w=-3),
               dict(w=8193)):
        call.k = kw.get('num_peaks', 5)
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(dict(p, **{k: v for k, v in kw.items() if k in p}), **{k: v for k, v in kw.items() if k not in p})
    call.k = 5
    for name in ('maps_ptr', 'n_found_ptr', 'centers_ptr', 'refineds_ptr', 'peak_values_ptr', 'peak_elevations_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(p, **{name: None})
    # nothing of that reached the results, and the search still works
    check_exact(call.run(p), pr.reference(maps, **p), maps)


# ---- through the plan: transforms and search ------------------------------------------------------------------------
class PlanCall:
    """one plan, a guarded tile, five guarded results for the search and four for correlate_peaks"""

    def __init__(self, frames, tmpl, num_peaks, max_batch, pad=0):
        from libertem_amd import hip
        n, h, w = frames.shape
        self.n, self.k, self.dtype = n, num_peaks, frames.dtype
        self.plan = hip.CorrPlan(0, h, w, max_batch, tmpl)
        fill = 'nan' if frames.dtype.kind == 'f' else 'max'
        self.tile = guarded.Region(n, h * w, h * w + pad, frames.dtype, init=frames.reshape((n, h * w)), fill=fill)
        self.out = result_regions(n, num_peaks)

    def find(self, p, **kw):
        args = dict(tile_ptr=self.tile.ptr, tile_dtype=self.dtype, n_frames=self.n, ld_tile=self.tile.ld,
                    n_found_ptr=self.out['n_found'].ptr, centers_ptr=self.out['centers'].ptr,
                    refineds_ptr=self.out['refineds'].ptr, peak_values_ptr=self.out['peak_values'].ptr,
                    peak_elevations_ptr=self.out['peak_elevations'].ptr, **p)
        args.update(kw)
        self.plan.find_peaks(**args)
        torch.cuda.synchronize()
        got = read_results(self.out, self.n, self.k)
        guarded.unchanged(self.tile, 'tile')
        return got

    def correlate(self, peaks, r, q):
        k = len(peaks)
        dev = torch.from_numpy(np.ascontiguousarray(peaks, dtype=np.int32).reshape(-1).copy()).cuda()
        out = {name: region for name, region in result_regions(self.n, k).items() if name != 'n_found'}
        self.plan.correlate_peaks(self.tile.ptr, self.dtype, self.n, self.tile.ld, dev.data_ptr(), k, r, q,
                                  out['centers'].ptr, out['refineds'].ptr, out['peak_values'].ptr,
                                  out['peak_elevations'].ptr)
        torch.cuda.synchronize()
        return {name: region.result().reshape((self.n, k, 2) if name in ('centers', 'refineds') else (self.n, k))
                for name, region in out.items()}


@pytest.mark.parametrize('case', pr.PLAN_CASES, ids=lambda c: c[0])
def test_plan_vs_definition_and_correlate_peaks(case):
    _, sig, n, max_batch, dtype, pad, _, _ = case
    frames, tmpl, p = pr.plan_case(case)
    call = PlanCall(frames, tmpl, p['num_peaks'], max_batch, pad)
    got = call.find(p)
    maps64 = np.stack([cr.correlation(f, tmpl) for f in frames])
    ref = pr.reference(maps64, **p)
    assert np.array_equal(got['n_found'], ref['n_found']), (got['n_found'], ref['n_found'])
    assert np.array_equal(got['centers'], ref['centers'])
    found = np.arange(p['num_peaks'])[None] < got['n_found'][:, None]
    assert found.sum() > 0
    bound = cr.value_bound(frames, tmpl)[:, None] * np.ones((1, p['num_peaks']))
    err = np.abs(got['peak_values'].astype(np.float64) - ref['peak_values'])
    ratio = (err[found] / bound[found]).max()
    print(f"{case[0]}: largest |device - float64| / B for peak_values = {ratio:.4f}")
    assert ratio <= 1.0, ratio
    assert np.abs(got['refineds'].astype(np.float64) - ref['refineds'])[found].max() <= pr.REFINED_TOL
    e_el = np.abs(got['peak_elevations'].astype(np.float64) - ref['peak_elevations'])[found]
    assert np.all(e_el <= pr.ELEVATION_RTOL * np.abs(ref['peak_elevations'][found]))
    assert np.all(got['centers'][~found] == -1) and np.all(np.isnan(got['peak_values'][~found]))
    kern = call.plan.last_kernel()
    for name in (f'k_corr_load<{np.dtype(dtype).name}>', 'hipfft_r2c', 'k_corr_mul', 'hipfft_c2r',
                 f'batch={max_batch}') + KERNELS:
        assert name in kern, kern
    again = call.find(p)
    for name in NAMES:
        assert got[name].tobytes() == again[name].tobytes(), name
    # the same plan, the whole tile, frame f's centres as the peak list, crop_radius = d: frame f's row is the same
    for f in range(n):
        k = int(got['n_found'][f])
        at = call.correlate(got['centers'][f, :k], p['min_distance'], p['refine_radius'])
        assert np.array_equal(at['centers'][f], got['centers'][f, :k])
        for name in ('peak_values', 'refineds', 'peak_elevations'):
            assert at[name][f].tobytes() == got[name][f, :k].tobytes(), (f, name)


def test_plan_nonfinite_frames_and_errors():
    frames, tmpl, p = pr.plan_case(pr.PLAN_CASES[3])         # float32, batches of 2
    frames = frames.copy()
    frames[1, 20, 7] = np.nan                                # (shares a batch with frame 0)
    frames[4, 3, 3] = np.inf
    call = PlanCall(frames, tmpl, p['num_peaks'], 2)
    got = call.find(p)
    assert got['n_found'][1] == 0 and got['n_found'][4] == 0
    assert np.all(got['centers'][[1, 4]] == -1) and np.all(np.isnan(got['refineds'][[1, 4]]))
    ok = [0, 2, 3]
    ref = pr.reference(np.stack([cr.correlation(frames[f], tmpl) for f in ok]), **p)
    assert np.array_equal(got['n_found'][ok], ref['n_found']) and np.array_equal(got['centers'][ok], ref['centers'])
    for kw in (dict(num_peaks=0), dict(min_distance=0), dict(border=16), dict(threshold_rel=2.0),
               dict(ld_tile=32 * 32 - 1), dict(n_frames=-1)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.find(dict(p, **{k: v for k, v in kw.items() if k in p}),
                      **{k: v for k, v in kw.items() if k not in p})
    with pytest.raises(ValueError, match=r'code -2'):
        call.find(p, tile_dtype=np.complex64)
    with pytest.raises(ValueError, match=r'null.*code -1'):
        call.find(p, n_found_ptr=None)
    none = PlanCall(frames[:0], tmpl, p['num_peaks'], 2)
    assert none.find(p)['centers'].shape == (0, p['num_peaks'], 2) and none.plan.last_kernel() == ''


def test_find_peaks_one_plan_on_two_streams():
    """`CorrPlan.find_peaks` of one plan on the default stream, on a second stream and on the default stream again,
    different frames each time, one synchronisation at the end (tests/plan_checks.py); 24 x 20 frames, 5 of them in
    batches of 2, so the memset of the tail runs too.  Every result is byte for byte what a fresh plan of the same
    arguments gives for the same frames on the default stream."""
    from libertem_amd import hip
    import plan_checks
    h, w = sig = (24, 20)
    tmpl = pr.template(sig)
    sets = [pr.make_frames(sig, 5, 50 + i, dtype='uint16')[0] for i in range(3)]
    p = pr.params(6, 2, threshold_abs=pr.threshold_for(sets[0], tmpl))
    k = p['num_peaks']
    tiles = [torch.from_numpy(s.view(np.int16).reshape(5, h * w)).cuda() for s in sets]

    def buffers():
        return [torch.full((5, n), -7, dtype=torch.int32, device='cuda') for n in (1, 2 * k)] + \
               [torch.full((5, n), np.inf, dtype=torch.float32, device='cuda') for n in (2 * k, k, k)]

    def run(plan, tile, out, stream):
        plan.find_peaks(tile.data_ptr(), np.uint16, 5, h * w, p['num_peaks'], p['min_distance'], p['border'],
                        p['threshold_abs'], p['threshold_rel'], p['refine_radius'], *[o.data_ptr() for o in out],
                        stream=stream)

    outs = [buffers() for _ in range(3)]
    plan = hip.CorrPlan(0, h, w, 2, tmpl)
    plan_checks.three_calls_on_two_streams(lambda i, stream: run(plan, tiles[i], outs[i], stream))
    plan.close()
    for i in range(3):
        fresh = hip.CorrPlan(0, h, w, 2, tmpl)
        ref = buffers()
        run(fresh, tiles[i], ref, None)
        torch.cuda.synchronize()
        fresh.close()
        for name, got, want in zip(NAMES, outs[i], ref):
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (i, name)
        assert np.all(ref[0].cpu().numpy() >= 1)                 # (something was found in every frame)
