"""
`ltmi_correlate_peaks` on the MI355X through hip.CorrPlan, against the float64 restatement of the definition
(tests/correlation_ref.py): square, non-power-of-two and odd-width frames, three batches with a partial last one,
padded tile rows, the stored dtypes, one and seven peaks, windows clipped at every border and a corner, crop and
refine radii, an exact tie, a NaN pixel, guard bytes around all four results, bitwise repeats, no frames, error codes.

Tolerances (correlation_ref.compare): peak_values within C eps32 log2(h w) |y| |t| with C = 8; centers equal,
refineds within 0.02 px and peak_elevations within 1e-3 relative (or the value derived from that bound where it is
larger) for every (frame, peak) whose float64 top-two gap exceeds twice the bound; at most 2 % of the pairs below it.
"""
import numpy as np
import pytest

import correlation_ref as cr
import guarded

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NAMES = ('centers', 'refineds', 'peak_values', 'peak_elevations')


class Call:
    """one plan, a guarded tile and four guarded result buffers"""

    def __init__(self, frames, template, peaks, max_batch, pad=0):
        from libertem_amd import hip
        n, h, w = frames.shape
        self.n, self.k = n, len(peaks)
        self.dtype = frames.dtype
        self.plan = hip.CorrPlan(0, h, w, max_batch, template)
        fill = 'nan' if frames.dtype.kind == 'f' else 'max'
        self.tile = guarded.Region(n, h * w, h * w + pad, frames.dtype, init=frames.reshape((n, h * w)), fill=fill)
        self.peaks = torch.from_numpy(np.ascontiguousarray(peaks, dtype=np.int32).reshape(-1).copy()).cuda()
        k = self.k
        self.out = {'centers': guarded.Region(n, 2 * k, 2 * k, np.int32),
                    'refineds': guarded.Region(n, 2 * k, 2 * k, np.float32),
                    'peak_values': guarded.Region(n, k, k, np.float32),
                    'peak_elevations': guarded.Region(n, k, k, np.float32)}

    def run(self, r, q, **kw):
        args = dict(tile_ptr=self.tile.ptr, tile_dtype=self.dtype, n_frames=self.n, ld_tile=self.tile.ld,
                    peaks_ptr=self.peaks.data_ptr(), n_peaks=self.k, crop_radius=r, refine_radius=q,
                    centers_ptr=self.out['centers'].ptr, refineds_ptr=self.out['refineds'].ptr,
                    peak_values_ptr=self.out['peak_values'].ptr,
                    peak_elevations_ptr=self.out['peak_elevations'].ptr)
        args.update(kw)
        self.plan.correlate_peaks(**args)
        torch.cuda.synchronize()
        got = {}
        for name in NAMES:
            guarded.unchanged_outside(self.out[name], name)
            a = self.out[name].result()
            got[name] = a.reshape((self.n, self.k, 2)) if name in ('centers', 'refineds') else a
        guarded.unchanged(self.tile, 'tile')
        return got


@pytest.mark.parametrize('case', cr.KERNEL_CASES, ids=lambda c: c[0])
def test_kernel_vs_definition(case):
    _, sig, n, max_batch, dtype, _, r, q, pad, _ = case
    frames, template, peaks, r, q = cr.kernel_case(case)
    call = Call(frames, template, peaks, max_batch, pad)
    got = call.run(r, q)
    ref = cr.reference(frames, template, peaks, r, q)
    stats = cr.compare(got, ref, frames, template, q)
    print(case[0], stats)
    kern = call.plan.last_kernel()
    for name in (f'k_corr_load<{np.dtype(dtype).name}>', 'hipfft_r2c', 'k_corr_mul', 'hipfft_c2r', 'k_corr_peaks',
                 f'batch={max_batch}'):
        assert name in kern, kern
    # no atomics: a second call gives the same bytes
    again = call.run(r, q)
    for name in NAMES:
        assert got[name].tobytes() == again[name].tobytes(), name


def test_exact_tie_takes_the_first_position():
    # a zero frame: its correlation is exactly constant, every window is one tie
    sig = (32, 32)
    peaks = cr.border_peaks(sig)
    frames, _, _ = cr.make_frames(sig, peaks, 6, 4, seed=2, dtype='uint16')
    frames[2] = 0
    template = cr.disk_template(sig)
    got = Call(frames, template, peaks, 4).run(6, 2)
    first = np.stack([np.maximum(peaks[:, 0] - 6, 0), np.maximum(peaks[:, 1] - 6, 0)], axis=1)
    assert np.array_equal(got['centers'][2], first)
    assert np.array_equal(got['refineds'][2], first.astype(np.float32))
    assert np.all(got['peak_values'][2] == 0) and np.all(got['peak_elevations'][2] == 0)
    ref = cr.reference(frames, template, peaks, 6, 2)
    assert np.array_equal(ref['centers'][2], first) and np.array_equal(ref['refineds'][2], first)
    cr.compare(got, ref, frames, template, 2, skip_frames=[2])


def test_nan_pixel_marks_its_frame_only():
    sig = (36, 50)
    peaks = cr.border_peaks(sig)
    frames, _, _ = cr.make_frames(sig, peaks, 6, 5, seed=1, dtype='float32')
    frames[3, 20, 7] = np.nan
    template = cr.disk_template(sig)
    got = Call(frames, template, peaks, 2).run(6, 1)          # (frame 3 shares a batch with frame 2)
    assert np.all(np.isnan(got['peak_values'][3]))
    ref = cr.reference(frames, template, peaks, 6, 1)
    assert np.all(np.isnan(ref['peak_values'][3]))
    assert np.all(np.isfinite(got['peak_values'][[0, 1, 2, 4]]))
    cr.compare(got, ref, frames, template, 1, skip_frames=[3])


def test_no_frames_launches_nothing():
    sig = (32, 32)
    peaks = cr.border_peaks(sig)
    frames = np.zeros((0,) + sig, np.float32)
    call = Call(frames, cr.disk_template(sig), peaks, 4)
    got = call.run(6, 1)
    assert got['centers'].shape == (0, 7, 2)
    assert call.plan.last_kernel() == ''


def test_error_codes():
    from libertem_amd import hip
    sig = (32, 32)
    peaks = np.array([(5, 5), (20, 9)], np.int32)
    frames, _, _ = cr.make_frames(sig, peaks, 3, 2, seed=1)
    template = cr.disk_template(sig)
    call = Call(frames, template, peaks, 2)
    for kw in (dict(crop_radius=0), dict(refine_radius=0), dict(ld_tile=32 * 32 - 1), dict(n_frames=-1),
               dict(n_peaks=-1)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(3, 1, **kw)
    for bad in ((32, 5), (5, 32), (-1, 5), (5, -1)):
        outside = torch.from_numpy(np.array([(5, 5), bad], np.int32).reshape(-1)).cuda()
        with pytest.raises(ValueError, match=r'outside.*code -3'):
            call.run(3, 1, peaks_ptr=outside.data_ptr())
    for dt in (np.complex64, np.uint64):
        with pytest.raises(ValueError, match=r'code -2'):
            call.run(3, 1, tile_dtype=dt)
    for name in ('tile_ptr', 'peaks_ptr', 'centers_ptr', 'refineds_ptr', 'peak_values_ptr', 'peak_elevations_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(3, 1, **{name: None})
    with pytest.raises(ValueError, match=r'code -1'):
        hip.CorrPlan(0, 32, 32, 0, template)
    with pytest.raises(ValueError):
        hip.CorrPlan(0, 32, 30, 2, template)
    # nothing of that reached the results, and the plan still works
    got = call.run(3, 1)
    cr.compare(got, cr.reference(frames, template, peaks, 3, 1), frames, template, 1)


# ---- one plan, two streams; plans that go away --------------------------------------------------------------------------
STREAM_SIG = (24, 20)        # 5 frames in batches of 2: the partial last batch puts the zero-tail memset on the stream


def test_one_plan_on_two_streams():
    """One plan called on the default stream, on a second stream and on the default stream again, different frames each
    time, one synchronisation at the end (tests/plan_checks.py): both transforms, the conversion, the multiply, the
    memset of the tail and the peak kernel follow the stream of their call.  Every result is byte for byte what a fresh
    plan of the same arguments gives for the same frames on the default stream."""
    from libertem_amd import hip
    import plan_checks
    h, w = STREAM_SIG
    peaks = cr.border_peaks(STREAM_SIG)
    k = len(peaks)
    template = cr.disk_template(STREAM_SIG)
    sets = [cr.make_frames(STREAM_SIG, peaks, 4, 5, seed=40 + i, dtype='uint16')[0] for i in range(3)]
    tiles = [torch.from_numpy(s.view(np.int16).reshape(5, h * w)).cuda() for s in sets]
    dev_peaks = torch.from_numpy(peaks.reshape(-1).copy()).cuda()

    def buffers():
        return [torch.full((5, 2 * k), -7, dtype=torch.int32, device='cuda')] + \
               [torch.full((5, n), np.nan, dtype=torch.float32, device='cuda') for n in (2 * k, k, k)]

    def run(plan, tile, out, stream):
        plan.correlate_peaks(tile.data_ptr(), np.uint16, 5, h * w, dev_peaks.data_ptr(), k, 4, 1,
                             *[o.data_ptr() for o in out], stream=stream)

    outs = [buffers() for _ in range(3)]
    plan = hip.CorrPlan(0, h, w, 2, template)
    plan_checks.three_calls_on_two_streams(lambda i, stream: run(plan, tiles[i], outs[i], stream))
    plan.close()
    for i in range(3):
        fresh = hip.CorrPlan(0, h, w, 2, template)
        ref = buffers()
        run(fresh, tiles[i], ref, None)
        torch.cuda.synchronize()
        fresh.close()
        for name, got, want in zip(NAMES, outs[i], ref):
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (i, name)
        assert np.all(np.isfinite(ref[2].cpu().numpy()))


CORR_PLAN_BYTES = 33554432


def test_plans_go_away_completely():
    """64 plans made and closed in a row; free memory after cycle 64 less than ONE live plan below that after cycle 8
    (tests/plan_checks.py).  CORR_PLAN_BYTES = 33554432 bytes: torch.cuda.mem_get_info() before minus after one
    `hip.CorrPlan(0, 24, 20, 2, template)` on the MI355X, measured at the commit before `ltmi::FftHandle` (the
    plans then destroyed their hipFFT handles by hand); a second and a third plan made beside live ones cost the same."""
    from libertem_amd import hip
    import plan_checks
    template = cr.disk_template(STREAM_SIG)
    plan_checks.assert_plans_go_away(lambda: hip.CorrPlan(0, STREAM_SIG[0], STREAM_SIG[1], 2, template),
                                     CORR_PLAN_BYTES, 'CorrPlan')
