"""
`ltmi_ssb_gather`, `ltmi_ssb_trotter` and `ltmi_ssb_reconstruct` on the MI355X through hip.ssb_gather /
hip.ssb_trotter / hip.SSBPlan (csrc/ltmi_ssb.hip).

The gather EXACTLY (a conversion to float32 leaves no freedom): every tile dtype, padded rows, lists of 1, 63, 64, 65
and 167 entries that hold the first and the last pixel of the frame, an index outside the frame, 70 000 frames of
4 x 4 pixels (past the 65535 grid rows), no frames, guard values around tile and result.

The trotter step on half spectra made by np.fft.rfft2 here, against the restatement's masked sums
(tests/ssb_ref.py) at the tolerance of the holography tests: scans 12 x 10, 9 x 7, 1 x 16, 16 x 1 and 2 x 2, 167
listed pixels (one pass of the 256 threads) and 332 (two), cutoff 1 and 4, a geometry in which most Q have no overlap;
no listed pixel within 1e-6 of a rim; two calls give the same bytes.

The whole plan on the generic fixture's bright-field pixels: batches of 50 (three full ones and one of 17), 64, 167
and more, padded ld_bf, the kernels it reports, repeats; the error codes of all three entry points.
"""
import ctypes

import numpy as np
import pytest

import guarded
import ssb_ref as sr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DTYPES = ['bool', 'uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32', 'float64']


# ---- the gather ---------------------------------------------------------------------------------------------------------
def pixel_list(n_px, n_idx, seed):
    """n_idx distinct frame indices in random order; from two entries on, the first and the last pixel among them"""
    rng = np.random.default_rng([11, seed, n_px, n_idx])
    idx = rng.permutation(n_px)[:n_idx]
    if n_idx >= 2:
        idx = idx[(idx != 0) & (idx != n_px - 1)][:n_idx - 2]
        idx = rng.permutation(np.concatenate([idx, [0, n_px - 1]]))
    assert len(idx) == n_idx
    return idx.astype(np.int32)


class Gather:
    """a guarded tile, a guarded result and the list on the device"""

    def __init__(self, frames, idx, pad_tile=0, pad_out=0):
        n, self.n_px = frames.shape
        self.frames, self.idx_host = frames, idx
        fill = 'nan' if frames.dtype.kind == 'f' else ('zero' if frames.dtype.kind == 'b' else 'max')
        self.tile = guarded.Region(n, self.n_px, self.n_px + pad_tile, frames.dtype, init=frames, fill=fill)
        self.out = guarded.Region(n, len(idx), len(idx) + pad_out, np.float32)
        self.idx = torch.from_numpy(idx.copy()).cuda()

    def run(self, **kw):
        from libertem_amd import hip
        args = dict(device=0, tile_ptr=self.tile.ptr, tile_dtype=self.frames.dtype, n_frames=self.frames.shape[0],
                    ld_tile=self.tile.ld, n_px=self.n_px, idx_ptr=self.idx.data_ptr(), n_idx=len(self.idx_host),
                    out_ptr=self.out.ptr, ld_out=self.out.ld)
        args.update(kw)
        hip.ssb_gather(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.out, 'bf')
        guarded.unchanged(self.tile, 'tile')
        return self.out.result()


def typed_frames(dtype, n, n_px, seed=0):
    frames = guarded.real_frames(np.random.default_rng([3, seed, n, n_px]), dtype, (n, n_px))
    if np.dtype(dtype) == np.uint32:
        frames[0, :4] = [2 ** 32 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 24 + 1]
    return frames


@pytest.mark.parametrize('dtype', DTYPES)
def test_gather_every_dtype(dtype):
    from libertem_amd.udf.ssb import bf_pixels
    h, w = sr.GENERIC_SIG
    idx = bf_pixels((h, w), 7.3, 11.6, 14.2)
    assert len(idx) == 167
    frames = typed_frames(dtype, 5, h * w)
    got = Gather(frames, idx, pad_tile=3, pad_out=2).run()
    assert got.dtype == np.float32
    assert np.array_equal(got, frames[:, idx].astype(np.float32))


@pytest.mark.parametrize('pads', [(0, 0), (5, 3)], ids=['contiguous', 'padded'])
@pytest.mark.parametrize('n_idx', [1, 63, 64, 65, 257])
def test_gather_list_lengths(n_idx, pads):
    n_px = 24 * 28
    idx = pixel_list(n_px, n_idx, 1)
    frames = typed_frames('uint16', 3, n_px, seed=n_idx)
    got = Gather(frames, idx, *pads).run()
    assert np.array_equal(got, frames[:, idx].astype(np.float32))


def test_gather_past_the_grid_rows():
    n, n_px = 70000, 16
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (n, n_px)).astype(np.uint8)
    idx = np.array([15, 0, 6, 9, 3], np.int32)
    got = Gather(frames, idx, pad_out=1).run()
    assert np.array_equal(got, frames[:, idx].astype(np.float32))


def test_gather_index_outside_the_frame_reads_nothing():
    n_px = 40
    frames = typed_frames('float32', 4, n_px)
    idx = np.array([0, -1, 39, 40, 2 ** 31 - 1, -2 ** 31, 7], np.int32)
    got = Gather(frames, idx).run()                  # (the tile's surroundings hold NaN)
    expected = np.zeros((4, 7), np.float32)
    expected[:, [0, 2, 6]] = frames[:, [0, 39, 7]]
    assert np.array_equal(got, expected)


def test_gather_no_frames_and_error_codes():
    n_px = 24 * 28
    idx = pixel_list(n_px, 65, 2)
    empty = Gather(np.zeros((0, n_px), np.uint16), idx)
    assert empty.run().shape == (0, 65)
    call = Gather(typed_frames('int16', 3, n_px), idx)
    assert np.array_equal(call.run(n_idx=0).view(np.uint8), call.out.view(call.out.host).view(np.uint8))
    #                                                  (an empty list launches nothing: the poison is still there)
    for kw in (dict(ld_tile=n_px - 1), dict(ld_out=64), dict(n_frames=-1), dict(n_idx=-1), dict(n_px=0)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for dt in (np.complex64, np.uint64, np.int64):
        with pytest.raises(ValueError, match=r'code -2'):
            call.run(tile_dtype=dt)
    for name in ('tile_ptr', 'idx_ptr', 'out_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    assert np.array_equal(call.run(), call.frames[:, idx].astype(np.float32))


# ---- the trotter step ---------------------------------------------------------------------------------------------------
# (scan, frame shape, parameters): the generic geometry on five scans, a disk of 332 pixels cut by the frame's edge, a
# detector so coarse that only the lowest frequencies overlap
WIDE = dict(sr.GENERIC, semiconv_pix=10.3, semiconv=0.031)
COARSE = dict(sr.GENERIC, semiconv=0.0031)
TROTTER_CASES = [
    ((12, 10), sr.GENERIC_SIG, sr.GENERIC), ((9, 7), sr.GENERIC_SIG, sr.GENERIC), ((1, 16), sr.GENERIC_SIG, sr.GENERIC),
    ((16, 1), sr.GENERIC_SIG, sr.GENERIC), ((2, 2), sr.GENERIC_SIG, sr.GENERIC),
    ((12, 10), sr.GENERIC_SIG, WIDE), ((9, 7), sr.GENERIC_SIG, WIDE), ((12, 10), sr.GENERIC_SIG, COARSE),
]


def trotter_id(case):
    nav, _, params = case
    return f"{nav[0]}x{nav[1]}-" + ('wide' if params is WIDE else 'coarse' if params is COARSE else 'generic')


def half_spectra(nav, n_idx, seed):
    """float32 bright-field pixels (Ny Nx, P) with a mean like a detector's, and their complex64 half spectra
    (Ny, Nx // 2 + 1, P) over the scan axes"""
    rng = np.random.default_rng([21, seed, nav[0], nav[1], n_idx])
    bf = rng.poisson(40., (nav[0] * nav[1], n_idx)).astype(np.float32)
    spec = np.fft.rfft2(bf.reshape(nav + (n_idx,)).astype(np.float64), axes=(0, 1)).astype(np.complex64)
    return bf, spec


class Trotter:
    """guarded half spectra, a guarded result and the list on the device"""

    def __init__(self, case, cutoff, pad_spec=0):
        from libertem_amd import hip
        from libertem_amd.udf.ssb import bf_pixels
        self.nav, self.sig, params = case
        self.params = dict(params, cutoff=cutoff)
        self.p = sr.full_params(self.sig, **self.params)
        self.idx_host = bf_pixels(self.sig, self.p['semiconv_pix'], self.p['cy'], self.p['cx'])
        n_idx = len(self.idx_host)
        _, self.spec_host = half_spectra(self.nav, n_idx, cutoff)
        n_rows = self.nav[0] * (self.nav[1] // 2 + 1)
        self.spec = guarded.Region(n_rows, n_idx, n_idx + pad_spec, np.complex64,
                                   init=self.spec_host.reshape((n_rows, n_idx)), fill='nan')
        self.out = guarded.Region(1, self.nav[0] * self.nav[1], self.nav[0] * self.nav[1], np.complex64)
        self.idx = torch.from_numpy(self.idx_host.copy()).cuda()
        self.geom = hip.ssb_geometry(self.p['lamb'], (self.p['dy'], self.p['dx']), self.p['semiconv'],
                                     self.p['semiconv_pix'], self.p['cy'], self.p['cx'], self.p['t'])

    def run(self, **kw):
        from libertem_amd import hip
        args = dict(device=0, spec_ptr=self.spec.ptr, ld_spec=self.spec.ld, nav_y=self.nav[0], nav_x=self.nav[1],
                    idx_ptr=self.idx.data_ptr(), n_idx=len(self.idx_host), sig_w=self.sig[1], geom=self.geom,
                    cutoff=self.p['cutoff'], fourier_ptr=self.out.ptr)
        args.update(kw)
        hip.ssb_trotter(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.out, 'fourier')
        guarded.unchanged(self.spec, 'spec')
        return self.out.result().reshape(self.nav)

    def reference(self):
        return sr.masked_sums(self.spec_host, self.sig, self.nav, self.idx_host, **self.params)


@pytest.mark.parametrize('cutoff', [1, 4])
@pytest.mark.parametrize('case', TROTTER_CASES, ids=trotter_id)
def test_trotter_vs_masked_sums(case, cutoff):
    call = Trotter(case, cutoff, pad_spec=3 if cutoff == 4 else 0)
    assert sr.rim_margin(call.sig, call.nav, call.p) >= 1e-6
    n_idx = len(call.idx_host)
    assert n_idx == (332 if case[2] is WIDE else 167)
    ref = call.reference()
    got = call.run()
    assert got.dtype == np.complex64
    sr.assert_fourier(got, ref, f"{trotter_id(case)} cutoff {cutoff}")
    # a Q the rule sets to zero is zero exactly, and nothing else is
    assert np.array_equal(got == 0, ref == 0)
    if case[2] is COARSE:
        assert 0 < (ref != 0).sum() < ref.size // 2
    # no atomics: a second call gives the same bytes
    assert call.run().tobytes() == got.tobytes()


def test_trotter_cutoff_branches_and_nyquist():
    call = Trotter(TROTTER_CASES[0], 4)
    ref = call.reference()
    assert (ref == 0).sum() == 7                           # both branches of the cutoff rule
    got = call.run()
    # the Nyquist row and column are computed from their own shift, not mirrored
    for q in ((6, 0), (6, 3), (0, 5), (2, 5)):
        assert ref[q] != 0 and abs(got[q] - ref[q]) <= 1e-5 * np.abs(ref).max(), q


def test_trotter_error_codes():
    call = Trotter(TROTTER_CASES[0], 4)
    n_idx = len(call.idx_host)
    bad_geom = []
    for i in range(5):                                     # lamb, dy, dx, semiconv, semiconv_pix: positive
        g = call.geom.copy()
        g[i] = 0.
        bad_geom.append(g)
    g = call.geom.copy()
    g[8] = np.nan
    bad_geom.append(g)
    for kw in [dict(nav_y=0), dict(nav_x=-1), dict(nav_y=1, nav_x=1), dict(n_idx=0), dict(sig_w=0), dict(cutoff=0), dict(ld_spec=n_idx - 1)] + \
            [dict(geom=g) for g in bad_geom]:
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for name in ('spec_ptr', 'idx_ptr', 'fourier_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    with pytest.raises(ValueError, match='11 values'):
        call.run(geom=call.geom[:10])
    sr.assert_fourier(call.run(), call.reference(), 'after the errors')


# ---- the plan -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def generic():
    """the generic fixture's bright-field pixels (120, 167) float32, the list, the restatement's fourier"""
    from libertem_amd.udf.ssb import bf_pixels
    frames = sr.generic_frames()
    idx = bf_pixels(sr.GENERIC_SIG, 7.3, 11.6, 14.2)
    bf = np.ascontiguousarray(frames.reshape(120, -1)[:, idx], dtype=np.float32)      # (a fancy index may return F order)
    return bf, idx, sr.reference(frames, **sr.GENERIC)['fourier']


def generic_geom():
    from libertem_amd import hip
    p = sr.full_params(sr.GENERIC_SIG, **sr.GENERIC)
    return hip.ssb_geometry(p['lamb'], (p['dy'], p['dx']), p['semiconv'], p['semiconv_pix'], p['cy'], p['cx'], p['t'])


@pytest.mark.parametrize('max_batch,pad', [(50, 0), (64, 5), (167, 0), (1000, 3), (1, 0)])
def test_reconstruct_batches(generic, max_batch, pad):
    from libertem_amd import hip
    bf_host, idx, ref = generic
    plan = hip.SSBPlan(0, 12, 10, 28, idx, max_batch, generic_geom(), 4)
    assert plan.last_kernel() == ''
    bf = guarded.Region(120, 167, 167 + pad, np.float32, init=bf_host, fill='nan')
    out = guarded.Region(1, 120, 120, np.complex64)

    def run():
        plan.reconstruct(bf.ptr, bf.ld, out.ptr)
        torch.cuda.synchronize()
        guarded.unchanged_outside(out, 'fourier')
        guarded.unchanged(bf, 'bf')
        return out.result().reshape(12, 10)

    got = run()
    sr.assert_fourier(got, ref, f"plan batch {max_batch}")
    assert np.array_equal(got == 0, ref == 0)
    assert plan.last_kernel() == f'k_transpose<4> + hipfft_r2c + k_transpose<8> + k_ssb_trotter batch={min(max_batch, 167)}'
    assert run().tobytes() == got.tobytes()
    plan.close()


def test_reconstruct_line_scans():
    # scans of one row and of one column: batched 1D transforms, the column as a row with the axes exchanged
    from libertem_amd import hip
    from libertem_amd.udf.ssb import bf_pixels
    idx = bf_pixels(sr.GENERIC_SIG, 7.3, 11.6, 14.2)
    for nav in ((1, 16), (16, 1), (1, 9), (7, 1), (1, 2), (2, 1)):
        rng = np.random.default_rng([31, nav[0], nav[1]])
        frames = rng.poisson(40., nav + sr.GENERIC_SIG).astype(np.uint16)
        p = sr.full_params(sr.GENERIC_SIG, **sr.GENERIC)
        assert sr.rim_margin(sr.GENERIC_SIG, nav, p) >= 1e-6
        ref = sr.reference(frames, **sr.GENERIC)['fourier']
        plan = hip.SSBPlan(0, nav[0], nav[1], 28, idx, 60, generic_geom(), 4)
        bf = torch.from_numpy(np.ascontiguousarray(frames.reshape(nav[0] * nav[1], -1)[:, idx], dtype=np.float32)).cuda()
        out = torch.empty(nav, dtype=torch.complex64, device='cuda')
        plan.reconstruct(bf.data_ptr(), 167, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        sr.assert_fourier(got, ref, f"plan {nav}")
        assert np.array_equal(got == 0, ref == 0)
        plan.close()


def test_reconstruct_error_codes(generic):
    from libertem_amd import hip
    bf_host, idx, ref = generic
    geom = generic_geom()
    plan = hip.SSBPlan(0, 12, 10, 28, idx, 50, geom, 4)
    bf = torch.from_numpy(bf_host).cuda()
    out = torch.empty((12, 10), dtype=torch.complex64, device='cuda')
    with pytest.raises(ValueError, match=r'code -3'):
        plan.reconstruct(bf.data_ptr(), 166, out.data_ptr())
    with pytest.raises(ValueError, match=r'null.*code -1'):
        plan.reconstruct(None, 167, out.data_ptr())
    with pytest.raises(ValueError, match=r'null.*code -1'):
        plan.reconstruct(bf.data_ptr(), 167, None)
    zero = geom.copy()
    zero[3] = 0.
    for args in ((0, 10, 28, idx, 50, geom, 4), (12, -1, 28, idx, 50, geom, 4), (12, 10, 0, idx, 50, geom, 4),
                 (12, 10, 28, idx[:0], 50, geom, 4), (1, 1, 28, idx, 50, geom, 4), (12, 10, 28, idx, 50, geom, 0), (12, 10, 28, idx, 50, zero, 4),
                 (46341, 46341, 28, idx, 1, geom, 4)):
        with pytest.raises(ValueError, match=r'code -3'):
            hip.SSBPlan(0, *args)
    with pytest.raises(ValueError, match=r'code -1'):
        hip.SSBPlan(0, 12, 10, 28, idx, 0, geom, 4)
    with pytest.raises(ValueError, match='11 values'):
        hip.SSBPlan(0, 12, 10, 28, idx, 50, geom[:7], 4)
    handle = ctypes.c_void_p()
    gp = geom.ctypes.data_as(ctypes.c_void_p)
    ip = idx.ctypes.data_as(ctypes.c_void_p)
    assert hip.lib().ltmi_ssb_plan_create(0, 12, 10, 28, None, 167, 50, gp, 4, ctypes.byref(handle)) == -1
    assert hip.lib().ltmi_ssb_plan_create(0, 12, 10, 28, ip, 167, 50, None, 4, ctypes.byref(handle)) == -1
    assert hip.lib().ltmi_ssb_plan_create(0, 12, 10, 28, ip, 167, 50, gp, 4, None) == -1
    assert not handle.value
    assert hip.lib().ltmi_ssb_reconstruct(None, bf.data_ptr(), 167, out.data_ptr(), None) == -1
    # nothing of that reached the plan, and it still works
    plan.reconstruct(bf.data_ptr(), 167, out.data_ptr())
    torch.cuda.synchronize()
    sr.assert_fourier(out.cpu().numpy(), ref, 'after the errors')
    plan.close()
    # ... and the creates that failed left nothing that keeps a new plan from working
    after = hip.SSBPlan(0, 12, 10, 28, idx, 50, geom, 4)
    out.zero_()
    after.reconstruct(bf.data_ptr(), 167, out.data_ptr())
    torch.cuda.synchronize()
    sr.assert_fourier(out.cpu().numpy(), ref, 'a plan made after the errors')
    after.close()


def test_one_plan_on_two_streams(generic):
    """One plan called on the default stream, on a second stream and on the default stream again, different scans each
    time, one synchronisation at the end (tests/plan_checks.py); the generic fixture's 167 pixels in batches of 50, so
    the sums of a Q wait in the accumulator between the batches.  Every result is byte for byte what a fresh plan of the
    same arguments gives for the same scan on the default stream."""
    from libertem_amd import hip
    import plan_checks
    bf_host, idx, _ = generic
    rng = np.random.default_rng(70)
    sets = [bf_host] + [rng.poisson(40., bf_host.shape).astype(np.float32) for _ in range(2)]
    bfs = [torch.from_numpy(s).cuda() for s in sets]
    geom = generic_geom()

    def run(plan, bf, out, stream):
        plan.reconstruct(bf.data_ptr(), 167, out.data_ptr(), stream=stream)

    outs = [torch.full((12, 10), np.nan, dtype=torch.complex64, device='cuda') for _ in range(3)]
    plan = hip.SSBPlan(0, 12, 10, 28, idx, 50, geom, 4)
    plan_checks.three_calls_on_two_streams(lambda i, stream: run(plan, bfs[i], outs[i], stream))
    plan.close()
    for i in range(3):
        fresh = hip.SSBPlan(0, 12, 10, 28, idx, 50, geom, 4)
        ref = torch.full((12, 10), np.nan, dtype=torch.complex64, device='cuda')
        run(fresh, bfs[i], ref, None)
        torch.cuda.synchronize()
        fresh.close()
        assert outs[i].cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), i
        assert np.all(np.isfinite(ref.cpu().numpy()))


SSB_PLAN_BYTES = 16777216


def test_plans_go_away_completely(generic):
    """64 plans made and closed in a row; free memory after cycle 64 less than ONE live plan below that after cycle 8
    (tests/plan_checks.py).  SSB_PLAN_BYTES = 16777216 bytes: torch.cuda.mem_get_info() before minus after one
    `hip.SSBPlan(0, 12, 10, 28, idx, 50, geom, 4)` on the MI355X, measured at the commit before `ltmi::FftHandle` (the
    plans then destroyed their hipFFT handles by hand); a second and a third plan made beside live ones cost the same."""
    from libertem_amd import hip
    import plan_checks
    _, idx, _ = generic
    geom = generic_geom()
    plan_checks.assert_plans_go_away(lambda: hip.SSBPlan(0, 12, 10, 28, idx, 50, geom, 4), SSB_PLAN_BYTES, 'SSBPlan')
