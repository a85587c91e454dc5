"""
`ltmi_wdd_filter`, `ltmi_wdd_dot`, `ltmi_wdd_finish` and `ltmi_wdd_reconstruct` on the MI355X through hip.wdd_filter /
hip.wdd_dot / hip.wdd_finish / hip.WDDPlan (csrc/ltmi_wdd.hip), with guard values around every input and result.

The filter alone against the restatement's F (tests/wdd_ref.py `filters`): the windows (16, 16), (16, 18) and (20, 16),
scans 12 x 10, 9 x 7, 1 x 16, 16 x 1 and 2 x 2, Q batches of 7 over 120 Qs (17 full ones and one of 1), a range of Qs
inside the scan, a geometry in which most Qs have no overlap (F = 0 exactly).  Tolerance: rtol 1e-5 and atol 1e-5
max|F|, unless the float32 restatement reaches a quarter of that (then 8 x its error).

The dot product alone on half spectra made by np.fft.rfft2 here and random complex64 filters, against a complex128 sum
(`dot`): 256 window pixels (one pass of the 256 threads) and 288 (two), padded leading dimensions, one call and two
calls over a split pixel range, scans with Nyquist rows and columns, the mirrored half.  The products of two float32
are exact in float64, so device and NumPy differ by the rounding of at most 288 additions each:
2 * 288 * 2^-53 sum|G||F| < 1e-13 sum|G||F|.

The plan on the generic fixture's window pixels: batches of 100 (two full, one of 56), of P = 167, of 256 = By Bx and more, padded
ld_bf, the kernels it reports, repeats byte for byte, line scans, every error code.
"""
import ctypes

import numpy as np
import pytest

import guarded
import ssb_ref as sr
import wdd_ref as wr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG = sr.GENERIC_SIG
COARSE = dict(wr.GENERIC, semiconv=0.0031)
EPS = wr.GENERIC_EPSILON


def geometry(params):
    from libertem_amd import hip
    p = sr.full_params(SIG, **params)
    return p, hip.ssb_geometry(p['lamb'], (p['dy'], p['dx']), p['semiconv'], p['semiconv_pix'], p['cy'], p['cx'], p['t'])


# ---- the filter ---------------------------------------------------------------------------------------------------------
# (scan, window, parameters, Qs per hipFFT execution)
FILTER_CASES = [
    ((12, 10), (16, 16), wr.GENERIC, 7), ((12, 10), (16, 18), wr.GENERIC, 7), ((12, 10), (20, 16), wr.GENERIC, 7),
    ((12, 10), (16, 18), wr.GENERIC, 1000), ((9, 7), (16, 18), wr.GENERIC, 16), ((1, 16), (20, 16), wr.GENERIC, 5),
    ((16, 1), (16, 16), wr.GENERIC, 5), ((2, 2), (16, 18), wr.GENERIC, 3), ((12, 10), (16, 18), COARSE, 7),
]


def filter_id(case):
    nav, window, params, q_batch = case
    return f"{nav[0]}x{nav[1]}-{window[0]}x{window[1]}-b{q_batch}" + ('-coarse' if params is COARSE else '')


class Filter:
    """a guarded result (n_q, By Bx) and the arguments of hip.wdd_filter"""

    def __init__(self, nav, window, params, q_batch, q0=0, n_q=None):
        self.nav, self.params = nav, params
        self.p, self.geom = geometry(params)
        self.window = wr.window_origin(self.p, window)
        self.n_k = window[0] * window[1]
        self.q0, self.n_q = q0, nav[0] * nav[1] if n_q is None else n_q
        self.q_batch = q_batch
        self.out = guarded.Region(self.n_q, self.n_k, self.n_k, np.complex64)

    def run(self, **kw):
        from libertem_amd import hip
        args = dict(device=0, nav_y=self.nav[0], nav_x=self.nav[1], window=self.window, geom=self.geom, epsilon=EPS,
                    q0=self.q0, n_q=self.n_q, q_batch=self.q_batch, filter_ptr=self.out.ptr)
        args.update(kw)
        hip.wdd_filter(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.out, 'F')
        return self.out.result()

    def reference(self, single=False):
        f = wr.filters(SIG, self.nav, self.window[2:], EPS, single=single, **self.params)
        return f.reshape(self.nav[0] * self.nav[1], self.n_k)[self.q0:self.q0 + self.n_q]


@pytest.mark.parametrize('case', FILTER_CASES, ids=filter_id)
def test_filter_vs_restatement(case):
    call = Filter(*case)
    assert sr.rim_margin(SIG, call.nav, call.p) >= 1e-6
    ref = call.reference()
    got = call.run()
    assert got.dtype == np.complex64
    wr.assert_filter(got, ref, call.reference(single=True), filter_id(case))
    # a Q without overlap is zero exactly, and no other Q is
    empty = np.all(ref == 0, axis=1)
    assert np.array_equal(np.all(got == 0, axis=1), empty)
    if case[2] is COARSE:
        assert 0 < (~empty).sum() < empty.size // 2
    # a second call gives the same bytes
    assert call.run().tobytes() == got.tobytes()


def test_filter_of_a_range_of_qs():
    whole = Filter((12, 10), (16, 18), wr.GENERIC, 7).run()
    part = Filter((12, 10), (16, 18), wr.GENERIC, 7, q0=13, n_q=30)        # four batches and one of 2
    assert part.run().tobytes() == whole[13:43].tobytes()
    nothing = Filter((12, 10), (16, 18), wr.GENERIC, 7, q0=120, n_q=0)
    assert nothing.run().shape == (0, 288)


def test_filter_error_codes():
    call = Filter((12, 10), (16, 18), wr.GENERIC, 7)
    bad_geom = []
    for i in range(5):                                     # lamb, dy, dx, semiconv, semiconv_pix: positive
        g = call.geom.copy()
        g[i] = 0.
        bad_geom.append(g)
    g = call.geom.copy()
    g[8] = np.nan
    bad_geom.append(g)
    y0, x0, by, bx = call.window
    for kw in [dict(nav_y=0), dict(nav_x=-1), dict(nav_y=1, nav_x=1, n_q=1), dict(window=(y0, x0, 0, bx)),
               dict(window=(y0, x0, by, -1)), dict(window=(0, 0, 2, 2)),       # (no pixel of the disk: P = 0)
               dict(epsilon=0.), dict(epsilon=-1.), dict(epsilon=np.nan), dict(epsilon=np.inf),
               dict(q0=-1), dict(q0=100, n_q=21), dict(n_q=-1)] + [dict(geom=g) for g in bad_geom]:
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    with pytest.raises(ValueError, match=r'code -1'):
        call.run(q_batch=0)
    with pytest.raises(ValueError, match=r'null.*code -1'):
        call.run(filter_ptr=None)
    with pytest.raises(ValueError, match='4 values'):
        call.run(window=(y0, x0, by))
    with pytest.raises(ValueError, match='11 values'):
        call.run(geom=call.geom[:10])
    wr.assert_filter(call.run(), call.reference(), call.reference(single=True), 'after the errors')


# ---- the dot product ----------------------------------------------------------------------------------------------------
class Dot:
    """guarded half spectra (Ny Nxc, K), a guarded filter (Ny Nx, K) and a guarded accumulator (Ny Nx, 2)"""

    def __init__(self, nav, n_k, pad_spec=0, pad_filt=0):
        self.nav, self.n_k = nav, n_k
        n = nav[0] * nav[1]
        rng = np.random.default_rng([41, nav[0], nav[1], n_k])
        bf = rng.poisson(40., (n, n_k)).astype(np.float32)
        self.spec_host = np.fft.rfft2(bf.reshape(nav + (n_k,)).astype(np.float64), axes=(0, 1)).astype(np.complex64)
        self.filt_host = (rng.normal(size=(n, n_k)) + 1j * rng.normal(size=(n, n_k))).astype(np.complex64)
        n_rows = nav[0] * (nav[1] // 2 + 1)
        self.spec = guarded.Region(n_rows, n_k, n_k + pad_spec, np.complex64,
                                   init=self.spec_host.reshape(n_rows, n_k), fill='nan')
        self.filt = guarded.Region(n, n_k, n_k + pad_filt, np.complex64, init=self.filt_host, fill='nan')
        self.acc = guarded.Region(n, 2, 2, np.float64)

    def run(self, k0=0, n_k=None, first=True, **kw):
        from libertem_amd import hip
        n_k = self.n_k if n_k is None else n_k
        args = dict(device=0, spec_ptr=self.spec.ptr + 8 * k0, ld_spec=self.spec.ld, nav_y=self.nav[0],
                    nav_x=self.nav[1], filter_ptr=self.filt.ptr, ld_filter=self.filt.ld, k0=k0, n_k=n_k,
                    acc_ptr=self.acc.ptr, first=first)
        args.update(kw)
        hip.wdd_dot(**args)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.acc, 'acc')
        guarded.unchanged(self.spec, 'spec')
        guarded.unchanged(self.filt, 'F')
        return self.acc.result().view(np.complex128).reshape(self.nav)

    def reference(self):
        filt = self.filt_host.reshape(self.nav + (self.n_k,))
        ref = wr.dot(self.spec_host, filt, self.nav)
        full = np.abs(wr.dot(np.abs(self.spec_host), np.abs(filt), self.nav))
        return ref, full


@pytest.mark.parametrize('n_k,pads', [(256, (0, 0)), (288, (0, 0)), (288, (3, 5))], ids=['256', '288', '288-padded'])
@pytest.mark.parametrize('nav', [(12, 10), (9, 7), (1, 16), (16, 1), (2, 2)], ids=str)
def test_dot_vs_complex128(nav, n_k, pads):
    call = Dot(nav, n_k, *pads)
    ref, scale = call.reference()
    got = call.run()
    err = np.abs(got - ref)
    print(f"{nav} {n_k}: max error {err.max():.3e}, {(err / scale).max():.3e} of sum|G||F|")
    assert np.all(err <= 1e-13 * scale)
    # the Nyquist row and column read their own spectra, the mirrored half the conjugates
    for q in ((nav[0] // 2, 0), (0, nav[1] // 2), (nav[0] - 1, nav[1] - 1)):
        assert abs(got[q] - ref[q]) <= 1e-13 * scale[q], q
    # no atomics: a second call gives the same bytes
    assert call.run().tobytes() == got.tobytes()
    # the pixel range in two calls: the sums of the first wait in the accumulator
    call.run(k0=0, n_k=100, first=True)
    split = call.run(k0=100, n_k=n_k - 100, first=False)
    assert np.all(np.abs(split - ref) <= 1e-13 * scale)
    assert call.run(k0=100, n_k=n_k - 100, first=False).tobytes() != split.tobytes()      # (it accumulates)


def test_finish_mirrors_conjugates_and_normalises():
    from libertem_amd import hip
    for nav in ((12, 10), (9, 7), (1, 16), (16, 1), (2, 2)):
        rng = np.random.default_rng([43, nav[0], nav[1]])
        sums = rng.normal(size=nav) + 1j * rng.normal(size=nav)
        acc = guarded.Region(nav[0] * nav[1], 2, 2, np.float64, init=sums.reshape(-1, 1).view(np.float64), fill='nan')
        out = guarded.Region(1, nav[0] * nav[1], nav[0] * nav[1], np.complex64)
        hip.wdd_finish(0, acc.ptr, nav[0], nav[1], 288, out.ptr)
        torch.cuda.synchronize()
        guarded.unchanged_outside(out, 'fourier')
        guarded.unchanged(acc, 'acc')
        got = out.result().reshape(nav)
        ref = wr.finish(sums, 288)
        # float64 throughout, one cast: half an ulp of complex64 per component, and a few of float64
        assert np.all(np.abs(got - ref) <= 1e-7 * np.abs(ref)), nav
    # all-zero sums: 0 / 0
    acc = guarded.Region(4, 2, 2, np.float64, init=np.zeros((4, 2)), fill='nan')
    out = guarded.Region(1, 4, 4, np.complex64)
    hip.wdd_finish(0, acc.ptr, 2, 2, 16, out.ptr)
    assert np.all(np.isnan(out.result()))


def test_dot_and_finish_error_codes():
    from libertem_amd import hip
    call = Dot((12, 10), 288, 3, 5)
    ref, scale = call.reference()
    for kw in (dict(nav_y=0), dict(nav_x=-1), dict(k0=-1), dict(n_k=0), dict(ld_spec=287), dict(ld_filter=287),
               dict(k0=6, ld_filter=293)):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for name in ('spec_ptr', 'filter_ptr', 'acc_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    assert np.all(np.abs(call.run() - ref) <= 1e-13 * scale)
    out = torch.empty(120, dtype=torch.complex64, device='cuda')
    for args in ((0, 10, 288), (12, 0, 288), (12, 10, 0)):
        with pytest.raises(ValueError, match=r'code -3'):
            hip.wdd_finish(0, call.acc.ptr, *args, out.data_ptr())
    with pytest.raises(ValueError, match=r'null.*code -1'):
        hip.wdd_finish(0, None, 12, 10, 288, out.data_ptr())
    with pytest.raises(ValueError, match=r'null.*code -1'):
        hip.wdd_finish(0, call.acc.ptr, 12, 10, 288, None)


# ---- the plan -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def generic():
    """window -> (the generic fixture's window pixels (120, By Bx) float32, the restatement's fourier)"""
    from libertem_amd.udf.wdd import window_pixels
    frames = sr.generic_frames()
    out = {}
    for window in wr.WINDOWS:
        idx = window_pixels(SIG, window, 11.6, 14.2)
        bf = np.ascontiguousarray(frames.reshape(120, -1)[:, idx], dtype=np.float32)
        out[window] = (bf, wr.reference(frames, window, EPS, **wr.GENERIC)['fourier'])
    return out


def make_plan(window, max_batch, nav=(12, 10), params=wr.GENERIC, epsilon=EPS):
    from libertem_amd import hip
    p, geom = geometry(params)
    return hip.WDDPlan(0, nav[0], nav[1], wr.window_origin(p, window), max_batch, geom, epsilon)


@pytest.mark.parametrize('window,max_batch,pad', [((16, 16), 100, 0), ((16, 16), 167, 0), ((16, 16), 256, 5), ((16, 16), 1000, 0),
                                                  ((16, 18), 100, 3), ((20, 16), 64, 0), ((16, 18), 1, 0)])
def test_reconstruct_batches(generic, window, max_batch, pad):
    bf_host, ref = generic[window]
    n_k = window[0] * window[1]
    plan = make_plan(window, max_batch)
    assert plan.last_kernel() == ''
    bf = guarded.Region(120, n_k, n_k + pad, np.float32, init=bf_host, fill='nan')
    out = guarded.Region(1, 120, 120, np.complex64)

    def run():
        plan.reconstruct(bf.ptr, bf.ld, out.ptr)
        torch.cuda.synchronize()
        guarded.unchanged_outside(out, 'fourier')
        guarded.unchanged(bf, 'bf')
        return out.result().reshape(12, 10)

    got = run()
    wr.assert_fourier(got, ref, f"plan {window} batch {max_batch}")
    assert np.array_equal(got == 0, ref == 0) and (ref == 0).sum() == 7
    assert plan.last_kernel() == \
        f'k_transpose<4> + hipfft_r2c + k_transpose<8> + k_wdd_dot + k_wdd_finish batch={min(max_batch, n_k)}'
    assert run().tobytes() == got.tobytes()
    plan.close()


def test_reconstruct_line_scans():
    # scans of one row and of one column: batched 1D transforms, the column as a row with the axes exchanged
    from libertem_amd.udf.wdd import window_pixels
    window = (16, 18)
    idx = window_pixels(SIG, window, 11.6, 14.2)
    for nav in ((1, 16), (16, 1), (1, 9), (7, 1), (1, 2), (2, 1)):
        rng = np.random.default_rng([31, nav[0], nav[1]])
        frames = rng.poisson(40., nav + SIG).astype(np.uint16)
        assert sr.rim_margin(SIG, nav, sr.full_params(SIG, **wr.GENERIC)) >= 1e-6
        ref = wr.reference(frames, window, EPS, **wr.GENERIC)['fourier']
        plan = make_plan(window, 100, nav=nav)
        bf = torch.from_numpy(np.ascontiguousarray(frames.reshape(nav[0] * nav[1], -1)[:, idx], dtype=np.float32)).cuda()
        out = torch.empty(nav, dtype=torch.complex64, device='cuda')
        plan.reconstruct(bf.data_ptr(), 288, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        wr.assert_fourier(got, ref, f"plan {nav}")
        assert np.array_equal(got == 0, ref == 0)
        plan.close()


def test_plan_error_codes(generic):
    from libertem_amd import hip
    window = (16, 16)
    bf_host, ref = generic[window]
    p, geom = geometry(wr.GENERIC)
    win = wr.window_origin(p, window)
    plan = hip.WDDPlan(0, 12, 10, win, 100, geom, EPS)
    bf = torch.from_numpy(bf_host).cuda()
    out = torch.empty((12, 10), dtype=torch.complex64, device='cuda')
    with pytest.raises(ValueError, match=r'code -3'):
        plan.reconstruct(bf.data_ptr(), 255, out.data_ptr())
    with pytest.raises(ValueError, match=r'null.*code -1'):
        plan.reconstruct(None, 256, out.data_ptr())
    with pytest.raises(ValueError, match=r'null.*code -1'):
        plan.reconstruct(bf.data_ptr(), 256, None)
    zero = geom.copy()
    zero[3] = 0.
    for args in ((0, 10, win, 100, geom, EPS), (12, -1, win, 100, geom, EPS), (1, 1, win, 100, geom, EPS),
                 (12, 10, (3, 6, 0, 16), 100, geom, EPS), (12, 10, (3, 6, 16, -2), 100, geom, EPS),
                 (12, 10, (0, 0, 2, 2), 100, geom, EPS), (12, 10, win, 100, zero, EPS), (12, 10, win, 100, geom, 0.),
                 (12, 10, win, 100, geom, np.nan), (46341, 46341, win, 1, geom, EPS)):
        with pytest.raises(ValueError, match=r'code -3'):
            hip.WDDPlan(0, *args)
    with pytest.raises(ValueError, match=r'code -1'):
        hip.WDDPlan(0, 12, 10, win, 0, geom, EPS)
    with pytest.raises(ValueError, match='4 values'):
        hip.WDDPlan(0, 12, 10, win[:3], 100, geom, EPS)
    with pytest.raises(ValueError, match='11 values'):
        hip.WDDPlan(0, 12, 10, win, 100, geom[:7], EPS)
    # a filter that cannot fit: 4096^2 Qs x 64^2 window pixels x 8 bytes = 512 GiB; nothing is allocated
    with pytest.raises(hip.LtmiError, match=r'needs 549755813888 bytes.*code -4'):
        hip.WDDPlan(0, 4096, 4096, (0, 0, 64, 64), 1, geom, EPS)
    handle = ctypes.c_void_p()
    gp = geom.ctypes.data_as(ctypes.c_void_p)
    wp = np.asarray(win, np.int32).ctypes.data_as(ctypes.c_void_p)
    assert hip.lib().ltmi_wdd_plan_create(0, 12, 10, None, 100, gp, EPS, ctypes.byref(handle)) == -1
    assert hip.lib().ltmi_wdd_plan_create(0, 12, 10, wp, 100, None, EPS, ctypes.byref(handle)) == -1
    assert hip.lib().ltmi_wdd_plan_create(0, 12, 10, wp, 100, gp, EPS, None) == -1
    assert not handle.value
    assert hip.lib().ltmi_wdd_reconstruct(None, bf.data_ptr(), 256, out.data_ptr(), None) == -1
    # nothing of that reached the plan, and it still works
    plan.reconstruct(bf.data_ptr(), 256, out.data_ptr())
    torch.cuda.synchronize()
    wr.assert_fourier(out.cpu().numpy(), ref, 'after the errors')
    plan.close()
    # ... and the creates that failed left nothing that keeps a new plan from working
    after = hip.WDDPlan(0, 12, 10, win, 100, geom, EPS)
    out.zero_()
    after.reconstruct(bf.data_ptr(), 256, out.data_ptr())
    torch.cuda.synchronize()
    wr.assert_fourier(out.cpu().numpy(), ref, 'a plan made after the errors')
    after.close()
