"""
`ltmi_plx_ramps`, `ltmi_plx_sum`, `ltmi_plx_mul`, `ltmi_plx_peaks` and the plan on the MI355X through hip.plx_* and
hip.ParallaxPlan (csrc/ltmi_parallax.hip), with guard values around every input and result.

The product alone against the explicit float32 NumPy expression, byte for byte.  The peaks alone against a float64
NumPy evaluation written out here, byte for byte, on crafted maps: a unique peak at every corner and edge of the
window (negative shifts wrap), a larger value outside the window, exact ties (the first in row-major (ty, tx) order
wins, also between lanes and for a constant map), d = 0 and d > 0 (no sub-pixel part), the clip at +- 0.5, max_shift
1 and 4, scans 12 x 10 and 9 x 16.  The ramps against libm's sin and cos of the same angle: 4 ulp.  The sum against
the complex128 sum over the same ramps: every component within 1.2e-7 |ref[Q]| + 1e-12 sum_K |G[K, Q]| (the rounding
to float32, and a float64 accumulation that is negligible) for zero, integer and fractional shifts and 1, 3, 5 and 58
pixels.  The plan on the fixture's bright-field pixels: batches of 16 (three full, one of 10) give the bytes of one
batch of 58, padded ld_bf, the kernels it reports, repeats byte for byte, every error code.
"""
import ctypes
import math

import numpy as np
import pytest

import guarded
import parallax_ref as pr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

NAV_IDS = ['12x10', '9x16']


def half(nav):
    return nav[0] * (nav[1] // 2 + 1)


def random_spectra(n, nav, seed):
    rng = np.random.default_rng(guarded.seed('plx', n, nav, seed))
    g = rng.normal(size=(n, half(nav))) + 1j * rng.normal(size=(n, half(nav)))
    return (g * rng.uniform(0.5, 2000., size=(n, 1))).astype(np.complex64)


# ---- the product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 58])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_mul_bytes(nav, n):
    from libertem_amd import hip
    g = random_spectra(n, nav, 'g')
    r = random_spectra(1, nav, 'r')[0]
    spec = guarded.Region(n, half(nav), half(nav), np.complex64, init=g, fill='nan')
    ref = guarded.Region(1, half(nav), half(nav), np.complex64, init=r[None], fill='nan')
    out = guarded.Region(n, half(nav), half(nav), np.complex64)
    hip.plx_mul(0, spec.ptr, n, nav[0], nav[1], ref.ptr, out.ptr)
    torch.cuda.synchronize()
    guarded.unchanged_outside(out, 'X')
    guarded.unchanged(spec, 'G')
    guarded.unchanged(ref, 'R')
    gr, gi, rr, ri = g.real, g.imag, r.real[None], r.imag[None]
    assert gr.dtype == np.float32 and rr.dtype == np.float32
    want = np.empty_like(g)
    want.real = gr * rr + gi * ri
    want.imag = gi * rr - gr * ri
    want[:, 0] = 0
    got = out.result()
    assert got.tobytes() == want.tobytes()
    assert np.abs(got - g * np.conj(r)[None])[:, 1:].max() <= 1e-6 * np.abs(got).max()
    hip.plx_mul(0, spec.ptr, 0, nav[0], nav[1], ref.ptr, out.ptr)              # nothing to do
    for kw in [dict(nav_y=0), dict(nav_x=-2), dict(n=-1)]:
        args = dict(device=0, spec_ptr=spec.ptr, n=n, nav_y=nav[0], nav_x=nav[1], ref_ptr=ref.ptr, x_ptr=out.ptr)
        with pytest.raises(ValueError, match='code -3'):
            hip.plx_mul(**dict(args, **kw))
    with pytest.raises(ValueError, match='null.*code -1'):
        hip.plx_mul(0, spec.ptr, n, nav[0], nav[1], None, out.ptr)


# ---- the peaks -----------------------------------------------------------------------------------------------------------
def parabola(cm, c0, cp):
    cm, c0, cp = np.float64(cm), np.float64(c0), np.float64(cp)
    d = cm - np.float64(2.) * c0 + cp
    if not d < 0:
        return np.float64(0.)
    return np.clip((cm - cp) / (np.float64(2.) * d), -0.5, 0.5)


def peaks_numpy(maps, m):
    """float64 from the stored float32 values; the first maximum in row-major (ty, tx) order"""
    n, ny, nx = maps.shape
    out = np.zeros((n, 2), np.float64)
    for f in range(n):
        best = None
        for ty in range(-m, m + 1):
            for tx in range(-m, m + 1):
                if best is None or maps[f, ty % ny, tx % nx] > maps[f, best[0] % ny, best[1] % nx]:
                    best = (ty, tx)
        ty, tx = best
        c0 = maps[f, ty % ny, tx % nx]
        out[f, 0] = ty + parabola(maps[f, (ty - 1) % ny, tx % nx], c0, maps[f, (ty + 1) % ny, tx % nx])
        out[f, 1] = tx + parabola(maps[f, ty % ny, (tx - 1) % nx], c0, maps[f, ty % ny, (tx + 1) % nx])
    return out


def crafted_maps(nav, m):
    """-> maps float32 (n, Ny, Nx), and for some of them the shift they must give (None: whatever NumPy says)"""
    ny, nx = nav
    rng = np.random.default_rng(guarded.seed('maps', nav, m))
    maps, expect = [], []

    def noise():
        return rng.random((ny, nx)).astype(np.float32)

    def put(a, ty, tx, v):
        a[ty % ny, tx % nx] = v

    # a unique peak at every corner, edge and the centre of the window; where the scan has room, a larger value just
    # outside the window
    for ty in (-m, 0, m):
        for tx in (-m, 0, m):
            a = noise()
            put(a, ty, tx, 10.)
            maps.append(a)
            expect.append(None)
            b = a.copy()
            if nx > 2 * m + 1:
                put(b, 0, m + 1, 50.)
            if ny > 2 * m + 1:
                put(b, m + 1, 0, 60.)
            maps.append(b)
            expect.append(None)
    # exact ties: (-1, 1) comes before (0, -m) although its row index is the last; within a row the smaller tx; the
    # first and the last candidate (different lanes, and for m = 4 different rounds of a lane)
    for first, second in [((-1, 1), (0, -m)), ((1, -1), (1, 1)), ((-m, -m), (m, m)), ((-m, m), (-m + 1, -m))]:
        a = noise()
        put(a, *first, 10.)
        put(a, *second, 10.)
        maps.append(a)
        expect.append(None)
    # a constant map: every candidate ties, d = 0 on both axes
    maps.append(np.full((ny, nx), 3.25, np.float32))
    expect.append((-m, -m))
    # zeros
    maps.append(np.zeros((ny, nx), np.float32))
    expect.append((-m, -m))
    # a plateau of two along x: d < 0 and the vertex at exactly + 0.5 from the first
    a = np.zeros((ny, nx), np.float32)
    put(a, 0, 0, 8.)
    put(a, 0, 1, 8.)
    maps.append(a)
    expect.append((0., 0.5))
    if nx > 2 * m + 1:
        # the maximum of the window at its edge, a larger neighbour outside: d > 0 -> no sub-pixel part along x
        a = np.zeros((ny, nx), np.float32)
        put(a, 0, m, 10.)
        put(a, 0, m + 1, 30.)
        maps.append(a)
        expect.append((0., float(m)))
        # ... a neighbour that is larger by less: d < 0 and a vertex beyond half a pixel, clipped to + 0.5 and - 0.5
        a = np.zeros((ny, nx), np.float32)
        put(a, 0, m, 10.)
        put(a, 0, m + 1, 15.)
        maps.append(a)
        expect.append((0., m + 0.5))
        if nx > 2 * m + 2:
            a = np.zeros((ny, nx), np.float32)
            put(a, 0, -m, 10.)
            put(a, 0, -m - 1, 15.)
            maps.append(a)
            expect.append((0., -m - 0.5))
    if ny > 2 * m + 2:
        a = np.zeros((ny, nx), np.float32)
        put(a, -m, 1, 10.)
        put(a, -m - 1, 1, 15.)
        put(a, -m, 2, 4.)
        maps.append(a)
        expect.append((-m - 0.5, 1 + 4. / 32.))                    # x: (0 - 4) / (2 (0 - 20 + 4))
    # smooth peaks with fractional vertices
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    for sy, sx in [(0.3, -1.7), (-2.2 if m > 2 else -0.6, 0.45)]:
        dy = (yy - sy + ny / 2) % ny - ny / 2
        dx = (xx - sx + nx / 2) % nx - nx / 2
        maps.append(np.exp(-(dy * dy + dx * dx) / 3.).astype(np.float32))
        expect.append(None)
    return np.stack(maps), expect


@pytest.mark.parametrize('m', [1, 4])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_peaks_bytes(nav, m):
    from libertem_amd import hip
    maps, expect = crafted_maps(nav, m)
    n = len(maps)
    want = peaks_numpy(maps, m)
    for f, e in enumerate(expect):
        if e is not None:
            assert tuple(want[f]) == tuple(float(v) for v in e), (f, want[f], e)
    assert np.all(np.abs(want) <= m + 0.5)
    src = guarded.Region(n, nav[0] * nav[1], nav[0] * nav[1], np.float32, init=maps.reshape(n, -1), fill='inf')
    out = guarded.Region(n, 2, 2, np.float64)
    hip.plx_peaks(0, src.ptr, n, nav[0], nav[1], m, out.ptr)
    torch.cuda.synchronize()
    guarded.unchanged_outside(out, 'shifts')
    guarded.unchanged(src, 'maps')
    got = out.result()
    assert got.tobytes() == want.tobytes(), np.flatnonzero((got != want).any(axis=1))
    # one map (one wave of the workgroup), and a second call
    one = guarded.Region(1, 2, 2, np.float64)
    hip.plx_peaks(0, src.ptr + 4 * 5 * nav[0] * nav[1], 1, nav[0], nav[1], m, one.ptr)
    torch.cuda.synchronize()
    guarded.unchanged_outside(one, 'one shift')
    assert one.result().tobytes() == want[5:6].tobytes()


def test_peaks_error_codes():
    from libertem_amd import hip
    maps = guarded.Region(2, 120, 120, np.float32, init=np.zeros((2, 120), np.float32), fill='inf')
    out = guarded.Region(2, 2, 2, np.float64)
    args = dict(device=0, maps_ptr=maps.ptr, n=2, nav_y=12, nav_x=10, max_shift=4, shifts_ptr=out.ptr)
    for kw in [dict(max_shift=0), dict(max_shift=5), dict(nav_y=8), dict(nav_y=0), dict(nav_x=-1), dict(n=-1),
               dict(max_shift=2 ** 30)]:
        with pytest.raises(ValueError, match='code -3'):
            hip.plx_peaks(**dict(args, **kw))
    with pytest.raises(ValueError, match='null.*code -1'):
        hip.plx_peaks(**dict(args, maps_ptr=None))
    hip.plx_peaks(**dict(args, n=0))
    torch.cuda.synchronize()
    guarded.unchanged_outside(out, 'after n = 0')
    assert out.result().tobytes() == guarded.poison(out.total)[out.start:out.start + 32].tobytes()


# ---- the ramps -----------------------------------------------------------------------------------------------------------
def ramps_libm(sh, nav):
    ny, nx = nav
    nxc = nx // 2 + 1
    ey = np.zeros((len(sh), ny), np.complex128)
    ex = np.zeros((len(sh), nxc), np.complex128)
    for k, (s_y, s_x) in enumerate(sh):
        for iy in range(ny):
            a = 6.283185307179586 * (float(pr.signed(iy, ny)) * s_y / float(ny))
            ey[k, iy] = complex(math.cos(a), math.sin(a))
        for ix in range(nxc):
            a = 6.283185307179586 * (float(pr.signed(ix, nx)) * s_x / float(nx))
            ex[k, ix] = complex(math.cos(a), math.sin(a))
    return ey, ex


def ulps(got, want):
    """the distance of every component in units of the last place of the wanted value"""
    got = np.ascontiguousarray(got).view(np.float64)
    want = np.ascontiguousarray(want).view(np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def shifts_for(n, kind, seed):
    rng = np.random.default_rng(guarded.seed('sh', n, kind, seed))
    if kind == 'zero':
        return np.zeros((n, 2))
    if kind == 'integer':
        return rng.integers(-4, 4, (n, 2), endpoint=True).astype(np.float64)
    return rng.uniform(-4.5, 4.5, (n, 2))


@pytest.mark.parametrize('kind', ['zero', 'integer', 'fractional'])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_ramps(nav, kind):
    from libertem_amd import hip
    ny, nxc = nav[0], nav[1] // 2 + 1
    n = 58
    sh = shifts_for(n, kind, nav)
    src = guarded.Region(n, 2, 2, np.float64, init=sh, fill='nan')
    ey = guarded.Region(n, ny, ny, np.complex128)
    ex = guarded.Region(n, nxc, nxc, np.complex128)
    hip.plx_ramps(0, src.ptr, n, nav[0], nav[1], ey.ptr, ex.ptr)
    torch.cuda.synchronize()
    guarded.unchanged_outside(ey, 'ey')
    guarded.unchanged_outside(ex, 'ex')
    guarded.unchanged(src, 'sh')
    want_y, want_x = ramps_libm(sh, nav)
    got_y, got_x = ey.result(), ex.result()
    assert ulps(got_y, want_y).max() <= 4 and ulps(got_x, want_x).max() <= 4
    if kind == 'zero':
        assert np.all(got_y == 1) and np.all(got_x == 1)
    # the Nyquist index of an even axis carries s = -n / 2
    if nav[1] % 2 == 0 and kind == 'fractional':
        assert np.abs(got_x[:, -1] - np.exp(-1j * np.pi * sh[:, 1])).max() < 1e-14
    with pytest.raises(ValueError, match='code -3'):
        hip.plx_ramps(0, src.ptr, n, 0, nav[1], ey.ptr, ex.ptr)
    with pytest.raises(ValueError, match='null.*code -1'):
        hip.plx_ramps(0, None, n, nav[0], nav[1], ey.ptr, ex.ptr)


# ---- the sum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['zero', 'integer', 'fractional'])
@pytest.mark.parametrize('n', [1, 3, 5, 58])
@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_sum_vs_float64(nav, n, kind):
    from libertem_amd import hip
    ny, nxc = nav[0], nav[1] // 2 + 1
    g = random_spectra(n, nav, kind)
    ey, ex = ramps_libm(shifts_for(n, kind, 'sum'), nav)
    spec = guarded.Region(n, half(nav), half(nav), np.complex64, init=g, fill='nan')
    d_ey = guarded.Region(n, ny, ny, np.complex128, init=ey, fill='nan')
    d_ex = guarded.Region(n, nxc, nxc, np.complex128, init=ex, fill='nan')
    out = guarded.Region(1, half(nav), half(nav), np.complex64)
    hip.plx_sum(0, spec.ptr, n, nav[0], nav[1], d_ey.ptr, d_ex.ptr, out.ptr)
    torch.cuda.synchronize()
    guarded.unchanged_outside(out, 'S')
    for region, what in ((spec, 'G'), (d_ey, 'ey'), (d_ex, 'ex')):
        guarded.unchanged(region, what)
    g64 = g.astype(np.complex128).reshape(n, ny, nxc)
    want = (g64 * ey[:, :, None] * ex[:, None, :]).sum(axis=0) / n
    got = out.result().reshape(ny, nxc).astype(np.complex128)
    bound = 1.2e-7 * np.abs(want) + 1e-12 * np.abs(g64).sum(axis=0)
    assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)
    if kind == 'zero':
        plain = g64.mean(axis=0)
        assert np.all(np.abs(got.real - plain.real) <= bound) and np.all(np.abs(got.imag - plain.imag) <= bound)
    # a second call gives the same bytes
    first = out.result().tobytes()
    hip.plx_sum(0, spec.ptr, n, nav[0], nav[1], d_ey.ptr, d_ex.ptr, out.ptr)
    torch.cuda.synchronize()
    assert out.result().tobytes() == first


def test_sum_error_codes():
    from libertem_amd import hip
    buf = guarded.Region(1, 72, 72, np.complex128, init=np.zeros((1, 72), np.complex128), fill='nan')
    out = guarded.Region(1, 72, 72, np.complex64)
    for kw in [dict(n=0), dict(n=-3), dict(nav_y=0), dict(nav_x=0)]:
        args = dict(device=0, spec_ptr=buf.ptr, n=1, nav_y=12, nav_x=10, ey_ptr=buf.ptr, ex_ptr=buf.ptr, s_ptr=out.ptr)
        with pytest.raises(ValueError, match='code -3'):
            hip.plx_sum(**dict(args, **kw))
    with pytest.raises(ValueError, match='null.*code -1'):
        hip.plx_sum(0, buf.ptr, 1, 12, 10, None, buf.ptr, out.ptr)


# ---- the plan ------------------------------------------------------------------------------------------------------------
def bf_of(nav):
    from libertem_amd.udf.ssb import bf_pixels
    idx = bf_pixels(pr.SIG, pr.SEMICONV_PIX, pr.CY, pr.CX)
    data = pr.counted(nav)
    return np.ascontiguousarray(data.reshape(nav[0] * nav[1], -1)[:, idx].astype(np.float32))


class PlanRun:
    """a plan, guarded bf (Ny Nx, P) at a leading dimension, guarded shifts and half spectra"""

    def __init__(self, nav, max_batch, pad=0, max_shift=pr.MAX_SHIFT):
        from libertem_amd import hip
        self.nav = nav
        bf = bf_of(nav)
        self.n = bf.shape[1]
        self.bf = guarded.Region(bf.shape[0], self.n, self.n + pad, np.float32, init=bf, fill='nan')
        self.plan = hip.ParallaxPlan(0, nav[0], nav[1], self.n, max_batch, max_shift, 1 << 30)
        self.sh = guarded.Region(self.n, 2, 2, np.float64, init=np.zeros((self.n, 2)), fill='nan')
        self.zero = guarded.Region(self.n, 2, 2, np.float64, init=np.zeros((self.n, 2)), fill='nan')
        self.half = guarded.Region(1, half(nav), half(nav), np.complex64)

    def run(self, iterations=2):
        """-> the shifts after every iteration, S(shifts), S(0), the kernels reported after each kind of call"""
        kernels, shifts = [], []
        self.sh.load(np.zeros((self.n, 2)))
        self.plan.load(self.bf.ptr, self.bf.ld)
        kernels.append(self.plan.last_kernel())
        for _ in range(iterations):
            self.plan.iterate(self.sh.ptr)
            torch.cuda.synchronize()
            guarded.unchanged_outside(self.sh, 'shifts')
            shifts.append(self.sh.result())
        kernels.append(self.plan.last_kernel())
        self.plan.sum(self.sh.ptr, self.half.ptr)
        torch.cuda.synchronize()
        guarded.unchanged_outside(self.half, 'S')
        image = self.half.result()
        self.plan.sum(self.zero.ptr, self.half.ptr)
        torch.cuda.synchronize()
        kernels.append(self.plan.last_kernel())
        guarded.unchanged(self.bf, 'bf')
        guarded.unchanged(self.zero, 'zero shifts')
        return shifts, image, self.half.result(), kernels


@pytest.mark.parametrize('nav', pr.NAVS, ids=NAV_IDS)
def test_plan_batches_give_the_same_bytes(nav):
    from libertem_amd.udf.parallax import parallax_bf
    whole = PlanRun(nav, 58)
    assert whole.plan.last_kernel() == ''
    shifts, image, bright, kernels = whole.run()
    assert kernels == ['k_transpose<4> + hipfft_r2c batch=58',
                       'k_plx_ramps + k_plx_sum + k_plx_herm + k_plx_mul + hipfft_c2r + k_plx_peaks batch=58',
                       'k_plx_ramps + k_plx_sum + k_plx_herm']
    parts = PlanRun(nav, 16, pad=3)                       # three full batches and one of 10; rows of bf 61 apart
    p_shifts, p_image, p_bright, p_kernels = parts.run()
    assert p_kernels[0] == 'k_transpose<4> + hipfft_r2c batch=16' and p_kernels[1].endswith('k_plx_peaks batch=16')
    for a, b in zip(shifts, p_shifts):
        assert a.tobytes() == b.tobytes()
    assert image.tobytes() == p_image.tobytes() and bright.tobytes() == p_bright.tobytes()
    more = PlanRun(nav, 1000)                             # a batch above P is P
    assert more.run()[0][1].tobytes() == shifts[1].tobytes()
    # a second run of the same plan repeats byte for byte
    again = whole.run()
    assert again[0][1].tobytes() == shifts[1].tobytes() and again[1].tobytes() == image.tobytes()
    # what comes out is the reconstruction: the NumPy branch on the same pixels, loosely (tests/test_parallax_gpu.py
    # holds the measured tolerance)
    host = parallax_bf(bf_of(nav), nav, pr.SIG, **pr.PARAMS)
    assert np.abs(shifts[1] - host['shifts']).max() < 1e-2
    got = np.fft.irfft2(image.reshape(nav[0], -1).astype(np.complex128), s=nav)
    assert np.abs(got - host['image']).max() < 1e-4 * np.abs(host['image']).max()
    for run in (whole, parts, more):
        run.plan.close()


def test_plan_error_codes():
    from libertem_amd import hip
    # the store of 58 x 12 x 6 spectra takes 33408 bytes
    with pytest.raises(hip.LtmiError, match=r'need 33408 bytes.*limit is 1000.*code -4'):
        hip.ParallaxPlan(0, 12, 10, 58, 16, 4, 1000)
    with pytest.raises(hip.LtmiError, match=r'code -4'):
        hip.ParallaxPlan(0, 12, 10, 58, 16, 4, 33407)
    hip.ParallaxPlan(0, 12, 10, 58, 16, 4, 33408).close()
    # a store that cannot fit the device: 10^5 pixels x 4096 x 2049 Qs x 8 bytes = 6.7 TB; nothing is allocated
    with pytest.raises(hip.LtmiError, match=r'need 6714163200000 bytes.*free.*code -4'):
        hip.ParallaxPlan(0, 4096, 4096, 100000, 1, 4, 1 << 60)
    for args in [(0, 12, 10, 58, 16, 5), (0, 12, 10, 58, 16, 0), (0, 8, 16, 58, 16, 4), (0, 0, 10, 58, 16, 1),
                 (0, 12, 10, 0, 16, 4), (0, 12, 10, -1, 16, 4), (0, 40000, 40000, 58, 58, 4)]:
        with pytest.raises(ValueError, match='code -3'):
            hip.ParallaxPlan(*args, 1 << 30)
    with pytest.raises(ValueError, match='code -1'):
        hip.ParallaxPlan(0, 12, 10, 58, 0, 4, 1 << 30)
    assert hip.lib().ltmi_plx_plan_create(0, 12, 10, 58, 16, 4, 1 << 30, None) == -1
    run = PlanRun((12, 10), 16)
    with pytest.raises(ValueError, match='ltmi_plx_plan_load comes first.*code -1'):
        run.plan.iterate(run.sh.ptr)
    with pytest.raises(ValueError, match='ltmi_plx_plan_load comes first.*code -1'):
        run.plan.sum(run.sh.ptr, run.half.ptr)
    with pytest.raises(ValueError, match='ld_bf.*code -3'):
        run.plan.load(run.bf.ptr, 57)
    with pytest.raises(ValueError, match='null.*code -1'):
        run.plan.load(None, 58)
    run.plan.load(run.bf.ptr, run.bf.ld)
    with pytest.raises(ValueError, match='null.*code -1'):
        run.plan.iterate(None)
    with pytest.raises(ValueError, match='null.*code -1'):
        run.plan.sum(run.sh.ptr, None)
    null = ctypes.c_void_p()
    assert hip.lib().ltmi_plx_plan_load(null, run.bf.ptr, 58, None) == -1
    assert hip.lib().ltmi_plx_plan_last_kernel(null) == b''
    assert hip.lib().ltmi_plx_plan_destroy(null) == 0
    # the plan still works after the refused calls
    fresh = PlanRun((12, 10), 16)
    assert run.run()[0][1].tobytes() == fresh.run()[0][1].tobytes()
    run.plan.close()
    fresh.plan.close()
    assert run.plan._ptr is None
