"""
Shifted masks (`ApplyMasksUDF(shifts=...)`, the descan correction) at the kernel level: both entry points of the
C ABI, `ltmi_apply_masks_shifted` (shifts on the device, always the per-frame kernel `k_dense_shifted`) and
`ltmi_apply_masks_shifted_host` (shifts on the host: the matrix-core routes with the image of the shifted stack
where they apply), called through `hip.MaskHandle` and compared with a float64 / complex128 restatement written
here that slices frame AND masks to the overlap first, as the reference does (udf/masks.py:85-124).  `-m gpu` only.

The two arithmetics behind the entry point -- walk the overlap / multiply the whole frame with a zero-filled image --
agree on finite pixels only: the non-finite tests put NaN and +-Inf where they differ.  Every tile and every output
lies inside a larger device buffer filled with a poison pattern that is compared whole after the call, and every
test asserts the route it means to hit through `last_kernel()`.

Tolerances are the project's own for these kernels: 1e-5 (scale + 1) for float32 / complex64 results, 2e-6 (scale + 1)
on the float16-piece route, 1e-12 (scale + 1) for float64 / complex128, scale = sum |x| |w| over the overlap; integer
results are equal to the int64 product wrapped to the result dtype.
"""
import ctypes
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 256          # poison bytes in front of and behind every region; keeps the region's base 256-byte aligned
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31

TILE_DTYPES = ['bool', 'uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'uint64', 'int64',
               'float32', 'float64', 'complex64', 'complex128']
RESULT_DTYPES = ['float32', 'complex64', 'float64', 'complex128', 'int16', 'uint64']


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert _hip.device_count() >= 1
    return _hip


def _seed(*what):
    """a seed that is the same in every process (str hashes are salted per process)"""
    return zlib.crc32(repr(what).encode())


def _poison(n):
    """n bytes, none of them zero, with a period (251) that no row length here shares"""
    return np.resize(((np.arange(251) * 151 + 7) % 251 + 1).astype(np.uint8), n)


class _Region:
    """(rows, cols) of `dtype` at leading dimension `ld` (elements) inside a poisoned device buffer; the region
    starts `shift` elements behind a 256-byte boundary.  `init` fills the owned elements, padding stays poison."""

    def __init__(self, rows, cols, ld, dtype, shift=0, init=None):
        self.dt = np.dtype(dtype)
        self.rows, self.cols, self.ld = int(rows), int(cols), int(ld)
        assert self.ld >= self.cols
        self.start = GUARD + shift * self.dt.itemsize
        self.nbytes = self.rows * self.ld * self.dt.itemsize
        self.host = _poison(self.start + self.nbytes + GUARD)
        if init is not None:
            self.view(self.host)[...] = init
        self.dev = torch.from_numpy(self.host).cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.start

    def view(self, image):
        """the owned elements inside a host image of the whole buffer"""
        flat = image[self.start:self.start + self.nbytes].view(self.dt)
        return flat.reshape(self.rows, self.ld)[:, :self.cols]

    def download(self):
        return self.dev.cpu().numpy()


def _unchanged(region, what):
    torch.cuda.synchronize()
    assert np.array_equal(region.download(), region.host), f"{what}: buffer was written"


# ---- the reference --------------------------------------------------------------------------------------------

def _as_int64(a):
    """integers modulo 2^64 as int64 (uint64 above 2^63 wraps: products and sums modulo 2^64 stay the same)"""
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)


def _overlap(h, w, dy, dx):
    """frame rows / columns [y0, y1) x [x0, x1) that the mask shifted by (dy, dx) covers; Python integers"""
    return max(0, dy), min(h, h + dy), max(0, dx), min(w, w + dx)


def _slice_ref(data3d, masks3d, shifts, result_dtype):
    """out[f, k] = sum over the overlap of frame[f][y, x] * mask_k[y - dy, x - dx]: frame and masks SLICED to the
    overlap before the product, zeros for an empty overlap (udf/masks.py:85-124).  float64 / complex128, or -- integer
    results -- int64 arithmetic modulo 2^64.  Returns (out, scale) with scale = sum |x| |w| over the overlap
    (finite pixels only)."""
    rd = np.dtype(result_dtype)
    n, h, w = data3d.shape
    n_masks = len(masks3d)
    exact = rd.kind in 'iu'
    cplx = rd.kind == 'c' or np.iscomplexobj(data3d)
    acc = np.int64 if exact else (np.complex128 if cplx else np.float64)
    mm = _as_int64(masks3d) if exact else masks3d.astype(acc)
    dd = _as_int64(data3d) if exact else data3d.astype(acc)
    out = np.zeros((n, n_masks), dtype=acc)
    scale = np.zeros((n, n_masks))
    with np.errstate(all='ignore'):
        for f in range(n):
            y0, y1, x0, x1 = _overlap(h, w, int(shifts[f][0]), int(shifts[f][1]))
            if y1 <= y0 or x1 <= x0:
                continue
            dy, dx = int(shifts[f][0]), int(shifts[f][1])
            fr = dd[f, y0:y1, x0:x1].reshape(-1)
            ms = mm[:, y0 - dy:y1 - dy, x0 - dx:x1 - dx].reshape(n_masks, -1)
            if cplx and not np.iscomplexobj(data3d):
                # real frames against complex masks: two real products, each part on its own (`a + 1j * b` would
                # multiply b by 0 + 1j and carry a non-finite b into the real part as 0 * b = NaN)
                out[f].real = ms.real @ fr.real
                out[f].imag = ms.imag @ fr.real
            else:
                out[f] = ms @ fr
            if not exact:
                fa = np.abs(fr)
                scale[f] = np.abs(ms) @ np.where(np.isfinite(fa), fa, 0.0)
    return out, scale


def _tol(rd, kern=''):
    rd = np.dtype(rd)
    if rd in (np.float64, np.complex128):
        return 1e-12
    return 2e-6 if ',f16' in kern else 1e-5


def _check(region, want, scale, tol, what):
    """the owned elements match `want` (NaN at the same places, +-Inf at the same places with the same sign, the
    finite rest within tol (scale + 1); integers equal) and every other byte of the buffer is what it was"""
    torch.cuda.synchronize()
    got_img = region.download()
    got = region.view(got_img).copy()
    rd = region.dt
    if rd.kind in 'iu':
        want = want.astype(rd)                          # wraps
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} differ, first at {tuple(bad[0])}: " \
                              f"got {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"
    else:
        parts = [(got, want)] if rd.kind == 'f' else [(got.real, want.real), (got.imag, want.imag)]
        for g, e in parts:
            assert np.array_equal(np.isnan(g), np.isnan(e)), \
                f"{what}: NaN in rows {np.flatnonzero((np.isnan(g) != np.isnan(e)).any(axis=1))[:8]} " \
                f"(got {int(np.isnan(g).sum())} NaN, expected {int(np.isnan(e).sum())})"
            inf = np.isinf(e)
            assert np.array_equal(np.isinf(g), inf) and np.array_equal(np.sign(g[inf]), np.sign(e[inf])), \
                f"{what}: +-Inf at other places"
        fin = np.isfinite(want) & np.isfinite(got)
        err = np.where(fin, np.abs(np.where(fin, got, 0) - np.where(fin, want, 0)), 0.0)
        over = err > tol * (scale + 1)
        assert not over.any(), f"{what}: {int(over.sum())} beyond {tol} (scale + 1), worst " \
                               f"{(err / (scale + 1)).max():.3g} at {tuple(np.argwhere(over)[0])}"
    # everything the call does not own
    rest_got, rest_want = got_img.copy(), region.host.copy()
    region.view(rest_got)[...] = 0
    region.view(rest_want)[...] = 0
    if not np.array_equal(rest_got, rest_want):
        b = int(np.flatnonzero(rest_got != rest_want)[0])
        where = 'front guard' if b < region.start else 'rear guard'
        if region.start <= b < region.start + region.nbytes:
            r, c = divmod((b - region.start) // rd.itemsize, region.ld)
            where = f"row {r} column {c} (padding)"
        raise AssertionError(f"{what}: wrote outside its result, first at byte {b}, {where}")
    return got


# ---- inputs ---------------------------------------------------------------------------------------------------

def _frames(rng, dtype, shape, wide=False):
    """finite frames: small magnitudes for float results (sums stay far from overflow), the dtype's whole range with
    `wide` (integer results wrap)"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.integers(0, 2, shape).astype(np.bool_)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        if wide:
            return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
        return rng.integers(max(info.min, -3000), min(info.max, 3000), shape, endpoint=True).astype(dt)
    a = rng.standard_normal(shape) * 50.0
    if dt.kind == 'c':
        a = a + 1j * rng.standard_normal(shape) * 50.0
    return a.astype(dt)


def _masks(rng, dtype, n_masks, sig, wide=False):
    dt = np.dtype(dtype)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        lo, hi = (info.min, info.max) if wide else (max(info.min, -3), min(info.max, 9))
        return rng.integers(lo, hi, (n_masks,) + sig, dtype=dt, endpoint=True)
    m = rng.random((n_masks,) + sig) - 0.25
    if dt.kind == 'c':
        m = m + 1j * (rng.random((n_masks,) + sig) - 0.5)
    return m.astype(dt)


def _ramp_masks(dtype, n_masks, sig):
    """a distinct value at every (mask, pixel), exact in float32 and in two float16 pieces: (k n_px + p + 1) / 8"""
    n_px = sig[0] * sig[1]
    m = (np.arange(n_masks * n_px, dtype=np.float64).reshape((n_masks,) + sig) + 1) / 8
    dt = np.dtype(dtype)
    if dt.kind == 'c':
        m = m - 1j * m[::-1]
    return m.astype(dt)


def _edge_shifts(h, w):
    """every edge of the overlap arithmetic: nothing cut, one row / column cut on each side, one pixel left in each
    corner, one row / column left on each side, the first shifts without an overlap, shifts beyond them, and the four
    at the ends of int32 (no overlap: exactly 0)"""
    s = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]
    s += [(a * (h - 1), b * (w - 1)) for a in (1, -1) for b in (1, -1)]
    s += [(h - 1, 0), (-(h - 1), 0), (0, w - 1), (0, -(w - 1))]
    s += [(h, 0), (-h, 0), (0, w), (0, -w), (h, -w)]
    s += [(a * (h + 1), b * (w + 1)) for a in (1, -1) for b in (1, -1)]
    s += [(4 * h, -4 * w), (-4 * h, 4 * w)]
    s += [(I32_MAX, 0), (0, I32_MAX), (I32_MIN, I32_MIN), (I32_MAX - 1, -I32_MAX)]
    return np.array(s, dtype=np.int64)


def _empty(h, w, shifts):
    return np.array([(lambda o: o[1] <= o[0] or o[3] <= o[2])(_overlap(h, w, int(a), int(b))) for a, b in shifts])


def _base(rng, rd, shape):
    rd = np.dtype(rd)
    if rd.kind in 'iu':
        return rng.integers(0, 50, shape).astype(rd)
    b = rng.random(shape) + 0.5
    if rd.kind == 'c':
        b = b + 1j * rng.random(shape)
    return b.astype(rd)


def _run(hip, h, data3d, shifts, entry, acc=False, base=None, ld_tile=None, ld_out=None, tile_shift=0,
         out_shift=0):
    """one call of `entry` ('device': ltmi_apply_masks_shifted, 'host': ltmi_apply_masks_shifted_host) on poisoned
    buffers; returns (tile region, out region, route)"""
    n, sh, sw = data3d.shape
    n_px = sh * sw
    tile = _Region(n, n_px, ld_tile or n_px, data3d.dtype, tile_shift, init=data3d.reshape(n, n_px))
    out = _Region(n, h.n_masks, ld_out or h.n_masks, h.result_dtype, out_shift, init=base if acc else None)
    s32 = np.ascontiguousarray(shifts, dtype=np.int32)
    if entry == 'device':
        sdev = torch.from_numpy(s32).cuda()
        h.apply_shifted(tile.ptr, data3d.dtype, n, tile.ld, sh, sw, sdev.data_ptr(), out.ptr, out.ld, acc)
    else:
        h.apply_shifted_host(tile.ptr, data3d.dtype, n, tile.ld, sh, sw, s32, out.ptr, out.ld, acc)
    torch.cuda.synchronize()
    return tile, out, h.last_kernel()


def _run_and_check(hip, h, data3d, masks3d, shifts, entry, route, what, accs=(False, True), rng=None, **kw):
    rng = rng or np.random.default_rng(_seed(what))
    rd = h.result_dtype
    ref, scale = _slice_ref(data3d, masks3d.astype(rd), shifts, rd)
    results = []
    for acc in accs:
        base = _base(rng, rd, ref.shape)
        tile, out, kern = _run(hip, h, data3d, shifts, entry, acc, base, **kw)
        w = f"{what} acc={int(acc)} [{kern}]"
        for part in ([route] if isinstance(route, str) else route):
            if part.startswith('!'):
                assert part[1:] not in kern, w
            else:
                assert part in kern, w
        if rd.kind in 'iu':
            want = (ref + _as_int64(base)) if acc else ref
        else:
            want = ref + base.astype(ref.dtype) if acc else ref
        got = _check(out, want, scale + (np.abs(base) if acc else 0), _tol(rd, kern), w)
        _unchanged(tile, w + ' (tile)')
        empty = _empty(data3d.shape[1], data3d.shape[2], shifts)
        if empty.any():
            assert np.array_equal(got[empty], base[empty] if acc else np.zeros_like(got[empty])), \
                f"{w}: a frame without overlap is not exactly {'the base' if acc else '0'}"
        results.append(got)
    return results


# the routes of ltmi_apply_masks_shifted_host: (name, tile dtype, result dtype, sig, n_masks, what last_kernel says)
LDS, F16, L64, MF64, PER = 'k_dense_lds<', ',f16', 'k_dense_lds64', 'k_dense_mfma_f64', 'k_dense_shifted<'
ROUTES = {
    'per-frame':   ('uint16', 'float32', (15, 15), 4, [PER]),
    'lds-f32':     ('float32', 'float32', (17, 23), 3, [LDS, 'shifted', '!' + F16]),
    'lds-f16':     ('uint16', 'float32', (16, 16), 5, [LDS, 'shifted' + F16]),
    'lds-c64':     ('int16', 'complex64', (12, 40), 17, [LDS, 'shifted']),
    'lds64':       ('uint16', 'float64', (12, 40), 3, [L64, 'shifted, ']),
    'lds64-i64':   ('uint8', 'int64', (16, 16), 4, [L64, 'shifted, ']),
    'mfma-f64':    ('int32', 'float64', (8, 16), 5, [MF64, 'shifted, ']),
}


# ---- a. the per-frame kernel, every dtype pair -----------------------------------------------------------------

def _generic_accepts(tile_dtype, result_dtype):
    """the dtype pairs of apply_generic (csrc/ltmi_dense.hip): integer results take integer / bool frames only, real
    results no complex frames, complex64 results no complex128 frames"""
    t, r = np.dtype(tile_dtype), np.dtype(result_dtype)
    if r.kind in 'iu':
        return t.kind in 'biu'
    if r.kind == 'f':
        return t.kind != 'c'
    return not (r == np.complex64 and t == np.complex128)


@pytest.mark.parametrize('result_dtype', RESULT_DTYPES)
@pytest.mark.parametrize('tile_dtype', TILE_DTYPES)
def test_per_frame_kernel_dtype_matrix(hip, tile_dtype, result_dtype):
    """`ltmi_apply_masks_shifted` (shifts on the device) for every tile dtype of `enum ltmi_dtype` against a float32,
    complex64, float64, complex128, narrow-integer and 64-bit-integer stack; 1, 3, 4, 5 and 9 masks (GEN_MASKS = 4:
    a full, a ragged and a single-mask last block); written and accumulated on a non-zero base.  Integer results wrap
    (frames and masks over the whole range of their dtypes).  Pairs the dispatch refuses: LTMI_E_DTYPE, nothing
    written."""
    sig, n = (15, 15), 9
    rng = np.random.default_rng(_seed('matrix', tile_dtype, result_dtype))
    rd = np.dtype(result_dtype)
    exact = rd.kind in 'iu'
    data = _frames(rng, tile_dtype, (n,) + sig, wide=exact)
    shifts = np.array([(0, 0), (2, -3), (-14, 14), (15, 0), (-1, 0), (0, 1), (14, 14), (-3, 16), (7, -7)])
    for n_masks in (1, 3, 4, 5, 9):
        masks = _masks(rng, rd, n_masks, sig, wide=exact)
        h = hip.MaskHandle.dense(0, masks.reshape(n_masks, -1), rd)
        what = f"k_dense_shifted {tile_dtype} x {result_dtype}, {n_masks} masks"
        if _generic_accepts(tile_dtype, result_dtype):
            _run_and_check(hip, h, data, masks, shifts, 'device', PER, what, rng=rng, ld_out=n_masks + 2)
        else:
            for acc in (False, True):
                tile = _Region(n, 225, 225, tile_dtype, init=data.reshape(n, -1))
                out = _Region(n, n_masks, n_masks + 2, rd, init=_base(rng, rd, (n, n_masks)))
                sdev = torch.from_numpy(shifts.astype(np.int32)).cuda()
                with pytest.raises(ValueError, match=r'code -2'):
                    h.apply_shifted(tile.ptr, tile_dtype, n, 225, 15, 15, sdev.data_ptr(), out.ptr, out.ld, acc)
                with pytest.raises(ValueError, match=r'code -2'):
                    h.apply_shifted_host(tile.ptr, tile_dtype, n, 225, 15, 15, shifts, out.ptr, out.ld, acc)
                _unchanged(out, what + ' (refused)')
        h.close()


# ---- b. strides and bases --------------------------------------------------------------------------------------

@pytest.mark.parametrize('pad_tile,pad_out,tile_shift,out_shift,n', [
    (1, 0, 0, 0, 129), (8, 3, 0, 0, 127), (13, 3, 0, 1, 300), (0, 0, 1, 0, 129), (13, 3, 1, 1, 1), (0, 3, 0, 0, 300),
])
@pytest.mark.parametrize('route', ['per-frame', 'lds-f32', 'lds-f16', 'lds-c64', 'lds64', 'mfma-f64'])
@pytest.mark.parametrize('entry', ['device', 'host'])
def test_strides_and_bases(hip, entry, route, pad_tile, pad_out, tile_shift, out_shift, n):
    """padded tile rows (n_px + 1, + 8, + 13), padded result rows (n_masks + 3), a tile and a result that start one
    element behind a 256-byte boundary: nothing but the result is written -- neither the padding, nor the guards,
    nor (rows of the -1 padding of a shift group's row list) anything in front of the buffer.  The device entry is
    always the per-frame kernel.  The host entry keeps its route whatever the alignment: gfx950 serves the vector /
    LDS-DMA loads from any element-aligned address (`vector_loads_ok`), so a base moved by one element stays on the
    matrix-core kernels."""
    tile_dtype, result_dtype, sig, n_masks, expect = ROUTES[route]
    rng = np.random.default_rng(_seed('strides', route, pad_tile, pad_out, tile_shift, out_shift, n))
    data = _frames(rng, tile_dtype, (n,) + sig)
    masks = _masks(rng, result_dtype, n_masks, sig)
    # three shift groups of uneven size (one of more than 128 frames when n allows) and a frame without overlap
    shifts = np.array([(2, -3), (2, -3), (2, -3), (-1, 4), (2, -3), (0, 0), (2, -3)])[np.arange(n) % 7]
    shifts[n // 2] = (0, -sig[1])
    h = hip.MaskHandle.dense(0, masks.reshape(n_masks, -1), result_dtype)
    n_px = sig[0] * sig[1]
    _run_and_check(hip, h, data, masks, shifts, entry, PER if entry == 'device' else expect,
                   f"{entry} entry, {route}, ld_tile +{pad_tile}, ld_out +{pad_out}, bases +{tile_shift} / +{out_shift}",
                   rng=rng, ld_tile=n_px + pad_tile, ld_out=n_masks + pad_out, tile_shift=tile_shift,
                   out_shift=out_shift)
    h.close()


def _aligned_only_child():
    """(in a process started with LTMI_ALIGNED_DMA_ONLY=1) a tile base moved by one element, then padded rows that are
    no multiple of 16 bytes: the host entry leaves the matrix-core route for the per-frame kernel; an aligned tile
    stays on it"""
    from libertem_amd import hip
    hip.lib()
    tile_dtype, result_dtype, sig, n_masks, expect = ROUTES['lds-f32']
    rng = np.random.default_rng(_seed('aligned only'))
    n, n_px = 129, sig[0] * sig[1]
    data = _frames(rng, tile_dtype, (n,) + sig)
    masks = _masks(rng, result_dtype, n_masks, sig)
    shifts = np.array([(2, -3), (-1, 4), (0, 0)])[np.arange(n) % 3]
    h = hip.MaskHandle.dense(0, masks.reshape(n_masks, -1), result_dtype)
    for ld_tile, tile_shift, route in ((n_px + 1, 1, [PER]), (n_px + 2, 0, [PER]), (n_px + 1, 0, expect)):   # 392 floats: 16 B
        _run_and_check(hip, h, data, masks, shifts, 'host', route, f"aligned DMA only, ld {ld_tile}, base +{tile_shift}",
                       rng=rng, ld_tile=ld_tile, ld_out=n_masks + 3, tile_shift=tile_shift)
    h.close()
    print('aligned-only child ok')


def test_unaligned_base_with_aligned_dma_only(hip):
    """`LTMI_ALIGNED_DMA_ONLY=1` (read once per process, hence a child process) restores the conservative dispatch:
    only then does an unaligned tile take the host entry off the matrix-core route, to the per-frame kernel."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, LTMI_ALIGNED_DMA_ONLY='1')
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; "
            "import test_shifted_kernels_gpu as t; t._aligned_only_child()")
    r = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0 and 'aligned-only child ok' in r.stdout, r.stdout[-3000:]


# ---- c. the edges of the overlap, every route ------------------------------------------------------------------

@pytest.mark.parametrize('route', ['per-frame', 'lds-f32', 'lds-f16', 'lds-c64', 'lds64', 'lds64-1', 'lds64-i64',
                                   'mfma-f64', 'device'])
def test_overlap_edges(hip, route):
    """One tile whose frames carry `_edge_shifts`: masks with a distinct value at every (mask, pixel), random
    frames, so that a window that is off by one pixel, row or column gives another number, not a nearby one (a
    missing row is 1 / h of the sum, a mask read one pixel off changes every product by 1 / 8 x: both far above the
    tolerance); frames without overlap give exactly 0 (exactly the base when accumulating).  'lds64-1' runs every
    shift as a tile of its own: one shift group, the whole tile in one product.  'device': the device-shift entry."""
    tile_dtype, result_dtype, sig, n_masks, expect = ROUTES[{'lds64-1': 'lds64', 'device': 'per-frame'}.get(route, route)]
    rng = np.random.default_rng(_seed('edges', route))
    edge = _edge_shifts(*sig)
    masks = _ramp_masks(result_dtype, n_masks, sig)
    h = hip.MaskHandle.dense(0, masks.reshape(n_masks, -1), result_dtype)
    if route == 'lds64-1':
        data = _frames(rng, tile_dtype, (5,) + sig)
        data[data == 0] = 1
        for s in edge:
            _run_and_check(hip, h, data, masks, np.tile(s, (5, 1)), 'host', expect + ['1 group'],
                           f"{route} shift {tuple(s)}", rng=rng, ld_out=n_masks + 1)
    else:
        n = 3 * len(edge) + 1
        data = _frames(rng, tile_dtype, (n,) + sig)
        data[data == 0] = 1
        shifts = edge[rng.permutation(n) % len(edge)]
        entry = 'device' if route == 'device' else 'host'
        more = [f'{len(edge)} groups'] if route == 'lds64' else []       # one image per distinct (dy, dx), as given
        _run_and_check(hip, h, data, masks, shifts, entry, expect + more, f"{route} edge shifts", rng=rng,
                       ld_out=n_masks + 1)
    h.close()


# ---- d. non-finite pixels --------------------------------------------------------------------------------------

NF_ROUTES = {
    # name: (tile dtype, result dtype, sig, entry, constant shift?, what last_kernel says)
    'lds-f32':        ('float32', 'float32', (17, 23), 'host', False, [LDS, 'shifted']),
    'lds-f32-c64':    ('float32', 'complex64', (16, 16), 'host', False, [LDS, 'shifted']),
    'per-frame-f32':  ('float32', 'float32', (15, 15), 'host', False, [PER]),
    'lds64-groups':   ('float32', 'float64', (12, 40), 'host', False, [L64, 'groups']),
    'lds64-groups-f64': ('float64', 'float64', (12, 40), 'host', False, [L64, 'groups']),
    'lds64-1':        ('float64', 'float64', (12, 40), 'host', True, [L64, '1 group']),
    'lds64-1-f32':    ('float32', 'complex128', (16, 16), 'host', True, [L64, '1 group']),
    'mfma-f64':       ('float32', 'float64', (8, 16), 'host', False, [MF64, 'shifted, ']),
    'per-frame-f64':  ('float64', 'float64', (12, 40), 'device', False, [PER]),
    'per-frame-dev':  ('float32', 'float32', (17, 23), 'device', False, [PER]),
    # integer pixels cannot hold a non-finite value: their routes run as they did, no listing, no redo
    'lds-f16-int':    ('uint16', 'float32', (16, 16), 'host', False, [LDS, 'shifted' + F16, '!+nf']),
    'lds64-int':      ('int16', 'float64', (12, 40), 'host', False, [L64, 'groups', '!+nf']),
}


def _nonfinite_tile(rng, dtype, n, sig, shifts, n_masks):
    """frames and masks for the non-finite cases; every fifth frame gets NaN, +Inf or -Inf (in turn)
      (i)   frames 5j + 1: only in the rows / columns its shift cuts off -- the reference never reads them;
      (ii)  frames 5j + 3: inside the overlap, at the frame pixel under mask pixel (5, 5), where the even masks are 0
            and the odd ones positive: NaN for every mask under NaN, NaN (0 * Inf) for the even and +-Inf for the odd
            masks under +-Inf;
      (iii) frames without overlap: anywhere, the result is exactly 0;
    the frames between them stay clean.  Returns (data, masks, kind per frame)."""
    h, w = sig
    dt = np.dtype(dtype)
    data = _frames(rng, dtype, (n,) + sig)
    masks = _masks(rng, 'float64', n_masks, sig)
    masks[:, 5, 5] = np.where(np.arange(n_masks) % 2 == 0, 0.0, 0.75)
    kind = np.zeros(n, dtype=int)
    if dt.kind != 'f':
        return data, masks, kind
    specials = [np.nan, np.inf, -np.inf]
    for f in range(n):
        dy, dx = int(shifts[f][0]), int(shifts[f][1])
        y0, y1, x0, x1 = _overlap(h, w, dy, dx)
        v = specials[(f // 5) % 3]
        if y1 <= y0 or x1 <= x0:
            if f % 2:
                kind[f] = 3
                data[f][rng.integers(0, h), rng.integers(0, w)] = v
                data[f][h - 1, w - 1] = specials[f % 3]
        elif f % 5 == 1 and (y1 - y0 < h or x1 - x0 < w):
            kind[f] = 1
            cut = np.ones(sig, dtype=bool)
            cut[y0:y1, x0:x1] = False
            pos = np.argwhere(cut)
            for y, x in pos[rng.permutation(len(pos))[:3]]:
                data[f][y, x] = v
        elif f % 5 == 3 and y0 <= 5 + dy < y1 and x0 <= 5 + dx < x1:
            kind[f] = 2
            data[f][5 + dy, 5 + dx] = v
    return data, masks, kind


@pytest.mark.parametrize('n', [40, 300])
@pytest.mark.parametrize('route', list(NF_ROUTES))
def test_non_finite_pixels(hip, route, n):
    """NaN and +-Inf pixels in float32 / float64 frames, on every route that takes such frames: outside the overlap
    they do not exist for the reference (it slices first), inside it they reach every mask (0 * NaN = NaN), and a
    frame without overlap gives exactly 0 whatever it holds.  The routes that multiply the WHOLE frame with the
    zero-filled image of the shifted stack give NaN for every mask of a frame of kind (i) and (iii) unless the
    frames with a non-finite result are computed again by the overlap walk.  300 frames: the large shift group
    spans two workgroups of 128 frames; written and accumulated on a non-zero base; clean frames lie between the
    others, and their rows must not change."""
    tile_dtype, result_dtype, sig, entry, constant, expect = NF_ROUTES[route]
    n_masks = 5
    rng = np.random.default_rng(_seed('non-finite', route, n))
    if constant:
        shift_sets = [np.tile((2, -3), (n, 1)), np.tile((-sig[0], 1), (n, 1))]
    else:
        cyc = np.array([(2, -3), (2, -3), (-1, 4), (2, -3), (2, -3), (sig[0], 0), (2, -3), (0, 0), (2, -3),
                        (1, -sig[1]), (2, -3)])
        shift_sets = [cyc[np.arange(n) % len(cyc)]]
    for shifts in shift_sets:
        data, masks, kind = _nonfinite_tile(rng, tile_dtype, n, sig, shifts, n_masks)
        if np.dtype(tile_dtype).kind == 'f':
            empty = _empty(sig[0], sig[1], shifts)
            assert empty.all() or {1, 2} <= set(kind)
            assert not empty.any() or 3 in set(kind)
            assert (kind == 0).sum() >= n // 3 or empty.all()
        masks = masks.astype(result_dtype)
        h = hip.MaskHandle.dense(0, masks.reshape(n_masks, -1), result_dtype)
        _run_and_check(hip, h, data, masks, shifts, entry, expect, f"non-finite pixels, {route}, {n} frames",
                       rng=rng, ld_out=n_masks + 3)
        h.close()


# ---- e. the image cache ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('tile_dtype,result_dtype,expect', [
    ('uint16', 'float32', [LDS, 'shifted' + F16]), ('float32', 'float32', [LDS, 'shifted']),
    ('float32', 'float64', [L64, 'groups']), ('uint16', 'float64', [L64, 'groups']),
])
def test_image_cache(hip, tile_dtype, result_dtype, expect):
    """One handle, call after call: other shifts (cached images of the first call and new ones), the same number of
    pixels as (32, 16) instead of (16, 32) (every cached image is of the wrong shape), back again, tuning code 37
    (float32 images instead of float16 pieces) and back.  Float frames carry a NaN in a corner: the rows that are
    computed again use the shifts and the shape of THIS call."""
    n, n_masks = 150, 5
    rng = np.random.default_rng(_seed('cache', tile_dtype, result_dtype))
    flat = _frames(rng, tile_dtype, (n, 512))
    if np.dtype(tile_dtype).kind == 'f':
        flat[::4, 0] = np.nan
        flat[1::4, 511] = np.inf
    mflat = _masks(rng, result_dtype, n_masks, (512,))
    h = hip.MaskHandle.dense(0, mflat, result_dtype)
    sets = [rng.integers(-2, 3, (n, 2)), rng.integers(-3, 2, (n, 2)), np.tile((1, -1), (n, 1))]
    sets[0][5], sets[1][6] = (40, 0), (0, -40)

    def once(sig, shifts, route, what):
        _run_and_check(hip, h, flat.reshape((n,) + sig), mflat.reshape((n_masks,) + sig), shifts, 'host', route,
                       f"cache {tile_dtype} -> {result_dtype}: {what}", rng=rng)

    once((16, 32), sets[0], expect, 'first call')
    once((16, 32), sets[1], expect, 'other shifts')
    once((32, 16), sets[1], expect, '(32, 16)')
    once((16, 32), sets[0], expect, '(16, 32) again')
    once((16, 32), sets[2], [expect[0], '1 group' if expect[0] == L64 else 'shift groups=1'], 'one shift')
    if F16 in expect[1]:
        h.set_tuning(mt=0, waves=hip.Variant.DENSE_F32_INSTR, ksplit=0)
        once((16, 32), sets[1], [LDS, 'shifted', '!' + F16], 'tuning 37')
        h.set_tuning(mt=0, waves=0, ksplit=0)
        once((16, 32), sets[0], expect, 'tuning 0 again')
    h.close()


# ---- f. argument checks ----------------------------------------------------------------------------------------

def test_argument_checks(hip):
    """what both entries refuse, by return code, with the result buffer byte for byte as it was; no frames: OK and
    nothing touched (not even looked at: null pointers pass)"""
    import scipy.sparse as sp
    L = hip.lib()
    E_INVALID, E_DTYPE, E_SHAPE = -1, -2, -3
    n, sig, n_masks = 6, (16, 16), 3
    rng = np.random.default_rng(_seed('arguments'))
    data = _frames(rng, 'uint16', (n, 256))
    masks = _masks(rng, 'float32', n_masks, (256,))
    dense = hip.MaskHandle.dense(0, masks, np.float32)
    csr = hip.MaskHandle.csr(0, sp.csr_matrix(np.where(masks.T > 0.5, masks.T, 0).astype(np.float32)), np.float32)
    tile = _Region(n, 256, 260, 'uint16', init=data)
    out = _Region(n, n_masks, n_masks + 2, 'float32')
    s_host = np.ascontiguousarray(rng.integers(-2, 3, (n, 2)).astype(np.int32))
    s_dev = torch.from_numpy(s_host).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    U16 = hip.dtype_code(np.uint16)

    def call(entry, h=dense, t=tile.ptr, dt=U16, frames=n, ld_tile=260, sh=16, sw=16, shifts='ok', o=out.ptr,
             ld_out=n_masks + 2):
        fn = L.ltmi_apply_masks_shifted if entry == 'device' else L.ltmi_apply_masks_shifted_host
        if shifts == 'ok':
            shifts = s_dev.data_ptr() if entry == 'device' else s_host.ctypes.data
        rc = fn(h._ptr, ctypes.c_void_p(t), dt, frames, ld_tile, sh, sw, ctypes.c_void_p(shifts), ctypes.c_void_p(o),
                ld_out, 0, ctypes.c_void_p(stream))
        _unchanged(out, f"{entry} entry, rc {rc}")
        return rc

    for entry in ('device', 'host'):
        assert call(entry, sh=16, sw=15) == E_SHAPE            # sig_h * sig_w != n_px
        assert call(entry, sh=8, sw=16) == E_SHAPE
        assert call(entry, sh=0, sw=256) == E_SHAPE            # sig_h <= 0
        assert call(entry, sh=-16, sw=-16) == E_SHAPE          # ... although the product is n_px
        assert call(entry, sh=256, sw=0) == E_SHAPE
        assert call(entry, ld_tile=255) == E_SHAPE
        assert call(entry, ld_out=n_masks - 1) == E_SHAPE
        assert call(entry, frames=-1) == E_SHAPE
        assert call(entry, dt=13) == E_DTYPE                   # behind the last code of enum ltmi_dtype
        assert call(entry, dt=-1) == E_DTYPE
        assert call(entry, t=None) == E_INVALID
        assert call(entry, o=None) == E_INVALID
        assert call(entry, shifts=None) == E_INVALID
        assert call(entry, h=csr) == E_INVALID
        assert call(entry, frames=0) == 0
        assert call(entry, frames=0, t=None, o=None, shifts=None) == 0
    # ... and both still work afterwards
    ref, scale = _slice_ref(data.reshape((n,) + sig), masks.reshape((n_masks,) + sig), s_host, np.float32)
    for entry in ('device', 'host'):
        fn = dense.apply_shifted if entry == 'device' else dense.apply_shifted_host
        fn(tile.ptr, np.uint16, n, 260, 16, 16, s_dev.data_ptr() if entry == 'device' else s_host, out.ptr,
           n_masks + 2, False)
        _check(out, ref, scale, 1e-5, f"{entry} entry after the refusals")
    dense.close()
    csr.close()


# ---- g. through run_udf ----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.mark.parametrize('shift_kind', ['constant', 'aux'])
def test_run_udf_nan_border(ctx, shift_kind):
    """ApplyMasksUDF(shifts=...) on float32 frames of 16 x 16 whose outermost rows and columns are NaN (dead pixels
    at the detector's edge), a constant shift and per-frame shifts of +-3, host-resident (streamed) and
    device-resident: NaN where `oracle.path.apply_masks_shifted` has NaN (the border rows the shift leaves inside the
    overlap reach every mask; the ones it cuts off reach none -- a shift of (3, 3) and more in both directions would
    be NaN-free only with a border on one side), the rest within rtol 1e-5, atol 1e-3."""
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.common.hiparray import HipArray
    from oracle import path as opath
    rng = np.random.default_rng(_seed('run_udf', shift_kind))
    nav, sig = (12, 25), (16, 16)
    data = (rng.random(nav + sig) * 100).astype(np.float32)
    # dead pixels: the first row and the first column of every frame, all four borders of every third frame
    data[..., 0, :] = np.nan
    data[..., :, 0] = np.nan
    third = np.arange(nav[0] * nav[1]).reshape(nav) % 3 == 0
    data[third, -1, :] = np.nan
    data[third, :, -1] = np.nan
    masks = (rng.random((4,) + sig) - 0.25).astype(np.float32)
    if shift_kind == 'constant':
        shifts = np.array([2, 1])
        sh = (2, 1)
    else:
        shifts = rng.integers(-3, 4, nav + (2,))
        sh = ApplyMasksUDF.aux_data(shifts.reshape((-1, 2)).ravel(), kind='nav', extra_shape=(2,),
                                    dtype=shifts.dtype)
    with np.errstate(all='ignore'):
        ref = opath.apply_masks_shifted(data, masks, shifts)
    nan = np.isnan(ref)
    assert nan.any() and not nan.all()                      # both kinds of frame are in the scan
    for ds in (ctx.load('memory', data=data, num_partitions=3, sig_dims=2),
               ctx.load('memory', data=HipArray.from_numpy(data, 0), num_partitions=3, sig_dims=2)):
        got = ctx.run_udf(dataset=ds, udf=ApplyMasksUDF(mask_factories=lambda: masks, shifts=sh))['intensity'].data
        assert got.shape == ref.shape and got.dtype == ref.dtype
        assert np.array_equal(np.isnan(got), nan), \
            f"{int(np.isnan(got).sum())} NaN results, the reference has {int(nan.sum())}"
        assert np.allclose(got[~nan], ref[~nan], rtol=1e-5, atol=1e-3)
