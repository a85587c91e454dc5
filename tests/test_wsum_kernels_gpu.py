"""
`ltmi_wsum_frames` (csrc/ltmi_wsum.hip) through the C ABI (ctypes) against float64 NumPy: out[c, p] (+)=
sum_n weights[n, c] * frame_n[p].  `-m gpu` only.

As in tests/test_reduce_kernels_gpu.py every buffer the kernel touches lies inside a larger device buffer filled with
a poison pattern; after the call the whole buffer is compared byte by byte: the padding columns of the output rows,
the gaps between components (comp_stride larger than a frame), the guards around the output and around a workspace
of exactly the queried size must be unchanged, and the tile and the weights are not written.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 256

DTYPES = ['bool', 'uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32']


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _poison(n):
    return np.resize(((np.arange(251) * 151 + 7) % 251 + 1).astype(np.uint8), n)


class _Region:
    """(rows, cols) of `dtype` at leading dimension `ld` (elements) inside a poisoned device buffer, starting `shift`
    elements behind a 256-byte boundary; `init` fills the owned elements, everything else stays poison"""

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
        flat = image[self.start:self.start + self.nbytes].view(self.dt)
        return flat.reshape(self.rows, self.ld)[:, :self.cols]

    def download(self):
        return self.dev.cpu().numpy()


class _Out:
    """k components of (rows, cols) float32 at row stride ld_out and component stride comp_stride, poisoned around
    and in between; `init` (k, rows, cols) fills the owned elements"""

    def __init__(self, k, rows, cols, ld_out, comp_stride, init=None, shift=0):
        assert ld_out >= cols and (k == 1 or comp_stride >= (rows - 1) * ld_out + cols)
        self.k, self.rows, self.cols, self.ld_out, self.comp_stride = k, rows, cols, ld_out, comp_stride
        self.start = GUARD + 4 * shift
        self.n_elems = (k - 1) * comp_stride + (rows - 1) * ld_out + cols
        self.host = _poison(self.start + 4 * self.n_elems + GUARD)
        if init is not None:
            self.view(self.host)[...] = init
        self.dev = torch.from_numpy(self.host).cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.start

    def view(self, image):
        flat = image[self.start:self.start + 4 * self.n_elems].view(np.float32)
        return np.lib.stride_tricks.as_strided(
            flat, (self.k, self.rows, self.cols), (4 * self.comp_stride, 4 * self.ld_out, 4))

    def download(self):
        return self.dev.cpu().numpy()

    def untouched_outside(self, image, what):
        """every byte that is not an owned element is what it was"""
        mask = np.ones(image.size, dtype=bool)
        owned = np.zeros(self.n_elems, dtype=bool)
        np.lib.stride_tricks.as_strided(owned, (self.k, self.rows, self.cols),
                                        (self.comp_stride, self.ld_out, 1))[...] = True
        mask[self.start:self.start + 4 * self.n_elems] = ~np.repeat(owned, 4)
        assert np.array_equal(image[mask], self.host[mask]), f"{what}: wrote outside the owned output elements"


def _frames(rng, dtype, n, n_px, signed_values=True):
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.integers(0, 2, (n, n_px)).astype(np.bool_)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        lo, hi = max(info.min, -(1 << 20)), min(info.max, 1 << 20)
        return rng.integers(lo, hi, (n, n_px), endpoint=True).astype(dt)
    return (rng.standard_normal((n, n_px)) * 10.0 ** rng.integers(-2, 3, (n, n_px))).astype(dt)


def _run(hip, x, w, sig=None, pad=0, shift=0, ld_w=None, out0=None, pad_out=0, gap=0, out_shift=0):
    """one call on fresh buffers -> (out image bytes, _Out, got (k, rows, cols) float32)"""
    n, n_px = x.shape
    k = w.shape[1]
    rows, cols = sig if sig is not None else (1, n_px)
    assert rows * cols == n_px
    tile = _Region(max(n, 1), n_px, n_px + pad, x.dtype, shift, init=x if n else None)
    ld_w = k + 3 if ld_w is None else ld_w
    wreg = _Region(max(n, 1), k, ld_w, np.float32, init=w if n else None)
    ld_out = cols + pad_out
    comp_stride = (rows - 1) * ld_out + cols + gap
    out = _Out(k, rows, cols, ld_out, comp_stride, init=out0, shift=out_shift)
    nbytes = hip.wsum_workspace(n, n_px, k)
    assert (nbytes > 0) == (n > 0)
    ws = _Region(1, max(nbytes, 1), max(nbytes, 1), np.uint8)
    hip.wsum_frames(0, tile.ptr, x.dtype, n, n_px, tile.ld, wreg.ptr, k, ld_w, out.ptr, comp_stride,
                    out0 is not None, ws.ptr, cols=cols, ld_out=ld_out)
    torch.cuda.synchronize()
    what = f"ltmi_wsum_frames {x.dtype} ({n}, {n_px}) k={k}"
    image = out.download()
    out.untouched_outside(image, what)
    ws_image = ws.download()
    end = ws.start + (nbytes if n else 0)
    assert np.array_equal(ws_image[:ws.start], ws.host[:ws.start]), f"{what}: wrote in front of the workspace"
    assert np.array_equal(ws_image[end:], ws.host[end:]), f"{what}: wrote behind the {nbytes} workspace bytes"
    assert np.array_equal(tile.download(), tile.host), f"{what}: the tile was written"
    assert np.array_equal(wreg.download(), wreg.host), f"{what}: the weights were written"
    return image, out, out.view(image).copy()


def _reference(x, w, out0=None):
    """-> (ref, bound) float64 (k, n_px): sum_n w x and sum_n |w| |x|, plus what the output held"""
    with np.errstate(all='ignore'):
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        ref = w64.T @ x64
        bound = np.abs(w64).T @ np.abs(x64)
        if out0 is not None:
            ref = ref + out0.reshape(ref.shape).astype(np.float64)
            bound = bound + np.abs(out0.reshape(ref.shape).astype(np.float64))
    return ref, bound


def _check_bound(got, ref, bound, what):
    err = np.abs(got.reshape(ref.shape).astype(np.float64) - ref)
    lim = 1e-5 * bound + 1e-30
    worst = float((err / lim).max()) if err.size else 0.0
    print(f"{what}: largest error / bound = {worst:.3g}")
    assert (err <= lim).all(), f"{what}: error {err.max()} above the bound, {worst:.3g} x"


# (n_frames, sig, k, dtype, accumulate): every value of every axis, and the two pairs of the specification
CASES = [
    (1000, (3, 515), 17, 'uint16', False),
    (1, (16, 16), 64, 'float32', False),
    (7, (16, 16), 1, 'uint8', True),
    (33, (3, 515), 3, 'int16', True),
    (33, (16, 16), 16, 'bool', False),
    (7, (3, 515), 64, 'int8', False),
    (1000, (16, 16), 3, 'uint32', True),
    (33, (3, 515), 17, 'int32', False),
    (1000, (3, 515), 16, 'float32', True),
    (1, (3, 515), 1, 'uint16', True),
]


@pytest.mark.parametrize('n,sig,k,dtype,accumulate', CASES)
def test_wsum_signed_weights_within_the_bound(hip, n, sig, k, dtype, accumulate):
    """|got - ref64| <= 1e-5 sum_n |w| |x| + 1e-30 per entry (the project's bound for signed float32 sums,
    test_run_udf_elementwise_error_bound), signed weights; the (3, 515) slices start one element behind an aligned
    address with ld_tile = n_px + 5, every output has padded rows and a gap between its components; two calls give
    identical bytes"""
    rng = np.random.default_rng(_seed('wsum', n, sig, k, dtype))
    n_px = sig[0] * sig[1]
    x = _frames(rng, dtype, n, n_px)
    w = rng.standard_normal((n, k)).astype(np.float32)
    odd = sig == (3, 515)
    out0 = (rng.standard_normal((k,) + sig) * 100.0).astype(np.float32) if accumulate else None
    kw = dict(sig=sig, pad=5 if odd else 0, shift=1 if odd else 0, out0=out0, pad_out=3, gap=7,
              out_shift=1 if odd else 0)
    image_a, _, got = _run(hip, x, w, **kw)
    image_b, _, _ = _run(hip, x, w, **kw)
    assert np.array_equal(image_a, image_b), "two calls differ"
    ref, bound = _reference(x, w, out0)
    _check_bound(got, ref, bound, f"{dtype} ({n}, {sig}) k={k} acc={accumulate}")


def test_wsum_no_frames_is_a_no_op(hip):
    for accumulate in (False, True):
        x = np.zeros((0, 256), dtype=np.uint16)
        w = np.zeros((0, 3), dtype=np.float32)
        out0 = np.arange(3 * 256, dtype=np.float32).reshape(3, 16, 16) if accumulate else None
        image, out, got = _run(hip, x, w, sig=(16, 16), out0=out0, pad_out=2, gap=5)
        assert np.array_equal(image, out.host)


def test_wsum_many_frames_positive_weights(hip):
    """8192 frames of (8, 32) uint16 with positive weights: 256 slabs of 32 frames (k = 1) and 32 slabs of 256
    (k = 16), merged in float64"""
    rng = np.random.default_rng(_seed('wsum long'))
    x = rng.integers(0, 65535, (8192, 256), endpoint=True).astype(np.uint16)
    for k in (1, 16):
        w = rng.uniform(0.1, 2.0, (8192, k)).astype(np.float32)
        _, _, got = _run(hip, x, w, sig=(8, 32))
        ref, bound = _reference(x, w)
        _check_bound(got, ref, bound, f"8192 frames, positive weights, k={k}")


@pytest.mark.parametrize('dtype', ['bool', 'uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32'])
def test_wsum_integer_weights_are_exact(hip, dtype):
    """integer frames, integer-valued weights in [-3, 3], every sum_n |w| |x| < 2^24: equality"""
    rng = np.random.default_rng(_seed('wsum exact', dtype))
    dt = np.dtype(dtype)
    for n, sig, k in [(1000, (3, 515), 17), (33, (16, 16), 64), (7, (16, 16), 3)]:
        n_px = sig[0] * sig[1]
        top = 1 if dt == np.bool_ else min(int(np.iinfo(dt).max), (1 << 24) // (3 * n) - 1)
        low = 0 if dt.kind in 'ub' else -top
        x = rng.integers(low, top, (n, n_px), endpoint=True).astype(dt)
        w = rng.integers(-3, 3, (n, k), endpoint=True).astype(np.float32)
        ref, bound = _reference(x, w)
        assert bound.max() < 1 << 24
        odd = sig == (3, 515)
        _, _, got = _run(hip, x, w, sig=sig, pad=5 if odd else 0, shift=1 if odd else 0)
        assert np.array_equal(got.reshape(ref.shape).astype(np.float64), ref), f"{dtype} ({n}, {sig}) k={k}"


def test_wsum_non_finite_pixels_stay_in_their_pixel(hip):
    """one NaN and one inf pixel in float32 frames, one column of zero weights: exactly those pixels' outputs are
    non-finite, in every component (0 * NaN is NaN, as in NumPy's dense W.T @ X), the others are within the bound"""
    rng = np.random.default_rng(_seed('wsum nonfinite'))
    for n, sig, k in [(33, (16, 16), 3), (1000, (3, 515), 17)]:
        n_px = sig[0] * sig[1]
        x = rng.standard_normal((n, n_px)).astype(np.float32)
        w = rng.standard_normal((n, k)).astype(np.float32)
        w[:, 1] = 0.0
        p_nan, p_inf = 5, n_px - 2
        x[n // 2, p_nan] = np.nan
        x[n - 1, p_inf] = np.inf
        _, _, got = _run(hip, x, w, sig=sig, pad=5, shift=1)
        got = got.reshape((k, n_px))
        bad = np.zeros((k, n_px), dtype=bool)
        bad[:, [p_nan, p_inf]] = True
        with np.errstate(all='ignore'):
            dense = w.astype(np.float64).T @ x.astype(np.float64)
        assert np.array_equal(~np.isfinite(dense), bad)                     # what NumPy's dense product does
        assert np.array_equal(~np.isfinite(got), bad)
        assert np.isnan(got[:, p_nan]).all() and np.isnan(got[1, p_inf])
        good = [p for p in range(n_px) if p not in (p_nan, p_inf)]
        ref, bound = _reference(x[:, good], w)
        _check_bound(got[:, good], ref, bound, f"finite pixels beside a NaN and an inf, ({n}, {sig}) k={k}")


def test_wsum_refusals_write_nothing(hip):
    x = np.ones((4, 12), dtype=np.uint16)
    tile = _Region(4, 12, 12, np.uint16, init=x)
    ftile = _Region(4, 12, 12, np.float64, init=x.astype(np.float64))
    ctile = _Region(4, 12, 12, np.complex64, init=x.astype(np.complex64))
    w = _Region(4, 65, 65, np.float32, init=np.ones((4, 65), dtype=np.float32))
    out = _Region(65, 12, 12, np.float32)
    ws = _Region(1, 1 << 16, 1 << 16, np.uint8)

    def call(tile_region=tile, dtype=np.uint16, k=2, cols=12, ld_out=12):
        hip.wsum_frames(0, tile_region.ptr, dtype, 4, 12, 12, w.ptr, k, 65, out.ptr, 12, False, ws.ptr, cols=cols,
                        ld_out=ld_out)

    with pytest.raises(ValueError, match=r'k = 0 .*code -3'):
        call(k=0)
    with pytest.raises(ValueError, match=r'k = 65 .*code -3'):
        call(k=65)
    with pytest.raises(ValueError, match=r'float64.*code -2'):
        call(ftile, np.float64)
    with pytest.raises(ValueError, match=r'complex64.*code -2'):
        call(ctile, np.complex64)
    with pytest.raises(ValueError, match=r'code -3'):
        call(cols=5, ld_out=5)                                              # cols does not divide n_px
    torch.cuda.synchronize()
    for region in (out, ws, tile, w):
        assert np.array_equal(region.download(), region.host), "a refused call wrote"
