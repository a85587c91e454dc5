"""
The kernels of csrc/ltmi_reduce.hip that run before and after the main computation, called through the C ABI
(ctypes) and compared with plain NumPy / Python restatements written here: detector correction (`ltmi_correct`,
`ltmi_repair_pixels`), the ROI frame gather (`ltmi_gather_rows`), the sig-buffer merge (`ltmi_add2d`,
`ltmi_axpy`) and the two sum reductions (`ltmi_sum_sig`, `ltmi_sum_frames`).  `-m gpu` only.

Every buffer a kernel writes lies inside a larger device buffer filled with a poison pattern: after the call
the whole buffer is compared byte by byte, so padding columns, the guard bytes in front of and behind an output
and behind a workspace of exactly the queried size, and imaginary parts a call does not own must be unchanged.
"""
import math
import zlib

import numpy as np
import pytest

from oracle import corrections as ocorr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 256          # poison bytes in front of and behind every region; keeps the region's base 256-byte aligned

REAL_DTYPES = ['bool', 'uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'uint64', 'int64',
               'float32', 'float64']
INT_DTYPES = ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'uint64', 'int64']
ALL_DTYPES = REAL_DTYPES + ['complex64', 'complex128']


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
        assert self.host.nbytes <= 1 << 30
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

    def values(self):
        return self.view(self.download()).copy()


def _check(region, expected, what):
    """`region` holds `expected` bit for bit -- NaN where `expected` is NaN, whatever its payload and sign: a
    NaN that an operation creates has another sign bit on the host -- and every other byte of the buffer is what
    it was before the call.  Returns the downloaded image."""
    expected = np.asarray(expected)
    assert expected.dtype == region.dt and expected.shape == (region.rows, region.cols), what
    got = region.download()
    want = region.host.copy()
    region.view(want)[...] = expected
    if region.dt.kind in 'fc':
        g = region.view(got)
        nan = np.isnan(expected)
        assert np.array_equal(np.isnan(g), nan), f"{what}: NaN at other positions"
        g[nan] = expected[nan]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        b = int(bad[0])
        where = 'front guard' if b < region.start else 'rear guard'
        if region.start <= b < region.start + region.nbytes:
            e = (b - region.start) // region.dt.itemsize
            r, c = divmod(e, region.ld)
            where = f"row {r} column {c}" + (' (padding)' if c >= region.cols else
                                             f": got {region.view(got)[r, c]!r}, expected {expected[r, c]!r}")
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at byte {b}, {where}")
    return got


def _unchanged(region, what):
    assert np.array_equal(region.download(), region.host), f"{what}: buffer was written"


def _check_guards(region, image, what):
    """the bytes in front of and behind the region (a workspace of exactly the queried size) are untouched"""
    end = region.start + region.nbytes
    assert np.array_equal(image[:region.start], region.host[:region.start]), f"{what}: wrote in front of it"
    assert np.array_equal(image[end:], region.host[end:]), f"{what}: wrote behind its {region.nbytes} bytes"


def _sprinkle(rng, arr, specials):
    """put the `specials` at random places of `arr` (all of them if it has room)"""
    flat = arr.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, 10 * len(specials))]
    flat[pos] = np.resize(np.array(specials, dtype=arr.dtype), pos.size)
    return arr


def _full_range(rng, dtype, shape):
    """integers over the whole range of the dtype with its min, max and 0 (64-bit: mostly above 2^53); floats
    of both signs with NaN and +-inf"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.integers(0, 2, shape).astype(np.bool_)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
        return _sprinkle(rng, a, [info.min, info.max, 0])
    a = (rng.standard_normal(shape) * 1000.0).astype(dt)
    return _sprinkle(rng, a, [np.nan, np.inf, -np.inf])


# ---- 1. ltmi_correct --------------------------------------------------------------------------------------

def _dark_gain(rng, n_px, mode):
    """float64 tables with full mantissas; some gains negative or zero, one dark NaN.  |(x - dark) * gain| of a
    finite x is 0 or far above the smallest normal float32."""
    dark = rng.uniform(-300.0, 300.0, n_px)
    gain = rng.uniform(0.5, 2.0, n_px)
    gain[1::7] *= -1.0
    gain[2::11] = 0.0
    if n_px >= 3:
        dark[n_px // 2] = np.nan
    return (dark if mode in ('both', 'dark') else None), (gain if mode in ('both', 'gain') else None)


def _correct_ref(x, dark, gain, out_dtype):
    with np.errstate(all='ignore'):
        d = 0.0 if dark is None else dark
        g = 1.0 if gain is None else gain
        return ((x.astype(np.float64) - d) * g).astype(out_dtype)


def _run_correct(hip, x, dark, gain, out_dtype, ld_tile=None, ld_out=None, tile_shift=0, out_shift=0):
    n_frames, n_px = x.shape
    tile = _Region(n_frames, n_px, ld_tile or n_px, x.dtype, tile_shift, init=x)
    out = _Region(n_frames, n_px, ld_out or n_px, out_dtype, out_shift)
    d = None if dark is None else torch.from_numpy(dark).cuda()
    g = None if gain is None else torch.from_numpy(gain).cuda()
    hip.correct(0, tile.ptr, x.dtype, n_frames, n_px, tile.ld, None if d is None else d.data_ptr(),
                None if g is None else g.data_ptr(), out.ptr, out_dtype, out.ld)
    return tile, out


@pytest.mark.parametrize('mode', ['both', 'dark', 'gain', 'neither'])
@pytest.mark.parametrize('out_dtype', ['float32', 'float64'])
@pytest.mark.parametrize('tile_dtype', REAL_DTYPES)
def test_correct_every_dtype(hip, tile_dtype, out_dtype, mode):
    # (17, 2056) contiguous: the vector kernel; (15, 9) and padded rows: the scalar kernel
    for n_frames, n_px, pad_t, pad_o in [(17, 2056, 0, 0), (15, 9, 2, 3), (17, 2056, 8, 4)]:
        rng = np.random.default_rng(_seed('correct', tile_dtype, out_dtype, mode, n_px))
        x = _full_range(rng, tile_dtype, (n_frames, n_px))
        dark, gain = _dark_gain(rng, n_px, mode)
        tile, out = _run_correct(hip, x, dark, gain, out_dtype, n_px + pad_t, n_px + pad_o)
        what = f"ltmi_correct {tile_dtype}->{out_dtype} {mode} ({n_frames}, {n_px}) ld +{pad_t} / +{pad_o}"
        _check(out, _correct_ref(x, dark, gain, out_dtype), what)
        _unchanged(tile, what + ' (tile)')


@pytest.mark.parametrize('n_frames', [1, 15, 16, 17, 1000])
@pytest.mark.parametrize('n_px', [1, 3, 8, 9, 2047, 2048, 2056, 4099, 16384])
@pytest.mark.parametrize('tile_dtype,out_dtype', [('uint16', 'float32'), ('float64', 'float64')])
def test_correct_pixel_and_frame_counts(hip, tile_dtype, out_dtype, n_px, n_frames):
    rng = np.random.default_rng(_seed('correct shapes', tile_dtype, n_px, n_frames))
    x = _full_range(rng, tile_dtype, (n_frames, n_px))
    dark, gain = _dark_gain(rng, n_px, 'both')
    _, out = _run_correct(hip, x, dark, gain, out_dtype)
    _check(out, _correct_ref(x, dark, gain, out_dtype), f"ltmi_correct ({n_frames}, {n_px})")


@pytest.mark.parametrize('tile_dtype,out_dtype', [
    ('uint8', 'float32'), ('uint16', 'float32'), ('float32', 'float32'), ('uint16', 'float64'),
    ('int64', 'float32'), ('float64', 'float64'), ('bool', 'float64'),
])
def test_correct_vector_path_conditions_one_at_a_time(hip, tile_dtype, out_dtype):
    """n_px % 8, tile base % (8 * sizeof(TIn)), ld_tile % 8, out base % (4 * sizeof(TOut)), ld_out % 4 all hold
    for (17, 2048) contiguous regions at 256-byte boundaries; n_px % 8 is broken by the pixel counts above"""
    n_frames, n_px = 17, 2048
    rng = np.random.default_rng(_seed('correct alignment', tile_dtype, out_dtype))
    x = _full_range(rng, tile_dtype, (n_frames, n_px))
    dark, gain = _dark_gain(rng, n_px, 'both')
    ref = _correct_ref(x, dark, gain, out_dtype)
    _, out = _run_correct(hip, x, dark, gain, out_dtype)
    _check(out, ref, 'all aligned')
    aligned = out.values()
    isz = np.dtype(out_dtype).itemsize
    for name, kw in [
        ('tile base + 1 element', dict(tile_shift=1)),
        ('ld_tile = n_px + 1', dict(ld_tile=n_px + 1)),
        ('ld_tile = n_px + 8', dict(ld_tile=n_px + 8)),          # still the vector kernel, now with padding
        ('out base + 1 element', dict(out_shift=1)),
        ('ld_out = n_px + 1', dict(ld_out=n_px + 1)),
        ('ld_out = n_px + 4', dict(ld_out=n_px + 4)),            # still the vector kernel, now with padding
    ]:
        _, out = _run_correct(hip, x, dark, gain, out_dtype, **kw)
        _check(out, ref, name)
        got = out.values()
        assert np.array_equal(got.view(f'u{isz}'), aligned.view(f'u{isz}')), f"{name}: differs from all aligned"


def test_correct_argument_checks(hip):
    x = np.arange(32, dtype=np.uint16).reshape(4, 8)
    tile = _Region(4, 8, 8, np.uint16, init=x)
    ctile = _Region(4, 8, 8, np.complex64)
    out = _Region(4, 8, 8, np.float32)
    iout = _Region(4, 8, 8, np.int32)
    with pytest.raises(ValueError):
        hip.correct(0, tile.ptr, np.uint16, 4, 8, 7, None, None, out.ptr, np.float32, 8)      # ld_tile < n_px
    with pytest.raises(ValueError):
        hip.correct(0, tile.ptr, np.uint16, 4, 8, 8, None, None, out.ptr, np.float32, 7)      # ld_out < n_px
    with pytest.raises(ValueError):
        hip.correct(0, None, np.uint16, 4, 8, 8, None, None, out.ptr, np.float32, 8)          # null tile
    with pytest.raises(ValueError):
        hip.correct(0, ctile.ptr, np.complex64, 4, 8, 8, None, None, out.ptr, np.float32, 8)  # complex tile
    with pytest.raises(ValueError):
        hip.correct(0, tile.ptr, np.uint16, 4, 8, 8, None, None, iout.ptr, np.int32, 8)       # integer output
    hip.correct(0, tile.ptr, np.uint16, 0, 8, 8, None, None, out.ptr, np.float32, 8)          # no frames
    hip.correct(0, tile.ptr, np.uint16, 4, 0, 8, None, None, out.ptr, np.float32, 8)          # no pixels
    torch.cuda.synchronize()
    _unchanged(out, 'refused and empty ltmi_correct calls')
    _unchanged(iout, 'refused ltmi_correct call')


# ---- 2. ltmi_repair_pixels --------------------------------------------------------------------------------

REPAIR_MAX_ENV = 11          # three slots more than the eight neighbours of a 2-D pixel


def _repair_case(n_excl):
    """-> (sig shape, list of bad pixel coordinates)"""
    if n_excl == 1:
        return (5, 6), [(4, 5)]                                     # a corner: three neighbours
    if n_excl == 5:
        # (0, 0) has only bad neighbours (count 0: left alone), its three neighbours see each other
        return (6, 7), [(0, 0), (0, 1), (1, 0), (1, 1), (5, 3)]
    h, w = 40, 50
    rng = np.random.default_rng(_seed('repair coords', n_excl))
    fixed = [(0, 0), (0, 1), (1, 0), (1, 1), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 20), (17, 0),
             (h - 1, 30), (22, w - 1), (10, 10), (10, 11), (11, 10)]
    rest = [divmod(int(p), w) for p in rng.permutation(h * w)]
    coords = fixed + [c for c in rest if c not in fixed][:n_excl - len(fixed)]
    return (h, w), coords


def _repair_tables(sig_shape, coords):
    """int32 device tables of REPAIR_MAX_ENV slots per entry; the slots behind the count name `sentinel`, a good
    pixel that is nobody's neighbour where there is one"""
    excl, env, cnt = ocorr.repair_tables(sig_shape, coords)
    n_px = int(np.prod(sig_shape))
    used = set(excl.tolist())
    for e in range(len(excl)):
        used.update(env[e, :cnt[e]].tolist())
    candidates = [p for p in range(n_px) if p not in used] + \
        [p for p in range(n_px) if p not in set(excl.tolist())] + [0]
    sentinel = candidates[0]
    table = np.full((len(excl), REPAIR_MAX_ENV), sentinel, dtype=np.int32)
    for e in range(len(excl)):
        table[e, :cnt[e]] = env[e, :cnt[e]]
    assert cnt.max() < REPAIR_MAX_ENV
    return excl.astype(np.int32), table, cnt.astype(np.int32), sentinel


def _repair_ref(buf, excl, table, cnt):
    """per entry a float64 running sum over its neighbours in table order, divided by the count, rounded once"""
    out = buf.copy()
    with np.errstate(all='ignore'):
        for e in range(len(excl)):
            if cnt[e] <= 0:
                continue
            acc = np.zeros(buf.shape[0], dtype=np.float64)
            for j in range(cnt[e]):
                acc = acc + buf[:, table[e, j]].astype(np.float64)
            out[:, excl[e]] = (acc / np.float64(cnt[e])).astype(buf.dtype)
    return out


def _run_repair(hip, buf, excl, table, cnt, pad=3):
    n_frames, n_px = buf.shape
    region = _Region(n_frames, n_px, n_px + pad, buf.dtype, init=buf)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (excl, table, cnt)]
    hip.repair_pixels(0, region.ptr, buf.dtype, n_frames, region.ld, t[0].data_ptr(), t[1].data_ptr(),
                      t[2].data_ptr(), len(excl), table.shape[1])
    return region


@pytest.mark.parametrize('n_excl', [1, 5, 300])
@pytest.mark.parametrize('n_frames', [1, 255, 256, 257, 5000])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_repair_pixels(hip, dtype, n_frames, n_excl):
    sig_shape, coords = _repair_case(n_excl)
    assert len(coords) == n_excl
    excl, table, cnt, sentinel = _repair_tables(sig_shape, coords)
    if n_excl == 5:
        assert cnt[0] == 0 and 0 < cnt[1] < 8
    rng = np.random.default_rng(_seed('repair', dtype, n_frames, n_excl))
    buf = (rng.standard_normal((n_frames, int(np.prod(sig_shape)))) * 100.0).astype(dtype)
    buf[:, sentinel] = 1e30                       # read only by a loop that runs past the count
    e_nan = int(np.flatnonzero(cnt > 0)[-1])
    f_nan = n_frames // 2
    buf[f_nan, table[e_nan, 0]] = np.nan          # one NaN neighbour: that frame's repaired pixel is NaN
    ref = _repair_ref(buf, excl, table, cnt)
    assert np.isnan(ref[f_nan, excl[e_nan]])
    assert np.array_equal(ref[:, excl[cnt == 0]].view('u1'), buf[:, excl[cnt == 0]].view('u1'))
    region = _run_repair(hip, buf, excl, table, cnt)
    _check(region, ref, f"ltmi_repair_pixels {dtype} {n_frames} frames, {n_excl} entries")


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_repair_pixels_entry_without_good_neighbours(hip, dtype):
    """a (1, 3) frame whose three pixels are all bad: every count is 0, nothing is written"""
    excl, table, cnt, _ = _repair_tables((1, 3), [(0, 0), (0, 1), (0, 2)])
    assert not cnt.any()
    buf = np.arange(1, 22, dtype=dtype).reshape(7, 3)
    region = _run_repair(hip, buf, excl, table, cnt)
    _check(region, buf, 'ltmi_repair_pixels with counts of 0')


def test_repair_pixels_argument_checks(hip):
    excl, table, cnt, _ = _repair_tables((4, 4), [(1, 1)])
    buf = np.arange(64, dtype=np.float32).reshape(4, 16)
    region = _Region(4, 16, 16, np.float32, init=buf)
    ibuf = _Region(4, 16, 16, np.int32, init=buf.astype(np.int32))
    t = [torch.from_numpy(a).cuda() for a in (excl, table, cnt)]
    p = [a.data_ptr() for a in t]
    with pytest.raises(ValueError):
        hip.repair_pixels(0, region.ptr, np.float32, -1, 16, p[0], p[1], p[2], 1, REPAIR_MAX_ENV)   # negative
    with pytest.raises(ValueError):
        hip.repair_pixels(0, region.ptr, np.float32, 4, 16, p[0], p[1], p[2], -1, REPAIR_MAX_ENV)
    with pytest.raises(ValueError):
        hip.repair_pixels(0, region.ptr, np.float32, 4, 16, p[0], None, p[2], 1, REPAIR_MAX_ENV)    # null table
    with pytest.raises(ValueError):
        hip.repair_pixels(0, ibuf.ptr, np.int32, 4, 16, p[0], p[1], p[2], 1, REPAIR_MAX_ENV)        # not a float
    hip.repair_pixels(0, region.ptr, np.float32, 4, 16, p[0], p[1], p[2], 0, REPAIR_MAX_ENV)        # no entries
    torch.cuda.synchronize()
    _unchanged(region, 'refused and empty ltmi_repair_pixels calls')
    _unchanged(ibuf, 'refused ltmi_repair_pixels call')


# ---- 3. ltmi_gather_rows ----------------------------------------------------------------------------------

def _run_gather(hip, rng, n_src, row_bytes, ld_src, idx, src_shift=0, dest_shift=0, what=''):
    data = rng.integers(0, 256, (n_src, row_bytes), dtype=np.uint8)
    src = _Region(n_src, row_bytes, ld_src, np.uint8, src_shift, init=data)
    dest = _Region(len(idx), row_bytes, row_bytes, np.uint8, dest_shift)
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    idx_dev = torch.from_numpy(idx).cuda()
    hip.gather_rows(0, src.ptr, ld_src, idx_dev.data_ptr(), len(idx), row_bytes, dest.ptr)
    _check(dest, data[idx], what)
    _unchanged(src, what + ' (source)')


def _index_lists(rng, n_src):
    return {
        'identity': np.arange(n_src),
        'reversed': np.arange(n_src)[::-1],
        'permutation': rng.permutation(n_src),
        'repeats': np.array([3, 3, 0, n_src - 1, n_src - 1, n_src - 1, 0, 3]),
        'first and last': np.array([0, n_src - 1]),
    }


# copy width = the alignment that src | dest | ld_src_bytes | row_bytes share; 64 workgroups of 256 threads per
# row, so rows above 16384 units of the width take the grid-stride loop
@pytest.mark.parametrize('width,row_bytes,pad', [
    (16, 16, 0), (16, 48, 16), (16, 4096, 32), (16, 262144 + 16, 16),
    (4, 4, 4), (4, 12, 0), (4, 12, 20), (4, 600004, 8),
    (1, 1, 0), (1, 3, 2), (1, 3, 0), (1, 300001, 5),
])
def test_gather_rows_copy_widths(hip, width, row_bytes, pad):
    ld = row_bytes + pad
    assert ld % width == 0 and row_bytes % width == 0 and (width == 16 or (ld | row_bytes) % (4 * width))
    n_src = 9
    rng = np.random.default_rng(_seed('gather', row_bytes, pad))
    for name, idx in _index_lists(rng, n_src).items():
        _run_gather(hip, rng, n_src, row_bytes, ld, idx, what=f"ltmi_gather_rows {row_bytes} B rows, ld {ld}, {name}")


@pytest.mark.parametrize('src_shift,dest_shift', [(1, 0), (0, 1), (4, 0), (0, 4), (4, 4), (1, 4), (0, 0)])
def test_gather_rows_width_forced_by_a_base_pointer(hip, src_shift, dest_shift):
    """rows of 4096 bytes at a stride of 4112: the 16-byte copy unless a base pointer is off by 1 or 4 bytes"""
    rng = np.random.default_rng(_seed('gather bases', src_shift, dest_shift))
    for name, idx in _index_lists(rng, 6).items():
        _run_gather(hip, rng, 6, 4096, 4112, idx, src_shift, dest_shift,
                    what=f"ltmi_gather_rows src + {src_shift}, dest + {dest_shift}, {name}")


@pytest.mark.parametrize('row_bytes', [16, 3])
@pytest.mark.parametrize('n_rows', [65535, 65536, 2 * 65535 + 1])
def test_gather_rows_more_rows_than_one_grid(hip, n_rows, row_bytes):
    """the host walks slabs of 65535 rows (the grid's y limit): 1, 2 and 3 launches"""
    n_src = 7
    rng = np.random.default_rng(_seed('gather slabs', n_rows, row_bytes))
    idx = rng.integers(0, n_src, n_rows)
    idx[[0, 65534, -1]] = [n_src - 1, 0, n_src - 2]
    _run_gather(hip, rng, n_src, row_bytes, row_bytes + (16 if row_bytes == 16 else 2), idx,
                what=f"ltmi_gather_rows {n_rows} rows of {row_bytes} B")


def test_gather_rows_argument_checks(hip):
    src = _Region(4, 32, 32, np.uint8, init=np.arange(128, dtype=np.uint8).reshape(4, 32))
    dest = _Region(4, 32, 32, np.uint8)
    idx = torch.arange(4, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        hip.gather_rows(0, src.ptr, 16, idx.data_ptr(), 4, 32, dest.ptr)        # ld_src_bytes < row_bytes
    with pytest.raises(ValueError):
        hip.gather_rows(0, src.ptr, 32, idx.data_ptr(), -1, 32, dest.ptr)       # negative sizes
    with pytest.raises(ValueError):
        hip.gather_rows(0, src.ptr, 32, idx.data_ptr(), 4, -1, dest.ptr)
    for s, i, d in [(None, idx.data_ptr(), dest.ptr), (src.ptr, None, dest.ptr), (src.ptr, idx.data_ptr(), None)]:
        with pytest.raises(ValueError):
            hip.gather_rows(0, s, 32, i, 4, 32, d)                              # null pointers
    hip.gather_rows(0, src.ptr, 32, idx.data_ptr(), 0, 32, dest.ptr)            # no rows
    hip.gather_rows(0, src.ptr, 32, idx.data_ptr(), 4, 0, dest.ptr)             # no bytes
    torch.cuda.synchronize()
    _unchanged(dest, 'refused and empty ltmi_gather_rows calls')


# ---- 4. ltmi_add2d / ltmi_axpy ----------------------------------------------------------------------------

def _merge_values(rng, dtype, shape):
    """integers within 100 of the ends of their range (so that += and -= wrap), floats of both signs"""
    dt = np.dtype(dtype)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        lo = rng.integers(0, 101, shape, dtype=np.uint64)
        ends = np.where(rng.integers(0, 2, shape) == 1, np.uint64(info.max) - lo,
                        (np.uint64(info.min % (1 << 64)) + lo))
        return ends.astype(f'u{dt.itemsize}').view(dt)          # modulo 2^bits, read in the dtype
    if dt.kind == 'c':
        part = np.float32 if dt == np.complex64 else np.float64
        return (_merge_values(rng, part, shape) + 1j * _merge_values(rng, part, shape)).astype(dt)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(dt)


def _merge_ref(dest, src, negate):
    """NumPy's in-place arithmetic in the same dtype; integers on the unsigned view of the same width"""
    dt = dest.dtype
    if dt.kind in 'iu':
        u = f'u{dt.itemsize}'
        d, s = dest.view(u), np.broadcast_to(src, dest.shape).copy().view(u)
        return (d - s if negate else d + s).view(dt)
    return (dest - src if negate else dest + src).astype(dt)


ADD2D_SHAPES = [
    # rows, cols, ld_dest, ld_src
    (1, 1000, 1000, 1000),
    (1000, 1, 1, 1),
    (1000, 1, 3, 2),
    (7, 13, 16, 13),              # ld_dest > cols
    (7, 13, 13, 17),              # ld_src > cols
    (7, 13, 13, 0),               # one source row for every row
    (7, 13, 19, 0),
    (33, 47, 50, 49),             # 1551 elements: seven workgroups, the last one ragged
]


@pytest.mark.parametrize('negate', [False, True])
@pytest.mark.parametrize('dtype', [d for d in ALL_DTYPES if d != 'bool'])
def test_add2d(hip, dtype, negate):
    for rows, cols, ld_dest, ld_src in ADD2D_SHAPES:
        rng = np.random.default_rng(_seed('add2d', dtype, negate, rows, cols, ld_dest, ld_src))
        d0 = _merge_values(rng, dtype, (rows, cols))
        s0 = _merge_values(rng, dtype, (1 if ld_src == 0 else rows, cols))
        dest = _Region(rows, cols, ld_dest, dtype, init=d0)
        src = _Region(s0.shape[0], cols, ld_src or cols, dtype, init=s0)
        hip.add2d(0, dest.ptr, ld_dest, src.ptr, ld_src, dtype, rows, cols, negate)
        what = f"ltmi_add2d {dtype} ({rows}, {cols}) ld {ld_dest} / {ld_src} negate={negate}"
        with np.errstate(all='ignore'):
            _check(dest, _merge_ref(d0, s0, negate), what)
        _unchanged(src, what + ' (source)')


@pytest.mark.parametrize('dtype', [d for d in ALL_DTYPES if d != 'bool'])
def test_axpy(hip, dtype):
    rng = np.random.default_rng(_seed('axpy', dtype))
    for n in (1, 255, 257, 1551):
        d0 = _merge_values(rng, dtype, (1, n))
        s0 = _merge_values(rng, dtype, (1, n))
        dest = _Region(1, n, n, dtype, init=d0)
        src = _Region(1, n, n, dtype, init=s0)
        hip.axpy(0, dest.ptr, src.ptr, dtype, n)
        with np.errstate(all='ignore'):
            _check(dest, _merge_ref(d0, s0, False), f"ltmi_axpy {dtype} n={n}")
    hip.axpy(0, dest.ptr, src.ptr, dtype, 0)                                     # nothing to add
    with pytest.raises(ValueError):
        hip.axpy(0, dest.ptr, src.ptr, dtype, -1)
    for rows, cols, ld_d, ld_s in [(-1, 4, 4, 4), (4, -1, 4, 4), (1, 4, -4, 4), (1, 4, 4, -4)]:
        with pytest.raises(ValueError):
            hip.add2d(0, dest.ptr, ld_d, src.ptr, ld_s, dtype, rows, cols)
    with np.errstate(all='ignore'):
        _check(dest, _merge_ref(d0, s0, False), f"ltmi_axpy {dtype}: refused and empty calls")


def test_merge_refuses_bool(hip):
    """NumPy's `+=` on bool is a logical or and its `-=` a TypeError; adding the bytes would leave 2 in a bool.
    Nothing in the package merges a bool buffer, so the two entry points refuse the dtype."""
    assert np.dtype(bool) not in hip.AXPY_DTYPES
    assert hip.AXPY_DTYPES == frozenset(np.dtype(d) for d in ALL_DTYPES if d != 'bool')
    ones = np.ones((1, 16), dtype=bool)
    dest = _Region(1, 16, 16, bool, init=ones)
    src = _Region(1, 16, 16, bool, init=ones)
    with pytest.raises(ValueError):
        hip.axpy(0, dest.ptr, src.ptr, bool, 16)
    for negate in (False, True):
        with pytest.raises(ValueError):
            hip.add2d(0, dest.ptr, 16, src.ptr, 16, bool, 1, 16, negate)
    torch.cuda.synchronize()
    _unchanged(dest, 'refused bool merge')


# ---- 5. ltmi_sum_sig / ltmi_sum_frames --------------------------------------------------------------------

def _small_positive(rng, dtype, shape):
    """strictly positive integers <= 7 (bool: True; complex: both parts): 2049 * 7 and 4099 * 7 are far below
    2^24, so every partial sum is exact in float32 in any order"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return np.ones(shape, dtype=np.bool_)
    if dt.kind == 'c':
        return (rng.integers(1, 8, shape) + 1j * rng.integers(1, 8, shape)).astype(dt)
    return rng.integers(1, 8, shape).astype(dt)


def _wrap(values, dtype):
    """Python integers modulo 2^bits, read as `dtype`"""
    dt = np.dtype(dtype)
    values = np.asarray(values, dtype=object)
    u = np.array([int(v) % (1 << (8 * dt.itemsize)) for v in values.reshape(-1)], dtype=f'u{dt.itemsize}')
    return u.view(dt).reshape(values.shape)


def _exact_sum(x, axis, out_dtype, out0):
    """sum along `axis` in Python integers (complex: exact in complex128) plus `out0`, as `out_dtype`"""
    out_dtype = np.dtype(out_dtype)
    if out_dtype.kind in 'iu':
        if x.dtype.itemsize < 8 or int(x.max()) < 1 << 32:
            s = x.astype(np.int64).sum(axis=axis).astype(object)        # cannot overflow: fewer than 2^31 addends
        else:
            s = x.astype(object).sum(axis=axis)
        if out0 is not None:
            s = s + out0.astype(object)
        return _wrap(s, out_dtype)
    s = x.astype(np.complex128 if x.dtype.kind == 'c' else np.float64).sum(axis=axis)
    if out_dtype.kind == 'c' and out0 is None:
        s = s + 0j
    if out0 is not None:
        s = s + out0.astype(np.complex128 if out_dtype.kind == 'c' else np.float64)
    res = s.astype(out_dtype)
    assert np.array_equal(res, s)                   # representable: the reference itself did not round
    return res


def _run_sum(hip, entry, x, out_dtype, out0=None, pad=0, shift=0):
    """one call of ltmi_sum_sig ('sig') / ltmi_sum_frames ('frames') on fresh buffers; accumulates into `out0`
    if given.  -> (out region, workspace region or None)"""
    n_frames, n_px = x.shape
    tile = _Region(n_frames, n_px, n_px + pad, x.dtype, shift, init=x)
    n_out = n_frames if entry == 'sig' else n_px
    out = _Region(1, n_out, n_out, out_dtype, init=out0)
    ws = None
    if entry == 'sig':
        hip.sum_sig(0, tile.ptr, x.dtype, n_frames, n_px, tile.ld, out.ptr, out_dtype, out0 is not None)
    else:
        nbytes = hip.sum_frames_workspace(n_frames, n_px, out_dtype)
        ws = _Region(1, nbytes, nbytes, np.uint8)
        hip.sum_frames(0, tile.ptr, x.dtype, n_frames, n_px, tile.ld, out.ptr, out_dtype, out0 is not None,
                       ws.ptr)
    return out, ws


def _check_workspace(ws, what):
    if ws is not None:
        _check_guards(ws, ws.download(), what + ' (workspace)')


def _sum_exactly(hip, entry, x, out_dtype, out0, pad, shift, what):
    """two runs on fresh buffers: both equal to the exact sum, and bit-identical to each other"""
    ref = _exact_sum(x, 1 if entry == 'sig' else 0, out_dtype, None if out0 is None else out0[0])[None, :]
    images = []
    for _ in range(2):
        out, ws = _run_sum(hip, entry, x, out_dtype, out0, pad, shift)
        images.append(_check(out, ref, what))
        _check_workspace(ws, what)
    assert np.array_equal(images[0], images[1]), f"{what}: two runs differ"


def _out0(rng, out_dtype, n):
    """what an accumulating call adds to: small positive integers (complex: in both parts)"""
    return _small_positive(rng, out_dtype, (1, n))


def _sum_pairs():
    sig = [(t, o) for t in REAL_DTYPES for o in ('float32', 'float64')]
    cplx = [('complex64', 'complex64'), ('complex64', 'complex128'), ('complex128', 'complex128')]
    frames = [(t, o) for t in REAL_DTYPES for o in ('float32', 'float64', 'complex64', 'complex128')]
    ints = [(t, o) for t in ['bool'] + INT_DTYPES for o in INT_DTYPES]
    return [('sig',) + p for p in sig + cplx] + [('frames',) + p for p in frames + cplx + ints]


# (n_frames, n_px, pad, shift, accumulate): one slab / two ragged slabs (9 + 8 frames) / 256 slabs of 9 frames
# with slabs 228 .. 255 empty; whole vectors and ragged ends; rows at any element boundary
SUM_LAYOUTS = [
    (8, 256, 0, 0, False),
    (17, 257, 0, 0, True),
    (16, 4099, 5, 1, False),
    (2049, 9, 3, 1, True),
    (2049, 2048, 0, 0, False),
]


@pytest.mark.parametrize('entry,tile_dtype,out_dtype', _sum_pairs())
def test_sums_exact_every_dtype(hip, entry, tile_dtype, out_dtype):
    for n_frames, n_px, pad, shift, accumulate in SUM_LAYOUTS:
        rng = np.random.default_rng(_seed('sums', entry, tile_dtype, out_dtype, n_frames, n_px))
        x = _small_positive(rng, tile_dtype, (n_frames, n_px))
        out0 = _out0(rng, out_dtype, n_frames if entry == 'sig' else n_px) if accumulate else None
        _sum_exactly(hip, entry, x, out_dtype, out0, pad, shift,
                     f"ltmi_sum_{entry} {tile_dtype}->{out_dtype} ({n_frames}, {n_px}) +{pad} @{shift} acc={accumulate}")


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('n_frames', [1, 8, 15, 16, 17, 2049])
@pytest.mark.parametrize('n_px', [1, 7, 8, 9, 255, 256, 257, 4099])
def test_sums_exact_every_shape(hip, n_px, n_frames, accumulate):
    if n_frames == 2049 and n_px > 2048:
        n_px = 2048                                  # the empty slabs need n_px <= 2048
    for entry, tile_dtype, out_dtype in [
            ('sig', 'uint16', 'float32'), ('sig', 'float64', 'float64'), ('sig', 'complex64', 'complex64'),
            ('frames', 'uint8', 'float32'), ('frames', 'float64', 'float64'), ('frames', 'complex64', 'complex128'),
            ('frames', 'int32', 'int16'), ('frames', 'float32', 'complex64')]:
        for pad, shift in ((0, 0), (3, 1)):
            rng = np.random.default_rng(_seed('sum shapes', entry, tile_dtype, n_frames, n_px, pad))
            x = _small_positive(rng, tile_dtype, (n_frames, n_px))
            out0 = _out0(rng, out_dtype, n_frames if entry == 'sig' else n_px) if accumulate else None
            _sum_exactly(hip, entry, x, out_dtype, out0, pad, shift,
                         f"ltmi_sum_{entry} {tile_dtype}->{out_dtype} ({n_frames}, {n_px}) +{pad} @{shift} acc={accumulate}")


@pytest.mark.parametrize('out_dtype', INT_DTYPES)
@pytest.mark.parametrize('tile_dtype', INT_DTYPES)
def test_sum_frames_integer_outputs_wrap(hip, tile_dtype, out_dtype):
    """sums beyond the output width (uint64 frames: values above 2^63, so the int64 accumulation itself wraps)
    equal the Python-integer sum modulo 2^bits"""
    for n_frames, n_px, pad, shift in [(40, 300, 0, 0), (700, 33, 3, 1)]:
        rng = np.random.default_rng(_seed('sum wrap', tile_dtype, out_dtype, n_frames))
        x = _full_range(rng, tile_dtype, (n_frames, n_px))
        if tile_dtype == 'uint64':
            assert (x > np.uint64(1 << 63)).any()
        true = x.astype(object).sum(axis=0)
        info = np.iinfo(out_dtype)
        if np.dtype(tile_dtype).itemsize >= np.dtype(out_dtype).itemsize:
            assert any(not info.min <= int(v) <= info.max for v in true)
        for accumulate in (False, True):
            out0 = _full_range(rng, out_dtype, (1, n_px)) if accumulate else None
            _sum_exactly(hip, 'frames', x, out_dtype, out0, pad, shift,
                         f"ltmi_sum_frames {tile_dtype}->{out_dtype} ({n_frames}, {n_px}) acc={accumulate}")


def test_sum_frames_complex_output_of_real_frames_keeps_imaginary_parts(hip):
    """real frames into a complex buffer: imaginary parts zero after a plain call, bit-unchanged -- also a NaN
    with a payload and a negative zero -- after an accumulating one"""
    for tile_dtype, out_dtype in (('uint16', 'complex64'), ('float32', 'complex64'), ('float64', 'complex128'),
                                  ('int64', 'complex128')):
        part = 'float32' if out_dtype == 'complex64' else 'float64'
        bits = 'u4' if out_dtype == 'complex64' else 'u8'
        for n_frames, n_px in ((5, 300), (64, 1000)):
            rng = np.random.default_rng(_seed('complex out', tile_dtype, n_frames))
            x = _small_positive(rng, tile_dtype, (n_frames, n_px))
            s = x.astype(np.float64).sum(axis=0)
            out, ws = _run_sum(hip, 'frames', x, out_dtype)
            got = out.values()[0]
            assert np.array_equal(got.real, s) and np.array_equal(got.imag.view(bits), np.zeros(n_px, dtype=bits))
            _check_workspace(ws, 'complex output')
            out0 = _out0(rng, out_dtype, n_px)
            im = np.array(out0.imag[0], dtype=part)
            im.view(bits)[0] = np.array([-1], dtype='i8').astype(bits)[0] >> 1          # a NaN with a payload
            im[1] = -0.0
            im[2] = np.inf
            pairs = out0.view(part).reshape(n_px, 2)
            pairs[:, 1] = im
            out, ws = _run_sum(hip, 'frames', x, out_dtype, out0)
            got = out.values()[0].view(part).reshape(n_px, 2)
            assert np.array_equal(got[:, 0], pairs[:, 0] + s)
            assert np.array_equal(got[:, 1].view(bits), im.view(bits))
            _check_guards(out, out.download(), 'complex output, accumulating')
            _check_workspace(ws, 'complex output, accumulating')


def _fsum_axis(x, axis):
    """correctly rounded sums along `axis` (math.fsum), complex parts separately"""
    if x.dtype.kind == 'c':
        return _fsum_axis(x.real, axis) + 1j * _fsum_axis(x.imag, axis)
    x = np.moveaxis(x.astype(np.float64), axis, -1)
    return np.array([math.fsum(row) for row in x])


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('entry,tile_dtype,out_dtype', [
    ('sig', 'float32', 'float32'), ('sig', 'float32', 'float64'), ('sig', 'float64', 'float32'),
    ('sig', 'float64', 'float64'), ('sig', 'complex64', 'complex64'), ('sig', 'complex64', 'complex128'),
    ('sig', 'complex128', 'complex128'),
    ('frames', 'float32', 'float32'), ('frames', 'float32', 'float64'), ('frames', 'float64', 'float32'),
    ('frames', 'float64', 'float64'), ('frames', 'complex64', 'complex64'), ('frames', 'complex64', 'complex128'),
    ('frames', 'complex128', 'complex128'), ('frames', 'float32', 'complex64'), ('frames', 'float64', 'complex128'),
])
def test_sums_of_signed_floats(hip, entry, tile_dtype, out_dtype, accumulate):
    """data that cancel: |got - ref| <= n u sum|x| + u |ref| per real part, n addends, u the unit round-off of the
    accumulate type (float for float32 / complex64 outputs, else double) -- the bound of recursive summation
    in any order, with one more rounding for the result; ref = math.fsum"""
    u = 2.0 ** -24 if out_dtype in ('float32', 'complex64') else 2.0 ** -53
    axis = 1 if entry == 'sig' else 0
    for n_frames, n_px, pad, shift in [(100, 700, 0, 0), (33, 1537, 3, 1), (2049, 40, 0, 0)]:
        rng = np.random.default_rng(_seed('float sums', entry, tile_dtype, out_dtype, n_frames, accumulate))
        re = rng.standard_normal((n_frames, n_px)) * 10.0 ** rng.integers(-2, 3, (n_frames, n_px))
        if np.dtype(tile_dtype).kind == 'c':
            x = (re + 1j * rng.standard_normal((n_frames, n_px)) * 100.0).astype(tile_dtype)
        else:
            x = re.astype(tile_dtype)
        n_out = x.shape[1 - axis]
        n = x.shape[axis]
        out0 = None
        if accumulate:
            out0 = rng.standard_normal((1, n_out)) * 1000.0
            if np.dtype(out_dtype).kind == 'c':
                out0 = out0 + 1j * rng.standard_normal((1, n_out)) * 1000.0
            out0 = out0.astype(out_dtype)
            n += 1
        images = []
        for _ in range(2):
            out, ws = _run_sum(hip, entry, x, out_dtype, out0, pad, shift)
            images.append(out.download())
            _check_workspace(ws, 'float sums')
        assert np.array_equal(images[0], images[1]), "two runs differ"
        _check_guards(out, images[0], 'float sums')
        got = out.view(images[0])[0].astype(np.complex128)
        terms = x.astype(np.complex128)
        if accumulate:
            terms = np.concatenate([terms, out0.astype(np.complex128)] if axis == 0 else
                                   [terms, out0.astype(np.complex128).T], axis=axis)
        ref = _fsum_axis(terms, axis)
        worst = 0.0
        for part in ('real', 'imag'):
            if part == 'imag' and np.dtype(out_dtype).kind != 'c':
                continue
            t, g, r = getattr(terms, part), getattr(got, part), getattr(ref, part)
            if part == 'imag' and np.dtype(tile_dtype).kind != 'c':
                # imaginary parts of a complex buffer fed with real frames: zero, or what they were
                want = np.zeros(n_out) if out0 is None else out0[0].imag.astype(np.float64)
                assert np.array_equal(g, want)
                continue
            bound = n * u * _fsum_axis(np.abs(t), axis) + u * np.abs(r)
            err = np.abs(g - r)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"({n_frames}, {n_px}) {part}: error {err.max()} above the bound"
        print(f"ltmi_sum_{entry} {tile_dtype}->{out_dtype} ({n_frames}, {n_px}) acc={accumulate}: "
              f"largest error / bound = {worst:.3g}")


def test_sums_argument_checks(hip):
    x = np.ones((4, 8), dtype=np.float32)
    tile = _Region(4, 8, 8, np.float32, init=x)
    out = _Region(1, 8, 8, np.float32)
    ws = _Region(1, 64, 64, np.uint8)
    with pytest.raises(ValueError):
        hip.sum_sig(0, tile.ptr, np.float32, 4, 8, 7, out.ptr, np.float32, False)                # ld < n_px
    with pytest.raises(ValueError):
        hip.sum_frames(0, tile.ptr, np.float32, 4, 8, 7, out.ptr, np.float32, False, ws.ptr)
    with pytest.raises(ValueError):
        hip.sum_sig(0, tile.ptr, np.float32, 4, 8, 8, out.ptr, np.int32, False)                  # integer sums of
    with pytest.raises(ValueError):                                                                # float frames
        hip.sum_frames(0, tile.ptr, np.float32, 4, 8, 8, out.ptr, np.int32, False, ws.ptr)
    with pytest.raises(ValueError):
        hip.sum_frames(0, tile.ptr, np.uint8, 4, 8, 8, out.ptr, np.bool_, False, ws.ptr)         # bool sums
    with pytest.raises(ValueError):
        hip.sum_sig(0, tile.ptr, np.complex128, 2, 2, 2, out.ptr, np.complex64, False)           # narrower
    hip.sum_sig(0, tile.ptr, np.float32, 0, 8, 8, out.ptr, np.float32, False)                    # no frames
    hip.sum_frames(0, tile.ptr, np.float32, 0, 8, 8, out.ptr, np.float32, False, ws.ptr)
    hip.sum_frames(0, tile.ptr, np.float32, 4, 0, 8, out.ptr, np.float32, False, ws.ptr)         # no pixels
    torch.cuda.synchronize()
    _unchanged(out, 'refused and empty sum calls')
    _unchanged(ws, 'refused and empty sum calls (workspace)')
