"""
The unshifted mask products -- `ltmi_apply_masks`, `ltmi_apply_masks_rows`, `ltmi_apply_masks_csr` -- on every kernel
route behind them (the table in tests/guarded.py), with every buffer inside a guarded allocation.  `-m gpu` only.

Per route, tile dtype and shape:
  A  the call writes its (n_frames, n_masks) rectangle of `out` (ld_out = n_masks + 3, one element behind a 256-byte
     boundary) and nothing else; the tile buffer is unchanged; with no frames nothing changes at all;
  B  what surrounds the tile -- row padding, the elements before the first and after the last frame -- does not reach
     the result: 0, quiet NaN and +Inf there (integer frames: 0 and the dtype's maximum) give the same bits;
  C  frames do not reach each other: NaN / +Inf in every third frame of a contiguous tile leave the rows of the clean
     frames bit for bit, and the bad frames' rows are what the handle's arithmetic says (dense: every weight is
     multiplied, 0 * NaN = NaN; CSR: stored entries only); k_dense_split, which takes whole slots only, at those;
  D  a row list over a tile whose unnamed frames are NaN gives the bits of the product of the gathered frames: of the
     row-list kernel over the list 0 .. n - 1 always, and of the frame-range kernel wherever the two sum in the same
     order (all launches but k_dense_lds in 8, 16, 32 or 64 pixel parts: guarded.parts_in_turn);
  E  small integers in both factors: every partial sum is an integer below 2^24 (2^53), so the result IS the int64
     product, whatever the summation order -- zero tolerance for a dropped, doubled or swapped element.
Every call asserts its route through `last_kernel()`: a route the dispatch no longer takes fails, it does not skip.
B, C and D compare bits of two runs of the same kernel, E compares with exact integers.  The one tolerance below is
D's for the launches named there: row-list and frame-range result each against the float64 product, 1e-5 (scale + 1),
2e-6 (scale + 1) on the float16-piece route.
"""
import re

import numpy as np
import pytest

import guarded as G

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PARAMS = G.case_params()
SPARSE_SWITCHES = ('LTMI_SPARSE_BELL', 'LTMI_SPARSE_SCATTER', 'LTMI_SPARSE_BAND', 'LTMI_BELL_F16', 'LTMI_DENSE_F16',
                   'LTMI_DENSE_F32_INSTR', 'LTMI_SPLIT')


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert _hip.device_count() >= 1
    return _hip


class Route:
    """the handle of one (case, pixel shape) and the calls through it; every call asserts the route"""

    def __init__(self, hip, monkeypatch, case, tile_dtype, shape, integer):
        self.case, self.dt = case, np.dtype(tile_dtype)
        self.n_px, self.sig, centre = shape
        for k in SPARSE_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        self.stack = G.make_stack(case, self.n_px, self.sig, centre, integer)
        self.dense = G.dense_of(self.stack)
        self.n_masks = self.dense.shape[0]
        self.rd = np.dtype(case.result)
        if case.sparse():
            self.h = hip.MaskHandle.csr(0, self.stack, self.rd)
        else:
            self.h = hip.MaskHandle.dense(0, self.stack, self.rd)
        if self.sig is not None:
            self.h.set_sig_shape(*self.sig)
        if case.handle == 'band':
            assert self.h.kind() == 3, "no banded image"
        if case.tuning is not None:
            self.h.set_tuning(*case.tuning)
        self.seen, self.parts = set(), set()

    def what(self, *more):
        return f"{self.case.id} {self.dt} n_px={self.n_px} " + ' '.join(str(m) for m in more)

    def run(self, tile, out, n, acc, rows=None):
        if rows is None:
            self.h.apply(tile.ptr, self.dt, n, tile.ld, out.ptr, out.ld, acc)
        else:
            assert self.h.apply_rows(tile.ptr, self.dt, rows.data_ptr(), n, tile.ld, out.ptr, out.ld, acc), \
                self.what("row list not handled")
        torch.cuda.synchronize()
        kern = self.h.last_kernel()
        if n > 0:
            for e in self.case.expect + ((',rows',) if rows is not None else ()):
                assert (e[1:] not in kern) if e.startswith('!') else (e in kern), self.what("took", kern)
            self.seen.add(kern.split(' grid=')[0] + (' +nf' if kern.endswith('+nf') else ''))
            grid = re.search(r'grid=\((\d+),(\d+)', kern)
            if grid:
                self.parts.add(int(grid.group(2)))
                if self.case.parts and self.n_px == max(self.case.n_px):
                    assert int(grid.group(2)) == self.case.parts, self.what("took", kern)
        return kern

    def guarded(self):
        """float frames on a CSR handle's fast images go through the non-finite guard (ltmi_guard.hip)"""
        return self.case.sparse() and self.dt == np.float32 and 'sell' not in self.case.id

    def close(self):
        print(f"ROUTE {self.case.id} {self.dt}: {sorted(self.seen)} grid.y {sorted(self.parts)}")
        self.h.close()

    def tile(self, data, placement, fill):
        ld, shift = placement
        return G.Region(data.shape[0], self.n_px, ld, self.dt, shift=shift, init=data, fill=fill)

    def out(self, n, base=None):
        return G.Region(n, self.n_masks, self.n_masks + 3, self.rd, shift=1, init=base)

    def base(self, rng, n):
        """integer-valued results to accumulate into"""
        b = rng.integers(-100, 100, (n, self.n_masks), endpoint=True)
        if self.rd.kind == 'c':
            return (b + 1j * rng.integers(-100, 100, (n, self.n_masks), endpoint=True)).astype(self.rd)
        return b.astype(self.rd)


def _bad_fill(dt):
    return 'nan' if np.dtype(dt).kind in 'fc' else 'max'


def _same_non_finite(res, ref):
    for part in ((np.real, np.imag) if np.iscomplexobj(ref) or np.iscomplexobj(res) else (np.asarray,)):
        a, b = part(res), part(ref)
        if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
                and np.array_equal(np.isneginf(a), np.isneginf(b))):
            return False
    return True


def _all_nan(res):
    return bool(np.all(np.isnan(res.real)) and np.all(np.isnan(res.imag))) if np.iscomplexobj(res) \
        else bool(np.all(np.isnan(res)))


# ---- A: write containment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('param', PARAMS, ids=G.param_id)
def test_writes_stay_inside_the_result_rectangle(hip, monkeypatch, param):
    case, tile_dtype = param
    for shape in case.pixel_shapes():
        r = Route(hip, monkeypatch, case, tile_dtype, shape, integer=False)
        rng = np.random.default_rng(G.seed('A', case.id, tile_dtype, shape[0]))
        for n in case.frames:
            data = G.real_frames(rng, tile_dtype, (n, r.n_px))
            base = r.base(rng, n)
            for placement in G.placements(case, r.n_px, r.dt.itemsize):
                tile = r.tile(data, placement, 'zero')
                out = r.out(n, base)
                for acc in (False, True):
                    out.load(base)
                    r.run(tile, out, n, acc)
                    G.unchanged_outside(out, r.what('n_frames', n, 'ld_tile', placement[0], 'accumulate', acc))
                    G.unchanged(tile, r.what('n_frames', n))
                    assert not np.array_equal(out.result(), base), r.what("nothing was written")
        # no frames: nothing at all changes
        tile = r.tile(G.real_frames(rng, tile_dtype, (1, r.n_px)), G.placements(case, r.n_px, r.dt.itemsize)[0], 'zero')
        out = r.out(1, r.base(rng, 1))
        r.run(tile, out, 0, False)
        G.unchanged(out, r.what('n_frames 0'))
        G.unchanged(tile, r.what('n_frames 0'))
        r.close()


# ---- B: surroundings do not reach the result ------------------------------------------------------------------------
@pytest.mark.parametrize('param', PARAMS, ids=G.param_id)
def test_surroundings_of_the_tile_do_not_reach_the_result(hip, monkeypatch, param):
    case, tile_dtype = param
    fills = G.input_fills(tile_dtype)
    for shape in case.pixel_shapes():
        r = Route(hip, monkeypatch, case, tile_dtype, shape, integer=False)
        rng = np.random.default_rng(G.seed('B', case.id, tile_dtype, shape[0]))
        for n in case.frames:
            data = G.real_frames(rng, tile_dtype, (n, r.n_px))
            for placement in G.placements(case, r.n_px, r.dt.itemsize):
                tile = r.tile(data, placement, fills[0])
                out = r.out(n)
                got = {}
                for fill in (fills[0],) + fills:            # the first twice: the kernels are repeatable
                    tile.load(fill=fill)
                    out.load()
                    r.run(tile, out, n, False)
                    res = out.result()
                    what = r.what('n_frames', n, 'ld_tile', placement[0], 'surroundings', fill)
                    if fill not in got:
                        got[fill] = res
                    else:
                        assert res.tobytes() == got[fill].tobytes(), what + ": two runs differ (precondition)"
                    assert res.tobytes() == got[fills[0]].tobytes(), \
                        what + f": {int((res != got[fills[0]]).sum())} results differ from the run with 0 around " \
                               f"the tile, {int((~np.isfinite(res)).sum()) if res.dtype.kind in 'fc' else 0} not finite"
                    if case.sparse() and r.dt.kind == 'f':
                        assert r.h.nonfinite_frames() == 0, what + ": the guard repaired a read"
        r.close()


# ---- C: frames do not reach each other ------------------------------------------------------------------------------
C_PARAMS = [p for p in PARAMS if p[1] in ('float32', 'float64') and G.c_shapes(p[0])[0]]


@pytest.mark.parametrize('param', C_PARAMS, ids=G.param_id)
def test_frames_do_not_reach_each_other(hip, monkeypatch, param):
    case, tile_dtype = param
    shapes, frames = G.c_shapes(case)
    for shape in shapes:
        r = Route(hip, monkeypatch, case, tile_dtype, shape, integer=False)
        rng = np.random.default_rng(G.seed('C', case.id, tile_dtype, shape[0]))
        for n in frames:
            clean = G.real_frames(rng, tile_dtype, (n, r.n_px))
            bad = G.bad_frames(n)
            assert (~bad).sum() >= 2
            tile = r.tile(clean, (r.n_px, 0), 'zero')                 # ld_tile == n_px: frame after frame
            out = r.out(n)
            r.run(tile, out, n, False)
            base = out.result()
            assert np.all(np.isfinite(base))
            for whole in (False, True):
                px_bad = G.bad_pixels(r.n_px, whole)
                for value in (np.nan, np.inf):
                    dirty = clean.copy()
                    dirty[np.ix_(bad, px_bad)] = value
                    tile.load(dirty)
                    out.load()
                    kern = r.run(tile, out, n, False)
                    res = out.result()
                    what = r.what('n_frames', n, 'whole frame' if whole else '40 + 40 pixels', value)
                    assert res[~bad].tobytes() == base[~bad].tobytes(), \
                        what + f": clean frames changed, rows {np.flatnonzero((res != base).any(axis=1) & ~bad)[:8]}"
                    if case.sparse():
                        ref = G.stored_entries_ref(dirty[bad], r.stack)
                        assert _same_non_finite(res[bad], ref), what + ": not the stored entries' pattern"
                        hit = int((~np.isfinite(ref.real) | ~np.isfinite(ref.imag)).any(axis=1).sum())
                        if r.guarded():
                            assert kern.endswith('+nf'), kern
                            assert r.h.nonfinite_frames() == hit, what
                        else:
                            assert r.h.nonfinite_frames() == 0, what
                    elif np.isnan(value):
                        assert _all_nan(res[bad]), what + ": a bad frame's result is not NaN"
                    elif 'k_dense_split' in kern:
                        # (the opt-in split route may return NaN for an infinity: its header says so)
                        assert not np.isfinite(res[bad].view(np.float32)).any(), what
                    else:
                        assert _same_non_finite(res[bad], G.elementwise_ref(dirty[bad], r.dense)), \
                            what + ": not the element-by-element pattern"
        r.close()


# ---- D: row lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('param', [p for p in PARAMS if p[0].rows], ids=G.param_id)
def test_row_lists_read_the_named_frames_only(hip, monkeypatch, param):
    case, tile_dtype = param
    for shape in case.pixel_shapes():
        r = Route(hip, monkeypatch, case, tile_dtype, shape, integer=False)
        rng = np.random.default_rng(G.seed('D', case.id, tile_dtype, shape[0]))
        placement = G.placements(case, r.n_px, r.dt.itemsize)[0]
        for n in (f for f in case.frames if f >= 2):
            n_tile, rows = G.row_list(rng, n)
            assert len(set(rows.tolist())) == n - 1
            data = np.full((n_tile, r.n_px), G.fill_value(tile_dtype, _bad_fill(tile_dtype)), dtype=r.dt)
            data[np.unique(rows)] = G.real_frames(rng, tile_dtype, (n - 1, r.n_px))
            tile = r.tile(data, placement, _bad_fill(tile_dtype))
            gathered = r.tile(data[rows], placement, 'zero')
            rows_dev = torch.from_numpy(rows).cuda()
            one_by_one = torch.arange(n, dtype=torch.int32).cuda()
            base = r.base(rng, n)
            for acc in (False, True):
                out, out_g, out_r = r.out(n, base), r.out(n, base), r.out(n, base)
                r.run(tile, out, n, acc, rows=rows_dev)
                what = r.what('rows', n, 'of', n_tile, 'accumulate', acc)
                G.unchanged_outside(out, what)
                if case.sparse() and r.dt.kind == 'f':
                    assert r.h.nonfinite_frames() == 0, what + ": the guard repaired a read"
                res = out.result()
                # the same kernel over the gathered frames, named one by one
                r.run(gathered, out_r, n, acc, rows=one_by_one)
                want = out_r.result()
                assert res.tobytes() == want.tobytes(), \
                    what + f": rows {np.flatnonzero((res != want).any(axis=1))[:8]} differ from the gathered frames' " \
                           f"through the list 0 .. n - 1"
                # the frame-range kernel over the gathered frames
                kern = r.run(gathered, out_g, n, acc)
                want = out_g.result()
                if not G.parts_in_turn(kern):
                    assert res.tobytes() == want.tobytes(), \
                        what + f": rows {np.flatnonzero((res != want).any(axis=1))[:8]} differ from the gathered frames'"
                else:
                    # (its parts sum other pixels than the row-list kernel's: both against the float64 product, within
                    # the tolerance of this route's tests in test_kernels_gpu.py)
                    assert r.rd == np.float32 and r.dt.kind != 'c'
                    ref, scale = G.float64_product(data[rows], r.dense)
                    if acc:
                        ref, scale = ref + base, scale + np.abs(base)
                    tol = (2e-6 if ',f16' in kern else 1e-5) * (scale + 1)
                    for name, got in (('row list', res), ('frame range', want)):
                        err = np.abs(got - ref)
                        print(f"{what} {name}: max error / tolerance {float((err / tol).max()):.3g}")
                        assert np.all(err <= tol), what + f": {name}: {int((err > tol).sum())} results are off the " \
                                                          f"float64 product by up to {float((err / tol).max()):.3g} tol"
            G.unchanged(tile, what)
        r.close()


# ---- E: exact sums --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('param', PARAMS, ids=G.param_id)
def test_integer_sums_are_exact(hip, monkeypatch, param):
    case, tile_dtype = param
    limit = G.exact_limit(case.result)
    for shape in case.pixel_shapes():
        r = Route(hip, monkeypatch, case, tile_dtype, shape, integer=True)
        rng = np.random.default_rng(G.seed('E', case.id, tile_dtype, shape[0]))
        placement = G.placements(case, r.n_px, r.dt.itemsize)[0]
        for n in case.frames:
            x = G.int_frames(rng, tile_dtype, (n, r.n_px))
            re, im, bound = G.int_product(x, r.dense)
            assert bound + 200 < limit
            tile = r.tile(x, placement, _bad_fill(tile_dtype))
            base = r.base(rng, n)
            out = r.out(n, base)
            for acc in (False, True):
                out.load(base)
                r.run(tile, out, n, acc)
                what = r.what('n_frames', n, 'accumulate', acc)
                want = G.as_result(re + (base.real.astype(np.int64) if acc else 0),
                                   (0 if im is None else im) + (base.imag.astype(np.int64) if acc else 0), r.rd)
                got = out.result()
                wrong = np.argwhere(got != want)
                assert wrong.size == 0, what + f": {len(wrong)} of {got.size} differ from the integer product, " \
                                               f"first at {tuple(wrong[0])}: {got[tuple(wrong[0])]} for " \
                                               f"{want[tuple(wrong[0])]}"
                G.unchanged_outside(out, what)
        r.close()


# ---- ltmi_apply_masks_csr: frames stored as CSR ----------------------------------------------------------------------
def _csr_frames(rng, n_frames, n_px, dtype):
    """sparse frames with integer counts in [1, 63]: an empty frame, a full one, the rest about one pixel in ten"""
    import scipy.sparse as sps
    dense = np.where(rng.random((n_frames, n_px)) < 0.1, rng.integers(1, 63, (n_frames, n_px), endpoint=True), 0)
    if n_frames > 3:
        dense[3] = 0
        dense[2] = rng.integers(1, 63, n_px, endpoint=True)
    m = sps.csr_matrix(dense.astype(dtype))
    m.sort_indices()
    return m


@pytest.mark.parametrize('result_dtype,n_masks', G.FRAME_CSR_CASES, ids=lambda v: str(v))
def test_stored_frames_write_containment_and_exact_sums(hip, result_dtype, n_masks):
    """k_apply_csr, a frame range and a row list: A (padding of `out` and its guard bands) and E"""
    rd = np.dtype(result_dtype)
    for n_frames, n_px in G.FRAME_CSR_SHAPES:
        rng = np.random.default_rng(G.seed('csr-frames', result_dtype, n_masks, n_px))
        m = _csr_frames(rng, 3 * n_frames, n_px, np.uint16 if rd == np.float32 else np.int32)
        masks = rng.integers(-3, 3, (n_masks, n_px), endpoint=True).astype(rd)
        h = hip.MaskHandle.dense(0, masks, rd)
        indptr = torch.from_numpy(m.indptr.astype(np.int64)).cuda()
        indices = torch.from_numpy(m.indices.astype(np.int32)).cuda()
        data = torch.from_numpy(m.data.view(np.int16) if m.dtype == np.uint16 else m.data).cuda()
        dense = m.toarray().astype(np.int64)
        _, rows = G.row_list(rng, n_frames)
        rows_dev = torch.from_numpy(rows).cuda()
        for sel, rows_ptr, row0 in ((np.arange(n_frames, 2 * n_frames), 0, n_frames), (rows, rows_dev.data_ptr(), 0)):
            re, _, bound = G.int_product(dense[sel], masks)
            assert bound + 200 < G.exact_limit(rd)
            base = rng.integers(-100, 100, (n_frames, n_masks), endpoint=True).astype(rd)
            for acc in (False, True):
                out = G.Region(n_frames, n_masks, n_masks + 3, rd, shift=1, init=base)
                assert h.apply_csr(indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), m.dtype, rows_ptr, row0,
                                   n_frames, out.ptr, out.ld, acc)
                torch.cuda.synchronize()
                kern = h.last_kernel()
                assert kern.startswith('k_apply_csr<'), kern
                what = f"k_apply_csr {rd} n_masks={n_masks} n_frames={n_frames} n_px={n_px} " \
                       f"{'rows' if rows_ptr else 'range'} accumulate {acc}"
                G.unchanged_outside(out, what)
                want = (re + (base.astype(np.int64) if acc else 0)).astype(rd)
                assert np.array_equal(out.result(), want), what
        out = G.Region(1, n_masks, n_masks + 3, rd, shift=1, init=base[:1])
        assert h.apply_csr(indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), m.dtype, 0, 0, 0, out.ptr, out.ld,
                           False)
        G.unchanged(out, "k_apply_csr, no frames")
        print(f"ROUTE k_apply_csr {rd} {n_masks}: {kern.split(' grid=')[0]}")
        h.close()
