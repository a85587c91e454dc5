"""
The case table of tests/test_apply_bounds_gpu.py (tests/guarded.py), checked without a GPU: every kernel route of the
unshifted mask products has a case, the exact-sum inputs stay below the bound that makes them exact, poison never
lands on an owned element, and the folded stacks keep their mirror symmetry after rounding.
"""
import numpy as np
import pytest

import guarded as G

# the routes behind ltmi_apply_masks / ltmi_apply_masks_rows -> the cases that must force them
ROUTES = {
    'k_dense_mfma mt=1 waves=4': ['mfma-mt1'],
    'k_dense_mfma mt=2 waves=4': ['mfma-mt2'],
    'k_dense_mfma waves=8 (uint16)': ['mfma-waves8'],
    'k_dense_lds NG=1 (16 masks)': ['lds-ng1'],
    'k_dense_lds NG=2 (24)': ['lds-ng2'],
    'k_dense_lds NG=3, (40)': ['lds-ng3'],
    'k_dense_lds NG=4 (64)': ['lds-ng4'],
    'k_dense_lds NG=1+2 VALU (17)': ['lds-ng1+2valu'],
    'k_dense_lds NG=2+4 VALU (35)': ['lds-ng2+4valu'],
    'k_dense_lds NG=3+2 VALU (50)': ['lds-ng3+2valu'],
    'k_dense_lds NG=0+ (3 masks, float32 frames)': ['lds-ng0+valu'],
    'column blocks (70)': ['lds-column-blocks'],
    ',f16 (default dispatch)': ['f16-ng1', 'f16-ng2', 'f16-ng3', 'f16-ng4'],
    'code 37 on the same frames': ['f32instr-ng1', 'f32instr-ng3', 'f32instr-ng4'],
    'k_dense_split (code 36)': ['split-ng2', 'split-ng4'],
    'k_dense_fold, float32 and uint16 frames': ['fold-f32', 'fold-u16'],
    'complex64 stacks of 8 and 25 masks': ['c64-8', 'c64-25'],
    'ksplit 0, 3, 8 on NG=1': ['lds-ng1-ksplit0', 'lds-ng1-ksplit3', 'lds-ng1-ksplit8'],
    'ksplit 0, 3, 8 on NG=4': ['lds-ng4-ksplit0', 'lds-ng4-ksplit3', 'lds-ng4-ksplit8'],
    'ksplit 0, 3, 8 on the fold': ['fold-ksplit0', 'fold-ksplit3', 'fold-ksplit8'],
    'k_dense_lds64': ['lds64', 'lds64-3groups', 'c128'],
    'k_dense_mfma_f64 (mt=1, n_px < 256)': ['mfma-f64-mt1', 'mfma-f64-short-rows'],
    'exact-int': ['exact-int', 'exact-int-short-rows'],
    'generic (complex64 frames; int64 frames)': ['generic-c64', 'generic-i64'],
    'float64 ksplit 0 and 3': ['lds64-ksplit0', 'lds64-ksplit3', 'mfma-f64-ksplit3'],
    'k_sell_apply (tuning 41, float32 and float64 results)': ['sell-f32', 'sell-f64'],
    'k_bell_apply, k_bell_flat, k_scatter': ['bell-apply', 'bell-flat', 'scatter'],
    'banded image (kind 3)': ['band-f32', 'band-u16'],
}
BY_ID = {c.id: c for c in G.CASES}


def test_every_route_has_a_case():
    ids = [c.id for c in G.CASES]
    assert len(ids) == len(set(ids))
    wanted = [i for v in ROUTES.values() for i in v]
    assert sorted(wanted) == sorted(ids)
    for c in G.CASES:
        assert c.tiles and c.expect and c.pixel_shapes() and c.frames in (G.FRAMES, G.FRAMES_SMALL), c.id
    assert BY_ID['fold-f32'].tiles == ('float32',) and BY_ID['fold-u16'].tiles == ('uint16',)
    assert BY_ID['mfma-waves8'].tiles == ('uint16',)
    assert BY_ID['generic-c64'].tiles == ('complex64',) and BY_ID['generic-i64'].tiles == ('int64',)
    # ltmi_apply_masks_rows on every route that reports `handled`: the LDS-DMA kernels, the fold, every CSR image
    for c in G.CASES:
        takes_rows = any(e in ''.join(c.expect) for e in ('k_dense_lds', 'k_dense_fold', 'column blocks')) or \
            c.sparse() or c.id == 'exact-int'
        assert c.rows == takes_rows, c.id
    assert sorted(G.FRAME_CSR_CASES) == sorted([('float32', n) for n in (1, 3, 17, 64)] +
                                               [('float64', n) for n in (1, 3, 64)])


def test_pixel_shapes():
    """full mask slots plus tails of 0, 1, 9, 33 pixels, 391 for odd rows, one count below a slot where it is taken"""
    assert G.px(256) == (256, 257, 391, 521, 545)
    assert G.px(128, below=True) == (100, 128, 129, 265, 289, 391)
    assert G.px(128, two=True) == (256, 257, 265, 289, 391)          # two slots + 0, 1, 9, 33
    assert BY_ID['lds-ng0+valu'].n_px == BY_ID['lds-column-blocks'].n_px == G.px(128, two=True)
    for c in G.CASES:
        for n_px, sig, _ in c.pixel_shapes():
            if 'k_dense_lds<' in c.expect:           # (rows shorter than a mask slot go to k_dense_mfma)
                assert n_px >= (256 if c.n_masks <= 16 or c.n_masks > 64 else 128), c.id
            assert c.whole_slots == c.id.startswith('split')
            if c.whole_slots:
                assert n_px % 128 == 0 and n_px >= 1024
            if sig is not None:
                assert n_px == sig[0] * sig[1]


@pytest.mark.parametrize('case', G.CASES, ids=lambda c: c.id)
def test_exact_sum_inputs_stay_below_the_bound(case):
    """E with the reference alone: sum |x||w| (+ what `out` held) is below 2^24 / 2^53 for every shape and dtype"""
    limit = G.exact_limit(case.result)
    assert limit == (2 ** 24 if case.result in ('float32', 'complex64') else 2 ** 53)
    for n_px, sig, centre in case.pixel_shapes():
        w = G.dense_of(G.make_stack(case, n_px, sig, centre, integer=True))
        wr, wi = w.real, w.imag
        assert np.array_equal(wr, np.rint(wr)) and np.array_equal(wi, np.rint(wi))
        assert np.abs(wr).max() <= 3 and np.abs(wi).max() <= 3 and np.abs(wr).max() >= 1
        for tile_dtype in case.tiles:
            rng = np.random.default_rng(G.seed('E', case.id, tile_dtype, n_px))
            x = G.int_frames(rng, tile_dtype, (max(case.frames), n_px))
            assert x.dtype == np.dtype(tile_dtype)
            lo, hi = (-31, 31) if G.signed_pixels(tile_dtype) else (0, 63)
            assert x.real.min() >= lo and x.real.max() <= hi and x.imag.min() >= lo and x.imag.max() <= hi
            re, im, bound = G.int_product(x, w)
            assert bound + 200 < limit, (case.id, n_px, bound)
            assert np.abs(re).max() <= bound and (im is None or np.abs(im).max() <= bound)
            # the int64 product is the float64 one (far below 2^53)
            ref = x.astype(np.complex128) @ w.astype(np.complex128).T
            assert np.array_equal(re, ref.real) and np.array_equal(np.zeros_like(re) if im is None else im, ref.imag)


@pytest.mark.parametrize('case', G.CASES, ids=lambda c: c.id)
def test_poison_never_lands_on_an_owned_element(case):
    """B: the fills around a tile; C: bad frames and bad pixels; D: the frames a row list does not name"""
    for n_px, sig, centre in case.pixel_shapes():
        for tile_dtype in case.tiles:
            dt = np.dtype(tile_dtype)
            rng = np.random.default_rng(n_px)
            for n in case.frames:
                data = G.real_frames(rng, dt, (n, n_px))
                assert np.all(np.isfinite(data))
                for ld, shift in G.placements(case, n_px, dt.itemsize):
                    if case.aligned:
                        assert (ld * dt.itemsize) % 16 == 0 and (shift * dt.itemsize) % 16 == 0
                    for fill in G.input_fills(dt):
                        r = G.Region(n, n_px, ld, dt, shift=shift, init=data, fill=fill, upload=False)
                        assert r.guard >= 4096 and (r.start - shift * dt.itemsize) % 256 == 0
                        assert r.total - r.start - r.nbytes >= 4096
                        assert np.array_equal(r.view(r.host), data)
                        owned = r.owned_mask()
                        assert owned.sum() == n * n_px * dt.itemsize
                        rest = r.host[~owned].view(dt)
                        v = G.fill_value(dt, fill)
                        if fill == 'nan':
                            assert np.all(np.isnan(rest.real)) and (dt.kind != 'c' or np.all(np.isnan(rest.imag)))
                        else:
                            assert np.all(rest == v)
                            assert dt.kind != 'c' or fill != 'inf' or np.all(rest.imag == np.inf)
                        assert rest.size == (r.total // dt.itemsize) - n * n_px
            # D: named frames are clean, every other frame is poison
            for n in (f for f in case.frames if f >= 2):
                n_tile, rows = G.row_list(np.random.default_rng(n), n)
                assert n_tile == 3 * n and len(rows) == n and len(set(rows.tolist())) == n - 1
                assert rows.min() >= 0 and rows.max() < n_tile and list(rows) != sorted(rows)
    # C
    shapes, frames = G.c_shapes(case)
    for n_px, sig, _ in shapes:
        assert sig is not None or n_px % 128 != 0 or case.whole_slots
        for whole in (False, True):
            m = G.bad_pixels(n_px, whole)
            assert m.sum() == (n_px if whole else 80) and m[0] and m[-1]
    for n in frames:
        bad = G.bad_frames(n)
        assert (~bad).sum() >= 2 and bad.sum() >= 1 and not bad[0]
        assert np.array_equal(np.flatnonzero(bad), np.arange(1, n, 3))
    assert shapes and frames == [f for f in case.frames if f > 1]


def test_output_region_layout():
    base = np.arange(12, dtype=np.float32).reshape(4, 3)
    r = G.Region(4, 3, 6, np.float32, shift=1, init=base, upload=False)
    assert r.start == 256 + 4 and r.total == 256 + 4 + 4 * 6 * 4 + 256 and r.fill == 'poison'
    assert np.array_equal(r.view(r.host), base)
    owned = r.owned_mask()
    assert owned.sum() == 48 and not owned[:r.start].any() and not owned[r.start + 12:r.start + 24].any()
    assert np.array_equal(r.host[~owned], G.poison(r.total)[~owned]) and (G.poison(1000) != 0).all()
    assert G.where_is(r, 0) == 'front guard' and G.where_is(r, r.total - 1) == 'rear guard'
    assert G.where_is(r, r.start + 6 * 4 + 3 * 4) == 'row 1 column 3 (row padding)'
    empty = G.Region(0, 3, 6, np.float32, shift=1, upload=False)
    assert empty.view(empty.host).shape == (0, 3) and not empty.owned_mask().any()


@pytest.mark.parametrize('case', [c for c in G.CASES if c.handle == 'fold'], ids=lambda c: c.id)
def test_folded_integer_stacks_keep_the_row_mirror(case):
    """the integer-rounded radial-Fourier stack: real parts even, imaginary parts odd under the mirror of the detector
    rows about the centre, bit for bit, on the rows whose partner lies inside the frame"""
    for n_px, (h, w), centre in case.pixel_shapes():
        cy = h / 2 if centre is None else centre[0]
        st = G.make_stack(case, n_px, (h, w), centre, integer=True).reshape(-1, h, w)
        assert st.shape[0] == case.n_masks and np.abs(st.real).max() == 3
        paired = 0
        for y in range(h):
            yp = int(round(2 * cy)) - y
            if 0 <= yp < h and yp != y:
                paired += 1
                assert np.array_equal(st[:, y].real, st[:, yp].real), (case.id, y)
                assert np.array_equal(st[:, y].imag, -st[:, yp].imag), (case.id, y)
        assert paired >= h - 2
        if centre is not None:
            assert paired < h               # (rows whose partner lies beyond the frame)


def test_which_launches_sum_in_another_order_than_the_row_list_kernel():
    """property D compares with the frame-range kernel's bits but where that kernel takes its pixel parts in turn"""
    lds = "k_dense_lds<f,NG=1,ring=4,tiles=2%s> grid=(1,%d,1)"
    assert [p for p in range(1, 70) if G.parts_in_turn(lds % ('', p))] == [8, 16, 32, 64]
    assert not any(G.parts_in_turn(lds % (',rows', p)) for p in range(1, 70))
    assert G.parts_in_turn("2 column blocks, last: " + lds % (',f16', 8))
    assert not G.parts_in_turn("k_dense_fold<f,even=2,odd=2,rows 31+2=64> grid=(1,8)")
    assert not G.parts_in_turn("k_dense_lds64<d> grid=(1,8,1)")
    assert not G.parts_in_turn("k_sell_apply<f,f32>")
    x = np.array([[1., -2., 3.]])
    w = np.array([[2., 2., -1.], [0., 1., 0.]], dtype=np.float32)
    ref, scale = G.float64_product(x, w)
    assert ref.tolist() == [[-5., -2.]] and scale.tolist() == [[9., 2.]]
