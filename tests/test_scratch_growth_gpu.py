"""
The buffers a handle grows on demand -- K-split partial sums, the float64 workspace and scratch result, the non-finite
guard's lists and scratch, the shift cache, the corrected-crystallinity workspace -- through a growth step.  `-m gpu`.

Every case runs ONE handle at a small frame count, at a larger one that outgrows what the first call allocated, and at
the small one again (the third call finds more room than it needs).  Each result is held to the NumPy float64 product
with the tolerance tests/test_apply_bounds_gpu.py uses on that route -- 1e-5 (scale + 1) on float routes, 2e-6 (scale + 1)
on the float16-piece route, equality for integer results --, and the third result has the bits of the first.  Every
call asserts its route through `last_kernel()`: a case the dispatch no longer takes onto its grower fails.
"""
import re

import numpy as np
import pytest

import guarded as G
from libertem_amd.hip import Variant as V

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GROW = (16, 272, 16)            # one 128-row workgroup, three of them (no multiple of 16 x 16), one


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


def _dev(arr):
    arr = np.ascontiguousarray(arr)
    if arr.dtype == np.uint16:
        arr = arr.view(np.int16)
    return torch.from_numpy(arr).cuda()


def _expect(kern, expect, what):
    for e in expect:
        assert (e[1:] not in kern) if e.startswith('!') else (e in kern), f"{what}: took {kern}"


def _check(res, ref, scale, kern, what):
    """integer results: the integer product; float results: the route's tolerance around the float64 product"""
    if res.dtype.kind in 'iu':
        assert np.array_equal(res, ref.astype(res.dtype)), what
        return
    tol = (2e-6 if ',f16' in kern else 1e-5) * (scale + 1)
    err = np.abs(res - ref)
    print(f"{what}: max error / tolerance {float((err / tol).max()):.3g}")
    assert np.all(err <= tol), f"{what}: off the float64 product by up to {float((err / tol).max()):.3g} tol"


def _grow(run, frames, what):
    """run(n) -> result of a call over the first n frames; small, large, small again"""
    first = run(frames[0])
    run(frames[1])
    again = run(frames[2])
    assert again.tobytes() == first.tobytes(), f"{what}: the call after the growth step differs from the first"


# ---- ltmi_apply_masks / ltmi_apply_masks_rows ----------------------------------------------------------------------
# (id, handle, result dtype, tile dtype, n_masks, n_px, tuning, rows, expect, parts: grid.y of a K split)
PRODUCTS = [
    # K-split partials of the handle (ensure_partials), four parts
    ('lds-ksplit4', 'dense', 'float32', 'float32', 16, 4096, (0, V.DENSE_DEFAULT, 4), False, ('k_dense_lds<',), 4),
    ('mfma-ksplit4', 'dense', 'float32', 'float32', 16, 4096, (1, 4, 4), False, ('k_dense_mfma<',), 4),
    # ... of the bf16 split image
    ('split-ksplit4', 'dense', 'float32', 'float32', 32, 4096, (0, V.DENSE_SPLIT_BF16, 4), False, ('k_dense_split<',), 4),
    # float64 workspace: the LDS-DMA kernel (frame range and row list) and the direct-load kernel
    ('lds64-ksplit2', 'dense', 'float64', 'float64', 3, 1024, (0, 0, 2), False, ('k_dense_lds64<',), 2),
    ('lds64-ksplit2-rows', 'dense', 'float64', 'float64', 3, 1024, (0, 0, 2), True, ('k_dense_lds64<', ',rows'), 2),
    ('mfma-f64-ksplit2', 'dense', 'float64', 'float64', 3, 1024, (1, 0, 2), False, ('k_dense_mfma_f64<',), 2),
    # float64 scratch result of integer stacks: its two growers
    ('exact-int-dense', 'dense', 'int32', 'uint16', 7, 1024, (0, 0, 1), False, ('k_dense_lds64<', 'exact-int'), None),
    ('exact-int-csr', 'csr', 'int32', 'uint16', 20, 1024, None, False, ('k_sell_apply<', 'exact-int'), None),
]


@pytest.mark.parametrize('param', PRODUCTS, ids=lambda p: p[0])
def test_product_through_a_growth_step(hip, param):
    name, handle, result, tile_dtype, n_masks, n_px, tuning, rows, expect, parts = param
    rd, dt = np.dtype(result), np.dtype(tile_dtype)
    rng = np.random.default_rng(G.seed('growth', name))
    integer = rd.kind in 'iu'
    case = G.Case(name, handle, result, tuning, expect, (tile_dtype,), n_masks, (n_px,))
    stack = G.make_stack(case, n_px, integer=integer)
    dense = G.dense_of(stack)
    h = hip.MaskHandle.csr(0, stack, rd) if handle == 'csr' else hip.MaskHandle.dense(0, stack, rd)
    if tuning is not None:
        h.set_tuning(*tuning)
    n_max = max(GROW)
    data = G.int_frames(rng, dt, (n_max, n_px)) if integer else G.real_frames(rng, dt, (n_max, n_px))
    if integer:
        ref, _, bound = G.int_product(data, dense)
        assert bound < G.exact_limit('float64')
        scale = None
    else:
        ref, scale = G.float64_product(data, dense)
    n_tile, order = n_max, None
    if rows:
        order = rng.permutation(n_max).astype(np.int32)               # frames [order[i]] of the tile, unsorted
    tile = _dev(data)
    order_dev = None if order is None else _dev(order)
    seen = set()

    def run(n):
        out = _dev(np.full((n, n_masks), 7, dtype=rd))
        if rows:
            assert h.apply_rows(tile.data_ptr(), dt, order_dev.data_ptr(), n, n_px, out.data_ptr(), n_masks, False), \
                f"{name}: row list not handled"
        else:
            h.apply(tile.data_ptr(), dt, n, n_px, out.data_ptr(), n_masks, False)
        torch.cuda.synchronize()
        kern = h.last_kernel()
        seen.add(kern)
        _expect(kern, expect, f"{name} {n} frames")
        if parts:                                            # (a split of one part has no workspace)
            grid = re.search(r'grid=\((\d+),(\d+)', kern)
            assert grid and int(grid.group(2)) == parts, f"{name} {n} frames: took {kern}"
        res = out.cpu().numpy()
        sel = order[:n] if rows else slice(0, n)
        _check(res, ref[sel], None if scale is None else scale[sel], kern, f"{name} {n} of {n_tile} frames")
        return res

    _grow(run, GROW, name)
    print(f"ROUTE {name}: {sorted(seen)}")
    h.close()


# ---- the non-finite guard: lists and scratch ------------------------------------------------------------------------
def test_guard_lists_and_scratch_through_a_growth_step(hip):
    """a densified sparse stack (ltmi_masks_set_sparse_origin) on float32 frames of which every fourth holds a NaN in a
    stored pixel: `out += product` sends the product through the guard's scratch, the flagged frames through its lists"""
    import scipy.sparse as sps
    n_masks, n_px, frames = 20, 1024, (8, 300, 8)
    rng = np.random.default_rng(G.seed('growth', 'guard'))
    sup = G.sparse_support(n_px, n_masks)
    csr = sps.csr_matrix(((rng.random((n_px, n_masks)) + 0.25) * sup).astype(np.float32))
    dense = G.dense_of(csr)
    h = hip.MaskHandle.dense(0, dense, np.float32)
    h.set_sparse_origin(hip.MaskHandle.csr(0, csr, np.float32, gather_only=True))
    data = G.real_frames(rng, np.float32, (max(frames), n_px))
    bad = np.arange(max(frames)) % 4 == 1
    assert sup[100].any() and not sup[100].all()
    data[bad, 100] = np.nan                                   # the masks that store pixel 100, no others
    base = rng.integers(-100, 100, (max(frames), n_masks), endpoint=True).astype(np.float32)
    ref = G.stored_entries_ref(data, csr) + base
    finite = np.where(np.isfinite(data), data, 0)
    scale = np.abs(finite).astype(np.float64) @ np.abs(dense).astype(np.float64).T + np.abs(base)
    tile = _dev(data)

    def run(n):
        out = _dev(base[:n])
        h.apply(tile.data_ptr(), np.float32, n, n_px, out.data_ptr(), n_masks, True)
        torch.cuda.synchronize()
        kern = h.last_kernel()
        assert 'k_dense_' in kern and kern.endswith('+nf'), kern
        assert h.nonfinite_frames() == int(bad[:n].sum()), (n, h.nonfinite_frames())
        res = out.cpu().numpy()
        want = ref[:n]
        assert np.array_equal(np.isnan(res), np.isnan(want)) and not np.isinf(res).any(), f"guard {n} frames"
        assert int(np.isnan(res).any(axis=1).sum()) == int(bad[:n].sum())
        ok = np.isfinite(want)
        _check(np.where(ok, res, 0), np.where(ok, want, 0), scale[:n], kern, f"guard {n} frames")
        return res

    _grow(run, frames, 'guard')
    h.close()


# ---- the shift cache ------------------------------------------------------------------------------------------------
def _shifted_product(data3d, masks3d, shifts):
    """out[f, k] = sum over the overlap of frame f and mask k moved by (dy, dx), in float64; and of the magnitudes"""
    n, h, w = data3d.shape
    out = np.zeros((n, len(masks3d)))
    scale = np.zeros((n, len(masks3d)))
    for f in range(n):
        dy, dx = int(shifts[f, 0]), int(shifts[f, 1])
        moved = np.zeros(masks3d.shape)
        y0, y1, x0, x1 = max(0, dy), min(h, h + dy), max(0, dx), min(w, w + dx)
        if y0 < y1 and x0 < x1:
            moved[:, y0:y1, x0:x1] = masks3d[:, y0 - dy:y1 - dy, x0 - dx:x1 - dx]
        fr = data3d[f].astype(np.float64)
        out[f] = np.tensordot(moved, fr, axes=([1, 2], [0, 1]))
        scale[f] = np.tensordot(np.abs(moved), np.abs(fr), axes=([1, 2], [0, 1]))
    return out, scale


@pytest.mark.parametrize('dtype,n_masks,expect', [
    ('float32', 5, ('k_dense_lds<', 'shifted', 'shift groups=%d')),       # row lists, image pointers, shifts, images
    ('float64', 3, ('k_dense_lds64<', 'shifted, %d groups')),             # frame numbers, gather, results, images
])
def test_shift_cache_through_a_growth_step(hip, dtype, n_masks, expect):
    """ltmi_apply_masks_shifted_host, 16 x 16 detector: 8 frames with 2 shifts, 200 frames with 7 shifts in another
    grouping, the first call again.  Float frames: the product is checked for non-finite rows, so the shifts go to the
    device as well."""
    sig = (16, 16)
    dt = np.dtype(dtype)
    rng = np.random.default_rng(G.seed('growth', 'shift', dtype))
    table = np.array([(1, 0), (0, -2), (3, 3), (-4, 1), (0, 0), (-1, -1), (2, -5)], dtype=np.int32)
    few = table[[0, 1, 0, 0, 1, 0, 1, 0]]
    many = table[np.concatenate([np.arange(7)[::-1], rng.integers(0, 7, 193)])]
    masks = (rng.random((n_masks,) + sig) - 0.25).astype(dt)
    data = ((rng.random((200,) + sig) - 0.3) * 50).astype(dt)
    h = hip.MaskHandle.dense(0, masks.reshape(n_masks, -1), dt)
    tile = _dev(data.reshape(200, -1))
    calls = {8: (few, 2), 200: (many, 7)}

    def run(n):
        shifts, groups = calls[n]
        out = _dev(np.full((n, n_masks), 7, dtype=dt))
        h.apply_shifted_host(tile.data_ptr(), dt, n, sig[0] * sig[1], sig[0], sig[1], shifts, out.data_ptr(), n_masks,
                             False)
        torch.cuda.synchronize()
        kern = h.last_kernel()
        _expect(kern, [e % groups if '%d' in e else e for e in expect] + ['+nf'], f"shifted {dtype} {n} frames")
        if n == 200:
            free, total = torch.cuda.mem_get_info()
            print(f"MEMORY shifted {dtype}: {total - free} bytes in use after the large call")
        ref, scale = _shifted_product(data[:n], masks, shifts)
        res = out.cpu().numpy()
        _check(res, ref, scale, kern, f"shifted {dtype} {n} frames")
        return res

    _grow(run, (8, 200, 8), f"shifted {dtype}")
    h.close()


# ---- the FFT plan's workspace of the corrected frames' patches ------------------------------------------------------
def test_corrected_crystallinity_workspace_through_a_growth_step(hip):
    """ltmi_crystallinity_corrected on a 256 x 256 plan with two excluded pixels, 2 -> 12 -> 2 frames, against
    ltmi_crystallinity on the frames corrected by ltmi_correct + ltmi_repair_pixels: 2e-6, what
    test_crystallinity_corrected_and_float64_frames_take_the_fused_kernel holds the fused corrections to against the
    conversion pass"""
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf.crystallinity import crystallinity_masks, mask_box
    sig, n_max = 256, 12
    rng = np.random.default_rng(G.seed('growth', 'cryst'))
    data = rng.integers(0, 3000, (n_max, sig * sig)).astype(np.uint16)
    dark = rng.random((sig, sig)) * 6
    gain = rng.random((sig, sig)) * 0.6 + 0.7
    bad = np.zeros((sig, sig), dtype=bool)
    bad[10, 40] = bad[sig // 2, sig // 2] = True
    real_mask, half = crystallinity_masks((sig, sig), sig // 16, sig // 4, (sig // 2, sig // 2), sig // 10)
    tables = CorrectionSet(dark=dark, gain=gain, excluded_pixels=bad).device_tables(0, (sig, sig))
    assert tables['n_excl'] == 2
    t = _dev(data)
    rm = _dev(real_mask.astype(np.float32))
    hm = _dev(half.astype(np.float32))
    box = mask_box(half)

    def ptr(x):
        return None if x is None else x.data_ptr()

    # the reference: corrected float32 frames through the uncorrected entry point, on a plan of its own
    corrected = torch.empty((n_max, sig * sig), dtype=torch.float32, device='cuda')
    hip.correct(0, t.data_ptr(), np.uint16, n_max, sig * sig, sig * sig, ptr(tables['dark']), ptr(tables['gain']),
                corrected.data_ptr(), np.float32, sig * sig)
    hip.repair_pixels(0, corrected.data_ptr(), np.float32, n_max, sig * sig, ptr(tables['excl']), ptr(tables['env']),
                      ptr(tables['cnt']), tables['n_excl'], tables['max_env'])
    ref_plan = hip.FFTPlan(0, sig, sig, 8)
    ref_out = torch.empty((n_max,), dtype=torch.float32, device='cuda')
    ref_plan.crystallinity(corrected.data_ptr(), np.float32, n_max, sig * sig, rm.data_ptr(), hm.data_ptr(), box,
                           ref_out.data_ptr(), False)
    torch.cuda.synchronize()
    assert ref_plan.last_kernel().startswith('k_cryst_fused<float32'), ref_plan.last_kernel()
    ref = ref_out.cpu().numpy()
    ref_plan.close()
    assert np.all(ref > 0)

    plan = hip.FFTPlan(0, sig, sig, 8)

    def run(n):
        out = torch.full((n,), 7.0, dtype=torch.float32, device='cuda')
        plan.crystallinity_corrected(t.data_ptr(), np.uint16, n, sig * sig, tables, rm.data_ptr(), hm.data_ptr(), box,
                                     out.data_ptr(), False)
        torch.cuda.synchronize()
        kern = plan.last_kernel()
        assert kern.startswith('k_cryst_fused<uint16,corrected') and kern.endswith('patches=2'), kern
        res = out.cpu().numpy()
        rel = np.abs(res - ref[:n]) / np.abs(ref[:n])
        print(f"corrected crystallinity {n} frames: max relative difference {float(rel.max()):.3g}")
        assert np.all(rel <= 2e-6), f"{n} frames: off the corrected frames' crystallinity by {float(rel.max()):.3g}"
        return res

    _grow(run, (2, n_max, 2), 'corrected crystallinity')
    plan.close()
