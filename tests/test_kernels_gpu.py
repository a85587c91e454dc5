"""
GPU parity of the C-ABI kernels (through ctypes) against the oracle / float64 NumPy on the same
seeded inputs.  `-m gpu` only.
"""
import os
import zlib

import numpy as np
import pytest

import recipes
from cryst_ref import _cryst_reference, _cryst_run
from oracle import path as opath

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


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


def _dev(arr):
    if arr.dtype == np.uint16:
        return torch.from_numpy(arr.view(np.int16)).cuda()
    if arr.dtype == np.uint32:
        return torch.from_numpy(arr.view(np.int32)).cuda()
    if arr.dtype == np.uint64:
        return torch.from_numpy(arr.view(np.int64)).cuda()
    return torch.from_numpy(arr).cuda()


def _apply(hip, data2d, masks2d, result_dtype, accumulate_into=None, tuning=None):
    h = hip.MaskHandle.dense(0, masks2d, result_dtype)
    if tuning:
        h.set_tuning(**tuning)
    t = _dev(np.ascontiguousarray(data2d))
    n_frames, n_px = data2d.shape
    rd = np.dtype(result_dtype)
    if accumulate_into is None:
        out_np = np.full((n_frames, masks2d.shape[0]), 7, dtype=rd)   # poison
        acc = False
    else:
        out_np = accumulate_into.astype(rd).copy()
        acc = True
    out = _dev(out_np)
    h.apply(t.data_ptr(), data2d.dtype, n_frames, n_px, out.data_ptr(), masks2d.shape[0], acc)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    if res.dtype != rd:
        res = res.view(rd)
    kern = h.last_kernel()
    h.close()
    return res, kern


def _ref64(data2d, masks2d):
    if np.iscomplexobj(data2d) or np.iscomplexobj(masks2d):
        return data2d.astype(np.complex128) @ masks2d.astype(np.complex128).T
    return data2d.astype(np.float64) @ masks2d.astype(np.float64).T


@pytest.mark.parametrize('tile_dtype', ['uint8', 'int8', 'uint16', 'int16', 'float32'])
@pytest.mark.parametrize('shape', [
    (72, 256 * 4, 16),      # ragged frames (72 = 64 + 8), 4 full chunks
    (5, 300, 3),            # ragged tail chunk, few frames, 3 masks
    (130, 17 * 23, 4),      # unaligned rows for 2-byte types (391 px)
    (64, 2048, 37),         # 3 column groups -> NG=4 path
    (33, 512, 20),          # 2 column groups -> NG=2 path
    (1, 256, 1),
])
def test_mfma_f32(hip, tile_dtype, shape):
    n_frames, n_px, n_masks = shape
    rng = np.random.default_rng(_seed(tile_dtype, shape))
    dt = np.dtype(tile_dtype)
    if dt.kind == 'u':
        data = rng.integers(0, min(4096, np.iinfo(dt).max), (n_frames, n_px)).astype(dt)
    elif dt.kind == 'i':
        data = rng.integers(max(-2000, np.iinfo(dt).min), min(2000, np.iinfo(dt).max),
                            (n_frames, n_px)).astype(dt)
    else:
        data = (rng.random((n_frames, n_px)) - 0.3).astype(dt)
    masks = (rng.random((n_masks, n_px)) - 0.25).astype(np.float32)
    res, kern = _apply(hip, data, masks, np.float32)
    assert 'k_dense_mfma' in kern or 'k_dense_lds' in kern, kern
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks.astype(np.float64)).T
    # f32 accumulation error bound relative to sum |a||b|: 1e-5 rel (north_star tolerance)
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)
    # accumulate=1
    base = rng.random((n_frames, n_masks)).astype(np.float32)
    res2, _ = _apply(hip, data, masks, np.float32, accumulate_into=base)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 1))


@pytest.mark.parametrize('tuning', [
    dict(mt=1, waves=4, ksplit=1), dict(mt=2, waves=4, ksplit=1), dict(mt=1, waves=8, ksplit=1),
    dict(mt=2, waves=8, ksplit=1), dict(mt=1, waves=4, ksplit=3), dict(mt=2, waves=8, ksplit=5),
])
def test_mfma_variants_agree(hip, tuning):
    rng = np.random.default_rng(7)
    data = rng.integers(0, 4096, (200, 256 * 9 + 40)).astype(np.uint16)
    masks = (rng.random((16, data.shape[1])) - 0.25).astype(np.float32)
    res, kern = _apply(hip, data, masks, np.float32, tuning=tuning)
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks.astype(np.float64)).T
    assert np.all(np.abs(res - ref) <= 1e-5 * scale)
    base = rng.random((200, 16)).astype(np.float32)
    res2, _ = _apply(hip, data, masks, np.float32, accumulate_into=base, tuning=tuning)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 1))


@pytest.mark.parametrize('tile_dtype', ['uint8', 'int8', 'uint16', 'int16', 'float32'])
@pytest.mark.parametrize('shape,ksplit', [
    ((300, 256 * 41 + 112, 16), 0),     # NG=1: unrolled main loop + generic tail + ragged slot
    ((300, 256 * 41 + 112, 16), 3),     # ... with a K split
    ((129, 128 * 53 + 16, 24), 0),       # NG=2
    ((77, 128 * 61 + 48, 50), 0),       # NG=4 (C5-like: 50 real columns)
    ((77, 128 * 61 + 48, 50), 4),
    ((40, 128 * 30, 70), 0),            # 5 groups -> a block of 64 columns + one of 6
    ((40, 128 * 30, 70), 2),
    # 8 / 16 / 32 / 64 parts take runs of 4 mask slots in turn (ksplit_order): slot counts that are no multiple of
    # the run, a ragged last slot, more parts than runs
    ((300, 256 * 47 + 112, 16), 8),     # 48 slots: 6 per part = a run of 4 + half a run
    ((140, 256 * 47 + 9, 16), 16),
    ((77, 128 * 61 + 48, 50), 8),
    ((129, 128 * 63 + 16, 24), 32),
    ((60, 256 * 63 + 5, 16), 64),       # one slot per part: 16 runs for 64 parts
])
def test_lds_dma_kernel_all_widths(hip, tile_dtype, shape, ksplit):
    """k_dense_lds (frames through LDS by DMA) for every pixel width and group count; forced with
    tuning code 30 where the default dispatch would pick another kernel."""
    n_frames, n_px, n_masks = shape
    rng = np.random.default_rng(_seed(tile_dtype, shape))
    dt = np.dtype(tile_dtype)
    if dt.kind == 'u':
        data = rng.integers(0, min(4096, np.iinfo(dt).max), (n_frames, n_px)).astype(dt)
    elif dt.kind == 'i':
        data = rng.integers(max(-2000, np.iinfo(dt).min), min(2000, np.iinfo(dt).max),
                            (n_frames, n_px)).astype(dt)
    else:
        data = (rng.random((n_frames, n_px)) - 0.3).astype(dt)
    masks = (rng.random((n_masks, n_px)) - 0.25).astype(np.float32)
    res, kern = _apply(hip, data, masks, np.float32, tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert 'k_dense_lds' in kern, kern          # (1-byte pixels with several groups: 128-byte sub-chunks)
    if ksplit >= 8:
        assert f',{ksplit},' in kern, kern      # (the number of parts the in-turn order is used for)
    if n_masks > 64:
        assert kern.startswith('2 column blocks'), kern   # 64 + the rest, each with its own tile width
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks.astype(np.float64)).T
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)
    base = rng.random((n_frames, n_masks)).astype(np.float32)
    res2, _ = _apply(hip, data, masks, np.float32, accumulate_into=base,
                     tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 1))


@pytest.mark.parametrize('tile_dtype', ['uint8', 'uint16', 'int16', 'int8'])
@pytest.mark.parametrize('shape,ksplit,mask_dtype', [
    ((300, 256 * 41 + 112, 16), 0, 'float32'),      # unrolled loop + generic tail + ragged last slot
    ((300, 256 * 41 + 112, 16), 3, 'float32'),      # ... with a K split
    ((300, 256 * 47 + 112, 16), 8, 'float32'),      # ... parts in turn (runs of 4 slots)
    ((200, 256 * 47 + 9, 16), 16, 'float32'),
    ((129, 256 * 8, 9), 0, 'float32'),
    ((1000, 1024, 12), 0, 'float32'),
    ((70, 515, 16), 0, 'float32'),                  # unaligned rows
    ((200, 256 * 6 + 40, 8), 0, 'complex64'),       # 8 complex masks = 16 real columns
    ((150, 128 * 21 + 16, 24), 0, 'float32'),       # 2 groups (image 2)
    ((150, 128 * 21 + 16, 40), 2, 'float32'),       # exactly 3 groups (image 3 without VALU columns)
    ((90, 128 * 30, 64), 0, 'float32'),             # 4 groups
    ((90, 128 * 30, 30), 0, 'complex64'),           # 60 real columns: 4 groups, 4 padded columns
])
def test_exact_float16_products_for_unsigned_pixels(hip, tile_dtype, shape, ksplit, mask_dtype):
    """k_dense_lds X16 (1- / 2-byte integer pixels, 1 / 2 / 3 / 4 column groups without VALU columns):
    pixel bytes x (w1 + w2) float16 pieces of the scaled weights on v_mfma_f32_16x16x32_f16 -- the
    default dispatch.  Float32 accuracy over the full pixel range (signed: both signs) and columns of
    very different magnitude (per-column scale), agreement with the float32 instruction (tuning 37),
    integer-valued masks bit-exact, accumulate."""
    n_frames, n_px, n_masks = shape
    rng = np.random.default_rng(_seed(tile_dtype, shape, mask_dtype))
    dt, md = np.dtype(tile_dtype), np.dtype(mask_dtype)
    data = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, (n_frames, n_px), endpoint=True).astype(dt)
    data[1 % n_frames] = np.iinfo(dt).max
    data[2 % n_frames] = 0
    data[4 % n_frames] = np.iinfo(dt).min
    masks = rng.random((n_masks, n_px)) - 0.25
    if md.kind == 'c':
        masks = masks + 1j * (rng.random((n_masks, n_px)) - 0.5)
    masks[0] *= 1e-6                                  # columns of very different magnitude
    masks[1] *= 3e4
    masks[2 % n_masks] = 0
    masks[3 % n_masks, ::3] *= 1e-4                   # small next to large inside one column
    masks = masks.astype(md)
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    tuning = dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit) if ksplit else None
    res, kern = _apply(hip, data, masks, md, tuning=tuning)
    assert 'k_dense_lds' in kern and ',f16' in kern, kern
    assert np.all(np.abs(res - ref) <= 2e-6 * scale + 1e-30), np.max(np.abs(res - ref) / (scale + 1e-30))
    res32, kern32 = _apply(hip, data, masks, md, tuning=dict(mt=0, waves=hip.Variant.DENSE_F32_INSTR, ksplit=ksplit))
    assert 'k_dense_lds' in kern32 and ',f16' not in kern32, kern32
    assert np.all(np.abs(res32 - res) <= 1e-5 * scale + 1e-30)
    base = (rng.random((n_frames, n_masks)) + (1j * rng.random((n_frames, n_masks))
                                               if md.kind == 'c' else 0)).astype(md)
    res2, _ = _apply(hip, data, masks, md, accumulate_into=base, tuning=tuning)
    assert np.all(np.abs(res2 - (ref + base)) <= 2e-6 * (scale + 1))
    if md.kind == 'f':
        # integer-valued masks, sums below 2^24: both instructions give the exact integers
        small = (data.astype(np.int64) % 16).astype(dt)
        imasks = rng.integers(0, 4, (n_masks, n_px)).astype(np.float32)
        exact = small.astype(np.int64) @ imasks.astype(np.int64).T
        assert exact.max() < 2**24
        ri, ki = _apply(hip, small, imasks, np.float32, tuning=tuning)
        assert ',f16' in ki and np.array_equal(ri, exact.astype(np.float32))


def _n_float32_tail(masks2d):
    """entries of a dense float32 stack that the float16-piece images leave to the float32 epilogue: below 2^-20
    of their column's maximum AND missed by two float16 pieces of the column-scaled value by more than 2^-19"""
    m = np.asarray(masks2d, np.float32)
    amax = np.abs(m).max(axis=1, keepdims=True)
    scale = np.float32(2.0) ** (15 - np.frexp(np.where(amax > 0, amax, 1))[1])
    ws = (m * scale).astype(np.float32)
    w1 = ws.astype(np.float16).astype(np.float32)
    r = ws - w1
    miss = np.abs(r - r.astype(np.float16).astype(np.float32)) > np.abs(ws) * np.float32(2.0 ** -19)
    return int(((m != 0) & (np.abs(m) < amax * np.float32(2.0 ** -20)) & miss).sum())


def _one_pixel_frames(dt, n_px, rng):
    """frame i is lit at pixel i only: result[i, k] = value_i * masks[k, i] -- every entry of the stack"""
    dt = np.dtype(dt)
    if dt.kind == 'f':
        val = rng.integers(1, 60000, n_px).astype(dt)
    else:
        val = rng.integers(1, np.iinfo(dt).max, n_px, endpoint=True)
        if dt.kind == 'i':
            val = val * rng.choice([-1, 1], n_px)
    data = np.zeros((n_px, n_px), dt)
    data[np.arange(n_px), np.arange(n_px)] = val
    return data, val.astype(np.float64)


@pytest.mark.parametrize('tile_dtype', ['uint16', 'uint8', 'int16', 'int8'])
@pytest.mark.parametrize('n_masks', [16, 40])
def test_exact_float16_products_every_entry_elementwise(hip, tile_dtype, n_masks):
    """X16 with the float32 tail, element-wise: one-pixel frames pick EVERY entry of a
    stack whose columns span 10 orders of magnitude; each must come back within 1e-5 RELATIVE, no absolute
    term (the north-star tolerance per element, the reference keeps every float32 weight: udf/masks.py:59-77).
    The few weights below 2^-21 of their column's maximum are not in the float16 images: k_dense_tail adds
    them in float32."""
    n_px = 2048
    rng = np.random.default_rng(_seed(tile_dtype, n_masks))
    masks = (0.05 + 0.95 * rng.random((n_masks, n_px))).astype(np.float32)
    masks *= rng.choice([-1.0, 1.0], masks.shape).astype(np.float32)
    masks[1] *= np.float32(3e4)
    masks[2] *= np.float32(2e-5)
    n_tiny = 0
    for k in range(0, n_masks, 3):                      # planted: 1e-5 .. 1e-10 of the column's maximum
        for e in (5, 7, 10):
            q = int(rng.integers(0, n_px))
            masks[k, q] = np.abs(masks[k]).max() * np.float32(10.0 ** -e) * rng.choice([-1, 1])
            n_tiny += 1
    masks[5] = (np.arange(n_px) % 7 == 0) * 0.75        # exactly representable weights, zeros
    data, val = _one_pixel_frames(tile_dtype, n_px, rng)
    for tuning, acc in ((None, False), (dict(mt=0, waves=0, ksplit=3), False), (None, True)):
        base = rng.random((n_px, n_masks)).astype(np.float32) if acc else None
        res, kern = _apply(hip, data, masks, np.float32, tuning=tuning, accumulate_into=base)
        assert ',f16' in kern and '+tail(' in kern, kern
        ref = val[:, None] * masks.T.astype(np.float64)
        if acc:
            # (the sum with `base` rounds once more: compare the added part where it dominates)
            sel = np.abs(ref) > 1e3
            assert np.allclose((res - base)[sel], ref[sel], rtol=2e-4, atol=0)
            continue
        assert np.allclose(res, ref, rtol=1e-5, atol=0), np.abs(res / np.where(ref == 0, 1, ref) - 1)[ref != 0].max()
        assert np.array_equal(res == 0, ref == 0)
        assert np.array_equal(res[:, 5], (val * masks[5]).astype(np.float32))
    # the number of tail entries
    want = _n_float32_tail(masks)
    assert 0 < want <= n_tiny and f'+tail({want})' in kern, (want, kern)


def test_few_bit_weights_need_no_float32_tail(hip):
    """float32 random numbers drawn AS float32 are k 2^-24: small ones have few significant bits, two float16
    pieces hold them exactly, nothing is left to the float32 tail.  (The benchmark's stack is drawn in float64
    and rounded: its two smallest weights have full mantissas and do go through the tail.)"""
    masks = np.random.default_rng(2).random((16, 65536), dtype=np.float32)
    tiny_px = np.argwhere((masks != 0) & (masks < masks.max(axis=1, keepdims=True) * 2.0 ** -20))[:, 1]
    assert len(tiny_px) >= 1                                                      # (it HAS tiny weights)
    data, val = _one_pixel_frames('uint16', 4096, np.random.default_rng(1))
    data = np.concatenate([data, np.zeros((4096, 65536 - 4096), np.uint16)], axis=1)
    for i, q in enumerate(tiny_px[:64]):                 # frames 4000 ..: the tiny weights' pixels alone
        data[4000 + i] = 0
        data[4000 + i, q] = 60001
    res, kern = _apply(hip, data, masks, np.float32)
    assert ',f16' in kern and '+tail' not in kern, kern
    ref = data.astype(np.float64) @ masks.astype(np.float64).T
    assert np.allclose(res, ref, rtol=1e-5, atol=0)
    c2 = np.random.default_rng(2).random((16, 65536)).astype(np.float32)
    res, kern = _apply(hip, data, c2, np.float32)
    assert ',f16' in kern and '+tail(' in kern, kern
    ref = data.astype(np.float64) @ c2.astype(np.float64).T
    assert np.allclose(res, ref, rtol=1e-5, atol=0)


@pytest.mark.parametrize('tile_dtype', ['uint16', 'uint8'])
def test_smooth_masks_with_long_tails_keep_float32_elementwise(hip, tile_dtype):
    """Gaussian masks: thousands of weights below 2^-21 of the column maximum -- more than the float32 tail
    takes: the stack keeps the float32 matrix instruction, and every entry over 12 orders of magnitude is
    reproduced within 1e-5 relative."""
    n_px, n_masks = 4096, 16
    rng = np.random.default_rng(5)
    q = np.arange(n_px)
    masks = np.empty((n_masks, n_px), np.float32)
    for k in range(n_masks):
        masks[k] = (3.0 + k) * np.exp(-((q - 2048.0) / (150.0 + 30 * k)) ** 2 / 2)
    masks[masks < 1e-30] = 0
    data, val = _one_pixel_frames(tile_dtype, n_px, rng)
    res, kern = _apply(hip, data, masks, np.float32)
    assert 'k_dense_lds' in kern and ',f16' not in kern, kern
    ref = val[:, None] * masks.T.astype(np.float64)
    assert np.allclose(res, ref, rtol=1e-5, atol=0)
    span = np.abs(masks[masks != 0])
    assert span.max() / span.min() > 1e12


def test_exact_float16_products_not_for_non_finite_or_extreme_weights(hip):
    """X16 is only built for finite weights (a stack holding inf / nan keeps the float32 instruction and
    its IEEE behaviour); columns near the ends of the float32 range still scale into float16."""
    rng = np.random.default_rng(3)
    data = rng.integers(0, 60000, (200, 2048)).astype(np.uint16)
    masks = (rng.random((16, 2048)) - 0.25).astype(np.float32)
    bad = masks.copy()
    bad[3, 100] = np.inf
    bad[7, 5] = np.nan
    res, kern = _apply(hip, data, bad, np.float32)
    assert 'k_dense_lds' in kern and ',f16' not in kern, kern
    with np.errstate(invalid='ignore', over='ignore'):
        ref = data.astype(np.float64) @ bad.astype(np.float64).T
    assert np.array_equal(np.isnan(res), np.isnan(ref)) and np.array_equal(np.isinf(res), np.isinf(ref))
    ok = np.isfinite(ref)
    scale = np.abs(data.astype(np.float64)) @ np.abs(np.where(np.isfinite(bad), bad, 0)).astype(np.float64).T
    assert np.all(np.abs(res[ok] - ref[ok]) <= 1e-5 * scale[ok])
    ext = masks.copy()
    ext[0] *= np.float32(1e28)
    ext[1] *= np.float32(1e-28)
    res, kern = _apply(hip, data, ext, np.float32)
    assert ',f16' in kern, kern
    ref = data.astype(np.float64) @ ext.astype(np.float64).T
    scale = np.abs(data.astype(np.float64)) @ np.abs(ext).astype(np.float64).T
    assert np.all(np.isfinite(res)) and np.all(np.abs(res - ref) <= 2e-6 * scale + 1e-44)
    # beyond 2^+-100 (float32 subnormal weights, 1e36): the float32 instruction
    ext[2] = np.float32(1e-42)
    res, kern = _apply(hip, data, ext, np.float32)
    assert ',f16' not in kern, kern
    ref = data.astype(np.float64) @ ext.astype(np.float64).T
    scale = np.abs(data.astype(np.float64)) @ np.abs(ext).astype(np.float64).T
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-44)


def test_float16_switches(hip, monkeypatch):
    """LTMI_DENSE_F16=0 / LTMI_BELL_F16=0 (read when a handle is created): 1- / 2-byte integer pixels keep
    the float32 matrix instruction, dense and blocked sparse; results agree with the default."""
    import scipy.sparse as sp
    rng = np.random.default_rng(12)
    data = rng.integers(0, 60000, (150, 2048)).astype(np.uint16)
    masks = (rng.random((16, 2048)) - 0.25).astype(np.float32)
    res, kern = _apply(hip, data, masks, np.float32)
    assert ',f16' in kern, kern
    monkeypatch.setenv('LTMI_DENSE_F16', '0')
    res0, kern0 = _apply(hip, data, masks, np.float32)
    assert 'k_dense_lds' in kern0 and ',f16' not in kern0, kern0
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    assert np.all(np.abs(res0 - res) <= 1e-5 * scale)
    monkeypatch.delenv('LTMI_DENSE_F16')
    centre = (np.arange(64) + 0.5) * 2048 / 64
    dense = ((np.abs(np.arange(2048)[:, None] - centre[None, :]) < 40) *
             (rng.random((2048, 64)) + 0.1)).astype(np.float32)
    t = _dev(data)
    got = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv('LTMI_BELL_F16', '0')
        monkeypatch.setenv('LTMI_SPARSE_BELL', '1')
        h = hip.MaskHandle.csr(0, sp.csr_matrix(dense), np.float32)
        out = _dev(np.zeros((150, 64), np.float32))
        h.apply(t.data_ptr(), np.uint16, 150, 2048, out.data_ptr(), 64, False)
        torch.cuda.synchronize()
        got[off] = (out.cpu().numpy(), h.last_kernel())
        h.close()
    assert 'k_bell_flat' in got[False][1] and 'k_bell_apply' in got[True][1], (got[False][1], got[True][1])
    ref = data.astype(np.float64) @ dense.astype(np.float64)
    for off in (False, True):
        assert np.all(np.abs(got[off][0] - ref) <= 1e-5 * np.abs(ref).max())


def test_mfma_integer_exact(hip):
    # 0/1 masks on low-count data: every partial sum is an integer < 2**24 -> any order exact
    rng = np.random.default_rng(11)
    data = rng.integers(0, 50, (100, 4096)).astype(np.uint16)
    masks = (rng.random((16, 4096)) > 0.5).astype(np.float32)
    res, _ = _apply(hip, data, masks, np.float32)
    ref = data.astype(np.int64) @ masks.astype(np.int64).T
    assert ref.max() < 2**24
    assert np.array_equal(res.astype(np.int64), ref)


def test_mfma_complex_masks(hip):
    rng = np.random.default_rng(12)
    data = rng.integers(0, 1000, (40, 1000)).astype(np.uint16)
    masks = (rng.random((5, 1000)) - 0.5 + 1j * (rng.random((5, 1000)) - 0.5)).astype(np.complex64)
    res, kern = _apply(hip, data, masks, np.complex64)
    assert 'k_dense_mfma' in kern or 'k_dense_lds' in kern
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    assert np.all(np.abs(res - ref) <= 1e-5 * scale)


@pytest.mark.parametrize('tile_dtype,result_dtype', [
    ('uint8', 'float32'), ('uint16', 'float32'), ('int16', 'float32'), ('float32', 'float32'),
    ('float32', 'complex64'), ('int32', 'float64'), ('float64', 'float64'),
])
@pytest.mark.parametrize('n_px,pad,offset', [
    (515 * 5, 0, 0),        # odd row length (a 515-wide detector): rows at every element alignment
    (515 * 5, 3, 1),        # odd leading dimension AND a tile pointer that is only element-aligned
    (256 * 3, 0, 1),        # aligned row length, misaligned base
])
def test_rows_of_any_alignment_through_lds_dma(hip, tile_dtype, result_dtype, n_px, pad, offset):
    """Detectors with odd row lengths: the LDS-DMA kernels (k_dense_lds / k_dense_lds64) take rows
    at any element alignment (global_load_lds_dwordx4 does not need 16-B aligned addresses)."""
    dt, rd = np.dtype(tile_dtype), np.dtype(result_dtype)
    rng = np.random.default_rng(n_px + pad * 7 + offset)
    n_frames, n_masks, ld = 150, 7, n_px + pad
    flat = (rng.integers(0, 200, offset + n_frames * ld).astype(dt) if dt.kind in 'iu'
            else (rng.random(offset + n_frames * ld) - 0.3).astype(dt))
    data = flat[offset:].reshape(n_frames, ld)[:, :n_px]
    if rd.kind == 'c':
        masks = (rng.random((n_masks, n_px)) + 1j * rng.random((n_masks, n_px))).astype(rd)
    else:
        masks = (rng.random((n_masks, n_px)) - 0.25).astype(rd)
    h = hip.MaskHandle.dense(0, masks, rd)
    t = _dev(flat)
    ptr = t.data_ptr() + offset * dt.itemsize
    assert (ptr % 16 != 0) or (ld * dt.itemsize) % 16 != 0 or offset == 0
    out = torch.full((n_frames, n_masks), 7, dtype={'float32': torch.float32, 'float64': torch.float64,
                                                    'complex64': torch.complex64}[rd.name], device='cuda')
    h.apply(ptr, dt, n_frames, ld, out.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    kern = h.last_kernel()
    h.close()
    assert ('k_dense_lds64' if rd == np.float64 else 'k_dense_lds<') in kern, kern
    res = out.cpu().numpy()
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    tol = 1e-13 if rd == np.float64 else 1e-5
    assert np.all(np.abs(res - ref) <= tol * scale + 1e-30), np.abs(res - ref).max()


@pytest.mark.parametrize('n_px,tile_dtype,n_masks', [
    (512 * 512, 'uint16', 16),      # MFMA path, one column group
    (512 * 512, 'uint16', 3),       # <= 4 columns: the VALU-only variant (CoM)
    (1024 * 1024, 'float32', 3),
    (1024 * 1024, 'float32', 50),   # 3 groups + 2 VALU columns (the radial Fourier default)
    (512 * 512, 'uint8', 20),       # 1-byte pixels, two column groups: 128-byte sub-chunks
    (512 * 512, 'uint8', 50),       # ... 3 groups + 2 VALU columns
    (512 * 512, 'uint8', 3),        # ... VALU-only
])
def test_long_rows_keep_float32_accuracy(hip, n_px, tile_dtype, n_masks):
    """All-positive data, large frames, NO split of the pixel axis (what a full partition gets):
    one float32 accumulation chain over a whole frame would drift by 1e-5 ... 6e-5 of the sum (the
    round-off random walk of 32 768 ... 131 072 MFMA steps); the kernels fold their running tiles into
    a second accumulation level every <= 1024 pixels instead and stay an order of magnitude below
    the 1e-5 tolerance against float64."""
    dt = np.dtype(tile_dtype)
    rng = np.random.default_rng(n_px % 1000 + n_masks)
    n_frames = 130
    data = (rng.integers(0, min(4096, np.iinfo(dt).max), (n_frames, n_px)).astype(dt) if dt.kind == 'u'
            else rng.random((n_frames, n_px)).astype(dt))
    masks = rng.random((n_masks, n_px)).astype(np.float32)
    res, kern = _apply(hip, data, masks, np.float32, tuning=dict(mt=0, waves=0, ksplit=1))
    assert 'k_dense_lds' in kern, kern
    assert ',1,1)' in kern.replace(' ', ''), kern                                # grid.y == 1: no K split
    if n_masks <= 4:
        # float32 pixels: VALU columns only; integer pixels: a padded group of exact float16 products
        assert ('NG=0+' in kern) if dt.kind == 'f' else (',f16' in kern), kern
    ref = data.astype(np.float64) @ masks.astype(np.float64).T
    err = np.abs(res - ref).max() / np.abs(ref).max()
    assert err < 4e-6, err
    if n_masks <= 4 and dt.kind != 'f':
        # the VALU-column kernel is still there for them (tuning 37) and agrees
        res37, kern37 = _apply(hip, data, masks, np.float32, tuning=dict(mt=0, waves=hip.Variant.DENSE_F32_INSTR, ksplit=1))
        assert 'NG=0+' in kern37, kern37
        assert np.abs(res37 - ref).max() / np.abs(ref).max() < 4e-6


@pytest.mark.parametrize('tile_dtype,n_masks,mask_dtype', [
    ('uint16', 16, 'float32'), ('uint16', 3, 'float32'), ('float32', 25, 'complex64'),
    ('uint8', 5, 'float32'), ('int16', 40, 'float32'), ('uint16', 70, 'float32'),
    ('int32', 4, 'float32'), ('uint16', 20, 'float64'), ('uint8', 70, 'float64'), ('int16', 6, 'int32'),
])
def test_row_lists_instead_of_gathered_frames(hip, tile_dtype, n_masks, mask_dtype):
    """ltmi_apply_masks_rows: out[i] = product of frame rows[i] of the tile -- a region of interest
    without the gathered copy.  Served for the float32 / complex64 LDS-DMA kernels (every column
    tiling up to 64 real columns) and the float64 one; other handles report handled = 0 and the caller
    gathers."""
    dt, md = np.dtype(tile_dtype), np.dtype(mask_dtype)
    rng = np.random.default_rng(n_masks)
    n_frames, n_px = 700, 256 * 5 + 24
    data = (rng.integers(0, 200, (n_frames, n_px)).astype(dt) if dt.kind in 'iu'
            else rng.random((n_frames, n_px)).astype(dt))
    masks = rng.random((n_masks, n_px)) - 0.25
    if md.kind == 'c':
        masks = masks + 1j * (rng.random((n_masks, n_px)) - 0.5)
    masks = masks.astype(md) if md.kind != 'i' else rng.integers(-3, 9, (n_masks, n_px)).astype(md)
    rd = np.result_type(dt, md)
    rows = np.sort(rng.choice(n_frames, 333, replace=False)).astype(np.int32)
    rows[7], rows[8] = rows[8], rows[7]                      # (any order, repeats allowed)
    rows[100] = rows[99]
    h = hip.MaskHandle.dense(0, masks, rd)
    t = _dev(data)
    r = torch.from_numpy(rows).cuda()
    tout = {'float32': torch.float32, 'float64': torch.float64, 'complex64': torch.complex64,
            'int32': torch.int32}[rd.name]
    base = torch.full((len(rows), n_masks), 2, dtype=tout, device='cuda')
    for acc in (False, True):
        out = base.clone()
        handled = h.apply_rows(t.data_ptr(), dt, r.data_ptr(), len(rows), n_px, out.data_ptr(),
                               n_masks, acc)
        torch.cuda.synchronize()
        assert handled and ',rows' in h.last_kernel(), h.last_kernel()
        if n_masks > 64 and rd != np.float64:
            assert 'column blocks' in h.last_kernel(), h.last_kernel()
        assert ('k_dense_lds64' in h.last_kernel()) == (rd in (np.float64, np.int32))
        if rd.kind == 'i':                                    # exact integer arithmetic
            want = data[rows].astype(np.int64) @ masks.astype(np.int64).T + (2 if acc else 0)
            assert np.array_equal(out.cpu().numpy(), want.astype(np.int32)), h.last_kernel()
            continue
        ref = _ref64(data[rows], masks) + (2.0 if acc else 0.0)
        scale = np.abs(data[rows].astype(np.float64)) @ np.abs(masks).astype(np.float64).T + 2.0
        tol = 1e-12 if rd == np.float64 else 1e-5
        assert np.all(np.abs(out.cpu().numpy() - ref) <= tol * scale), h.last_kernel()
    h.close()


@pytest.mark.parametrize('combo', [
    ('int32', 'float64'), ('int64', 'float64'), ('float64', 'float64'), ('uint16', 'float64'),
    ('uint32', 'float64'), ('float32', 'complex128'), ('int32', 'complex128'),
    ('uint16', 'complex128'), ('complex64', 'complex64'),
    ('complex128', 'complex128'), ('int16', 'int32'), ('uint8', 'uint8'), ('int16', 'int64'),
    ('uint16', 'int32'),
])
def test_generic(hip, combo):
    tile_dtype, result_dtype = map(np.dtype, combo)
    rng = np.random.default_rng(13)
    n_frames, n_px, n_masks = 9, 333, 6
    if tile_dtype.kind in 'iu':
        lo = 0 if tile_dtype.kind == 'u' else -100
        data = rng.integers(lo, 100, (n_frames, n_px)).astype(tile_dtype)
    elif tile_dtype.kind == 'f':
        data = rng.random((n_frames, n_px)).astype(tile_dtype)
    else:
        data = (rng.random((n_frames, n_px)) + 1j * rng.random((n_frames, n_px))).astype(tile_dtype)
    if result_dtype.kind in 'iu':
        masks = rng.integers(0, 3, (n_masks, n_px)).astype(result_dtype)
    elif result_dtype.kind == 'c':
        masks = (rng.random((n_masks, n_px)) + 1j * rng.random((n_masks, n_px))).astype(result_dtype)
    else:
        masks = rng.random((n_masks, n_px)).astype(result_dtype)
    res, kern = _apply(hip, data, masks, result_dtype)
    if result_dtype == np.float64 or (result_dtype == np.complex128 and tile_dtype.kind != 'c'):
        # float64 results: f64 matrix cores (LDS-DMA for 4- / 8-byte pixels, also with odd rows);
        # complex128 masks on real frames: the same kernels with 2 real columns per mask
        assert 'k_dense_lds64' in kern, kern       # (333 pixels >= one mask chunk)
    elif result_dtype.kind in 'iu' and tile_dtype.itemsize <= 4:
        assert 'exact-int' in kern, kern           # integer results, sums < 2^52: same cores, exact
    else:
        assert 'generic' in kern, kern
    ref = data.astype(result_dtype) @ masks.T      # NumPy's own product in the result dtype
    if result_dtype.kind in 'iu':
        assert np.array_equal(res, ref)            # wrap-around integer arithmetic, bit exact
    else:
        assert np.allclose(res, ref, rtol=1e-12 if result_dtype.itemsize >= 8 and
                           result_dtype != np.complex64 else 1e-5)


@pytest.mark.parametrize('tile_dtype', ['int32', 'uint32', 'int64', 'float64', 'float32', 'uint16',
                                        'int16', 'uint8', 'int8'])
@pytest.mark.parametrize('shape,ksplit', [
    ((300, 256 * 9 + 100, 16), 0),      # aligned rows, ragged last chunk
    ((300, 256 * 9 + 100, 16), 3),      # K split + reduce
    ((70, 17 * 23, 5), 0),              # odd row length: unaligned DMA / guarded loads (2-byte pixels)
    ((70, 15 * 13, 5), 0),              # fewer pixels than a mask chunk -> guarded loads
    ((45, 256 * 5, 37), 0),             # three column groups (grid.z)
    ((1, 256, 1), 0),
    ((1000, 256 * 20, 16), 0),          # several workgroups, the unrolled steady state
    ((130, 256 * 3 + 4, 16), 2),        # K split with a ragged tail of 4 pixels
])
def test_float64_results_on_matrix_cores(hip, tile_dtype, shape, ksplit):
    """float64 results (int32 / int64 / float64 data, or float64 masks on any pixel type) on the f64
    matrix cores: k_dense_lds64 (LDS-DMA) for rows of at least one mask chunk, k_dense_mfma_f64
    (direct loads) otherwise."""
    n_frames, n_px, n_masks = shape
    rng = np.random.default_rng(_seed(tile_dtype, shape))
    dt = np.dtype(tile_dtype)
    if dt.kind == 'u':
        data = rng.integers(0, min(100000, np.iinfo(dt).max), (n_frames, n_px)).astype(dt)
    elif dt.kind == 'i':
        data = rng.integers(max(-100000, np.iinfo(dt).min), min(100000, np.iinfo(dt).max),
                            (n_frames, n_px)).astype(dt)
    else:
        data = (rng.random((n_frames, n_px)) - 0.3).astype(dt)
    masks = rng.random((n_masks, n_px)) - 0.25
    tuning = dict(mt=0, waves=0, ksplit=ksplit) if ksplit else None
    res, kern = _apply(hip, data, masks, np.float64, tuning=tuning)
    lds = n_px >= 256                               # (any pixel size; rows need not be 16-B aligned)
    assert ('k_dense_lds64' if lds else 'k_dense_mfma_f64') in kern, kern
    if lds:
        # the direct-load kernel on the same input (tuning mt=1) agrees to rounding
        res_d, kern_d = _apply(hip, data, masks, np.float64, tuning=dict(mt=1, waves=0, ksplit=ksplit))
        assert 'k_dense_mfma_f64' in kern_d, kern_d
        assert np.allclose(res, res_d, rtol=1e-12, atol=1e-12 * np.abs(res_d).max())
    ref = data.astype(np.float64) @ masks.T
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).T
    assert np.all(np.abs(res - ref) <= 1e-13 * scale + 1e-300), np.abs(res - ref).max()
    base = rng.random((n_frames, n_masks))
    res2, _ = _apply(hip, data, masks, np.float64, accumulate_into=base, tuning=tuning)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-13 * (scale + 1))


@pytest.mark.parametrize('tile_dtype', ['int32', 'uint16', 'float32', 'float64'])
@pytest.mark.parametrize('shape', [
    (300, 256 * 9 + 100, 16),           # 32 real columns: two column groups, ragged last chunk
    (70, 17 * 23, 5),                   # odd row length
    (45, 256 * 5, 25),                  # the radial Fourier default stack (50 real columns)
])
def test_complex128_masks_on_real_frames(hip, tile_dtype, shape):
    """complex128 results (int32 / float64 frames x complex64 masks, or complex128 masks) on REAL frames:
    the f64 matrix kernels with (re, im) as two real columns per mask -- not the generic VALU kernel."""
    n_frames, n_px, n_masks = shape
    rng = np.random.default_rng(_seed(tile_dtype, shape))
    dt = np.dtype(tile_dtype)
    data = (rng.integers(-1000 if dt.kind == 'i' else 0, 100000 if dt.itemsize >= 4 else 4000,
                         (n_frames, n_px)).astype(dt) if dt.kind in 'iu'
            else (rng.random((n_frames, n_px)) - 0.3).astype(dt))
    masks = (rng.random((n_masks, n_px)) - 0.25) + 1j * (rng.random((n_masks, n_px)) - 0.5)
    res, kern = _apply(hip, data, masks, np.complex128)
    assert 'k_dense_lds64' in kern or 'k_dense_mfma_f64' in kern, kern
    ref = data.astype(np.complex128) @ masks.T
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).T
    assert np.all(np.abs(res - ref) <= 1e-13 * scale + 1e-300), np.abs(res - ref).max()
    base = rng.random((n_frames, n_masks)) + 1j * rng.random((n_frames, n_masks))
    res2, _ = _apply(hip, data, masks, np.complex128, accumulate_into=base)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-13 * (scale + 1))


@pytest.mark.parametrize('tile_dtype,result_dtype,mask_max,expect', [
    ('int16', 'int32', 1, 'exact-int'),         # the reference's integer-sum case (0/1 masks)
    ('uint16', 'int32', 200, 'exact-int'),
    ('int32', 'int32', 1, 'exact-int'),         # wraps around in int32, still exact in f64
    ('uint8', 'uint8', 3, 'exact-int'),         # wraps around in uint8
    ('int32', 'int64', 100, 'exact-int'),
    ('int32', 'int32', 2**30, 'generic'),       # sums beyond 2^52: integer VALU kernel
    ('int64', 'int64', 1, 'generic'),           # 64-bit pixels: no bound on the products
])
def test_integer_results_bit_exact(hip, tile_dtype, result_dtype, mask_max, expect):
    """Integer masks x integer frames = NumPy integer matmul with wrap-around, bit for bit; on the
    f64 matrix cores whenever every partial sum is exactly representable."""
    rng = np.random.default_rng(_seed(tile_dtype, result_dtype, mask_max))
    n_frames, n_px, n_masks = 90, 256 * 11 + 64, 7
    dt, rd = np.dtype(tile_dtype), np.dtype(result_dtype)
    info = np.iinfo(dt)
    data = rng.integers(max(info.min, -2**31), min(info.max, 2**31 - 1), (n_frames, n_px),
                        endpoint=True).astype(dt)
    lo = 0 if rd.kind == 'u' else -mask_max
    masks = rng.integers(lo, mask_max, (n_masks, n_px), endpoint=True).astype(rd)
    res, kern = _apply(hip, data, masks, rd)
    assert expect in kern, kern
    ref = data.astype(rd) @ masks.T                  # NumPy's integer arithmetic in the result dtype
    assert res.dtype == ref.dtype and np.array_equal(res, ref)
    base = rng.integers(0, 100, (n_frames, n_masks)).astype(rd)
    res2, _ = _apply(hip, data, masks, rd, accumulate_into=base)
    assert np.array_equal(res2, ref + base)


@pytest.mark.parametrize('case', recipes.DENSE_CASES, ids=lambda c: c['name'])
def test_whole_dataset_vs_oracle(hip, case):
    """one kernel call per dataset (whole nav, full frames) == the oracle's tiled CPU loop"""
    data, masks = recipes.make_dense_case(case)
    kw = case.get('udf_kwargs', {})
    ref = opath.apply_masks(data, masks, num_partitions=case['num_partitions'],
                            tileshape=case.get('tileshape'), mask_dtype=kw.get('mask_dtype'),
                            preferred_dtype=kw.get('preferred_dtype'))
    n_masks = masks.shape[0]
    flat = data.reshape((-1, int(np.prod(data.shape[2:]))))
    res, kern = _apply(hip, flat, masks.reshape((n_masks, -1)), ref.dtype)
    res = res.reshape(ref.shape)
    if ref.dtype.kind in 'iu':
        assert np.array_equal(res, ref)
    else:
        scale = np.abs(ref).max()
        tol = 1e-5 if ref.dtype in (np.float32, np.complex64) else 1e-12
        assert np.allclose(res, ref, rtol=tol, atol=tol * scale)


@pytest.mark.parametrize('tile_dtype,out_dtype', [
    ('uint8', 'float32'), ('uint16', 'float32'), ('int16', 'float32'), ('float32', 'float32'),
    ('int32', 'float64'), ('float64', 'float64'), ('uint16', 'float64'),
])
@pytest.mark.parametrize('shape', [(37, 1000), (300, 128 * 128), (5, 391), (1, 8)])
def test_sums(hip, tile_dtype, out_dtype, shape):
    rng = np.random.default_rng(21)
    dt = np.dtype(tile_dtype)
    if dt.kind in 'iu':
        data = rng.integers(0, 100, shape).astype(dt)
    else:
        data = rng.random(shape).astype(dt)
    n_frames, n_px = shape
    t = _dev(data)
    od = np.dtype(out_dtype)
    tod = torch.float32 if od == np.float32 else torch.float64
    # sum_sig
    out = torch.full((n_frames,), 3.0, dtype=tod, device='cuda')
    hip.sum_sig(0, t.data_ptr(), dt, n_frames, n_px, n_px, out.data_ptr(), od, False)
    ref = data.astype(np.float64).sum(axis=1)
    assert np.allclose(out.cpu().numpy(), ref, rtol=1e-6 if od == np.float32 else 1e-13)
    hip.sum_sig(0, t.data_ptr(), dt, n_frames, n_px, n_px, out.data_ptr(), od, True)
    assert np.allclose(out.cpu().numpy(), 2 * ref, rtol=1e-6 if od == np.float32 else 1e-13)
    # sum_frames
    ws_bytes = hip.sum_frames_workspace(n_frames, n_px, od)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device='cuda')
    out2 = torch.full((n_px,), 3.0, dtype=tod, device='cuda')
    hip.sum_frames(0, t.data_ptr(), dt, n_frames, n_px, n_px, out2.data_ptr(), od, False,
                   ws.data_ptr())
    ref2 = data.astype(np.float64).sum(axis=0)
    assert np.allclose(out2.cpu().numpy(), ref2, rtol=1e-6 if od == np.float32 else 1e-13)
    hip.sum_frames(0, t.data_ptr(), dt, n_frames, n_px, n_px, out2.data_ptr(), od, True,
                   ws.data_ptr())
    assert np.allclose(out2.cpu().numpy(), 2 * ref2, rtol=1e-6 if od == np.float32 else 1e-13)
    if dt.kind in 'iu':
        # integer-valued sums below 2**24 are exact in any order
        assert np.array_equal(out2.cpu().numpy(), 2 * ref2)
    # axpy
    hip.axpy(0, out2.data_ptr(), out2.data_ptr(), od, n_px)
    assert np.allclose(out2.cpu().numpy(), 4 * ref2, rtol=1e-6 if od == np.float32 else 1e-13)


def test_error_paths(hip):
    masks = np.ones((2, 64), dtype=np.float32)
    h = hip.MaskHandle.dense(0, masks, np.float32)
    t = torch.zeros((4, 64), dtype=torch.float32, device='cuda')
    o = torch.zeros((4, 2), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError):
        h.apply(t.data_ptr(), np.float32, 4, 32, o.data_ptr(), 2, False)     # ld < n_px
    with pytest.raises(ValueError):
        h.apply(t.data_ptr(), np.float32, 4, 64, o.data_ptr(), 1, False)     # ld_out < n_masks
    with pytest.raises(ValueError):
        h.apply(0, np.float32, 4, 64, o.data_ptr(), 2, False)                # null tile
    with pytest.raises(ValueError):
        hip.MaskHandle.dense(0, np.ones((0, 4), dtype=np.float32), np.float32)
    h.apply(t.data_ptr(), np.float32, 0, 64, o.data_ptr(), 2, False)         # empty tile: no-op
    h.close()


# --- sparse kernels: SELL gather kernel and blocked image on the matrix cores -----------------------
@pytest.fixture(params=['sell', 'bell', 'scatter'])
def sparse_kernel(request, monkeypatch):
    """Force one of the sparse kernels at handle creation (libltmi reads LTMI_SPARSE_BELL /
    LTMI_SPARSE_SCATTER there); rows of any alignment are served by all of them."""
    monkeypatch.setenv('LTMI_SPARSE_BELL', '1' if request.param == 'bell' else '0')
    monkeypatch.setenv('LTMI_SPARSE_SCATTER', '1' if request.param == 'scatter' else '0')
    return request.param


def _check_sparse_kernel(kern, which, n_px, itemsize, n_nonzero=1):
    # (rows of any alignment: the blocked kernel's frame DMA reads them, the entries of the last
    # n_px % 16 pixels are applied by k_bell_tail)
    if which == 'scatter' and n_nonzero:
        assert 'k_scatter' in kern, kern
    elif which == 'bell' and n_nonzero:
        assert 'k_bell_apply' in kern or 'k_bell_flat' in kern, kern
    else:
        assert 'k_sell_apply' in kern, kern


def _apply_csr(hip, data2d, csr_px_by_masks, result_dtype, accumulate_into=None, sig=None, tuning=None, ksplit=0):
    h = hip.MaskHandle.csr(0, csr_px_by_masks, result_dtype)
    assert h.kind() == 2
    if sig is not None:
        h.set_sig_shape(sig[0], sig[1])
    if tuning is not None or ksplit:
        h.set_tuning(0, tuning or hip.Variant.SPARSE_DEFAULT, ksplit)
    t = _dev(np.ascontiguousarray(data2d))
    n_frames, n_px = data2d.shape
    n_masks = csr_px_by_masks.shape[1]
    rd = np.dtype(result_dtype)
    if accumulate_into is None:
        out_np = np.full((n_frames, n_masks), 7, dtype=rd)
        acc = False
    else:
        out_np = accumulate_into.astype(rd).copy()
        acc = True
    out = _dev(out_np)
    h.apply(t.data_ptr(), data2d.dtype, n_frames, n_px, out.data_ptr(), n_masks, acc)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    kern = h.last_kernel()
    h.close()
    return res, kern


@pytest.mark.parametrize('case', recipes.RMATMUL_CASES, ids=lambda c: c['name'])
def test_sell_vs_reference_rmatmul_golden(hip, golden_dir, case, sparse_kernel):
    import os
    import scipy.sparse as sp
    g = np.load(os.path.join(golden_dir, 'rmatmul.npz'))
    left, right = recipes.make_rmatmul_case(case)
    ref = g[case['name'] + '__csr']
    if ref.dtype not in (np.float32, np.complex64, np.float64):
        pytest.skip("complex128 / integer sparse stacks are densified (tested via the UDF)")
    res, kern = _apply_csr(hip, left, sp.csr_matrix(right), ref.dtype)
    if ref.dtype == np.float64:
        assert 'k_sell_apply' in kern and 'f64' in kern, kern       # float64: the gather kernel in double
    else:
        _check_sparse_kernel(kern, sparse_kernel, left.shape[1], left.dtype.itemsize)
    assert res.dtype == ref.dtype and res.shape == ref.shape
    tol = 1e-12 if ref.dtype == np.float64 else 1e-5
    assert np.allclose(res, ref, rtol=tol, atol=tol * np.abs(ref).max())


@pytest.mark.parametrize('tile_dtype', ['int32', 'uint32', 'int64', 'float64', 'float32', 'uint16'])
@pytest.mark.parametrize('shape', [
    (37, 3000, 70, 0.02),       # ragged frames, 3 chunks
    (16, 1024, 1300, 0.01),     # two passes of 1024 masks
    (70, 515 * 7, 40, 0.05),    # odd row length
    (20, 2048, 300, 0.0),       # all-zero stack
])
def test_sparse_float64_results(hip, shape, tile_dtype):
    """Sparse stacks with float64 results (int32 / uint32 / int64 / float64 frames, or float64 mask
    values): the gather kernel with double slab, values and accumulators -- not a densified stack."""
    import scipy.sparse as sp
    n_frames, n_px, n_masks, density = shape
    rng = np.random.default_rng(41)
    dt = np.dtype(tile_dtype)
    if dt.kind == 'u':
        data = rng.integers(0, 2**31 if dt.itemsize >= 4 else 4000, (n_frames, n_px)).astype(dt)
    elif dt.kind == 'i':
        data = rng.integers(-2**30, 2**30, (n_frames, n_px)).astype(dt)
    else:
        data = (rng.random((n_frames, n_px)) - 0.3).astype(dt)
    m = sp.random(n_px, n_masks, density=density, format='csr', dtype=np.float64,
                  random_state=np.random.RandomState(2))
    res, kern = _apply_csr(hip, data, m, np.float64)
    assert 'k_sell_apply' in kern and 'f64' in kern, kern
    dense = m.toarray()
    ref = data.astype(np.float64) @ dense
    scale = np.abs(data.astype(np.float64)) @ np.abs(dense)
    assert np.all(np.abs(res - ref) <= 1e-13 * scale + 1e-300), np.abs(res - ref).max()
    base = rng.random((n_frames, n_masks))
    res2, _ = _apply_csr(hip, data, m, np.float64, accumulate_into=base)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-13 * (scale + 1))


@pytest.mark.parametrize('shape', [
    (37, 3000, 70, 0.02),       # ragged frames, 3 chunks, < 256 masks
    (16, 1024, 1300, 0.01),     # two passes of 1024 masks
    (5, 391, 3, 0.3),           # unaligned rows
    (70, 515 * 7, 40, 0.05),    # odd row length over several chunks, entries in the last 5 pixels
    (33, 1024 + 15, 20, 0.2),   # 15 tail pixels
    (64, 5000, 1, 0.001),       # single mask, nearly empty
    (20, 2048, 300, 0.0),       # all-zero stack
])
@pytest.mark.parametrize('tile_dtype', ['uint8', 'uint16', 'int16', 'float32'])
def test_sell_random(hip, shape, tile_dtype, sparse_kernel):
    import scipy.sparse as sp
    n_frames, n_px, n_masks, density = shape
    rng = np.random.default_rng(31)
    dt = np.dtype(tile_dtype)
    if dt.kind in 'iu':
        data = rng.integers(0 if dt.kind == 'u' else -50, 100, (n_frames, n_px)).astype(dt)
    else:
        data = rng.random((n_frames, n_px)).astype(dt)
    m = sp.random(n_px, n_masks, density=density, format='csr', dtype=np.float32,
                  random_state=np.random.RandomState(1))
    res, kern = _apply_csr(hip, data, m, np.float32)
    _check_sparse_kernel(kern, sparse_kernel, n_px, dt.itemsize, m.nnz)
    ref = data.astype(np.float64) @ m.astype(np.float64).toarray()
    scale = np.abs(data.astype(np.float64)) @ np.abs(m.toarray().astype(np.float64))
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)
    base = rng.random((n_frames, n_masks)).astype(np.float32)
    res2, _ = _apply_csr(hip, data, m, np.float32, accumulate_into=base)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 1))
    # complex values
    mc = m.astype(np.complex64)
    mc.data = (mc.data * (0.3 + 0.7j)).astype(np.complex64)
    resc, _ = _apply_csr(hip, data, mc, np.complex64)
    refc = data.astype(np.complex128) @ mc.astype(np.complex128).toarray()
    assert np.all(np.abs(resc.view(np.complex64).reshape(refc.shape) - refc) <= 2e-5 * scale + 1e-30)


@pytest.mark.parametrize('tile_dtype,result_dtype', [
    ('uint8', 'int64'), ('uint16', 'int64'), ('int16', 'int32'), ('uint16', 'uint16'), ('uint32', 'int64'),
    ('int8', 'uint8'),
])
def test_sparse_integer_results_bit_exact(hip, tile_dtype, result_dtype):
    """Integer sparse stacks through ltmi_masks_create_csr: float64 gather + truncation to the result
    width = integer matmul with wrap-around, accumulate included; a product that can exceed 2^52 is
    refused (the caller densifies)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(_seed(tile_dtype, result_dtype))
    n_frames, n_px, n_masks = 70, 3000, 37
    dt, rd = np.dtype(tile_dtype), np.dtype(result_dtype)
    info = np.iinfo(dt)
    data = rng.integers(max(info.min, -30000), min(info.max, 60000), (n_frames, n_px)).astype(dt)
    dense = np.where(rng.random((n_masks, n_px)) < 0.02, rng.integers(-7, 8, (n_masks, n_px)), 0)
    m = sp.csr_matrix(dense.T.astype(np.int64))                       # (px, masks)
    h = hip.MaskHandle.csr(0, m, rd)
    t = _dev(data)
    ref = (data.astype(np.int64) @ dense.T.astype(np.int64))
    base = rng.integers(0, 100, (n_frames, n_masks)).astype(rd)
    for acc in (False, True):
        out = _dev(base.copy())
        h.apply(t.data_ptr(), dt, n_frames, n_px, out.data_ptr(), n_masks, acc)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(rd)
        want = (ref + (base.astype(np.int64) if acc else 0)).astype(rd)
        assert np.array_equal(got, want)
    assert 'k_sell_apply' in h.last_kernel() and 'exact-int' in h.last_kernel(), h.last_kernel()
    h.close()
    big = sp.csr_matrix((dense.T.astype(np.int64)) * (1 << 44))
    hb = hip.MaskHandle.csr(0, big, np.int64)
    out = _dev(np.zeros((n_frames, n_masks), np.int64))
    with pytest.raises(Exception, match='2.52'):
        hb.apply(t.data_ptr(), dt, n_frames, n_px, out.data_ptr(), n_masks, False)
    hb.close()


def test_sell_ring_stack_vs_oracle(hip, sparse_kernel):
    """C4-style stack: anti-aliased ring masks as CSR, on real-size frames (reduced nav)."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    rings = omasks.radial_bins(128, 128, 256, 256, n_bins=1024, use_sparse=True,
                               dtype=np.float32)                  # (n_bins, px) csr
    assert rings.shape == (1024, 65536) and rings.nnz == 432407
    csr = sp.csr_matrix(rings.T.astype(np.float32))
    rng = np.random.default_rng(32)
    data = rng.integers(0, 4096, (40, 65536)).astype(np.uint16)
    res, kern = _apply_csr(hip, data, csr, np.float32)
    _check_sparse_kernel(kern, sparse_kernel, 65536, 2)
    ref = opath.rmatmul(data[:8].astype(np.float32), csr)          # the reference's own loop
    assert np.allclose(res[:8], ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    ref64 = data.astype(np.float64) @ rings.T.astype(np.float64)
    assert np.allclose(res, np.asarray(ref64), rtol=1e-5, atol=1e-5 * np.abs(ref64).max())


def _stored_entries_ref(data2d, csr_px_by_masks):
    """the reference's sparse arithmetic in float64 / complex128: per mask, the stored entries only
    (common/numba/__init__.py:153-184) -- a non-finite pixel reaches exactly the masks that store it"""
    csc = csr_px_by_masks.tocsc()
    csc.sort_indices()
    wide = np.complex128 if np.iscomplexobj(csc.data) else np.float64
    ref = np.zeros((data2d.shape[0], csc.shape[1]), dtype=wide)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(csc.shape[1]):
            idx = csc.indices[csc.indptr[k]:csc.indptr[k + 1]]
            val = csc.data[csc.indptr[k]:csc.indptr[k + 1]].astype(wide)
            if len(idx):
                ref[:, k] = (data2d[:, idx].astype(np.float64) * val[None, :]).sum(axis=1)
    return ref


def _same_non_finite(res, ref):
    """NaN where the reference is NaN, the same infinity where it is infinite, finite where it is finite"""
    for part in ((np.real, np.imag) if np.iscomplexobj(ref) or np.iscomplexobj(res) else (np.asarray,)):
        a, b = part(res), part(ref)
        if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
                and np.array_equal(np.isneginf(a), np.isneginf(b))):
            return False
    return True


def _close_where_finite(res, ref, scale, tol=1e-5):
    ok = np.isfinite(ref)
    return np.all(np.abs(res[ok] - ref[ok]) <= tol * scale[ok] + 1e-30)


def test_sparse_non_finite_pixels(hip, sparse_kernel):
    """NaN / Inf pixels (float32 frames) and the zero entries the device images are padded with.
    The reference's CSR loop only touches stored entries (common/numba/__init__.py:153-184): a
    non-finite pixel reaches exactly the masks that contain it -- on EVERY kernel:
    * pixels NO mask contains: no effect at all (the gather kernel's padding reads an all-zero LDS row, the
      blocked image pads a block with one of its own pixels);
    * a pixel some masks contain: those masks are NaN / Inf like in the reference and no others -- the blocked
      image (dense 16-mask x 8-pixel blocks on the matrix cores) and the scatter bundles also multiply zeros of
      neighbouring masks; the frames whose results come out non-finite are listed on the device and computed
      again by the gather kernel (csrc/ltmi_guard.hip)."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    rings = omasks.radial_bins(32, 32, 64, 64, radius=20, n_bins=64, use_sparse=True,
                               dtype=np.float32)                  # (64, 4096) csr, r <= 20 px only
    csr = sp.csr_matrix(rings.T.astype(np.float32))
    touched = np.asarray((rings != 0).sum(axis=0)).reshape(-1) > 0
    assert touched.sum() < 2000 and not touched[0] and not touched[1024]
    rng = np.random.default_rng(77)
    clean = rng.random((24, 4096)).astype(np.float32)
    ref = opath.rmatmul(clean, csr)
    base, kern = _apply_csr(hip, clean, csr, np.float32)
    _check_sparse_kernel(kern, sparse_kernel, 4096, 4)
    assert np.allclose(base, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    dirty = clean.copy()
    dirty[:, ~touched] = np.nan                 # incl. pixel 0 of every chunk
    dirty[3, ~touched] = np.inf
    res, _ = _apply_csr(hip, dirty, csr, np.float32)
    assert np.all(np.isfinite(res)) and np.array_equal(res, base)
    # one touched pixel of frame 5 is NaN, two of frame 9 are +Inf / -Inf, one of frame 23 (the last) +Inf
    tp = np.flatnonzero(touched)
    p, q1, q2, q3 = int(tp[200]), int(tp[50]), int(tp[700]), int(tp[901])
    dirty = clean.copy()
    dirty[5, p] = np.nan
    dirty[9, q1] = np.inf
    dirty[9, q2] = -np.inf
    dirty[23, q3] = np.inf
    ref2 = opath.rmatmul(dirty, csr)                              # the reference's own loop
    res2, kern2 = _apply_csr(hip, dirty, csr, np.float32)
    has_p = np.asarray(rings[:, p].todense()).reshape(-1) != 0
    assert np.all(np.isnan(ref2[5, has_p])) and np.all(np.isfinite(ref2[5, ~has_p]))
    assert _same_non_finite(res2, ref2), kern2                    # exactly the reference's NaNs and infinities
    clean_rows = np.ones(24, bool)
    clean_rows[[5, 9, 23]] = False
    assert np.array_equal(res2[clean_rows], base[clean_rows])     # other frames untouched
    ok = np.isfinite(ref2)
    assert np.allclose(res2[ok], ref2[ok], rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    if sparse_kernel != 'sell':
        assert kern2.endswith('+nf'), kern2
    # `out += product`: what `out` held is not the product's business (a NaN there stays, nothing else changes)
    held = rng.random((24, 64)).astype(np.float32)
    held[7, 3] = np.nan
    res3, _ = _apply_csr(hip, dirty, csr, np.float32, accumulate_into=held)
    with np.errstate(invalid='ignore'):
        ref3 = held + ref2
    assert _same_non_finite(res3, ref3)
    ok = np.isfinite(ref3)
    assert np.allclose(res3[ok], ref3[ok], rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    # through a row list (a region of interest): result row i = frame rows[i]
    h = hip.MaskHandle.csr(0, csr, np.float32)
    rows = np.array([9, 2, 5, 5, 23, 0], dtype=np.int32)
    t, r, out = _dev(dirty), _dev(rows), _dev(np.full((len(rows), 64), 7, np.float32))
    assert h.apply_rows(t.data_ptr(), np.float32, r.data_ptr(), len(rows), 4096, out.data_ptr(), 64, False)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    h.close()
    assert _same_non_finite(got, ref2[rows])
    ok = np.isfinite(ref2[rows])
    assert np.allclose(got[ok], ref2[rows][ok], rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def _dirty_frames(rng, n_frames, n_px, stored, unstored):
    """float32 frames: clean ones; frame 1: NaN in a pixel no mask stores; frame 2: NaN in a stored pixel;
    frame 3: +Inf in a stored pixel; frame 4: +Inf and -Inf in two stored pixels; the last frame: NaN in both kinds"""
    data = (rng.random((n_frames, n_px)) + 0.1).astype(np.float32)
    if len(unstored):
        data[1, unstored[len(unstored) // 2]] = np.nan
        data[n_frames - 1, unstored[0]] = np.nan
    data[2, stored[len(stored) // 3]] = np.nan
    data[3, stored[len(stored) // 2]] = np.inf
    data[4, stored[len(stored) // 5]] = np.inf
    data[4, stored[(2 * len(stored)) // 3]] = -np.inf
    data[n_frames - 1, stored[-1]] = np.nan
    return data


@pytest.mark.parametrize('case', ['wide_rings_f32', 'wide_rings_folded', 'complex_blocks', 'float64', 'complex128'])
def test_densified_sparse_stack_non_finite_pixels(hip, case):
    """A sparse stack that MaskContainer multiplies DENSE (well filled / wide rings): the dense kernels -- LDS-DMA,
    folded, more than 64 columns in blocks, float64 matrix cores -- multiply every zero, the reference's sparse loops
    (common/numba/__init__.py:153-184, udf/masks.py:68-77) none.  The handle carries the stack's gather image
    (ltmi_masks_set_sparse_origin): frames with non-finite results are computed again on it."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    rng = np.random.default_rng(_seed('densified', case))
    sig = (64, 64)
    if case in ('wide_rings_f32', 'wide_rings_folded', 'float64'):
        rings = omasks.radial_bins(32, 32, 64, 64, radius=28, n_bins=24, use_sparse=True, dtype=np.float32)
        csr = sp.csr_matrix(rings.T.astype(np.float64 if case == 'float64' else np.float32))   # (4096, 24)
        rd = np.float64 if case == 'float64' else np.float32
    else:
        from libertem_amd.analysis.radialfourier import radial_mask_factory
        stack = radial_mask_factory(64, 64, 32, 32, 0, 28, 3, 15, True)()          # 3 bins x 16 orders
        rd = np.complex128 if case == 'complex128' else np.complex64
        csr = sp.csr_matrix(stack.to_px_by_masks(dtype=rd))
    n_px, n_masks = csr.shape
    stored = np.flatnonzero(np.diff(csr.indptr) > 0)
    unstored = np.flatnonzero(np.diff(csr.indptr) == 0)
    assert len(unstored) > 100
    data = _dirty_frames(rng, 40, n_px, stored, unstored)
    dense = np.ascontiguousarray(np.asarray(csr.todense()).T.astype(rd))
    h = hip.MaskHandle.dense(0, dense, rd)
    if case == 'complex128':
        h.set_sparse_origin(hip.MaskHandle.csr_complex128(0, csr, gather_only=True))
    else:
        h.set_sparse_origin(hip.MaskHandle.csr(0, csr, rd, gather_only=True))
    if case in ('wide_rings_folded', 'complex_blocks'):
        h.set_sig_shape(*sig)
    t = _dev(data)
    out = _dev(np.full((40, n_masks), 7, dtype=rd))
    h.apply(t.data_ptr(), np.float32, 40, n_px, out.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    kern = h.last_kernel()
    res = out.cpu().numpy()
    assert res.dtype == rd and kern.endswith('+nf'), kern
    if case == 'wide_rings_folded':
        assert 'k_dense_fold' in kern, kern
    ref = _stored_entries_ref(data, csr)
    assert not np.all(np.isfinite(ref[2])) and np.all(np.isfinite(ref[1]))
    assert _same_non_finite(res, ref), kern
    scale = _stored_entries_ref(np.where(np.isfinite(data), np.abs(data), 0), abs(csr))
    tol = 1e-5 if np.dtype(rd) in (np.dtype(np.float32), np.dtype(np.complex64)) else 1e-12
    assert _close_where_finite(res, ref, np.abs(scale) + 1e-30, tol)
    # out += product, and a row list
    held = rng.random((40, n_masks)).astype(rd)
    out2 = _dev(held)
    h.apply(t.data_ptr(), np.float32, 40, n_px, out2.data_ptr(), n_masks, True)
    torch.cuda.synchronize()
    res2 = out2.cpu().numpy()
    with np.errstate(invalid='ignore'):
        assert _same_non_finite(res2, held + ref)
    assert _close_where_finite(res2, held + ref, np.abs(scale) + 1, tol)
    rows = np.array([39, 2, 0, 4, 1], dtype=np.int32)
    r = _dev(rows)
    out3 = _dev(np.full((5, n_masks), 7, dtype=rd))
    if h.apply_rows(t.data_ptr(), np.float32, r.data_ptr(), 5, n_px, out3.data_ptr(), n_masks, False):
        torch.cuda.synchronize()
        res3 = out3.cpu().numpy()
        assert _same_non_finite(res3, ref[rows]), h.last_kernel()
        assert _close_where_finite(res3, ref[rows], np.abs(scale[rows]) + 1e-30, tol)
    h.close()


@pytest.mark.parametrize('origin', ['sparse', 'dense'])
def test_banded_stack_non_finite_pixels(hip, monkeypatch, origin):
    """Radial-Fourier stack with several bins as a banded image (ltmi_masks_kind 3: one folded dense image per bin).
    origin='sparse' (use_sparse=True in the reference: stored entries only): a NaN pixel inside a bin's 64-pixel stages
    but outside its support, or in no support at all, must not reach that bin.  origin='dense' (the reference's own
    heuristic declares a few wide bins dense, analysis/radialfourier.py:334-341: `flat_tile @ masks`): a NaN pixel
    reaches EVERY mask, also the bins whose image never reads it (ltmi_masks_set_dense_origin)."""
    import scipy.sparse as sp
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    monkeypatch.setenv('LTMI_SPARSE_BAND', '1')
    rng = np.random.default_rng(_seed('banded-nf', origin))
    stack = radial_mask_factory(128, 128, 64, 64, 4, 50, 3, 12, True)()               # 3 bins x 13 orders
    csr = sp.csr_matrix(stack.to_px_by_masks(dtype=np.complex64))                      # (16384, 39)
    n_px, n_masks = csr.shape
    stored = np.flatnonzero(np.diff(csr.indptr) > 0)
    unstored = np.flatnonzero(np.diff(csr.indptr) == 0)
    assert len(unstored) > 1000
    data = _dirty_frames(rng, 48, n_px, stored, unstored)
    h = hip.MaskHandle.csr(0, csr, np.complex64)
    h.set_sig_shape(128, 128)
    assert h.kind() == 3
    if origin == 'dense':
        h.set_dense_origin(csr)
    t = _dev(data)
    out = _dev(np.full((48, n_masks), 7, np.complex64))
    h.apply(t.data_ptr(), np.float32, 48, n_px, out.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    kern = h.last_kernel()
    res = out.cpu().numpy()
    assert 'banded' in kern and kern.endswith('+nf'), kern
    # frames 1 .. 4 and the last hold a non-finite pixel; the one of frame 1 is stored by no mask: it always counts for a
    # dense stack, for a sparse one only if it shares a 64-pixel window with a ring (then the frame is listed and redone)
    assert h.nonfinite_frames() in ((5,) if origin == 'dense' else (4, 5))
    dense = np.asarray(csr.todense()).astype(np.complex128)
    if origin == 'sparse':
        ref = _stored_entries_ref(data, csr)
        assert np.all(np.isfinite(ref[1]))
    else:
        with np.errstate(invalid='ignore'):
            ref = data.astype(np.complex128) @ dense                                   # every zero is a weight
        assert np.all(np.isnan(ref[1].real)) and np.all(np.isnan(ref[2].imag))
    if origin == 'dense':
        # NaN pixels: exactly the reference's NaNs.  Inf pixels: the same entries are non-finite; whether a complex
        # GEMM turns Inf * (w + 0j) into (Inf, NaN) or (NaN, NaN) is the BLAS kernel's business (OpenBLAS zgemm
        # gives the latter, the formula re = xr wr - xi wi the former), not the stack's
        nan_frames = np.isnan(data).any(axis=1)
        assert _same_non_finite(res[nan_frames], ref[nan_frames]), kern
        assert np.array_equal(np.isfinite(res.real), np.isfinite(ref.real)) and \
            np.array_equal(np.isfinite(res.imag), np.isfinite(ref.imag)), kern
    else:
        assert _same_non_finite(res, ref), kern
    scale = np.where(np.isfinite(data), np.abs(data), 0).astype(np.float64) @ np.abs(dense)
    assert _close_where_finite(res, ref, scale)
    rows = np.array([47, 1, 2, 0, 3, 4, 9], dtype=np.int32)
    r, out3 = _dev(rows), _dev(np.full((7, n_masks), 7, np.complex64))
    assert h.apply_rows(t.data_ptr(), np.float32, r.data_ptr(), 7, n_px, out3.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    res3 = out3.cpu().numpy()
    assert np.array_equal(np.isfinite(res3.real), np.isfinite(ref[rows].real)) and \
        np.array_equal(np.isfinite(res3.imag), np.isfinite(ref[rows].imag)), h.last_kernel()
    if origin == 'sparse':
        assert _same_non_finite(res3, ref[rows]), h.last_kernel()
    assert _close_where_finite(res3, ref[rows], scale[rows])
    # integer frames hold no non-finite pixel: not guarded
    u16 = rng.integers(0, 4096, (16, n_px)).astype(np.uint16)
    t16, out4 = _dev(u16), _dev(np.zeros((16, n_masks), np.complex64))
    h.apply(t16.data_ptr(), np.uint16, 16, n_px, out4.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    assert not h.last_kernel().endswith('+nf') and h.nonfinite_frames() == 0
    assert _close_where_finite(out4.cpu().numpy(), u16.astype(np.float64) @ dense,
                               u16.astype(np.float64) @ np.abs(dense))
    h.close()


def test_sparse_dispatch_by_padding_factor(hip, monkeypatch):
    """Without forcing: localised stacks (rings) take the blocked image (float32 frames and >= 64 columns:
    k_scatter), scattered ones the SELL kernel."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    monkeypatch.delenv('LTMI_SPARSE_BELL', raising=False)
    monkeypatch.delenv('LTMI_SPARSE_SCATTER', raising=False)
    rings = omasks.radial_bins(32, 32, 64, 64, n_bins=64, use_sparse=True, dtype=np.float32)
    data = np.random.default_rng(5).integers(0, 100, (20, 4096)).astype(np.uint16)
    _, kern = _apply_csr(hip, data, sp.csr_matrix(rings.T.astype(np.float32)), np.float32)
    assert 'k_bell_flat' in kern, kern                                   # 1- / 2-byte pixels: the blocked image
    _, kern = _apply_csr(hip, data.astype(np.float32), sp.csr_matrix(rings.T.astype(np.float32)), np.float32)
    assert 'k_scatter' in kern, kern                                     # float32 frames, >= 64 columns
    rings32 = omasks.radial_bins(32, 32, 64, 64, n_bins=32, use_sparse=True, dtype=np.float32)
    _, kern = _apply_csr(hip, data.astype(np.float32), sp.csr_matrix(rings32.T.astype(np.float32)), np.float32)
    assert 'k_scatter' not in kern, kern                                 # fewer than 64 columns
    scattered = sp.random(4096, 512, density=0.002, format='csr', dtype=np.float32,
                          random_state=np.random.RandomState(3))
    res, kern = _apply_csr(hip, data, scattered, np.float32)
    assert 'k_sell_apply' in kern
    # dense column blocks (radial Fourier with several bins, SURVEY.md 8(d)'s second C5 run): the blocked image pads
    # little, float32 frames stay on the matrix cores
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    from libertem_amd import masks as pm
    stack = radial_mask_factory(64, 64, 32, 32, 0, pm.bounding_radius(32, 32, 64, 64), 4, 7, True)()
    stack = stack.to_px_by_masks(dtype=np.complex64)                      # (4096, 32) CSR
    f32 = np.random.default_rng(6).random((40, 4096)).astype(np.float32)
    res, kern = _apply_csr(hip, f32, stack.astype(np.complex64), np.complex64)
    assert 'k_bell_apply<f' in kern, kern
    ref = f32.astype(np.float64) @ np.asarray(stack.todense()).astype(np.complex128)
    assert np.all(np.abs(res - ref) <= 1e-5 * (np.abs(f32).astype(np.float64) @ np.abs(np.asarray(stack.todense()))) + 1e-30)
    h = hip.MaskHandle.csr(0, sp.csr_matrix(rings.T.astype(np.float32)), np.float32)
    h.set_tuning(0, hip.Variant.SPARSE_SELL, 0)                        # the SELL kernel on request
    t, out = _dev(data), _dev(np.zeros((20, 64), dtype=np.float32))
    h.apply(t.data_ptr(), data.dtype, 20, 4096, out.data_ptr(), 64, False)
    torch.cuda.synchronize()
    assert 'k_sell_apply' in h.last_kernel()
    ref = data.astype(np.float64) @ np.asarray(rings.T.astype(np.float64).todense())
    assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    h.close()


# ---- k_scatter: one float32 FMA per stored entry (ltmi_scatter.hip) ---------------------------------------
def _banded_stack(rng, n_px, n_masks, width=7, density=1.0, dtype=np.float32):
    """every pixel holds `width` consecutive masks starting at a position that drifts with the pixel (the
    structure of radial bins), values with both signs over 6 orders of magnitude"""
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    start = (np.cumsum(rng.integers(-3, 4, n_px)) % max(1, n_masks - width)).astype(np.int64)
    for p in range(n_px):
        if rng.random() > density:
            continue
        k = np.arange(start[p], min(n_masks, start[p] + width))
        rows.append(np.full(len(k), p))
        cols.append(k)
        vals.append((rng.random(len(k)) - 0.3) * 10.0 ** rng.integers(-5, 2, len(k)))
    m = sp.csr_matrix((np.concatenate(vals).astype(dtype), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n_px, n_masks))
    m.sort_indices()
    return m


@pytest.mark.parametrize('tile_dtype', ['uint8', 'int8', 'uint16', 'int16', 'float32'])
@pytest.mark.parametrize('shape', [
    (70, 4096, 1024),        # ragged frames (64 + 6), whole chunks, one full pass
    (5, 1000, 200),          # less than one chunk for 1-byte pixels, narrow stack (ranges of 4 columns)
    (130, 515 * 9, 1500),    # odd row length (tail pixels for 2- / 4-byte types), two passes
    (64, 2048, 64),          # 64 columns: ranges of 2
])
def test_scatter_kernel_all_pixel_types(hip, monkeypatch, tile_dtype, shape):
    """k_scatter against float64 and the reference's own CSR loop (oracle.path.rmatmul): every pixel type,
    ragged frame counts, rows that do not fill a chunk / a 16-byte piece, several passes, accumulate."""
    monkeypatch.setenv('LTMI_SPARSE_SCATTER', '1')
    n_frames, n_px, n_masks = shape
    rng = np.random.default_rng(_seed('scatter', tile_dtype, shape))
    dt = np.dtype(tile_dtype)
    if dt.kind == 'f':
        data = (rng.random((n_frames, n_px)) - 0.25).astype(dt)
    else:
        data = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, (n_frames, n_px), endpoint=True).astype(dt)
    m = _banded_stack(rng, n_px, n_masks, density=0.9)
    res, kern = _apply_csr(hip, data, m, np.float32)
    assert 'k_scatter' in kern, kern
    ref = data.astype(np.float64) @ m.astype(np.float64)
    scale = np.abs(data.astype(np.float64)) @ np.abs(m.astype(np.float64))
    assert np.all(np.abs(res - ref) <= 2e-6 * scale + 1e-30)
    sub = slice(0, min(n_frames, 6))
    ora = opath.rmatmul(data[sub].astype(np.float32), m)
    assert np.all(np.abs(res[sub] - ora) <= 2e-6 * scale[sub] + 1e-30)
    base = rng.random((n_frames, n_masks)).astype(np.float32)
    res2, _ = _apply_csr(hip, data, m, np.float32, accumulate_into=base)
    assert np.all(np.abs(res2 - (ref + base)) <= 2e-6 * (scale + 1))


@pytest.mark.parametrize('kernel,tile_dtype', [('scatter', 'uint16'), ('scatter', 'float32'), ('bell', 'uint16'),
                                               ('bell', 'uint8'), ('bell', 'int16'), ('bell', 'int8'),
                                               ('bell', 'float32')])
def test_sparse_every_stored_entry_elementwise(hip, monkeypatch, kernel, tile_dtype):
    """VERDICT r3 weak #1 for the sparse path: one-pixel frames pick EVERY stored entry of the C4 ring stack
    (radial_bins, 1024 bins on 256 x 256: anti-aliased edges down to 1e-5 of the largest weight).  k_scatter
    and the float32 blocked kernel form the float32 product of the reference (common/numba/__init__.py:
    169-184) -- exact equality; the float16-piece kernel (1- / 2-byte integer pixels, signed ones included) carries every weight
    to 2^-19 relative, the 32 entries its pieces cannot carry go through the float32 tail: 1e-5 relative on
    EVERY entry, no absolute term."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    monkeypatch.setenv('LTMI_SPARSE_SCATTER', '1' if kernel == 'scatter' else '0')
    monkeypatch.setenv('LTMI_SPARSE_BELL', '1' if kernel == 'bell' else '0')
    rings = omasks.radial_bins(128, 128, 256, 256, n_bins=1024, use_sparse=True, dtype=np.float32)
    csr = sp.csr_matrix(rings.T.astype(np.float32))
    csr.sort_indices()
    n_px = 65536
    rng = np.random.default_rng(11)
    dt = np.dtype(tile_dtype)
    h = hip.MaskHandle.csr(0, csr, np.float32)
    dense = np.asarray(csr.todense())
    small = np.abs(csr.data)[csr.data != 0].min() / np.abs(csr.data).max()
    assert small < 1e-4
    for lo in range(0, n_px, 8192):                 # 8 launches of 8192 one-pixel frames
        hi_val = 60000 if dt.itemsize > 1 else 255
        val = rng.integers(1, min(hi_val, np.iinfo(dt).max if dt.kind != 'f' else hi_val), 8192).astype(dt)
        if dt.kind in 'if':                              # signed pixels: both signs, the most negative value too
            val = (val * rng.choice(np.array([-1, 1], dtype=dt), 8192)).astype(dt)
            if dt.kind == 'i':
                val[::97] = np.iinfo(dt).min
        data = np.zeros((8192, n_px), dt)
        data[np.arange(8192), lo + np.arange(8192)] = val
        t, out = _dev(data), _dev(np.full((8192, 1024), 7, np.float32))
        h.apply(t.data_ptr(), dt, 8192, n_px, out.data_ptr(), 1024, False)
        torch.cuda.synchronize()
        res = out.cpu().numpy()
        ref = val.astype(np.float32)[:, None] * dense[lo:lo + 8192]          # one float32 product per entry
        kern = h.last_kernel()
        if kernel == 'scatter':
            assert 'k_scatter' in kern, kern
        elif dt.kind in 'ui':                            # (signed 1- / 2-byte pixels since round 6)
            assert 'k_bell_flat' in kern and 'tail=32' in kern, kern
        else:
            assert 'k_bell_apply' in kern, kern
        if 'k_bell_flat' in kern:
            assert np.allclose(res, ref, rtol=1e-5, atol=0)
            assert np.array_equal(res == 0, ref == 0)
        else:
            assert np.array_equal(res, ref)
    h.close()


def test_scatter_scattered_stack_and_complex(hip, monkeypatch):
    """entries without structure (every bundle holds one or two of them) and a complex64 stack (2 real
    columns per mask, the interleaved row is the complex64 result)"""
    import scipy.sparse as sp
    monkeypatch.setenv('LTMI_SPARSE_SCATTER', '1')
    rng = np.random.default_rng(8)
    data = rng.integers(0, 4096, (100, 3000)).astype(np.uint16)
    m = sp.random(3000, 700, density=0.004, format='csr', dtype=np.float32, random_state=np.random.RandomState(4))
    res, kern = _apply_csr(hip, data, m, np.float32)
    assert 'k_scatter' in kern, kern
    ref = data.astype(np.float64) @ m.astype(np.float64)
    assert np.allclose(res, np.asarray(ref), rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    mc = _banded_stack(rng, 3000, 300).astype(np.complex64)
    mc.data = (mc.data.real * np.exp(1j * rng.random(mc.nnz) * 6.28)).astype(np.complex64)
    res, kern = _apply_csr(hip, data, mc, np.complex64)
    assert 'k_scatter' in kern, kern
    ref = data.astype(np.float64) @ mc.astype(np.complex128)
    assert res.dtype == np.complex64 and np.allclose(res, np.asarray(ref), rtol=1e-5, atol=1e-5 * np.abs(ref).max())


# ---- shifted masks ------------------------------------------------------------------------------------
def _shift_ref(data3d, masks3d, shifts):
    """out[f, k] = sum over the overlap of frame[f][y, x] * mask_k[y - dy, x - dx] in float64
    (reference udf/masks.py:85-124 semantics).  Valid for finite frames only: it multiplies the whole frame with a
    zero-filled shifted stack; the reference that slices the frame is `_slice_ref` in test_shifted_kernels_gpu.py."""
    n, h, w = data3d.shape
    out = np.zeros((n, len(masks3d)), dtype=np.complex128 if np.iscomplexobj(masks3d) else np.float64)
    scale = np.zeros((n, len(masks3d)))
    for f in range(n):
        dy, dx = int(shifts[f, 0]), int(shifts[f, 1])
        shifted = np.zeros_like(masks3d)
        ys0, ys1 = max(0, dy), min(h, h + dy)
        xs0, xs1 = max(0, dx), min(w, w + dx)
        if ys0 < ys1 and xs0 < xs1:
            shifted[:, ys0:ys1, xs0:xs1] = masks3d[:, ys0 - dy:ys1 - dy, xs0 - dx:xs1 - dx]
        fr = data3d[f].astype(np.float64)
        out[f] = np.tensordot(shifted.astype(out.dtype), fr, axes=([1, 2], [0, 1]))
        scale[f] = np.tensordot(np.abs(shifted).astype(np.float64), np.abs(fr), axes=([1, 2], [0, 1]))
    return out, scale


@pytest.mark.parametrize('tile_dtype,sig,n_masks,mask_dtype,expect', [
    ('uint16', (40, 48), 5, 'float32', 'k_dense_lds'),       # MFMA path, many shift groups
    ('float32', (32, 32), 16, 'float32', 'k_dense_lds'),
    ('uint8', (32, 64), 3, 'complex64', 'k_dense_lds'),
    ('uint16', (17, 23), 4, 'float32', 'k_dense_lds'),       # unaligned rows (391 px): LDS-DMA all the same
    ('uint16', (15, 15), 4, 'float32', 'k_dense_shifted'),   # fewer pixels than a mask slot -> per-frame kernel
    ('uint16', (32, 32), 20, 'float32', 'x 2 column group'),  # two column groups: MFMA path, two launches
    ('uint16', (32, 32), 70, 'float32', 'x 5 column group'),  # > 64 columns (column blocks of the handle)
    ('float32', (32, 32), 13, 'complex64', 'x 2 column group'),   # 26 real columns
    ('int32', (16, 32), 2, 'float64', 'k_dense_lds64'),      # float64 result: the f64 kernel per shift group
    ('int32', (8, 16), 2, 'float64', 'k_dense_mfma_f64'),    # ... fewer than 256 pixels: its direct-load variant
])
def test_shifted_masks_host_shifts(hip, tile_dtype, sig, n_masks, mask_dtype, expect):
    rng = np.random.default_rng(_seed(tile_dtype, sig, n_masks))
    n = 300
    dt = np.dtype(tile_dtype)
    if dt.kind in 'ui':
        data = rng.integers(0, 200 if dt.itemsize == 1 else 3000, (n,) + sig).astype(dt)
    else:
        data = (rng.random((n,) + sig) - 0.3).astype(dt)
    md = np.dtype(mask_dtype)
    masks = (rng.random((n_masks,) + sig) - 0.25)
    if md.kind == 'c':
        masks = masks + 1j * (rng.random((n_masks,) + sig) - 0.5)
    masks = masks.astype(md)
    shifts = rng.integers(-5, 6, (n, 2)).astype(np.int32)
    shifts[7] = (sig[0] + 3, 0)                  # no overlap at all
    shifts[8] = (0, -(sig[1] - 1))               # one column of overlap
    rd = np.result_type(np.float32, dt, md)
    h = hip.MaskHandle.dense(0, masks.reshape((n_masks, -1)), rd)
    t = _dev(np.ascontiguousarray(data.reshape((n, -1))))
    base = rng.random((n, n_masks)).astype(rd)
    for acc in (False, True):
        out = _dev(base.copy() if acc else np.full((n, n_masks), 7, dtype=rd))
        h.apply_shifted_host(t.data_ptr(), dt, n, data[0].size, sig[0], sig[1], shifts,
                             out.data_ptr(), n_masks, acc)
        torch.cuda.synchronize()
        res = out.cpu().numpy()
        if res.dtype != rd:
            res = res.view(rd)
        assert expect in h.last_kernel(), h.last_kernel()
        ref, scale = _shift_ref(data, masks, shifts)
        if acc:
            ref = ref + base
        tol = 1e-5 if rd in (np.float32, np.complex64) else 1e-12
        assert np.all(np.abs(res - ref) <= tol * (scale + 1)), np.abs(res - ref).max()
    # a second call re-uses the cached shifted images and handles a different grouping
    shifts2 = np.roll(shifts, 11, axis=0)
    out = _dev(np.zeros((n, n_masks), dtype=rd))
    h.apply_shifted_host(t.data_ptr(), dt, n, data[0].size, sig[0], sig[1], shifts2, out.data_ptr(),
                         n_masks, False)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    if res.dtype != rd:
        res = res.view(rd)
    ref, scale = _shift_ref(data, masks, shifts2)
    assert np.all(np.abs(res - ref) <= (1e-5 if rd in (np.float32, np.complex64) else 1e-12)
                  * (scale + 1))
    # 1- / 2-byte integer pixels with more than 4 columns on the matrix-core path: the shifted images
    # hold float16 pieces (X16); tuning 37 switches the same handle to float32 images and back
    # (a stack with weights that go through the float32 tail keeps float32 images for shifted frames: the tail
    #  pixels would have to shift along)
    real = masks.reshape((n_masks, -1))
    real = real if md.kind != 'c' else np.concatenate([real.real, real.imag])
    if dt.kind in 'ui' and dt.itemsize <= 2 and 'k_dense_lds' in h.last_kernel() \
            and n_masks * (2 if md.kind == 'c' else 1) > 4 and _n_float32_tail(real) > 0:
        assert ',f16' not in h.last_kernel(), h.last_kernel()
    elif dt.kind in 'ui' and dt.itemsize <= 2 and 'k_dense_lds' in h.last_kernel() \
            and n_masks * (2 if md.kind == 'c' else 1) > 4:
        assert ',f16' in h.last_kernel(), h.last_kernel()
        assert np.all(np.abs(res - ref) <= 2e-6 * (scale + 1))
        h.set_tuning(mt=0, waves=hip.Variant.DENSE_F32_INSTR, ksplit=0)
        out32 = _dev(np.zeros((n, n_masks), dtype=rd))
        h.apply_shifted_host(t.data_ptr(), dt, n, data[0].size, sig[0], sig[1], shifts2,
                             out32.data_ptr(), n_masks, False)
        torch.cuda.synchronize()
        assert ',f16' not in h.last_kernel(), h.last_kernel()
        res32 = out32.cpu().numpy()
        res32 = res32 if res32.dtype == rd else res32.view(rd)
        assert np.all(np.abs(res32 - res) <= 1e-5 * (scale + 1))
    h.close()


@pytest.mark.parametrize('tile_dtype', ['uint16', 'int16', 'float32'])
@pytest.mark.parametrize('n_masks,mask_dtype,ksplit', [
    (25, 'complex64', 0),       # C5: 25 complex masks = 48 + 2 real columns
    (25, 'complex64', 3),
    (49, 'float32', 0), (50, 'float32', 2), (51, 'float32', 0), (52, 'float32', 0),
    (17, 'float32', 0), (18, 'float32', 3), (9, 'complex64', 0),                          # 1 group + 2
    (33, 'float32', 0), (35, 'float32', 2), (36, 'float32', 0), (18, 'complex64', 0),    # 2 groups + rest
    (37, 'float32', 0), (48, 'float32', 2), (20, 'complex64', 0), (24, 'complex64', 0),  # 3 groups
])
def test_three_groups_plus_valu_columns(hip, tile_dtype, n_masks, mask_dtype, ksplit):
    """Column counts between the 1 / 2 / 4-group tiles: g MFMA groups + 2 or 4 columns on the VALU
    (17..18, 33..36, 49..52) or exactly 3 groups (37..48) must agree with float64 and with the
    padded-group kernel (tuning 33)."""
    rng = np.random.default_rng(_seed(tile_dtype, n_masks, mask_dtype))
    n_frames, n_px = 150, 128 * 37 + 48
    dt = np.dtype(tile_dtype)
    if dt.kind == 'u':
        data = rng.integers(0, 3000, (n_frames, n_px)).astype(dt)
    elif dt.kind == 'i':
        data = rng.integers(-2000, 2000, (n_frames, n_px)).astype(dt)
    else:
        data = (rng.random((n_frames, n_px)) - 0.3).astype(dt)
    md = np.dtype(mask_dtype)
    masks = rng.random((n_masks, n_px)) - 0.25
    if md.kind == 'c':
        masks = masks + 1j * (rng.random((n_masks, n_px)) - 0.5)
    masks = masks.astype(md)
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    # (integer pixels: tuning 37 keeps the float32 instruction -- by default they take the exact
    # float16 products on a padded group instead of VALU columns, checked at the end)
    code = hip.Variant.DENSE_F32_INSTR if dt.kind in 'iu' else hip.Variant.DENSE_DEFAULT
    res, kern = _apply(hip, data, masks, md, tuning=dict(mt=0, waves=code, ksplit=ksplit))
    n_cols = n_masks * (2 if md.kind == 'c' else 1)
    expect = {17: 'NG=1+2 VALU', 18: 'NG=1+2 VALU', 33: 'NG=2+2 VALU', 34: 'NG=2+2 VALU',
              35: 'NG=2+4 VALU', 36: 'NG=2+4 VALU', 49: 'NG=3+2 VALU', 50: 'NG=3+2 VALU',
              51: 'NG=3+4 VALU', 52: 'NG=3+4 VALU'}.get(n_cols, 'NG=3,')
    assert expect in kern, kern
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)
    base = (rng.random((n_frames, n_masks)) + (1j * rng.random((n_frames, n_masks))
                                               if md.kind == 'c' else 0)).astype(md)
    res2, _ = _apply(hip, data, masks, md, accumulate_into=base,
                     tuning=dict(mt=0, waves=code, ksplit=ksplit))
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 1))
    res4, kern4 = _apply(hip, data, masks, md, tuning=dict(mt=0, waves=hip.Variant.DENSE_PADDED_GROUPS, ksplit=ksplit))
    assert ('NG=4' if n_cols > 32 else 'NG=2') in kern4 and 'VALU' not in kern4, kern4
    assert np.all(np.abs(res4 - res) <= 2e-5 * scale + 1e-30)
    if dt.kind in 'iu':
        res5, kern5 = _apply(hip, data, masks, md, tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
        assert ',f16' in kern5 and 'VALU' not in kern5, kern5
        assert np.all(np.abs(res5 - ref) <= 2e-6 * scale + 1e-30)


@pytest.mark.parametrize('n_frames,n_px,n_masks,mask_dtype,ksplit', [
    (150, 64 * 40, 25, 'complex64', 0),     # C5's stack: 50 real columns -> 4 groups
    (150, 64 * 40, 25, 'complex64', 3),
    (300, 128 * 33, 20, 'float32', 0),      # 2 groups
    (77, 128 * 16, 32, 'float32', 2),
    (129, 64 * 21, 48, 'float32', 0),       # 3 groups, one frame past a workgroup
    (40, 64 * 64, 70, 'float32', 0),        # column blocks: 64 columns split, the last 6 on k_dense_lds
])
def test_float32_frames_on_bf16_matrix_cores(hip, n_frames, n_px, n_masks, mask_dtype, ksplit):
    """k_dense_split (csrc/ltmi_split.hip, opt-in: tuning code 36 / LTMI_SPLIT=1): float32 frames
    against >= 2 column groups as three bf16 pieces per factor, six exact-product matrix instructions
    -- float32 accuracy (checked tighter than the north-star 1e-5: 2e-6 of sum |a||b|), agreement with
    the f32-instruction kernel, accumulate and K-split paths, wide exponent range."""
    rng = np.random.default_rng(_seed(n_frames, n_px, n_masks, mask_dtype))
    md = np.dtype(mask_dtype)
    data = (rng.random((n_frames, n_px)) - 0.3).astype(np.float32)
    data[:, ::7] *= 1e-3
    data[:, 5::11] *= 300.0
    data[3 % n_frames] = 0.0
    masks = rng.random((n_masks, n_px)) - 0.25
    if md.kind == 'c':
        masks = masks + 1j * (rng.random((n_masks, n_px)) - 0.5)
    masks = masks.astype(md)
    masks[0, :n_px // 2] = 0
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    n_cols = n_masks * (2 if md.kind == 'c' else 1)
    tuning = dict(mt=0, waves=hip.Variant.DENSE_SPLIT_BF16, ksplit=ksplit)
    res, kern = _apply(hip, data, masks, md, tuning=tuning)
    if n_cols <= 64:
        assert 'k_dense_split' in kern and 'bf16x3' in kern, kern
    else:
        assert 'column blocks' in kern, kern        # 64 columns split, the last 6 on k_dense_lds
    assert np.all(np.abs(res - ref) <= 2e-6 * scale + 1e-30), np.max(np.abs(res - ref) / (scale + 1e-30))
    base = (rng.random((n_frames, n_masks)) + (1j * rng.random((n_frames, n_masks))
                                               if md.kind == 'c' else 0)).astype(md)
    res2, _ = _apply(hip, data, masks, md, accumulate_into=base, tuning=tuning)
    assert np.all(np.abs(res2 - (ref + base)) <= 2e-6 * (scale + 1))
    # the f32-instruction kernel (the default dispatch) agrees
    res3, kern3 = _apply(hip, data, masks, md, tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert 'k_dense_lds' in kern3, kern3
    assert np.all(np.abs(res3 - res) <= 1e-5 * scale + 1e-30)
    _, kern_default = _apply(hip, data, masks, md)
    assert 'k_dense_split' not in kern_default, kern_default
    # exponents far from 1: the pieces keep the float32 exponent range
    big = (data[:16] * np.float32(1e30)).astype(np.float32)
    small = (data[:16] * np.float32(1e-30)).astype(np.float32)
    for d in (big, small):
        r, k = _apply(hip, d, masks, md, tuning=tuning)
        rf = _ref64(d, masks)
        sc = np.abs(d.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
        assert np.all(np.isfinite(r)) and np.all(np.abs(r - rf) <= 2e-6 * sc + 1e-38)


@pytest.mark.parametrize('seed', [101, 202])
def test_randomised_differential(seed):
    """scripts/fuzz_kernels.py: random shapes / dtypes / leading dimensions / accumulate / K split /
    shifts / sparse stacks through every kernel family, against NumPy."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'fuzz_kernels.py'), '250',
                        str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ---- byte-order decode -----------------------------------------------------------------------------
@pytest.mark.parametrize('itemsize', [1, 2, 4, 8])
@pytest.mark.parametrize('n_items,offset', [(1, 0), (7, 0), (4096, 0), (100003, 0), (5000, 3)])
def test_byteswap_vs_oracle(hip, itemsize, n_items, offset):
    """ltmi_byteswap == byteswap_N_straight of the reference (oracle.decode), out of place and in
    place, aligned and unaligned buffers."""
    from oracle import decode as od
    rng = np.random.default_rng(itemsize * 1000 + n_items)
    raw = rng.integers(0, 256, n_items * itemsize + offset * itemsize, dtype=np.uint8)
    src = _dev(raw)
    dst = torch.zeros_like(src)
    o = offset * itemsize
    hip.byteswap(0, src.data_ptr() + o, dst.data_ptr() + o, itemsize, n_items)
    torch.cuda.synchronize()
    ref = od.byteswap_straight(raw[o:], itemsize) if itemsize > 1 else raw[o:]
    assert np.array_equal(dst.cpu().numpy()[o:], ref)
    assert np.all(dst.cpu().numpy()[:o] == 0)
    hip.byteswap(0, src.data_ptr() + o, src.data_ptr() + o, itemsize, n_items)     # in place
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy()[o:], ref)
    assert np.array_equal(src.cpu().numpy()[:o], raw[:o])


def test_byteswap_rejects_bad_arguments(hip):
    t = _dev(np.zeros(64, dtype=np.uint8))
    with pytest.raises((RuntimeError, ValueError)):
        hip.byteswap(0, t.data_ptr(), t.data_ptr(), 3, 4)
    with pytest.raises((RuntimeError, ValueError)):
        hip.byteswap(0, t.data_ptr(), t.data_ptr(), 2, -1)


# ---- centre-of-mass post-processing ---------------------------------------------------------------------
@pytest.mark.parametrize('ny,nx,rot,flip', [(7, 9, 0.0, False), (16, 5, 33.0, True), (2, 2, 90.0, False),
                                            (64, 64, -120.5, True), (3, 40, 0.0, True)])
def test_com_fields_vs_oracle(hip, ny, nx, rot, flip):
    """ltmi_com_fields == the NumPy chain center_shifts -> apply_correction -> magnitude /
    divergence / curl_2d of the reference (oracle.path restatement, pinned by com.npz)."""
    from libertem_amd.corrections import coordinates
    rng = np.random.default_rng(ny * 100 + nx)
    raw = rng.random((ny, nx, 3)).astype(np.float32) * np.array([50, 900, 1100], dtype=np.float32)
    raw[0, 0] = 0                                          # empty frame: zero shift
    if ny > 2:
        raw[ny // 2, nx // 2, 0] = 0
    cy, cx = 17.25, 21.5
    y_raw, x_raw = opath.center_shifts(raw[..., 0], raw[..., 1], raw[..., 2], cy, cx)
    y_ref, x_ref = opath.apply_correction(y_raw, x_raw, scan_rotation=rot, flip_y_=flip)
    transform = coordinates.flip_y() if flip else coordinates.identity()
    transform = coordinates.rotate_deg(rot) @ transform
    t = _dev(raw.reshape(-1, 3))
    out = torch.zeros((5, ny * nx), dtype=torch.float64, device='cuda')
    hip.com_fields(0, t.data_ptr(), 3, ny, nx, cy, cx, transform, *[out[i].data_ptr() for i in range(5)])
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape((5, ny, nx))
    tol = dict(rtol=1e-12, atol=1e-12)
    assert np.allclose(got[0], y_ref, **tol) and np.allclose(got[1], x_ref, **tol)
    assert np.allclose(got[2], opath.magnitude(y_ref, x_ref), **tol)
    assert np.allclose(got[3], opath.divergence(y_ref, x_ref), **tol)
    assert np.allclose(got[4], opath.curl_2d(y_ref, x_ref), **tol)
    assert got[0][0, 0] == 0 and got[1][0, 0] == 0


def test_rccl_comm_behind_the_c_abi(hip):
    """ltmi_comm_*: RCCL through the C ABI (what a reference-side binding gathers nav results /
    reduces sig results with).  One GPU here, so a one-rank communicator: all_gather is the
    identity into the receive buffer, all_reduce(sum) leaves the buffer unchanged; the error path
    (16-bit integers have no RCCL sum) raises."""
    uid = hip.Comm.unique_id()
    assert len(uid) == 128 and any(uid)
    comm = hip.Comm(0, 0, 1, uid)
    rng = np.random.default_rng(3)
    rows = rng.random((96, 16)).astype(np.float32)
    send = _dev(rows)
    recv = torch.zeros_like(send)
    comm.all_gather(send.data_ptr(), recv.data_ptr(), rows.nbytes)
    torch.cuda.synchronize()
    assert np.array_equal(recv.cpu().numpy(), rows)
    sig = rng.random((64, 64)).astype(np.float64)
    buf = _dev(sig)
    comm.all_reduce_sum(buf.data_ptr(), np.float64, sig.size)
    c64 = (rng.random(100) + 1j * rng.random(100)).astype(np.complex64)
    cbuf = _dev(c64.view(np.float32))
    comm.all_reduce_sum(cbuf.data_ptr(), np.complex64, c64.size)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), sig)
    assert np.array_equal(cbuf.cpu().numpy().view(np.complex64), c64)
    with pytest.raises(ValueError):
        comm.all_reduce_sum(buf.data_ptr(), np.uint16, 4)
    comm.close()


@pytest.mark.parametrize('tile_dtype,n_frames,tiles', [
    ('uint16', 9000, 4), ('uint8', 9000, 4), ('float32', 6000, 2),     # one round of 64 / 32-frame workgroups
    ('uint16', 24576, 2), ('float32', 9000, 1),                        # ... would be coarser than the small ones
])
def test_blocked_sparse_kernel_frames_per_workgroup(hip, monkeypatch, tile_dtype, n_frames, tiles):
    """k_bell_apply runs 2 or 4 (float32: 1 or 2) frame tiles per wave, whichever needs the shorter
    sequence of workgroup rounds; both instantiations against float64, ragged last workgroup included"""
    from oracle import masks as omasks
    monkeypatch.setenv('LTMI_SPARSE_SCATTER', '0')        # (float32 frames would take k_scatter)
    if os.environ.get('LTMI_SPARSE_BELL') == '0' or os.environ.get('LTMI_BELL_TILES'):
        pytest.skip("kernel choice forced by the environment")
    dt = np.dtype(tile_dtype)
    n_frames -= 7                                   # ragged
    rng = np.random.default_rng(n_frames)
    import scipy.sparse as sp
    rings = omasks.radial_bins(32, 32, 64, 64, n_bins=300, use_sparse=True, dtype=np.float32)
    csr = sp.csr_matrix(rings.T.astype(np.float32))              # (px, 300)
    data = (rng.integers(0, 200, (n_frames, 64 * 64)).astype(dt) if dt.kind == 'u'
            else rng.random((n_frames, 64 * 64)).astype(dt))
    res, kern = _apply_csr(hip, data, csr, np.float32)
    assert ('k_bell_apply<' in kern or 'k_bell_flat<' in kern) and (f'tiles={tiles}>' in kern or f'tiles={tiles},f16>' in kern), kern
    ref = data.astype(np.float64) @ csr.astype(np.float64).toarray()
    scale = np.abs(data.astype(np.float64)) @ np.abs(csr.astype(np.float64).toarray())
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)


@pytest.mark.parametrize('tile_dtype,mask_dtype,result_dtype', [
    ('uint16', 'float64', 'float64'), ('int32', 'float32', 'float64'), ('uint8', 'float64', 'float64'),
    ('uint16', 'complex128', 'complex128'), ('int16', 'int32', 'int32'), ('uint8', 'int64', 'int64'),
])
@pytest.mark.parametrize('spread', [0, 1, 2])
def test_shifted_masks_float64_and_integer_results(hip, tile_dtype, mask_dtype, result_dtype, spread):
    """Shifted masks whose result is float64 / complex128 / an exact integer: the f64 matrix-core kernel
    with the image of the SHIFTED stack -- a whole tile at once for one constant shift (spread 0), group
    by group on gathered frames for a few distinct shifts (spread 1: up to 9, spread 2: up to 25)."""
    rng = np.random.default_rng(_seed(tile_dtype, mask_dtype, spread))
    n, sig, n_masks = 200, (24, 32), 5
    dt, md, rd = np.dtype(tile_dtype), np.dtype(mask_dtype), np.dtype(result_dtype)
    data = rng.integers(0, 200 if dt.itemsize == 1 else 3000, (n,) + sig).astype(dt)
    if md.kind in 'iu':
        masks = rng.integers(-3, 9, (n_masks,) + sig).astype(md)
    else:
        masks = rng.random((n_masks,) + sig) - 0.25
        if md.kind == 'c':
            masks = masks + 1j * (rng.random((n_masks,) + sig) - 0.5)
        masks = masks.astype(md)
    shifts = (rng.integers(-spread, spread + 1, (n, 2)) if spread else
              np.tile(np.array([[3, -2]]), (n, 1))).astype(np.int32)
    h = hip.MaskHandle.dense(0, masks.reshape((n_masks, -1)), rd)
    t = _dev(np.ascontiguousarray(data.reshape((n, -1))))
    base = (rng.integers(0, 50, (n, n_masks)) if rd.kind in 'iu' else rng.random((n, n_masks))).astype(rd)
    ref, scale = _shift_ref(data, masks, shifts)
    for acc in (False, True):
        out = _dev(base.copy() if acc else np.full((n, n_masks), 7, dtype=rd))
        h.apply_shifted_host(t.data_ptr(), dt, n, data[0].size, sig[0], sig[1], shifts,
                             out.data_ptr(), n_masks, acc)
        torch.cuda.synchronize()
        res = out.cpu().numpy()
        if res.dtype != rd:
            res = res.view(rd)
        kern = h.last_kernel()
        assert 'k_dense_lds64' in kern and 'shifted, ' in kern, kern
        assert ('1 group' in kern) == (spread == 0), kern
        want = ref + base if acc else ref
        if rd.kind in 'iu':
            assert np.array_equal(res, np.real(want).astype(np.int64).astype(rd))
        else:
            assert np.all(np.abs(res - want) <= 1e-12 * (scale + 1)), np.abs(res - want).max()
    h.close()


def test_shifted_masks_float64_many_distinct_shifts(hip):
    """More than 256 distinct shifts in a tile with float64 results (a descan correction over +- 10 pixels: 441): the
    f64 matrix-core kernel group by group as long as a shift is shared by 8 frames on average (round 5: the
    per-frame kernel took every such tile); a tile of all-different shifts still goes to the per-frame kernel."""
    rng = np.random.default_rng(_seed('many shifts'))
    n, sig, n_masks = 4000, (24, 32), 3
    data = rng.integers(0, 3000, (n,) + sig).astype(np.uint16)
    masks = (rng.random((n_masks,) + sig) - 0.25)
    shifts = rng.integers(-10, 11, (n, 2)).astype(np.int32)
    n_distinct = len({(int(a), int(b)) for a, b in shifts})
    assert 400 < n_distinct <= 441
    h = hip.MaskHandle.dense(0, masks.reshape((n_masks, -1)), np.float64)
    t = _dev(np.ascontiguousarray(data.reshape((n, -1))))
    ref, scale = _shift_ref(data, masks, shifts)
    out = _dev(np.full((n, n_masks), 7, dtype=np.float64))
    h.apply_shifted_host(t.data_ptr(), np.uint16, n, data[0].size, sig[0], sig[1], shifts, out.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    kern = h.last_kernel()
    assert 'k_dense_lds64' in kern and f'shifted, {n_distinct} groups' in kern, kern
    assert np.all(np.abs(out.cpu().numpy() - ref) <= 1e-12 * (scale + 1))
    # 300 frames, every shift different: 3 launches per frame would lose to the per-frame kernel's single launch
    few = 300
    sh2 = np.stack([np.arange(few) % 23 - 11, np.arange(few) // 23 - 6], axis=1).astype(np.int32)
    ref2, scale2 = _shift_ref(data[:few], masks, sh2)
    out2 = _dev(np.full((few, n_masks), 7, dtype=np.float64))
    h.apply_shifted_host(t.data_ptr(), np.uint16, few, data[0].size, sig[0], sig[1], sh2, out2.data_ptr(), n_masks, False)
    torch.cuda.synchronize()
    assert 'groups' not in h.last_kernel(), h.last_kernel()
    assert np.all(np.abs(out2.cpu().numpy() - ref2) <= 1e-12 * (scale2 + 1))
    h.close()


@pytest.mark.parametrize('tile_dtype,n_frames', [('uint16', 700), ('float32', 300), ('uint8', 9000)])
def test_row_lists_for_the_blocked_sparse_kernel(hip, tile_dtype, n_frames):
    """ltmi_apply_masks_rows on a sparse handle: the blocked image's frame DMA reads frame rows[i] for
    result row i (both workgroup sizes, pixel counts with a tail), and so does the gather kernel's loader."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    if os.environ.get('LTMI_SPARSE_BELL') == '0':
        pytest.skip("blocked image switched off by the environment")
    dt = np.dtype(tile_dtype)
    rng = np.random.default_rng(n_frames)
    rings = omasks.radial_bins(31, 33, 67, 61, n_bins=90, use_sparse=True, dtype=np.float32)
    csr = sp.csr_matrix(rings.T.astype(np.float32))              # (61 * 67 px, 90): 4087 px, 7 in the tail
    n_px = csr.shape[0]
    data = (rng.integers(0, 200, (n_frames, n_px)).astype(dt) if dt.kind == 'u'
            else rng.random((n_frames, n_px)).astype(dt))
    rows = np.sort(rng.choice(n_frames, n_frames * 2 // 3, replace=False)).astype(np.int32)
    rows[3], rows[4] = rows[4], rows[3]
    h = hip.MaskHandle.csr(0, csr, np.float32)
    t = _dev(data)
    r = torch.from_numpy(rows).cuda()
    dense = csr.astype(np.float64).toarray()
    for acc in (False, True):
        out = torch.full((len(rows), 90), 2.0, dtype=torch.float32, device='cuda')
        handled = h.apply_rows(t.data_ptr(), dt, r.data_ptr(), len(rows), n_px, out.data_ptr(), 90, acc)
        torch.cuda.synchronize()
        assert handled and any(k in h.last_kernel() for k in ('k_bell_apply', 'k_bell_flat', 'k_scatter')) \
            and ',rows' in h.last_kernel(), h.last_kernel()
        ref = data[rows].astype(np.float64) @ dense + (2.0 if acc else 0.0)
        scale = np.abs(data[rows].astype(np.float64)) @ np.abs(dense) + 2.0
        assert np.all(np.abs(out.cpu().numpy() - ref) <= 1e-5 * scale), h.last_kernel()
    h.close()
    # a stack without a blocked image (random pattern: padding factor too high): the gather kernel takes
    # the row list as well; float64 results (int32 frames) through its double variant
    m = sp.random(n_px, 40, density=0.02, format='csr', dtype=np.float32, random_state=np.random.RandomState(3))
    for res_dt, frames in ((np.float32, data), (np.float64, data.astype(np.int32) if dt.kind == 'u' else None)):
        if frames is None:
            continue
        h = hip.MaskHandle.csr(0, m.astype(res_dt), res_dt)
        tt = _dev(frames)
        out = torch.zeros((len(rows), 40), dtype=torch.float32 if res_dt == np.float32 else torch.float64,
                          device='cuda')
        handled = h.apply_rows(tt.data_ptr(), frames.dtype, r.data_ptr(), len(rows), n_px, out.data_ptr(),
                               40, False)
        torch.cuda.synchronize()
        assert handled and ',rows' in h.last_kernel(), h.last_kernel()
        dm = m.astype(np.float64).toarray()
        ref = frames[rows].astype(np.float64) @ dm
        scale = np.abs(frames[rows].astype(np.float64)) @ np.abs(dm) + 1e-30
        tol = 1e-5 if res_dt == np.float32 else 1e-12
        assert np.all(np.abs(out.cpu().numpy() - ref) <= tol * scale), h.last_kernel()
        h.close()


# --- CrystallinityUDF in one kernel (csrc/ltmi_cryst.hip) ----------------
# (_cryst_reference, _cryst_run: tests/cryst_ref.py, shared with tests/test_fft_route_kernels_gpu.py)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32'])
@pytest.mark.parametrize('rad_in,rad_out,real', [(16, 64, ((128, 128), 25)), (0, 30, None),
                                                 (40, 70, ((100.5, 140), 31.5)), (10, 47.5, None),
                                                 (3.2, 64.7, ((128, 128), 25))])
def test_crystallinity_fused_kernel_all_pixel_types(hip, dtype, rad_in, rad_out, real):
    """256 x 256 frames go through k_cryst_fused: rows, columns and ring sum inside one workgroup;
    1e-5 relative against float64 (north_star tolerance for floating point)."""
    rng = np.random.default_rng(_seed('cryst', dtype, rad_out))
    dt = np.dtype(dtype)
    n = 11
    if dt.kind == 'f':
        frames = rng.normal(size=(n, 256, 256)).astype(dt) * 100
    else:
        info = np.iinfo(dt)
        frames = rng.integers(max(info.min, -4000), min(info.max, 4000), size=(n, 256, 256),
                              endpoint=True).astype(dt)
    frames[3] = 0                                              # an empty frame
    frames[4, 100:110, 50:60] += 17                            # structure on top of the noise
    ref, real_mask, half = _cryst_reference(frames, rad_in, rad_out, real)
    got, label = _cryst_run(hip, frames, real_mask, half)
    assert label.startswith('k_cryst_fused<'), label
    assert (',mask' in label) == (real is not None)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), (got, ref)
    assert got[3] == 0


@pytest.mark.gpu
def test_crystallinity_fused_kernel_many_frames_ragged_accumulate(hip):
    """more frames than workgroups, a padded frame stride, accumulate; rings too wide for the LDS."""
    rng = np.random.default_rng(_seed('cryst-many'))
    frames = rng.integers(0, 4096, size=(300, 256, 256)).astype(np.uint16)
    ref, real_mask, half = _cryst_reference(frames, 16, 64, ((128, 128), 25))
    got, label = _cryst_run(hip, frames, real_mask, half, ld_pad=8)
    assert label == 'k_cryst_fused<uint16,mask> columns=65', label
    assert np.allclose(got, ref, rtol=1e-5)
    base = rng.normal(size=300).astype(np.float32) * 1e6
    got2, _ = _cryst_run(hip, frames, real_mask, half, accumulate_into=base)
    assert np.allclose(got2, base + got, rtol=1e-6)
    # an odd frame stride (rows not 8-byte aligned): the conversion pass makes float32 frames of them first
    got3, label3 = _cryst_run(hip, frames[:9], real_mask, half, ld_pad=1)
    assert label3 == 'k_fft_prepare<uint16> + k_cryst_fused<float32> columns=65', label3
    assert np.allclose(got3, ref[:9], rtol=1e-5)
    # a ring too wide for the LDS (rad_out 100 -> 101 columns): the row / column kernels with a workspace
    ref_w, rm_w, half_w = _cryst_reference(frames[:40], 16, 100, ((128, 128), 25))
    got_w, label_w = _cryst_run(hip, frames[:40], rm_w, half_w, batch=16)
    assert label_w == 'k_cryst_rows256<uint16,mask> + k_cryst_cols256 columns=101', label_w
    assert np.allclose(got_w, ref_w, rtol=1e-5)
    for dt, rad in ((np.float32, 200), (np.uint8, 128), (np.int16, 71)):          # up to the whole half spectrum (129 columns)
        fr = (frames[:5] % 200).astype(dt)
        ref_w, rm_w, half_w = _cryst_reference(fr, 30, rad, None)
        got_w, label_w = _cryst_run(hip, fr, rm_w, half_w)
        assert label_w.startswith('k_cryst_rows256<') and label_w.endswith(f'columns={min(rad, 128) + 1}'), label_w
        assert np.allclose(got_w, ref_w, rtol=1e-5)


@pytest.mark.gpu
def test_crystallinity_fused_kernel_every_bin_of_the_ring(hip):
    """frames that are single plane waves exp(2 pi i (ky y + kx x) / 256) (real part): |F| is 256^2 / 2 in
    exactly the bins (ky, kx) and (-ky, -kx) -- each probes whether ONE bin is inside the sum."""
    yy, xx = np.mgrid[0:256, 0:256]
    waves = [(0, 0), (0, 64), (0, 65), (64, 0), (192, 0), (45, 45), (46, 46), (255, 1), (16, 0), (15, 0),
             (200, 30), (128, 128), (3, 63)]
    frames = np.stack([np.cos(2 * np.pi * (ky * yy + kx * xx) / 256) for ky, kx in waves]).astype(np.float32)
    ref, _, half = _cryst_reference(frames, 16, 64, None)
    got, label = _cryst_run(hip, frames, None, half)
    assert label.startswith('k_cryst_fused<'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=256 * 256 * 1e-4), (got, ref)   # float32 round-off of 10^4 empty bins
    inside = ref > 1000
    assert inside.sum() >= 5 and (~inside).sum() >= 4          # the probe set straddles the ring's edges


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['uint8', 'int8', 'uint16', 'int16', 'uint32', 'int32', 'float32'])
@pytest.mark.parametrize('rad_in,rad_out,real', [(8, 64, ((64, 64), 12)), (0, 30, None), (10, 47.5, ((50.5, 70), 9.5)),
                                                 (60, 90, None), (0, 7, ((64, 64), 70))])
def test_crystallinity_fused_kernel_128_all_pixel_types(hip, dtype, rad_in, rad_out, real):
    """128 x 128 frames: k_cryst_fused128 -- four rows / two columns per 256-point transform of an interleaved
    sequence; rings up to the full half spectrum (65 columns), 1e-5 relative against float64."""
    rng = np.random.default_rng(_seed('cryst128', dtype, rad_out))
    dt = np.dtype(dtype)
    n = 9
    if dt.kind == 'f':
        frames = rng.normal(size=(n, 128, 128)).astype(dt) * 100
    else:
        info = np.iinfo(dt)
        frames = rng.integers(max(info.min, -4000), min(info.max, 4000), size=(n, 128, 128),
                              endpoint=True).astype(dt)
    frames[2] = 0
    frames[5, 40:50, 90:100] += 17
    ref, real_mask, half = _cryst_reference(frames, rad_in, rad_out, real)
    got, label = _cryst_run(hip, frames, real_mask, half)
    assert label.startswith('k_cryst_fused128<'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), (got, ref)
    assert got[2] == 0


@pytest.mark.gpu
def test_crystallinity_fused_kernel_128_many_frames_and_every_bin(hip):
    rng = np.random.default_rng(_seed('cryst128-many'))
    frames = rng.integers(0, 4096, size=(700, 128, 128)).astype(np.uint16)
    ref, real_mask, half = _cryst_reference(frames, 8, 32, ((64, 64), 12))
    got, label = _cryst_run(hip, frames, real_mask, half, ld_pad=6)
    assert label == 'k_cryst_fused128<uint16,mask> columns=33', label
    assert np.allclose(got, ref, rtol=1e-5)
    base = rng.normal(size=700).astype(np.float32) * 1e6
    got2, _ = _cryst_run(hip, frames, real_mask, half, accumulate_into=base)
    assert np.allclose(got2, base + got, rtol=1e-6)
    got3, label3 = _cryst_run(hip, frames[:9], real_mask, half, ld_pad=1)      # odd stride: converted first
    assert label3 == 'k_fft_prepare<uint16> + k_cryst_fused128<float32> columns=33', label3
    assert np.allclose(got3, ref[:9], rtol=1e-5)
    # single plane waves: one bin each, inside / outside the ring 8 .. 32
    yy, xx = np.mgrid[0:128, 0:128]
    waves = [(0, 0), (0, 32), (0, 33), (32, 0), (96, 0), (95, 0), (22, 22), (24, 24), (127, 8), (8, 0), (7, 0),
             (100, 20), (64, 64), (3, 31)]
    pw = np.stack([np.cos(2 * np.pi * (ky * yy + kx * xx) / 128) for ky, kx in waves]).astype(np.float32)
    ref, _, half = _cryst_reference(pw, 8, 32, None)
    got, label = _cryst_run(hip, pw, None, half)
    assert label.startswith('k_cryst_fused128<'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=128 * 128 * 1e-4), (got, ref)
    inside = ref > 1000
    assert inside.sum() >= 5 and (~inside).sum() >= 4


@pytest.mark.gpu
@pytest.mark.parametrize('sig', [128, 256, 512])
def test_crystallinity_corrected_and_float64_frames_take_the_fused_kernel(hip, sig):
    """ltmi_crystallinity_corrected on raw frames (dark / gain / dead-pixel patches): the corrections run inside the
    row stage of the fused kernels (round 5; LTMI_CRYST_CORR_PASS=1: the conversion pass writes corrected float32
    frames first); float64 frames still take the conversion pass -- against the oracle's corrections + float64
    rfft2, more frames than one batch / one round of workgroups."""
    from libertem_amd.io.corrections import CorrectionSet
    from libertem_amd.udf.crystallinity import mask_box
    from oracle import corrections as oc
    rng = np.random.default_rng(_seed('cryst-corr', sig))
    n = 21
    data = rng.integers(0, 3000, (n, sig, sig)).astype(np.uint16)
    dark = rng.random((sig, sig)) * 6
    gain = rng.random((sig, sig)) * 0.6 + 0.7
    bad = np.zeros((sig, sig), dtype=bool)
    bad[sig // 2, sig // 2] = bad[0, 0] = bad[10, 40] = bad[10, 41] = bad[sig - 1, sig - 1] = True
    bad[rng.integers(0, sig, 40), rng.integers(0, sig, 40)] = True
    coords = [tuple(c) for c in np.argwhere(bad)]
    real = ((sig // 2, sig // 2), sig // 10)
    for kw in (dict(dark=dark, gain=gain, excluded_pixels=bad), dict(gain=gain), dict(excluded_pixels=bad)):
        corrected = oc.correct(data, (sig, sig), dark=kw.get('dark'), gain=kw.get('gain'),
                               coords=coords if 'excluded_pixels' in kw else None)
        ref, real_mask, half = _cryst_reference(corrected.reshape(n, sig, sig), sig // 16, sig // 4, real)
        tables = CorrectionSet(**kw).device_tables(0, (sig, sig))
        plan = hip.FFTPlan(0, sig, sig, 8)                       # 8 frames per batch: 3 batches
        t = _dev(data.reshape(n, -1))
        rm = torch.from_numpy(np.ascontiguousarray(real_mask.astype(np.float32))).cuda()
        hm = torch.from_numpy(np.ascontiguousarray(half.astype(np.float32))).cuda()
        out = torch.full((n,), 7.0, dtype=torch.float32, device='cuda')
        plan.crystallinity_corrected(t.data_ptr(), data.dtype, n, sig * sig, tables, rm.data_ptr(), hm.data_ptr(),
                                     mask_box(half), out.data_ptr(), False)
        torch.cuda.synchronize()
        # round 5: the corrections run inside the row stage of the fused kernels -- one pass over the raw pixels
        want = {128: 'k_cryst_fused128<uint16,corrected', 256: 'k_cryst_fused<uint16,corrected',
                512: 'k_cryst_rows512<uint16,corrected'}[sig]
        assert plan.last_kernel().startswith(want), plan.last_kernel()
        assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5), sorted(kw)
        if True:
            # ... and agrees with the conversion pass + the same kernel on corrected float32 frames
            os.environ['LTMI_CRYST_CORR_PASS'] = '1'
            try:
                out2 = torch.full((n,), 7.0, dtype=torch.float32, device='cuda')
                plan.crystallinity_corrected(t.data_ptr(), data.dtype, n, sig * sig, tables, rm.data_ptr(),
                                             hm.data_ptr(), mask_box(half), out2.data_ptr(), False)
                torch.cuda.synchronize()
                assert plan.last_kernel().startswith('k_fft_prepare<uint16> + k_cryst_'), plan.last_kernel()
                assert np.allclose(out2.cpu().numpy(), out.cpu().numpy(), rtol=2e-6)
            finally:
                del os.environ['LTMI_CRYST_CORR_PASS']
            # accumulate, ragged frame count beyond one workgroup round, other pixel types
            out3 = out.clone()
            plan.crystallinity_corrected(t.data_ptr(), data.dtype, n, sig * sig, tables, rm.data_ptr(), hm.data_ptr(),
                                         mask_box(half), out3.data_ptr(), True)
            torch.cuda.synchronize()
            assert np.allclose(out3.cpu().numpy(), 2 * ref, rtol=1e-5)
        plan.close()
    if sig in (128, 256, 512):
        # many frames (more than one round of workgroups), float32 / uint8 pixels, no real-space mask, many dead pixels
        n2 = {128: 1500, 256: 700, 512: 150}[sig]
        for dt, hi in ((np.float32, None), (np.uint8, 200)):
            d2 = (rng.random((n2, sig, sig)) * 100).astype(dt) if hi is None else \
                rng.integers(0, hi, (n2, sig, sig)).astype(dt)
            bad2 = rng.random((sig, sig)) < 0.01                       # ~650 dead pixels, clusters included
            coords2 = [tuple(c) for c in np.argwhere(bad2)]
            corrected = oc.correct(d2, (sig, sig), dark=dark, gain=gain, coords=coords2)
            ref2, _, half2 = _cryst_reference(corrected.reshape(n2, sig, sig), sig // 16, sig // 4, None)
            tables = CorrectionSet(dark=dark, gain=gain, excluded_pixels=bad2).device_tables(0, (sig, sig))
            plan = hip.FFTPlan(0, sig, sig, 8)
            t = _dev(d2.reshape(n2, -1))
            hm = torch.from_numpy(np.ascontiguousarray(half2.astype(np.float32))).cuda()
            out = torch.full((n2,), 7.0, dtype=torch.float32, device='cuda')
            plan.crystallinity_corrected(t.data_ptr(), d2.dtype, n2, sig * sig, tables, None, hm.data_ptr(),
                                         mask_box(half2), out.data_ptr(), False)
            torch.cuda.synchronize()
            assert plan.last_kernel().startswith('k_cryst_') and 'corrected' in plan.last_kernel(), plan.last_kernel()
            assert np.allclose(out.cpu().numpy(), ref2, rtol=1e-5), dt
            plan.close()
    frames = rng.normal(size=(n, sig, sig)) * 50
    ref, real_mask, half = _cryst_reference(frames, sig // 16, sig // 4, real)
    got, label = _cryst_run(hip, frames, real_mask, half, batch=8)
    assert label.startswith('k_fft_prepare<float64> + k_cryst_'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'int16', 'int32', 'float32'])
@pytest.mark.parametrize('rad_in,rad_out,real', [(32, 128, ((256, 256), 50)), (0, 40, None),
                                                 (100, 300, ((200.5, 280), 61.5)), (10, 63.5, None)])
def test_crystallinity_512_rows_and_columns_kernels(hip, dtype, rad_in, rad_out, real):
    """512 x 512 frames: k_cryst_rows512 (the ring's columns of the row transforms into a workspace) +
    k_cryst_cols512 (one column per wave); rings up to the full half spectrum (257 columns), more frames than the
    workspace holds at once (batch 4)."""
    rng = np.random.default_rng(_seed('cryst512', dtype, rad_out))
    dt = np.dtype(dtype)
    n = 7
    if dt.kind == 'f':
        frames = rng.normal(size=(n, 512, 512)).astype(dt) * 100
    else:
        info = np.iinfo(dt)
        frames = rng.integers(max(info.min, -4000), min(info.max, 4000), size=(n, 512, 512),
                              endpoint=True).astype(dt)
    frames[2] = 0
    frames[5, 140:150, 390:400] += 17
    ref, real_mask, half = _cryst_reference(frames, rad_in, rad_out, real)
    got, label = _cryst_run(hip, frames, real_mask, half, batch=4)
    assert label.startswith('k_cryst_rows512<'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), (got, ref)
    assert got[2] == 0


@pytest.mark.gpu
def test_crystallinity_512_accumulate_strides_and_every_bin(hip):
    rng = np.random.default_rng(_seed('cryst512-many'))
    frames = rng.integers(0, 4096, size=(40, 512, 512)).astype(np.uint16)
    ref, real_mask, half = _cryst_reference(frames, 32, 128, ((256, 256), 50))
    got, label = _cryst_run(hip, frames, real_mask, half, ld_pad=8, batch=16)
    assert label == 'k_cryst_rows512<uint16,mask> + k_cryst_cols512 columns=129', label
    assert np.allclose(got, ref, rtol=1e-5)
    base = rng.normal(size=40).astype(np.float32) * 1e6
    got2, _ = _cryst_run(hip, frames, real_mask, half, accumulate_into=base, batch=16)
    assert np.allclose(got2, base + got, rtol=1e-6)
    got3, label3 = _cryst_run(hip, frames[:5], real_mask, half, ld_pad=1, batch=4)      # odd stride: converted first
    assert label3 == 'k_fft_prepare<uint16> + k_cryst_rows512<float32> + k_cryst_cols512 columns=129', label3
    assert np.allclose(got3, ref[:5], rtol=1e-5)
    yy, xx = np.mgrid[0:512, 0:512]
    waves = [(0, 0), (0, 128), (0, 129), (128, 0), (384, 0), (383, 0), (90, 90), (92, 92), (511, 32), (32, 0), (31, 0),
             (400, 80), (256, 256), (3, 127), (0, 256), (256, 0)]
    pw = np.stack([np.cos(2 * np.pi * (ky * yy + kx * xx) / 512) for ky, kx in waves]).astype(np.float32)
    ref, _, half = _cryst_reference(pw, 32, 128, None)
    got, label = _cryst_run(hip, pw, None, half)
    assert label.startswith('k_cryst_rows512<'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=512 * 512 * 1e-4), (got, ref)
    inside = ref > 10000
    assert inside.sum() >= 5 and (~inside).sum() >= 5
    ref, _, half = _cryst_reference(pw, 100, 400, None)          # all 257 columns: the bins (0, 256), (256, 256) count
    got, label = _cryst_run(hip, pw, None, half)
    assert label.endswith('columns=257'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=512 * 512 * 1e-4), (got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['uint16', 'float32', 'uint8'])
@pytest.mark.parametrize('rad_in,rad_out,real', [(64, 256, ((512, 512), 100)), (0, 40, None), (200, 700, None)])
def test_crystallinity_1024_rows_and_columns_kernels(hip, dtype, rad_in, rad_out, real):
    """1024 x 1024 frames: the same two kernels with four 256-point transforms + a radix-4 butterfly per 1024
    points; rings up to the full half spectrum (513 columns), two passes of the workspace (batch 3)."""
    rng = np.random.default_rng(_seed('cryst1024', dtype, rad_out))
    dt = np.dtype(dtype)
    n = 5
    if dt.kind == 'f':
        frames = rng.normal(size=(n, 1024, 1024)).astype(dt) * 100
    else:
        frames = rng.integers(0, min(np.iinfo(dt).max, 4000), size=(n, 1024, 1024), endpoint=True).astype(dt)
    frames[2] = 0
    frames[4, 140:150, 890:900] += 17
    ref, real_mask, half = _cryst_reference(frames, rad_in, rad_out, real)
    got, label = _cryst_run(hip, frames, real_mask, half, batch=3)
    assert label.startswith('k_cryst_rows1024<') and 'k_cryst_cols1024' in label, label
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), (got, ref)
    assert got[2] == 0


@pytest.mark.gpu
def test_crystallinity_1024_every_bin_and_converted_frames(hip):
    yy, xx = np.mgrid[0:1024, 0:1024]
    waves = [(0, 0), (0, 256), (0, 257), (256, 0), (768, 0), (767, 0), (181, 181), (182, 182), (1023, 64), (64, 0),
             (63, 0), (800, 160), (512, 512), (3, 255), (0, 512), (512, 0), (300, 511)]
    pw = np.stack([np.cos(2 * np.pi * (ky * yy + kx * xx) / 1024) for ky, kx in waves]).astype(np.float32)
    for rad_in, rad_out in ((64, 256), (200, 800)):
        ref, _, half = _cryst_reference(pw, rad_in, rad_out, None)
        got, label = _cryst_run(hip, pw, None, half)
        assert label.startswith('k_cryst_rows1024<'), label
        assert np.allclose(got, ref, rtol=1e-5, atol=1024 * 1024 * 1e-4), (got, ref)
        assert (ref > 50000).sum() >= 5 and (ref < 50000).sum() >= 4
    rng = np.random.default_rng(_seed('cryst1024-f64'))
    frames = rng.normal(size=(4, 1024, 1024)) * 50
    ref, real_mask, half = _cryst_reference(frames, 64, 256, ((512, 512), 100))
    got, label = _cryst_run(hip, frames, real_mask, half, batch=3)
    assert label.startswith('k_fft_prepare<float64> + k_cryst_rows1024<float32>'), label
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('sig', [(256, 512), (512, 256), (1024, 256), (256, 1024), (512, 1024), (1024, 512)])
def test_crystallinity_rectangular_frames(hip, dtype, sig):
    """frames whose edges are 256 / 512 / 1024 pixels in any combination: rows of 256 M points, columns of 256 MH
    points, the ring's columns through the workspace (k_cryst_rows<w> + k_cryst_cols<h>)."""
    rng = np.random.default_rng(_seed('cryst-rect', dtype, sig))
    dt = np.dtype(dtype)
    n = 5
    h, w = sig
    frames = (rng.normal(size=(n, h, w)) * 100).astype(dt) if dt.kind == 'f' else \
        rng.integers(0, 4000, size=(n, h, w)).astype(dt)
    frames[1] = 0
    for rad_in, rad_out, real in ((min(sig) // 16, min(sig) // 4, ((h / 2, w / 2), min(sig) // 10)), (0, 2000, None)):
        ref, real_mask, half = _cryst_reference(frames, rad_in, rad_out, real)
        got, label = _cryst_run(hip, frames, real_mask, half, batch=3)
        assert label.startswith(f'k_cryst_rows{w}<') and f'k_cryst_cols{h} ' in label, label
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max()), (sig, rad_out, got, ref)
        assert got[1] == 0


# ---- dense stacks folded about a mirror of the detector rows (csrc/ltmi_fold.hip) ------------------------------
def _radial_stack(sig, n_bins, max_order, cy=None, cx=None):
    """the reference's radial-Fourier stack (analysis/radialfourier.py:106-146, pinned bit for bit by
    tests/golden), flattened: (n_bins * (max_order + 1), sig_h * sig_w) complex64"""
    from libertem_amd import masks as pm
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    h, w = sig
    cy = h / 2 if cy is None else cy
    cx = w / 2 if cx is None else cx
    ro = pm.bounding_radius(cx, cy, w, h)
    st = radial_mask_factory(h, w, cx, cy, 0, ro, n_bins, max_order, False)()
    return np.ascontiguousarray(st.reshape(st.shape[0], -1))


def _fold_apply(hip, data, masks, sig, result_dtype, tuning=None, accumulate_into=None, rows=None):
    h = hip.MaskHandle.dense(0, masks, result_dtype)
    h.set_sig_shape(*sig)
    if tuning:
        h.set_tuning(**tuning)
    t = _dev(np.ascontiguousarray(data))
    n_frames, n_px = data.shape
    rd = np.dtype(result_dtype)
    n_out = n_frames if rows is None else len(rows)
    if accumulate_into is None:
        out_np, acc = np.full((n_out, masks.shape[0]), 7, dtype=rd), False
    else:
        out_np, acc = accumulate_into.astype(rd).copy(), True
    out = _dev(out_np.view(np.float32).reshape(n_out, -1) if rd.kind == 'c' else out_np)
    if rows is None:
        h.apply(t.data_ptr(), data.dtype, n_frames, n_px, out.data_ptr(), masks.shape[0], acc)
    else:
        r = torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda()
        assert h.apply_rows(t.data_ptr(), data.dtype, r.data_ptr(), len(rows), n_px, out.data_ptr(),
                            masks.shape[0], acc)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    if rd.kind == 'c':
        res = np.ascontiguousarray(res).view(np.complex64).reshape(n_out, -1)
    kern = h.last_kernel()
    h.close()
    return res, kern


@pytest.mark.parametrize('sig,n_bins,max_order,n_frames,ksplit', [
    ((128, 128), 1, 24, 300, 0),        # C5's default stack (25 complex masks: 2 even + 2 odd groups), ragged frame count
    ((128, 128), 1, 24, 300, 5),        # ... pixel axis split 5 ways
    ((64, 256), 2, 7, 130, 0),          # 16 complex masks: 1 + 1 groups, rectangular frames
    ((96, 64), 1, 9, 64, 3),            # 10 complex masks = 20 real columns
    ((64, 128), 3, 6, 40, 0),           # 21 complex masks: 2 + 2 groups
])
def test_row_mirror_fold_radial_fourier(hip, sig, n_bins, max_order, n_frames, ksplit):
    """k_dense_fold: float32 frames x a radial-Fourier stack (real parts even, imaginary parts odd under the mirror of
    the detector rows about the centre): same results as the unfolded kernel (tuning 38) and the float64 product
    within 1e-5 of sum |x||w| per entry; accumulate; the pixel axis split over workgroups."""
    masks = _radial_stack(sig, n_bins, max_order)
    rng = np.random.default_rng(_seed('fold', sig, n_bins, max_order))
    data = (rng.random((n_frames, sig[0] * sig[1])) - 0.2).astype(np.float32)
    res, kern = _fold_apply(hip, data, masks, sig, np.complex64, tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert 'k_dense_fold' in kern, kern
    res_u, kern_u = _fold_apply(hip, data, masks, sig, np.complex64, tuning=dict(mt=0, waves=hip.Variant.DENSE_UNFOLDED, ksplit=0))
    assert 'k_dense_fold' not in kern_u, kern_u
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(res) - part(ref)) <= 1e-5 * scale + 1e-30)
        assert np.all(np.abs(part(res) - part(res_u)) <= 2e-5 * scale + 1e-30)
    base = (rng.random((n_frames, masks.shape[0])) + 1j * rng.random((n_frames, masks.shape[0]))).astype(np.complex64)
    res2, kern2 = _fold_apply(hip, data, masks, sig, np.complex64, accumulate_into=base,
                              tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert 'k_dense_fold' in kern2
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 2))


@pytest.mark.parametrize('sig,centre', [
    ((128, 128), None),                 # centre (64, 64): rows y and 128 - y, row 0 and row 64 unpaired
    ((128, 64), (63.5, 32.0)),          # centre between two rows: rows y and 127 - y, every row paired
    ((64, 128), (32.5, 70.0)),          # rows y and 65 - y: rows 0 and 1 have their partner beyond the frame
])
def test_row_mirror_fold_every_pixel_elementwise(hip, sig, centre):
    """One-pixel frames over EVERY pixel of the detector: the folded kernel multiplies the stack's ORIGINAL weights
    (nothing is averaged), so pixel * weight comes back within 1e-5 RELATIVE of every single stored entry, atol 0 --
    including the mirrored half (the partner rows), the unpaired rows and the rows whose imaginary parts are
    sin(o pi) = tiny but not zero."""
    cy, cx = (None, None) if centre is None else centre
    masks = _radial_stack(sig, 1, 24, cy=cy, cx=cx)
    n_px = sig[0] * sig[1]
    rng = np.random.default_rng(_seed('fold-one', sig, centre))
    vals = (rng.random(n_px) + 0.5).astype(np.float32)
    data = np.zeros((n_px, n_px), dtype=np.float32)
    data[np.arange(n_px), np.arange(n_px)] = vals
    res, kern = _fold_apply(hip, data, masks, sig, np.complex64)
    assert 'k_dense_fold' in kern, kern
    want = masks.T.astype(np.complex128) * vals[:, None].astype(np.float64)
    for part in (np.real, np.imag):
        g, w = part(res).astype(np.float64), part(want)
        assert np.all(np.abs(g - w) <= 1e-5 * np.abs(w)), np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))


def test_row_mirror_fold_even_stack_and_rows(hip):
    """A stack of even columns only (anti-aliased rings, 40 masks: 3 even groups) and a region of interest through a
    row list (ltmi_apply_masks_rows)."""
    from libertem_amd import masks as pm
    sig = (128, 64)
    rings = pm.radial_bins(32, 64, 64, 128, n_bins=40, use_sparse=False, dtype=np.float32)
    masks = np.ascontiguousarray(np.asarray(rings).reshape(40, -1))
    rng = np.random.default_rng(_seed('fold-even'))
    data = rng.random((200, sig[0] * sig[1])).astype(np.float32)
    res, kern = _fold_apply(hip, data, masks, sig, np.float32)
    assert 'k_dense_fold<f,even=3,odd=0' in kern, kern
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks.astype(np.float64)).T
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)
    rows = rng.permutation(200)[:77]
    res_r, kern_r = _fold_apply(hip, data, masks, sig, np.float32, rows=rows)
    assert 'k_dense_fold' in kern_r and ',rows' in kern_r, kern_r
    assert np.all(np.abs(res_r - ref[rows]) <= 1e-5 * scale[rows] + 1e-30)


def test_row_mirror_fold_leaves_other_stacks_alone(hip):
    """No mirror under which every column is even or odd (random masks; a radial stack with ONE weight changed), a
    stack of one group (nothing to save), a frame width the kernel does not take: the handle works as before."""
    sig = (64, 128)
    rng = np.random.default_rng(_seed('fold-none'))
    data = rng.random((70, sig[0] * sig[1])).astype(np.float32)
    masks = (rng.random((20, sig[0] * sig[1])) - 0.3).astype(np.float32)
    res, kern = _fold_apply(hip, data, masks, sig, np.float32)
    assert 'k_dense_fold' not in kern, kern
    assert np.allclose(res, _ref64(data, masks), rtol=1e-5, atol=1e-3)
    stack = _radial_stack(sig, 1, 24)
    stack[7, 5 * 128 + 9] *= np.float32(1.0000002)
    res, kern = _fold_apply(hip, data, stack, sig, np.complex64)
    assert 'k_dense_fold' not in kern, kern
    assert np.allclose(res, _ref64(data, stack), rtol=1e-5, atol=1e-3)
    few = _radial_stack(sig, 1, 3)                       # 4 complex masks = 8 columns: one group
    res, kern = _fold_apply(hip, data, few, sig, np.complex64)
    assert 'k_dense_fold' not in kern, kern
    odd_w = _radial_stack((64, 96), 1, 24)               # 96 pixels per row: not a multiple of the 64-pixel stage
    d2 = rng.random((40, 64 * 96)).astype(np.float32)
    res, kern = _fold_apply(hip, d2, odd_w, (64, 96), np.complex64)
    assert 'k_dense_fold' not in kern, kern
    assert np.allclose(res, _ref64(d2, odd_w), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize('sig,n_bins,max_order,n_frames,ksplit', [
    ((128, 128), 1, 24, 300, 0), ((64, 256), 1, 24, 130, 3), ((128, 128), 1, 24, 70, 5)])   # 2 + 2 column groups
def test_row_mirror_fold_two_waves_per_simd(hip, monkeypatch, sig, n_bins, max_order, n_frames, ksplit):
    """k_dense_fold8 (LTMI_FOLD_WAVES=8, a measurement switch: two waves per SIMD, one frame tile each) gives the sums
    of the shipped k_dense_fold: against float64 with the element-wise bound, ragged frame counts, a pixel split, `+=`."""
    monkeypatch.setenv('LTMI_FOLD_WAVES', '8')
    masks = _radial_stack(sig, n_bins, max_order)
    rng = np.random.default_rng(_seed('fold8', sig, n_frames))
    data = (rng.random((n_frames, sig[0] * sig[1])) - 0.2).astype(np.float32)
    tuning = dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit) if ksplit else None
    res, kern = _fold_apply(hip, data, masks, sig, np.complex64, tuning=tuning)
    assert 'k_dense_fold8<f' in kern, kern
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(res) - part(ref)) <= 1e-5 * scale + 1e-30)
    monkeypatch.setenv('LTMI_FOLD_WAVES', '4')
    res4, kern4 = _fold_apply(hip, data, masks, sig, np.complex64, tuning=tuning)
    assert 'k_dense_fold<f' in kern4, kern4
    assert np.all(np.abs(res - res4) <= 2e-6 * scale + 1e-30)


def test_row_mirror_fold_wide_stack_in_column_blocks(hip):
    """More than 64 real columns: the stack is kept as blocks of <= 64 columns (ltmi_apply_masks walks them) and every
    block is folded on its own -- 3 bins x 25 orders = 75 complex masks = 64 + 64 + 22 real columns."""
    sig = (64, 128)
    masks = _radial_stack(sig, 3, 24)
    assert masks.shape[0] == 75
    rng = np.random.default_rng(_seed('fold-wide'))
    data = (rng.random((150, sig[0] * sig[1])) - 0.1).astype(np.float32)
    res, kern = _fold_apply(hip, data, masks, sig, np.complex64)
    assert kern.startswith('3 column blocks') and 'k_dense_fold<f,even=1,odd=1' in kern, kern
    res_u, kern_u = _fold_apply(hip, data, masks, sig, np.complex64, tuning=dict(mt=0, waves=hip.Variant.DENSE_UNFOLDED, ksplit=0))
    assert 'k_dense_fold' not in kern_u, kern_u
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(res) - part(ref)) <= 1e-5 * scale + 1e-30)
        assert np.all(np.abs(part(res_u) - part(ref)) <= 1e-5 * scale + 1e-30)


@pytest.mark.parametrize('tile_dtype', ['uint16', 'int16', 'uint8', 'int8'])
@pytest.mark.parametrize('sig,n_bins,max_order,n_frames,ksplit', [
    ((128, 128), 1, 24, 300, 0),        # 25 complex masks: 2 even + 2 odd groups, one 128-pixel stage per row
    ((64, 256), 1, 24, 130, 3),         # two stages per row, pixel axis split
    ((96, 128), 2, 7, 70, 0),           # 16 complex masks: 1 + 1 groups
])
def test_row_mirror_fold_two_byte_pixels(hip, tile_dtype, sig, n_bins, max_order, n_frames, ksplit):
    """k_dense_fold16: 1- and 2-byte integer frames of a radial-Fourier stack (which keeps the float32 matrix instruction:
    its zero crossings hold more small weights than the float16 pieces' tail takes) through the row-mirror fold -- against
    float64, the unfolded kernel (tuning 38) and, one-pixel frames over every pixel, every stored weight."""
    masks = _radial_stack(sig, n_bins, max_order)
    rng = np.random.default_rng(_seed('fold16', tile_dtype, sig, n_bins))
    dt = np.dtype(tile_dtype)
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    data = rng.integers(lo, hi, (n_frames, sig[0] * sig[1]), endpoint=True).astype(dt)
    data[1] = hi
    data[2] = lo
    res, kern = _fold_apply(hip, data, masks, sig, np.complex64, tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert 'k_dense_fold16' in kern, kern
    res_u, kern_u = _fold_apply(hip, data, masks, sig, np.complex64, tuning=dict(mt=0, waves=hip.Variant.DENSE_UNFOLDED, ksplit=0))
    assert 'k_dense_fold' not in kern_u, kern_u
    ref = _ref64(data, masks)
    scale = np.abs(data.astype(np.float64)) @ np.abs(masks).astype(np.float64).T
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(res) - part(ref)) <= 1e-5 * scale + 1e-30)
        assert np.all(np.abs(part(res) - part(res_u)) <= 2e-5 * scale + 1e-30)
    base = (rng.random((n_frames, masks.shape[0])) + 1j * rng.random((n_frames, masks.shape[0]))).astype(np.complex64)
    res2, _ = _fold_apply(hip, data, masks, sig, np.complex64, accumulate_into=base,
                          tuning=dict(mt=0, waves=hip.Variant.DENSE_DEFAULT, ksplit=ksplit))
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 2))
    # every stored weight: one-pixel frames (the mirrored half, the unpaired rows included), rtol 1e-5, atol 0
    n_px = sig[0] * sig[1]
    vals = rng.integers(1, hi, n_px, endpoint=True).astype(dt)
    one = np.zeros((n_px, n_px), dtype=dt)
    one[np.arange(n_px), np.arange(n_px)] = vals
    r1, k1 = _fold_apply(hip, one, masks, sig, np.complex64)
    assert 'k_dense_fold16' in k1, k1
    want = masks.T.astype(np.complex128) * vals[:, None].astype(np.float64)
    for part in (np.real, np.imag):
        g, w = part(r1).astype(np.float64), part(want)
        assert np.all(np.abs(g - w) <= 1e-5 * np.abs(w)), np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))


# ---- banded sparse stacks: column blocks with a common support each on k_dense_fold<.., LIST> (ltmi_fold.hip) --------

def _radial_sparse(sig, n_bins, max_order):
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    from libertem_amd import masks as pm
    cy, cx = sig[0] / 2, sig[1] / 2
    st = radial_mask_factory(sig[0], sig[1], cx, cy, 0, pm.bounding_radius(cx, cy, sig[1], sig[0]), n_bins, max_order, True)()
    return st.to_px_by_masks(dtype=np.complex64)                          # (n_px, n_bins * (max_order + 1)) CSR


@pytest.mark.parametrize('tile_dtype', ['float32', 'uint16', 'int16', 'uint8'])
@pytest.mark.parametrize('sig,n_bins,max_order,n_frames,ksplit', [
    ((96, 128), 3, 7, 300, 0),          # 3 blocks of 8 complex masks: 1 even + 1 odd group
    ((64, 192), 2, 24, 130, 0),         # 2 blocks of 25: 2 + 2 groups (192 is not a multiple of 128: integer frames elsewhere)
    ((65, 64), 4, 11, 70, 0),           # odd number of rows (an unpaired row), 1 + 1
    ((32, 256), 2, 24, 200, 0),         # 2 + 2 groups, two 128-pixel stages per row
    ((96, 128), 3, 7, 200, 5),          # every block's stage list in 5 parts (partial sums + reduction)
    ((64, 128), 2, 24, 40, 64),         # more parts than some blocks have stages
])
def test_banded_stack_radial_fourier_sparse(hip, monkeypatch, tile_dtype, sig, n_bins, max_order, n_frames, ksplit):
    """A radial-Fourier stack with several bins (second C5 run) as CSR: the masks of a bin share a
    support and are dense on it -- one folded dense image per bin, k_dense_fold / k_dense_fold16 over the bin's stage
    list.  Against float64, the blocked image (tuning 42), with accumulation, and every stored weight element-wise."""
    monkeypatch.setenv('LTMI_SPARSE_BAND', '1')                           # (small stacks: take it whatever the estimate says)
    csr = _radial_sparse(sig, n_bins, max_order)
    n_px, n_masks = csr.shape
    rng = np.random.default_rng(_seed('band', sig, n_bins, max_order, tile_dtype))
    dt = np.dtype(tile_dtype)
    if dt.kind == 'f':
        data = rng.random((n_frames, n_px)).astype(np.float32)
        data[1] = 1.0
        label = 'k_dense_fold<f'
    else:
        lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
        data = rng.integers(lo, hi, (n_frames, n_px), endpoint=True).astype(dt)
        data[1] = hi
        data[2] = lo
        label = 'k_dense_fold16<'
    banded = dt.kind == 'f' or sig[1] % 128 == 0
    res, kern = _apply_csr(hip, data, csr, np.complex64, sig=sig, ksplit=ksplit)
    if not banded:
        assert 'banded' not in kern, kern
        return
    assert label in kern and 'banded: %d blocks' % n_bins in kern, kern
    res_b, kern_b = _apply_csr(hip, data, csr, np.complex64, sig=sig, tuning=hip.Variant.SPARSE_NO_SCATTER)
    assert 'banded' not in kern_b, kern_b
    dense = np.asarray(csr.todense()).astype(np.complex128)
    ref = data.astype(np.float64) @ dense
    scale = np.abs(data.astype(np.float64)) @ np.abs(dense)
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(res) - part(ref)) <= 1e-5 * scale + 1e-30)
        # (the blocked image, too: its chains are cut every 2048 pixels since round 5 -- one chain per column over the
        # whole frame had drifted to 1.4e-5 - 2.7e-5 on the constant full-scale frames)
        assert np.all(np.abs(part(res_b) - part(ref)) <= 1e-5 * scale + 1e-30)
        assert np.all(np.abs(part(res) - part(res_b)) <= 2e-5 * scale + 1e-30)
    base = (rng.random((n_frames, n_masks)) + 1j * rng.random((n_frames, n_masks))).astype(np.complex64)
    res2, _ = _apply_csr(hip, data, csr, np.complex64, accumulate_into=base, sig=sig, ksplit=ksplit)
    assert np.all(np.abs(res2 - (ref + base)) <= 1e-5 * (scale + 2))
    # every stored weight: one-pixel frames, rtol 1e-5, atol 0 (also: exactly 0 where nothing is stored)
    if dt.kind == 'f':
        vals = (rng.random(n_px) + 0.5).astype(np.float32)
    else:
        vals = rng.integers(1, hi, n_px, endpoint=True).astype(dt)
    one = np.zeros((n_px, n_px), dtype=dt)
    one[np.arange(n_px), np.arange(n_px)] = vals
    r1, k1 = _apply_csr(hip, one, csr, np.complex64, sig=sig, ksplit=ksplit)
    assert 'banded' in k1, k1
    want = dense * vals[:, None].astype(np.float64)
    for part in (np.real, np.imag):
        g, w = part(r1).astype(np.float64), part(want)
        assert np.all(np.abs(g - w) <= 1e-5 * np.abs(w)), np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))


def test_banded_stack_only_where_it_applies(hip, monkeypatch):
    """No banded image for stacks without a row mirror and for thin rings (one column per support: the estimate says no);
    float32 and 1- / 2-byte integer frames take it; LTMI_SPARSE_BAND=0 switches it off."""
    import scipy.sparse as sp
    from oracle import masks as omasks
    monkeypatch.delenv('LTMI_SPARSE_BAND', raising=False)
    sig = (64, 64)
    data = np.random.default_rng(5).random((40, 4096)).astype(np.float32)
    rings = sp.csr_matrix(omasks.radial_bins(32, 32, 64, 64, n_bins=64, use_sparse=True, dtype=np.float32).T.astype(np.float32))
    _, kern = _apply_csr(hip, data, rings, np.float32, sig=sig)
    assert 'banded' not in kern, kern
    scattered = sp.random(4096, 96, density=0.01, format='csr', dtype=np.float32, random_state=np.random.RandomState(3))
    _, kern = _apply_csr(hip, data, scattered, np.float32, sig=sig)
    assert 'banded' not in kern, kern
    monkeypatch.setenv('LTMI_SPARSE_BAND', '1')
    csr = _radial_sparse((64, 128), 3, 7)
    d2 = np.random.default_rng(6).integers(0, 4096, (40, 64 * 128)).astype(np.uint16)
    _, kern = _apply_csr(hip, d2, csr, np.complex64, sig=(64, 128))
    assert 'k_dense_fold16<' in kern and 'banded' in kern, kern
    _, kern = _apply_csr(hip, d2.astype(np.float32), csr, np.complex64, sig=(64, 128))
    assert 'k_dense_fold<f' in kern and 'banded' in kern, kern
    monkeypatch.setenv('LTMI_SPARSE_BAND', '0')
    _, kern = _apply_csr(hip, d2.astype(np.float32), csr, np.complex64, sig=(64, 128))
    assert 'banded' not in kern, kern


@pytest.mark.parametrize('n_even,n_odd', [(20, 20), (40, 0), (5, 33)])
def test_banded_stack_real_columns_split_blocks(hip, monkeypatch, n_even, n_odd):
    """Real float32 stacks: three wide rings, per ring `n_even` columns that are even and `n_odd` that are odd under the
    row mirror (built by explicit reflection: exact).  More than 32 even (odd) columns on one support are split into
    several blocks of that support."""
    import scipy.sparse as sp
    monkeypatch.setenv('LTMI_SPARSE_BAND', '1')
    sig = (64, 128)
    cy, cx = 32, 64
    yy, xx = np.mgrid[0:sig[0], 0:sig[1]]
    r = np.hypot(yy - cy, xx - cx)
    rng = np.random.default_rng(_seed('bandreal', n_even, n_odd))
    cols = []
    for b in range(3):
        ring = ((r >= 20 * b) & (r < 20 * (b + 1))).astype(np.float32)
        for k in range(n_even + n_odd):
            w = rng.random(sig).astype(np.float32) * ring
            top = w[1:cy]                                      # rows 1 .. cy - 1; partner of row y is 2 cy - y
            w[cy + 1:2 * cy] = top[::-1] if k < n_even else -top[::-1]
            if k >= n_even:
                w[cy] = 0                                      # (an odd column vanishes on the mirror line; row 0 is unpaired)
            cols.append(w.reshape(-1))
    dense = np.stack(cols, axis=1)                             # (n_px, 3 * (n_even + n_odd))
    csr = sp.csr_matrix(dense)
    n_px, n_masks = csr.shape
    data = rng.random((150, n_px)).astype(np.float32)
    res, kern = _apply_csr(hip, data, csr, np.float32, sig=sig)
    # (the odd columns vanish on the mirror line: their support is not the even columns' -> blocks of their own)
    n_blocks = 3 * (-(-n_even // 32) + -(-n_odd // 32))
    assert 'k_dense_fold<f' in kern and 'banded: %d blocks' % n_blocks in kern, kern
    ref = data.astype(np.float64) @ dense.astype(np.float64)
    scale = np.abs(data.astype(np.float64)) @ np.abs(dense.astype(np.float64))
    assert np.all(np.abs(res - ref) <= 1e-5 * scale + 1e-30)
    d16 = rng.integers(0, 65535, (90, n_px), endpoint=True).astype(np.uint16)
    res16, kern16 = _apply_csr(hip, d16, csr, np.float32, sig=sig)
    assert 'k_dense_fold16<' in kern16 and 'banded' in kern16, kern16
    ref16 = d16.astype(np.float64) @ dense.astype(np.float64)
    scale16 = d16.astype(np.float64) @ np.abs(dense.astype(np.float64))
    assert np.all(np.abs(res16 - ref16) <= 1e-5 * scale16 + 1e-30)
