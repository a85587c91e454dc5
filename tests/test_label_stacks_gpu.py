"""
Detector binning through the product wiring: masks.bin_masks -> ApplyMasksUDF(use_sparse=True) -> MaskContainer -> CSR
handle with a label image (kind 4, LTMI_SPARSE_LABELS=1: not the default route) -> k_labels, against the oracle's restatement of the reference's CSR loop
(oracle.path.apply_masks_sparse).  A 6 x 7 scan of 67 x 45 frames: rows of odd length, six pixel chunks, edge bins.
"""
import numpy as np
import pytest

from oracle import path as opath

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAV, SIG, FACTOR = (6, 7), (67, 45), 4


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def labels_on(monkeypatch):
    """the library reads the switches when a handle is made"""
    for k in ('LTMI_SPARSE_LABELS', 'LTMI_SPARSE_BELL', 'LTMI_SPARSE_SCATTER', 'LTMI_SPARSE_BAND'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('LTMI_SPARSE_LABELS', '1')


def binning_udf():
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.masks import bin_masks_factory
    return ApplyMasksUDF(mask_factories=bin_masks_factory(SIG, FACTOR), use_sparse=True)


def run(ctx, ds, udf, **kw):
    """-> (result buffer, names of the mask kernels that ran)"""
    from libertem_amd import hip
    hip.KernelTimer.start()
    try:
        res = ctx.run_udf(dataset=ds, udf=udf, **kw)
    finally:
        kernels = {k.split(' ')[0] for _, _, k in hip.KernelTimer.stop()}
    return res['intensity'], kernels


@pytest.fixture(scope='module')
def scan():
    from libertem_amd.masks import bin_masks
    data = np.random.default_rng(31).integers(0, 65535, NAV + SIG, endpoint=True).astype(np.uint16)
    stack = bin_masks(SIG, FACTOR)
    ref = opath.apply_masks_sparse(data, stack)
    # weights 1, at most 16 pixels of 16 bits per bin: exact in float32
    exact = (stack.astype(np.int64) @ data.reshape((-1, SIG[0] * SIG[1])).astype(np.int64).T).T
    assert np.array_equal(ref.reshape(exact.shape), exact.astype(np.float32))
    return data, ref


def test_binning_udf(ctx, scan):
    data, ref = scan
    udf = binning_udf()
    ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=2)
    got, kernels = run(ctx, ds, udf)
    assert kernels and all(k.startswith('k_labels<') for k in kernels), kernels
    assert got.data.shape == ref.shape and got.data.dtype == np.float32
    assert np.array_equal(got.data, ref)
    handles = list(udf.masks._handle_cache.values())
    assert handles and all(h.kind() == 4 for h in handles)


def test_binning_udf_default_route(ctx, scan, monkeypatch):
    """without the switch: the gather kernel, the same sums"""
    monkeypatch.delenv('LTMI_SPARSE_LABELS')
    data, ref = scan
    ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=2)
    got, kernels = run(ctx, ds, binning_udf())
    assert kernels and all(k.startswith('k_sell_apply<') for k in kernels), kernels
    assert np.array_equal(got.data, ref)


def test_binning_udf_roi(ctx, scan):
    data, ref = scan
    roi = np.random.default_rng(32).random(NAV) < 0.4
    roi[0, 0] = roi[-1, -1] = True
    ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=2)
    got, kernels = run(ctx, ds, binning_udf(), roi=roi)
    assert kernels and all(k.startswith('k_labels<') for k in kernels), kernels
    assert np.array_equal(got.raw_data, ref[roi])


def test_binning_udf_result_on_device(ctx, scan):
    from libertem_amd.common.hiparray import HipArray
    data, ref = scan
    ds = ctx.load('memory', data=HipArray.from_numpy(data, 0), sig_dims=2, num_partitions=2)
    got, kernels = run(ctx, ds, binning_udf(), result_where='device')
    assert kernels and all(k.startswith('k_labels<') for k in kernels), kernels
    assert isinstance(got.device_data, HipArray)
    assert np.array_equal(got.data, ref)


def test_binning_udf_tiles_that_cut_the_frames(ctx, scan):
    """16 detector rows per tile: a label image per sig slice; the bins outside a slice are its empty columns, and the
    slices' sums are accumulated"""
    data, ref = scan
    ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=2, tileshape=(5, 16, SIG[1]))
    udf = binning_udf()
    got, kernels = run(ctx, ds, udf)
    assert kernels and all(k.startswith('k_labels<') for k in kernels), kernels
    assert len(udf.masks._handle_cache) > 1
    assert np.array_equal(got.data, ref)


@pytest.mark.parametrize('last_pixel', ['free', 0.75, 0.0])
def test_binning_udf_non_finite_float_frames(ctx, last_pixel):
    """weighted bins with free pixels (first detector row, a block in the middle) on float32 frames: a non-finite pixel
    no mask stores reaches no result, a stored one exactly its mask, a stored zero weight gives NaN.  The frame's last
    pixel is free (case a), stored with a weight (b) or with a stored zero (c), and non-finite in the last frame.
    (204 columns: such a stack is not densified.)"""
    import scipy.sparse as sp
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.masks import bin_masks
    from libertem_amd.common.sparse import SparseStack
    n_px = SIG[0] * SIG[1]
    full = bin_masks(SIG, FACTOR).tocoo()
    yy, xx = np.divmod(full.col, SIG[1])
    keep = (yy > 0) & ~((yy >= 30) & (yy < 37) & (xx >= 20) & (xx < 27))
    if last_pixel == 'free':
        keep &= full.col != n_px - 1
    px, k = full.col[keep], full.row[keep]
    w = (0.5 + 0.01 * (px % 11)).astype(np.float32)
    zero_i = len(px) // 3
    w[zero_i] = 0                                                         # a STORED zero
    if last_pixel != 'free':
        assert px[-1] == n_px - 1
        w[-1] = last_pixel
    stack = sp.csr_matrix((w, (k, px)), shape=full.shape)                 # (n_masks, n_px)
    assert stack.nnz == len(px) and stack.shape[0] == 204
    data = np.random.default_rng(33).standard_normal(NAV + SIG).astype(np.float32)
    flat = data.reshape((-1, n_px))
    free = np.flatnonzero(~np.isin(np.arange(n_px), px))
    assert 0 in free and (n_px - 1 in free) == (last_pixel == 'free')
    flat[4, free[50]] = np.nan                                            # (a) no mask stores it
    flat[-1, -1] = np.inf                                                 #     ... last pixel of the last frame
    flat[7, px[5]] = np.nan                                               # (b) one mask
    flat[-1, px[100]] = -np.inf
    flat[11, px[zero_i]] = np.inf                                         # (c) 0 * Inf
    flat[-1, px[zero_i]] = np.nan
    ref = opath.apply_masks_sparse(data, stack)
    assert np.isnan(ref.reshape((-1, 204))[11, k[zero_i]]) and k[100] != 203 and k[zero_i] != 203
    last_bin = ref.reshape((-1, 204))[-1, 203]                            # holds the last pixel of the last frame
    assert (~np.isfinite(ref)).sum() == (4 if last_pixel == 'free' else 5)
    assert np.isfinite(last_bin) if last_pixel == 'free' else (np.isposinf(last_bin) if last_pixel else np.isnan(last_bin))
    udf = ApplyMasksUDF(mask_factories=lambda: SparseStack(w, k, px, 204, SIG), use_sparse=True)
    ds = ctx.load('memory', data=data, sig_dims=2, num_partitions=2)
    got, kernels = run(ctx, ds, udf)
    assert kernels and all(k_.startswith('k_labels<') for k_ in kernels), kernels
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got.data), np.isnan(ref)) and np.array_equal(got.data[~fin & ~np.isnan(ref)],
                                                                                ref[~fin & ~np.isnan(ref)])
    scale = np.abs(np.nan_to_num(flat, nan=0, posinf=0, neginf=0)).astype(np.float64) @ np.abs(stack).T.toarray()
    assert np.all(np.abs(got.data - ref)[fin] <= 1e-5 * scale.reshape(ref.shape)[fin])
