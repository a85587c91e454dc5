"""
masks.bin_masks -- the box masks that bin a detector -- and masks.is_label_stack, the host-side twin of the rule by
which the library gives a sparse stack its label image (csrc/ltmi_labels.hip labels_qualifies).  No GPU.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from libertem_amd import masks as pm

SHAPES = [(7, 10), (16, 16), (67, 45)]
FACTORS = [1, 3, 4]


def block_sums(frame, b):
    """block-wise sums with partial blocks at the lower and right edge"""
    h, w = frame.shape
    ny, nx = -(-h // b), -(-w // b)
    out = np.zeros((ny, nx), dtype=frame.dtype)
    for y in range(ny):
        for x in range(nx):
            out[y, x] = frame[y * b:(y + 1) * b, x * b:(x + 1) * b].sum()
    return out


@pytest.mark.parametrize('factor', FACTORS)
@pytest.mark.parametrize('shape', SHAPES)
def test_bin_masks(shape, factor):
    h, w = shape
    stack = pm.bin_masks(shape, factor)
    ny, nx = -(-h // factor), -(-w // factor)
    assert sp.issparse(stack) and stack.format == 'csr'
    assert stack.shape == (ny * nx, h * w) and stack.dtype == np.float32
    # a partition of the frame: every pixel in exactly one mask, weight 1
    assert stack.nnz == h * w and np.all(stack.data == 1)
    assert np.array_equal(np.asarray(stack.sum(axis=0)).ravel(), np.ones(h * w))
    # the binned frame
    frame = np.random.default_rng(h * 100 + factor).integers(0, 1000, shape).astype(np.int64)
    assert np.array_equal(stack.astype(np.int64) @ frame.ravel(), block_sums(frame, factor).ravel())
    # mask k is bin (k // nx, k % nx)
    for k in {0, nx - 1, nx, ny * nx - 1} & set(range(ny * nx)):
        want = np.zeros(shape)
        want[(k // nx) * factor:(k // nx + 1) * factor, (k % nx) * factor:(k % nx + 1) * factor] = 1
        assert np.array_equal(stack[k].toarray().reshape(shape), want), k
    if factor == 1:
        assert (stack != sp.identity(h * w, format='csr')).nnz == 0


def test_bin_masks_dtype_and_arguments():
    assert pm.bin_masks((4, 6), 2, dtype=np.float64).dtype == np.float64
    with pytest.raises(ValueError):
        pm.bin_masks((4, 6), 0)
    with pytest.raises(ValueError):
        pm.bin_masks((0, 6), 2)


def test_bin_masks_as_mask_factory():
    """a bare 2-D scipy matrix is ONE mask for the container; the stack goes in as a SparseStack"""
    from libertem_amd.common.container import MaskContainer
    sig = (7, 10)
    c = MaskContainer(pm.bin_masks_factory(sig, 3), use_sparse=True)
    assert len(c) == 3 * 4
    frame = np.arange(70).reshape(sig)
    dense = np.asarray(c.computed_masks.todense())
    assert dense.shape == (12,) + sig
    assert np.array_equal((dense * frame).sum(axis=(1, 2)), block_sums(frame, 3).ravel())


def test_is_label_stack():
    part = pm.bin_masks((67, 45), 4).T.tocsr()                            # (n_px, n_masks)
    assert pm.is_label_stack(part)
    twice = part.tolil()
    twice[100, 7] = 1.0                                                   # pixel 100 also belongs to bin 2
    assert not pm.is_label_stack(twice.tocsr())
    assert not pm.is_label_stack(sp.csr_matrix((3015, 204), dtype=np.float32))     # an empty stack
    pts = sp.csr_matrix((np.ones(3, dtype=np.float32), ([5, 700, 2999], [0, 1, 2])), shape=(3015, 3))
    assert pm.is_label_stack(pts)                                         # a few labelled pixels are a partition too
    # a stored zero is a stored entry
    zero = part.copy()
    zero.data[17] = 0
    assert zero.nnz == part.nnz and pm.is_label_stack(zero)
