"""
`ltmi_transpose2d` through `libertem_amd.hip` (-m gpu): dst[c, r] = src[r, c] for elements of 1, 2, 4, 8 and 16
bytes, byte-equal to NumPy's `.T` -- bytes are moved, so there is no tolerance.

The source has `ld_src = cols + 3` and starts one element after a 16-byte boundary; the destination has
`ld_dst = rows + 5` and lies, again one element after a 16-byte boundary, inside a buffer poisoned with 0xAA that
is compared as a whole: the bytes in front of it, the 5 padding elements behind every row and the bytes behind it
must be unchanged.  Shapes: a single element, a single row, a single column, the sizes around the 64-element tile
edge in both directions, (129, 135) (several tiles, none full at the edges, also of the 128-element tiles of the
1- and 2-byte kernels) and (257, 31).

That no byte outside the rows x cols rectangle of src is READ cannot be observed from here; it follows from the
predicates of csrc/ltmi_transpose.hip (every load is under `r < rows && c < cols`, a 4-byte unit only if all of
it lies in front of `cols`).
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ITEM_BYTES = (1, 2, 4, 8, 16)
SHAPES = ((1, 1), (1, 200), (200, 1), (63, 65), (64, 64), (65, 63), (129, 135), (257, 31))
POISON = 0xAA
LEAD = 48                                           # bytes in front of src / dst, before the one-element shift
TAIL = 64


def hip():
    from libertem_amd import hip
    return hip


def host_source(rows, cols, ib, seed=0):
    """(rows, ld_src, ib) random bytes, ld_src = cols + 3"""
    return np.random.default_rng(1000 * ib + 7 * rows + cols + seed).integers(
        0, 256, (rows, cols + 3, ib), dtype=np.uint8)


def upload_source(src, ib):
    buf = torch.full((LEAD + ib + src.size,), 0x55, dtype=torch.uint8, device='cuda:0')
    buf[LEAD + ib:] = torch.from_numpy(src.reshape(-1)).cuda()
    ptr = buf.data_ptr() + LEAD + ib
    assert buf.data_ptr() % 16 == 0
    return buf, ptr


def poisoned_destination(rows, cols, ib):
    """-> (device buffer, address of dst[0, 0], ld_dst)"""
    ld_dst = rows + 5
    buf = torch.full((LEAD + ib + cols * ld_dst * ib + TAIL,), POISON, dtype=torch.uint8, device='cuda:0')
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + LEAD + ib, ld_dst


def expected_buffer(src, rows, cols, ib, before=None):
    """the whole destination buffer after the call: the transposed rectangle, everything else as it was"""
    ld_dst = rows + 5
    n = LEAD + ib + cols * ld_dst * ib + TAIL
    out = np.full(n, POISON, dtype=np.uint8) if before is None else before.copy()
    inner = out[LEAD + ib:LEAD + ib + cols * ld_dst * ib].reshape(cols, ld_dst, ib)
    inner[:, :rows] = src[:, :cols].transpose(1, 0, 2)
    return out


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize('ib', ITEM_BYTES)
def test_transpose_equals_numpy(ib, shape):
    rows, cols = shape
    src = host_source(rows, cols, ib)
    sbuf, sptr = upload_source(src, ib)
    dbuf, dptr, ld_dst = poisoned_destination(rows, cols, ib)
    hip().transpose2d(0, sptr, cols + 3, rows, cols, ib, dptr, ld_dst)
    got = dbuf.cpu().numpy()
    want = expected_buffer(src, rows, cols, ib)
    assert np.array_equal(got, want)
    assert hip().transpose_last_kernel() == f'k_transpose<{ib}>'
    # a second call with the same input: identical bytes
    hip().transpose2d(0, sptr, cols + 3, rows, cols, ib, dptr, ld_dst)
    assert np.array_equal(dbuf.cpu().numpy(), got)
    # another input through the same destination
    src2 = host_source(rows, cols, ib, seed=1)
    sbuf2, sptr2 = upload_source(src2, ib)
    hip().transpose2d(0, sptr2, cols + 3, rows, cols, ib, dptr, ld_dst)
    assert np.array_equal(dbuf.cpu().numpy(), expected_buffer(src2, rows, cols, ib))
    assert np.array_equal(sbuf.cpu().numpy()[LEAD + ib:], src.reshape(-1))     # (the source is only read)


@pytest.mark.parametrize('ib', ITEM_BYTES)
def test_typed_views_equal_numpy_T(ib):
    """the same through typed arrays: contiguous, ld = the row length, every dtype of that size"""
    dtype = {1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.complex64, 16: np.complex128}[ib]
    rows, cols = 129, 135
    a = np.random.default_rng(ib).integers(0, 256, rows * cols * ib, dtype=np.uint8).view(dtype).reshape(rows, cols)
    src = torch.from_numpy(a.view(np.uint8)).cuda()
    dst = torch.zeros(cols * rows * ib, dtype=torch.uint8, device='cuda:0')
    hip().transpose2d(0, src.data_ptr(), cols, rows, cols, ib, dst.data_ptr(), rows)
    got = dst.cpu().numpy().view(dtype).reshape(cols, rows)
    assert got.tobytes() == np.ascontiguousarray(a.T).tobytes()


@pytest.mark.parametrize('shape', ((0, 7), (7, 0), (0, 0)))
def test_empty_writes_nothing(shape):
    rows, cols = shape
    dbuf = torch.full((256,), POISON, dtype=torch.uint8, device='cuda:0')
    sbuf = torch.zeros(256, dtype=torch.uint8, device='cuda:0')
    for ib in ITEM_BYTES:
        hip().transpose2d(0, sbuf.data_ptr(), cols + 3, rows, cols, ib, dbuf.data_ptr() + 16, rows + 5)
        hip().transpose2d(0, 0, cols, rows, cols, ib, 0, rows)          # (null pointers without work are fine)
    assert bool((dbuf == POISON).all())


def test_argument_errors_touch_nothing():
    rows, cols, ib = 9, 11, 4
    src = host_source(rows, cols, ib)
    sbuf, sptr = upload_source(src, ib)
    dbuf, dptr, ld_dst = poisoned_destination(rows, cols, ib)
    h = hip()
    h.transpose2d(0, sptr, cols + 3, rows, cols, ib, dptr, ld_dst)
    name = h.transpose_last_kernel()
    dbuf.fill_(POISON)
    for kwargs in (dict(item_bytes=3), dict(ld_src=cols - 1), dict(ld_dst=rows - 1), dict(dst_ptr=0),
                   dict(src_ptr=0), dict(rows=-1), dict(cols=-1), dict(item_bytes=0), dict(item_bytes=32),
                   dict(rows=1 << 40, ld_dst=1 << 40, cols=1 << 40, ld_src=1 << 40)):
        call = dict(device=0, src_ptr=sptr, ld_src=cols + 3, rows=rows, cols=cols, item_bytes=ib, dst_ptr=dptr,
                    ld_dst=ld_dst)
        call.update(kwargs)
        with pytest.raises((ValueError, h.LtmiError)):
            h.transpose2d(**call)
    assert bool((dbuf == POISON).all())
    assert h.transpose_last_kernel() == name
