"""
`ltmi_frms6_decode` through the C ABI (-m gpu): frame records in a device buffer -> (n, 2 height binning,
width / 2) uint16, bit-equal to the NumPy decoder of tests/frms6_synth.py (which tests/test_frms6_cpu.py pins to
the reference's decoder).  Pixel patterns that tell positions, columns and rows apart; file and frame headers of
0xFF bytes, so that a header read as payload shows; a pre-filled destination with a guard region behind it.

Shapes (height, width / 2): the recipes' small ones, an odd half width, a half row of 13 pixels in a single
row, two rows of the real detector's width and the real detector itself (132 x 264 per half).  The upload puts
the first payload at an address = 0 mod 16; half rows of whole 16-byte pieces then take the kernel with 16-byte
loads and stores, every other shape -- and every shape with the payload moved to an address = 2 mod 16 -- the
one with a pixel per lane, as does a destination that is not 16-byte aligned.  Which kernel ran is asserted, not
only its result.
"""
import functools

import numpy as np
import pytest

import frms6_synth as synth

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GUARD = 1 << 12                                     # uint16 elements behind the frames
FILL = 0xAAAA
SHAPES = ((4, 8), (3, 12), (2, 5), (1, 13), (2, 264), (132, 264))
VEC, SCALAR = 'k_frms6_unfold16', 'k_frms6_unfold2'


def pattern(kind, n, h, w):
    f, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing='ij', sparse=True)
    if kind == 'position':
        return ((7 * y + 13 * x + 101 * f + 1) & 0xFFFF).astype(np.uint16)
    if kind == 'ones':
        return np.full((n, h, w), 0xFFFF, dtype=np.uint16)
    if kind == 'alt_x':
        return np.broadcast_to(np.where(x % 2 == 0, 0xFFFF, 0), (n, h, w)).astype(np.uint16)
    if kind == 'alt_y':
        return np.broadcast_to(np.where(y % 2 == 0, 0xFFFF, 0), (n, h, w)).astype(np.uint16)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def records(kind, n, h, x):
    """-> (the bytes of a .frms6 file of n raw frames of h x 2 x, every header byte 0xFF; the raw frames)"""
    raw = pattern(kind, n, h, 2 * x)
    return synth.file_bytes(raw, fill=0xFF), raw


def upload(host, shift):
    """the file bytes on the device, the first payload at an address = `shift` mod 16 -> (tensor, address)"""
    lead = (-(synth.FILE_HEADER + synth.FRAME_HEADER) + shift) % 16
    buf = torch.full((lead + len(host),), 0xFF, dtype=torch.uint8, device='cuda:0')
    buf[lead:] = torch.from_numpy(host).cuda()
    ptr = buf.data_ptr() + lead + synth.FILE_HEADER + synth.FRAME_HEADER
    assert buf.data_ptr() % 16 == 0 and ptr % 16 == shift
    return buf, ptr


def destination(n_px):
    """(n_px + guard) of int16 holding the bit pattern FILL"""
    return torch.full((n_px + GUARD,), FILL - 0x10000, dtype=torch.int16, device='cuda:0')


def as_u16(t):
    return t.cpu().numpy().view(np.uint16)


def expected_kernel(h, x, shift, dst_shift=0):
    stride = synth.FRAME_HEADER + h * 2 * x * 2
    return VEC if x % 8 == 0 and shift == 0 and stride % 16 == 0 and dst_shift == 0 else SCALAR


def run(kind, n, h, x, binning, shift, first=0, dst_shift=0):
    """dst_shift: the destination's address mod 16 (even); the elements in front of it keep the fill as well"""
    from libertem_amd import hip
    host, raw = records(kind, n, h, x)
    buf, ptr = upload(host, shift)
    stride = synth.FRAME_HEADER + h * 2 * x * 2
    m = n - first
    n_px = m * 2 * h * binning * x
    lead = dst_shift // 2
    dst = destination(lead + n_px)
    assert dst.data_ptr() % 16 == 0
    hip.frms6_decode(0, ptr + first * stride, stride, m, h, 2 * x, binning, dst.data_ptr() + dst_shift, np.uint16)
    torch.cuda.synchronize()
    got = as_u16(dst)
    assert np.array_equal(got[lead:lead + n_px].reshape(m, 2 * h * binning, x), synth.unfold(raw[first:], binning))
    assert np.all(got[:lead] == FILL) and np.all(got[lead + n_px:] == FILL)
    assert hip.frms6_last_kernel() == expected_kernel(h, x, shift, dst_shift)


@pytest.mark.parametrize('binning', (1, 2, 4))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_bit_equal(shape, binning):
    """every shape and binning: position-coded pixels, 1 and 3 frames, payloads at 0 and at 2 mod 16"""
    for n in (1, 3):
        for shift in (0, 2):
            run('position', n, shape[0], shape[1], binning, shift)


@pytest.mark.parametrize('kind', ('ones', 'alt_x', 'alt_y'))
@pytest.mark.parametrize('shape', ((4, 8), (2, 5), (132, 264)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_patterns(shape, kind):
    for binning, shift in ((1, 0), (2, 2), (4, 0)):
        run(kind, 3, shape[0], shape[1], binning, shift)


def test_the_real_detector_takes_the_vector_kernel():
    """132 x 528 raw frames, 64-byte frame headers: payloads, strides and half rows are multiples of 16 bytes"""
    assert expected_kernel(132, 264, 0) == VEC and expected_kernel(132, 264, 2) == SCALAR
    assert expected_kernel(4, 8, 0) == VEC and expected_kernel(2, 264, 0) == VEC
    for h, x in ((3, 12), (2, 5), (1, 13)):
        assert expected_kernel(h, x, 0) == SCALAR


@pytest.mark.parametrize('shape', ((4, 8), (2, 264)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_unaligned_destination_takes_the_scalar_kernel(shape):
    """half rows of whole 16-byte pieces and payloads at 0 mod 16, but a destination at 2 mod 16 (and at 8): no
    16-byte stores -- the host picks the pixel-per-lane kernel"""
    assert expected_kernel(shape[0], shape[1], 0) == VEC
    for binning, dst_shift in ((1, 2), (2, 2), (4, 8)):
        assert expected_kernel(shape[0], shape[1], 0, dst_shift) == SCALAR
        run('position', 3, shape[0], shape[1], binning, 0, dst_shift=dst_shift)


@pytest.mark.parametrize('shape', ((4, 8), (2, 5)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_frames_of_a_later_start(shape):
    """decoding from frame 1 of 3 gives frames 1 and 2"""
    run('position', 3, shape[0], shape[1], 2, 0, first=1)


@pytest.mark.parametrize('shift', (0, 2))
def test_more_frames_than_a_grid_dimension(shift):
    """frames are the grid's z dimension (at most 65 535): 65 537 frames of 1 x 16 raw pixels go in two launches"""
    run('position', 65537, 1, 8, 2, shift)


def test_no_frames_and_argument_errors_launch_nothing():
    """every case is refused by the host-side checks (or is n_frames == 0): the destination keeps its fill"""
    from libertem_amd import hip
    h, x = 4, 8
    host, _ = records('ones', 1, h, x)
    buf, ptr = upload(host, 0)
    stride = synth.FRAME_HEADER + h * 2 * x * 2
    dst = destination(2 * h * 4 * x)
    d = dst.data_ptr()
    hip.frms6_decode(0, ptr, stride, 0, h, 2 * x, 1, d, np.uint16)
    with pytest.raises(ValueError, match='null pointer'):
        hip.frms6_decode(0, None, stride, 1, h, 2 * x, 1, d, np.uint16)
    with pytest.raises(ValueError, match='null pointer'):
        hip.frms6_decode(0, ptr, stride, 1, h, 2 * x, 1, None, np.uint16)
    with pytest.raises(ValueError, match='even width, not 15'):
        hip.frms6_decode(0, ptr, stride, 1, h, 15, 1, d, np.uint16)
    for binning in (0, 3, 8, -1):
        with pytest.raises(ValueError, match=f'binning is 1, 2 or 4, not {binning}'):
            hip.frms6_decode(0, ptr, stride, 1, h, 2 * x, binning, d, np.uint16)
    for n, hh, ww in ((-1, h, 2 * x), (1, -4, 2 * x), (1, h, -16), (1, 65536, 2 * x), (1, h, 65536)):
        with pytest.raises(ValueError, match='bad geometry'):
            hip.frms6_decode(0, ptr, stride, n, hh, ww, 1, d, np.uint16)
    with pytest.raises(ValueError, match='bad geometry'):
        hip.frms6_decode(0, ptr, -stride, 1, h, 2 * x, 1, d, np.uint16)
    with pytest.raises(ValueError, match='multiples of 2 bytes'):
        hip.frms6_decode(0, ptr + 1, stride, 1, h, 2 * x, 1, d, np.uint16)
    with pytest.raises(ValueError, match='multiples of 2 bytes'):
        hip.frms6_decode(0, ptr, stride + 1, 2, h, 2 * x, 1, d, np.uint16)
    with pytest.raises(ValueError, match='not 2-byte aligned'):
        hip.frms6_decode(0, ptr, stride, 1, h, 2 * x, 1, d + 1, np.uint16)
    for dtype in (np.uint8, np.int16, np.uint32, np.float32):
        with pytest.raises(ValueError, match='decode to uint16'):
            hip.frms6_decode(0, ptr, stride, 1, h, 2 * x, 1, d, dtype)
    torch.cuda.synchronize()
    assert np.all(as_u16(dst) == FILL)
