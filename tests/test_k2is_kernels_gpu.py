"""
`ltmi_k2is_decode` through the C ABI (-m gpu): sector blocks in a device buffer -> (n, 1860, 2048) uint16,
bit-equal to the NumPy decoder of tests/k2is_synth.py (which tests/test_k2is_cpu.py pins to the reference's
decoder).  Pixel patterns that tell positions, nibbles and rows apart; headers of 0xFF bytes, so that a header
read as payload shows; a pre-filled destination with a guard region behind it; the 8 sector pointers at
different offsets of the upload.  A frame cannot be smaller than its format: 1 and 3 frames.
"""
import functools

import numpy as np
import pytest

import k2is_synth as synth

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

H, W = synth.FRAME_SHAPE
GUARD = 1 << 16                                     # uint16 elements behind the frames
FILL = 0xAAAA


def pattern(kind, n):
    f, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing='ij', sparse=True)
    if kind == 'position':
        return ((7 * y + 13 * x + 101 * f) & 0xFFF).astype(np.uint16)
    if kind == 'ones':
        return np.full((n, H, W), 0xFFF, dtype=np.uint16)
    if kind == 'alt_x':
        return np.broadcast_to(np.where(x % 2 == 0, 0xFFF, 0), (n, H, W)).astype(np.uint16)
    if kind == 'alt_y':
        return np.broadcast_to(np.where(y % 2 == 0, 0xFFF, 0), (n, H, W)).astype(np.uint16)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def upload(kind, n):
    """-> (host bytes of the upload, the 8 offsets of the sectors' first blocks, the frames the NumPy decoder reads
    from those bytes).  Offsets: all multiples of 8, no two sectors alike; sector 5 starts 3 blocks later."""
    frames = pattern(kind, n)
    parts, offsets, at = [], [], 0
    want = np.empty_like(frames)
    for s in range(synth.NUM_SECTORS):
        blocks = np.full((n, synth.BLOCKS_PER_FRAME, synth.BLOCK_SIZE), 0xFF, dtype=np.uint8)
        blocks[:, :, synth.HEADER_SIZE:] = synth.sector_payload(frames, s)
        want[:, :, 256 * s:256 * (s + 1)] = synth.decode_blocks(blocks)
        lead = 8 * (s + 1) + (3 * synth.BLOCK_SIZE if s == 5 else 0)
        parts += [np.full(lead, 0xFF, dtype=np.uint8), blocks.reshape(-1)]
        offsets.append(at + lead)
        at += lead + blocks.size
    assert np.array_equal(want, frames)
    assert all(o % 8 == 0 for o in offsets)
    assert len({o % synth.BLOCK_SIZE for o in offsets}) == 8
    return np.concatenate(parts), tuple(offsets), want


def destination(n):
    """(n frames + guard) of int16 holding the bit pattern FILL"""
    return torch.full((n * H * W + GUARD,), FILL - 0x10000, dtype=torch.int16, device='cuda:0')


def as_u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('kind', ('position', 'ones', 'alt_x', 'alt_y'))
def test_decode_bit_equal(kind, n):
    from libertem_amd import hip
    host, offsets, want = upload(kind, n)
    raw = torch.from_numpy(host).cuda()
    dst = destination(n)
    assert raw.data_ptr() % 8 == 0 and dst.data_ptr() % 16 == 0
    hip.k2is_decode(0, [raw.data_ptr() + o for o in offsets], n, dst.data_ptr(), np.uint16)
    torch.cuda.synchronize()
    got = as_u16(dst)
    assert np.array_equal(got[:n * H * W].reshape(n, H, W), want)
    assert np.all(got[n * H * W:] == FILL)


def test_frames_of_a_later_start():
    """the frames of a sector are 32 blocks apart: decoding from frame 1 on gives frames 1 and 2"""
    from libertem_amd import hip
    host, offsets, want = upload('position', 3)
    raw = torch.from_numpy(host).cuda()
    dst = destination(2)
    step = synth.BLOCKS_PER_FRAME * synth.BLOCK_SIZE
    hip.k2is_decode(0, [raw.data_ptr() + o + step for o in offsets], 2, dst.data_ptr(), np.uint16)
    torch.cuda.synchronize()
    got = as_u16(dst)
    assert np.array_equal(got[:2 * H * W].reshape(2, H, W), want[1:])
    assert np.all(got[2 * H * W:] == FILL)


def test_no_frames_and_argument_errors_launch_nothing():
    """every case is refused by the host-side checks (or is n_frames == 0): the destination keeps its fill"""
    from libertem_amd import hip
    host, offsets, _ = upload('ones', 1)
    raw = torch.from_numpy(host).cuda()
    dst = destination(1)
    ptrs = [raw.data_ptr() + o for o in offsets]
    hip.k2is_decode(0, ptrs, 0, dst.data_ptr(), np.uint16)
    with pytest.raises(ValueError, match='multiple of 8 bytes'):
        hip.k2is_decode(0, ptrs[:6] + [ptrs[6] + 4] + ptrs[7:], 1, dst.data_ptr(), np.uint16)
    with pytest.raises(ValueError, match='not 16-byte aligned'):
        hip.k2is_decode(0, ptrs, 1, dst.data_ptr() + 8, np.uint16)
    for dtype in (np.uint8, np.uint32, np.float32):
        with pytest.raises(ValueError, match='decode to uint16'):
            hip.k2is_decode(0, ptrs, 1, dst.data_ptr(), dtype)
    with pytest.raises(ValueError, match='null pointer'):
        hip.k2is_decode(0, ptrs, 1, None, np.uint16)
    with pytest.raises(ValueError, match='null pointer'):
        hip.k2is_decode(0, None, 1, dst.data_ptr(), np.uint16)
    with pytest.raises(ValueError, match=r'null pointer \(sector 2\)'):
        hip.k2is_decode(0, ptrs[:2] + [None] + ptrs[3:], 1, dst.data_ptr(), np.uint16)
    with pytest.raises(ValueError, match='bad geometry'):
        hip.k2is_decode(0, ptrs, -1, dst.data_ptr(), np.uint16)
    with pytest.raises(ValueError, match='8 sectors'):
        hip.k2is_decode(0, ptrs[:7], 1, dst.data_ptr(), np.uint16)
    torch.cuda.synchronize()
    assert np.all(as_u16(dst) == FILL)
