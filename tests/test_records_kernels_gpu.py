"""
`ltmi_records_gather` through the C ABI (-m gpu): frame records [frame header | payload | footer] in a device
buffer -> the payloads, contiguous, bit-equal to the NumPy decoder of tests/records_synth.py (which
tests/test_records_cpu.py pins to the reference's readers).  Payload bytes that tell positions and frames apart,
framing of 0xFF bytes (and the complements: 0x00 payloads in 0xFF framing, 0xFF payloads in 0x00 framing), so that
a framing byte in the output shows; a destination pre-filled with 0xAA with a guard region in front and behind.

Geometries (frames, frame header, payload, footer): the smallest at which each width W of `k_records<W>` is
taken -- W is the largest of 16, 8, 4, 2, 1 that divides the address of the first payload, the record stride, the
payload size and the address of the destination --, plus the records of EMPAD and of BLO with 144 x 144 patterns.
Which kernel ran is asserted against the W the test works out itself, not only the result.

That no byte outside the payloads is READ cannot be observed from here (an allocation is rounded up, a read
behind it does not fault): the last-record-without-footer cases check the result, the read contract itself is
verified by reading csrc/ltmi_records.hip (every access is `in[u]` with `u < per` inside frame `frame < n_frames`).
"""
import functools

import numpy as np
import pytest

import records_synth as synth

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

GUARD = 4096                                        # bytes in front of and behind the destination
FILL = 0xAA
# (n, frame header, payload, footer) -> W with source and destination at addresses = 0 mod 16
GEOMETRIES = {
    (1, 0, 1, 0): 1,                # one byte
    (3, 6, 25, 0): 1,               # BLO-like, odd payload
    (4, 6, 50, 0): 2,
    (3, 0, 100, 4): 4,
    (3, 0, 48, 8): 8,               # the SEQ footer
    (2, 0, 64, 16): 16,
    (2, 0, 65536, 1024): 16,        # EMPAD's record
    (3, 6, 20736, 0): 2,            # BLO, 144 x 144 uint8
}
# (source payload address, destination address) mod 16: each shift on its own, two mixed pairs
PLACEMENTS = ((0, 0), (1, 0), (2, 0), (4, 0), (8, 0), (0, 1), (0, 2), (0, 4), (0, 8), (2, 4), (8, 1))
IDS = [f"n{g[0]}_h{g[1]}_p{g[2]}_f{g[3]}" for g in GEOMETRIES]


def width(src, stride, payload, dst):
    """the rule of include/ltmi.h, worked out here"""
    return next(w for w in (16, 8, 4, 2, 1) if all(v % w == 0 for v in (src, stride, payload, dst)))


@functools.lru_cache(maxsize=None)
def payloads(kind, n, payload):
    f, b = np.meshgrid(np.arange(n), np.arange(payload), indexing='ij', sparse=True)
    if kind == 'position':
        return ((7 * b + 13 * f + 1) & 0xFF).astype(np.uint8)
    return np.full((n, payload), {'zeros': 0x00, 'ones': 0xFF}[kind], dtype=np.uint8)


def host_records(kind, n, frame_header, payload, footer, last_footer=True):
    """-> the bytes of n records; framing 0xFF, or 0x00 around payloads of 0xFF"""
    data = synth.records(payloads(kind, n, payload), frame_header, footer, last_footer).copy()
    if kind == 'ones':
        framing = np.ones(len(data), dtype=bool)
        stride = frame_header + payload + footer
        for i in range(n):
            framing[i * stride + frame_header:i * stride + frame_header + payload] = False
        data[framing] = 0x00
    return data


def upload(host, frame_header, shift):
    """the records on the device, the first payload at an address = `shift` mod 16 -> (tensor, that address); the
    buffer ends with the last byte of `host`"""
    lead = (shift - frame_header) % 16
    buf = torch.full((lead + len(host),), 0xFF, dtype=torch.uint8, device='cuda:0')
    buf[lead:] = torch.from_numpy(host).cuda()
    ptr = buf.data_ptr() + lead + frame_header
    assert buf.data_ptr() % 16 == 0 and ptr % 16 == shift
    return buf, ptr


def run(kind, geometry, src_shift=0, dst_shift=0, first=0, last_footer=True):
    from libertem_amd import hip
    n, frame_header, payload, footer = geometry
    stride = frame_header + payload + footer
    host = host_records(kind, n, frame_header, payload, footer, last_footer)
    buf, ptr = upload(host, frame_header, src_shift)
    m = n - first
    dst = torch.full((GUARD + dst_shift + m * payload + GUARD,), FILL, dtype=torch.uint8, device='cuda:0')
    d = dst.data_ptr() + GUARD + dst_shift
    assert dst.data_ptr() % 16 == 0 and d % 16 == dst_shift
    src = ptr + first * stride
    hip.records_gather(0, src, stride, m, payload, d)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    lo = GUARD + dst_shift
    want = synth.strip(host, 0, frame_header, payload, footer, n, np.uint8, (payload,))[first:]
    assert np.array_equal(want, payloads(kind, n, payload)[first:])
    assert np.array_equal(got[lo:lo + m * payload].reshape(m, payload), want)
    assert np.all(got[:lo] == FILL) and np.all(got[lo + m * payload:] == FILL)
    w = width(src, stride, payload, d)
    assert hip.records_last_kernel() == f"k_records<{w}>"
    return w


@pytest.mark.parametrize('geometry', GEOMETRIES, ids=IDS)
def test_placements_demote_the_width_and_keep_the_bytes(geometry):
    """source and destination at 0, 1, 2, 4, 8 mod 16: W is what divides all four, the result stays bit-equal"""
    n, frame_header, payload, footer = geometry
    stride = frame_header + payload + footer
    best = GEOMETRIES[geometry]
    assert width(0, stride, payload, 0) == best
    for src_shift, dst_shift in PLACEMENTS:
        w = run('position', geometry, src_shift, dst_shift)
        shifts = [s for s in (src_shift, dst_shift) if s]
        assert w == min([best] + shifts), (geometry, src_shift, dst_shift, w)


@pytest.mark.parametrize('kind', ('zeros', 'ones'))
@pytest.mark.parametrize('geometry', GEOMETRIES, ids=IDS)
def test_no_framing_byte_in_the_output(geometry, kind):
    """payloads of 0x00 in framing of 0xFF, payloads of 0xFF in framing of 0x00: one framing byte shows"""
    for src_shift, dst_shift in ((0, 0), (2, 4), (1, 0)):
        run(kind, geometry, src_shift, dst_shift)


@pytest.mark.parametrize('geometry', [g for g in GEOMETRIES if g[0] > 1], ids=[i for i in IDS if i[1] != '1'])
def test_frames_of_a_later_start(geometry):
    """the pointer advanced by `first * stride`: the frames from `first` on"""
    run('position', geometry, first=1)
    run('position', geometry, src_shift=2, first=geometry[0] - 1)


@pytest.mark.parametrize('geometry', [g for g in GEOMETRIES if g[3]], ids=[i for i in IDS if not i.endswith('f0')])
def test_last_record_without_its_footer(geometry):
    """the buffer ends with the last payload (see the module docstring for what this does and does not show)"""
    for kind in ('position', 'zeros'):
        assert run(kind, geometry, last_footer=False) == GEOMETRIES[geometry]
    run('position', geometry, src_shift=4, dst_shift=8, first=1, last_footer=False)


@pytest.mark.parametrize('shifts', ((0, 0), (2, 0), (0, 1)))
def test_more_frames_than_a_grid_dimension(shifts):
    """70 000 frames (a grid dimension takes 65 535): payloads of 16 bytes, 32 bytes apart"""
    w = run('position', (70000, 0, 16, 16), *shifts)
    assert w == min([16] + [s for s in shifts if s])


def test_offsets_beyond_4_gib():
    """4 payloads of 4096 bytes, 1.5 GiB + 16 apart, in an UNINITIALISED allocation of which only the payloads are
    written: byte offsets of up to 4.5 GiB"""
    from libertem_amd import hip
    free, _ = torch.cuda.mem_get_info(0)
    if free < 8 << 30:
        pytest.skip("less than 8 GiB of HBM free")
    n, payload, stride = 4, 4096, (3 << 29) + 16
    assert (n - 1) * stride > 1 << 32
    src = torch.empty((n - 1) * stride + payload, dtype=torch.uint8, device='cuda:0')
    want = payloads('position', n, payload)
    for i in range(n):
        src[i * stride:i * stride + payload] = torch.from_numpy(want[i]).cuda()
    dst = torch.full((GUARD + n * payload + GUARD,), FILL, dtype=torch.uint8, device='cuda:0')
    hip.records_gather(0, src.data_ptr(), stride, n, payload, dst.data_ptr() + GUARD)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[GUARD:GUARD + n * payload].reshape(n, payload), want)
    assert np.all(got[:GUARD] == FILL) and np.all(got[GUARD + n * payload:] == FILL)
    assert hip.records_last_kernel() == 'k_records<16>'
    del src


def test_no_frames_and_argument_errors_launch_nothing():
    """n_frames == 0 and every refused call leave the destination as it was"""
    from libertem_amd import hip
    host = host_records('ones', 2, 0, 64, 16)
    buf, ptr = upload(host, 0, 0)
    dst = torch.full((GUARD,), FILL, dtype=torch.uint8, device='cuda:0')
    d = dst.data_ptr()
    hip.records_gather(0, ptr, 80, 0, 64, d)
    hip.records_gather(0, None, 80, 0, 64, None)
    with pytest.raises(ValueError, match='n_frames is -1'):
        hip.records_gather(0, ptr, 80, -1, 64, d)
    for payload in (0, -64):
        with pytest.raises(ValueError, match=f'a payload of {payload} bytes'):
            hip.records_gather(0, ptr, 80, 2, payload, d)
    with pytest.raises(ValueError, match='records 63 bytes apart cannot hold payloads of 64 bytes'):
        hip.records_gather(0, ptr, 63, 2, 64, d)
    with pytest.raises(ValueError, match='do not fit 64-bit offsets'):
        hip.records_gather(0, ptr, 1 << 40, 1 << 40, 64, d)
    with pytest.raises(ValueError, match='null pointer'):
        hip.records_gather(0, None, 80, 2, 64, d)
    with pytest.raises(ValueError, match='null pointer'):
        hip.records_gather(0, ptr, 80, 2, 64, None)
    torch.cuda.synchronize()
    assert np.all(dst.cpu().numpy() == FILL)
