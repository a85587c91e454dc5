"""
`ltmi_records_gather` at the placements TVIPS brings (-m gpu), which tests/test_records_kernels_gpu.py does not hold:
image headers of 112 bytes in front of 96 payload bytes (version 2, 6 x 8 16-bit pixels: W = 16), of 12 in front of
72 (version 1, 6 x 6 16-bit: W = 4) and of 12 in front of 25 (version 1, 5 x 5 8-bit: W = 1), no footers.

Both buffers are guarded allocations (tests/guarded.py): the records lie between bands of 0xFF -- as do their image
headers --, the destination between bands of poison bytes, and after the launch every byte outside the payloads'
destination is what it was.  Bit-equal to the NumPy decoder of tests/records_synth.py; the kernel that ran is the
one the rule of include/ltmi.h names.
"""
import numpy as np
import pytest

import guarded as G
import records_synth as synth
from test_records_kernels_gpu import payloads, width

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

# (frames, image header, payload) -> W with both buffers at multiples of 16.  Frames: one, and as many as put the
# last record's start past a multiple of every W
GEOMETRIES = {(1, 112, 96): 16, (5, 112, 96): 16, (1, 12, 72): 4, (5, 12, 72): 4, (1, 12, 25): 1, (7, 12, 25): 1}
# (bytes the first record starts behind a 256-byte boundary, the same of the destination)
SHIFTS = ((0, 0), (4, 0), (0, 8), (1, 2))


@pytest.mark.parametrize('geometry', GEOMETRIES, ids=lambda g: "n%d_h%d_p%d" % g)
@pytest.mark.parametrize('kind', ('position', 'zeros'))
def test_tvips_records_between_guards(geometry, kind):
    from libertem_amd import hip
    n, header, payload = geometry
    stride = header + payload
    want = payloads(kind, n, payload)
    host = synth.records(want, header, 0)
    assert len(host) == n * stride and np.array_equal(synth.strip(host, 0, header, payload, 0, n, np.uint8, (payload,)),
                                                      want)
    for src_shift, dst_shift in SHIFTS:
        src = G.Region(1, n * stride, n * stride, np.uint8, shift=src_shift, init=host, fill='max')
        dst = G.Region(n, payload, payload, np.uint8, shift=dst_shift)
        first = src.ptr + header
        hip.records_gather(0, first, stride, n, payload, dst.ptr)
        w = width(first, stride, payload, dst.ptr)
        assert hip.records_last_kernel() == f"k_records<{w}>"
        if (src_shift, dst_shift) == (0, 0):
            assert w == GEOMETRIES[geometry]
        what = f"{geometry} {kind} shifts {src_shift}, {dst_shift}"
        assert np.array_equal(dst.result(), want), what
        G.unchanged_outside(dst, what)
        G.unchanged(src, what)
