"""
ltmi_count_events / ltmi_store_events (csrc/ltmi_count.hip) on the MI355X, through `hip.count_events` /
`hip.store_events` on guarded regions (tests/guarded.py), against the pixel-by-pixel loop of tests/count_ref.py.

Every input of count_ref's table -- all seven frame dtypes, tie-filled frames at shapes from 1 x 1 to 5 x 515 (widths
that are no multiple of 4, 64 or 256, heights of several strips), NaN and the infinities, the thresholds met exactly,
fractional dark and gain, a frame without events between frames with events, the densest possible frame -- and one
more built on the kernel's own strip height, each with contiguous frames on a 256-byte boundary and with padded frames
(NaN or the dtype's maximum in the padding) behind an element-aligned base.  n_events, indices and values are EQUAL to
the reference, a second run gives the same bytes, no byte around an input or an output changes.  A row pointer that
claims one event too few or too many, or a capacity that is too small, sets `status` and still writes nothing outside
the ranges.
"""
import numpy as np
import pytest

import count_ref as cr
from guarded import Region, unchanged, unchanged_outside

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

F32 = np.dtype('float32')


def hip():
    from libertem_amd import hip as h
    return h


class Setup:
    """the inputs of a case on the device, and its reference"""

    def __init__(self, frames, t_bg, t_x, dark, gain, ref, padded):
        self.frames, self.t_bg, self.t_x, self.ref = frames, t_bg, t_x, ref
        n, h, w = frames.shape
        self.n, self.h, self.w, npx = n, h, w, h * w
        self.ld, shift = (npx + 5, 1) if padded else (npx, 0)
        fill = 'nan' if frames.dtype.kind == 'f' else 'max'
        self.tile = Region(n, npx, self.ld, frames.dtype, shift=shift, init=frames.reshape((n, -1)), fill=fill)
        self.dark = self.gain = None
        if dark is not None:
            self.dark = Region(1, npx, npx, F32, shift=shift, init=dark.reshape((1, -1)), fill='nan')
        if gain is not None:
            self.gain = Region(1, npx, npx, F32, shift=shift, init=gain.reshape((1, -1)), fill='nan')
        self.inputs = [r for r in (self.tile, self.dark, self.gain) if r is not None]

    def head(self, n_frames=None, **over):
        a = dict(device=0, tile=self.tile.ptr, dtype=self.frames.dtype, n=self.n if n_frames is None else n_frames,
                 h=self.h, w=self.w, ld=self.ld, dark=self.dark.ptr if self.dark else None,
                 gain=self.gain.ptr if self.gain else None, t_bg=self.t_bg, t_x=self.t_x)
        a.update(over)
        return tuple(a[k] for k in ('device', 'tile', 'dtype', 'n', 'h', 'w', 'ld', 'dark', 'gain', 't_bg', 't_x'))

    def count(self):
        out = Region(1, self.n, self.n, np.int32)
        hip().count_events(*self.head(), out.ptr)
        got = out.result()[0]
        unchanged_outside(out, 'n_events')
        return got

    def store(self, values, indptr=None, base=0, capacity=None):
        """-> (indices, values | None, status) as the device holds them; the guards are checked"""
        indptr = self.ref[0] if indptr is None else indptr
        capacity = int(self.ref[0][-1]) if capacity is None else capacity
        ptr_r = Region(1, self.n + 1, self.n + 1, np.int64, init=(indptr + base)[None], fill='max')
        idx_r = Region(1, capacity, capacity, np.int32)
        val_r = None if values is None else Region(1, capacity, capacity, values)
        status = Region(1, 1, 1, np.int32, init=np.zeros((1, 1), np.int32))
        hip().store_events(*self.head(), ptr_r.ptr, base, capacity, idx_r.ptr, val_r.ptr if val_r else None,
                           values if values is not None else np.uint8, status.ptr)
        got = idx_r.result()[0], (val_r.result()[0] if val_r else None), int(status.result()[0, 0])
        for r, what in ((idx_r, 'indices'), (val_r, 'values'), (status, 'status')):
            if r is not None:
                unchanged_outside(r, what)
        unchanged(ptr_r, 'indptr')
        return got

    def inputs_unchanged(self):
        for r in self.inputs:
            unchanged(r, 'input')


def check(setup):
    indptr, indices, intensity = setup.ref
    n_events = setup.count()
    assert n_events.dtype == np.int32 and np.array_equal(n_events, np.diff(indptr))
    assert setup.count().tobytes() == n_events.tobytes()
    got_i, got_v, status = setup.store(np.uint8)
    assert status == 0 and np.array_equal(got_i, indices) and np.all(got_v == 1)
    got_i, got_v, status = setup.store(np.float32, base=1000)
    assert status == 0 and np.array_equal(got_i, indices)
    assert got_v.tobytes() == intensity.tobytes()
    again_i, again_v, _ = setup.store(np.float32, base=1000)
    assert again_i.tobytes() == got_i.tobytes() and again_v.tobytes() == got_v.tobytes()
    got_i, got_v, status = setup.store(None)
    assert status == 0 and got_v is None and np.array_equal(got_i, indices)
    setup.inputs_unchanged()
    vec = ' vec' if setup.w % 4 == 0 else ''
    assert hip().count_last_kernel() == 'k_store_events' + vec


@pytest.mark.parametrize('padded', (False, True), ids=('contiguous', 'padded'))
@pytest.mark.parametrize('name', sorted(cr.CASES))
def test_kernels_equal_the_definition(name, padded):
    check(Setup(*cr.case(name), cr.reference(name, 'intensity'), padded))


@pytest.mark.parametrize('w', (64, 515))
def test_events_on_the_strip_edges(w):
    strip = hip().count_strip_rows(4096, w)
    assert 1 < strip <= 30
    frames, t_bg, t_x, _, _ = cr.strip_edge(strip, w)
    assert frames.shape[1] == 2 * strip + 3 and hip().count_strip_rows(*frames.shape[1:]) == strip
    ref = cr.count_ref(frames, t_bg, t_x, values='intensity')
    rows = ref[1][:ref[0][1]] // w
    for y in (strip - 1, strip, 2 * strip - 1, 2 * strip):
        assert y in rows                                     # an event on the last and the first row of a strip
    check(Setup(frames, t_bg, t_x, None, None, ref, padded=True))


def test_one_frame_of_many():
    """a single frame: the one workgroup of the launch"""
    frames, t_bg, t_x, dark, gain = cr.case('ties-16x16')
    ref = cr.count_ref(frames[3:4], t_bg, t_x, values='intensity')
    check(Setup(frames[3:4], t_bg, t_x, dark, gain, ref, padded=True))


@pytest.mark.parametrize('delta', (-1, 1), ids=('one-too-few', 'one-too-many'))
def test_wrong_row_pointer_sets_status(delta):
    name = 'ties-16x16'
    setup = Setup(*cr.case(name), cr.reference(name, 'intensity'), padded=False)
    indptr, indices, _ = setup.ref
    assert indptr[4] - indptr[3] > 1
    wrong = indptr.copy()
    wrong[4:] += delta
    got_i, got_v, status = setup.store(np.float32, indptr=wrong, capacity=int(wrong[-1]))
    assert status != 0
    # the frames before the wrong one lie where they belong
    assert np.array_equal(got_i[:indptr[3]], indices[:indptr[3]])
    # a right row pointer on the same buffers' addresses afterwards: status stays 0
    assert setup.store(np.float32)[2] == 0


def test_capacity_too_small_sets_status():
    name = 'lattice'
    setup = Setup(*cr.case(name), cr.reference(name, 'intensity'), padded=True)
    indptr, indices, _ = setup.ref
    cap = int(indptr[-1]) - 5
    got_i, got_v, status = setup.store(np.uint8, capacity=cap)
    assert status != 0 and np.array_equal(got_i, indices[:cap]) and np.all(got_v == 1)
    got_i, _, status = setup.store(np.uint8, base=7, capacity=0)
    assert status != 0 and got_i.size == 0


def test_ranges_far_outside_write_nothing():
    name = 'ties-16x16'
    setup = Setup(*cr.case(name), cr.reference(name, 'intensity'), padded=False)
    n = setup.n
    cap = int(setup.ref[0][-1])
    for wild in (np.full(n + 1, -10 ** 18), np.full(n + 1, 10 ** 18), np.arange(n + 1) * -3,
                 np.array([0, 2 ** 62] + [2 ** 62] * (n - 1)), np.linspace(-2 ** 62, 2 ** 62, n + 1).astype(np.int64)):
        wild = wild.astype(np.int64)
        idx_r = Region(1, cap, cap, np.int32)
        ptr_r = Region(1, n + 1, n + 1, np.int64, init=wild[None], fill='max')
        status = Region(1, 1, 1, np.int32, init=np.zeros((1, 1), np.int32))
        hip().store_events(*setup.head(), ptr_r.ptr, 0, cap, idx_r.ptr, None, np.uint8, status.ptr)
        assert int(status.result()[0, 0]) != 0
        unchanged_outside(idx_r, 'indices')
        got = idx_r.download()
        inside = idx_r.owned_mask()
        lo = max(int(wild[0]), 0)
        hi = min(int(wild[-1]), cap)
        allowed = np.zeros(cap, bool)
        for f in range(n):                                       # the elements some frame's range covers
            a, b = max(int(wild[f]), 0), min(int(wild[f + 1]), cap)
            if a < b:
                allowed[a:b] = True
        changed = (got != idx_r.host)[inside].reshape((cap, 4)).any(axis=1)
        assert not np.any(changed & ~allowed), (lo, hi)


def test_no_frames_launches_nothing():
    name = 'ties-3x3'
    setup = Setup(*cr.case(name), cr.reference(name, 'intensity'), padded=False)
    out = Region(1, 4, 4, np.int32)
    hip().count_events(*setup.head(n_frames=0), out.ptr)
    hip().count_events(*setup.head(n_frames=0, tile=None), None)
    status = Region(1, 1, 1, np.int32, init=np.zeros((1, 1), np.int32))
    hip().store_events(*setup.head(n_frames=0), None, 0, 4, out.ptr, None, np.uint8, status.ptr)
    torch.cuda.synchronize()
    assert np.array_equal(out.download(), out.host) and int(status.result()[0, 0]) == 0


def test_error_codes():
    name = 'ties-3x3'
    setup = Setup(*cr.case(name), cr.reference(name, 'intensity'), padded=False)
    out = Region(1, 16, 16, np.int32)
    status = Region(1, 1, 1, np.int32, init=np.zeros((1, 1), np.int32))
    ptr_r = Region(1, setup.n + 1, setup.n + 1, np.int64, init=setup.ref[0][None], fill='max')

    def count(**over):
        hip().count_events(*setup.head(**over), out.ptr)

    def store(values=np.uint8, capacity=16, **over):
        hip().store_events(*setup.head(**over), ptr_r.ptr, 0, capacity, out.ptr, None, values, status.ptr)

    for call in (count, store):
        for dtype in (np.float64, np.uint64, np.int64, np.bool_, np.complex64):
            with pytest.raises(ValueError, match=r'code -2'):
                call(dtype=dtype)
        for over in (dict(h=0), dict(w=0), dict(w=4097, h=1), dict(h=65536, w=32768), dict(ld=8), dict(n=-1),
                     dict(t_bg=float('nan')), dict(t_x=float('nan'))):
            with pytest.raises(ValueError, match=r'code -3'):
                call(**over)
        with pytest.raises(ValueError, match=r'code -1'):
            call(tile=None)
    with pytest.raises(ValueError, match=r'code -2'):
        store(values=np.uint16)
    with pytest.raises(ValueError, match=r'code -3'):
        store(capacity=-1)
    torch.cuda.synchronize()
    assert np.array_equal(out.download(), out.host)          # none of them launched
