"""
`ltmi_lattice_fit` on the MI355X through hip.lattice_fit, against the frame-by-frame float64 restatement of the
definition (tests/lattice_ref.py): 1 to 130 peaks (below, at and above one wave's 64 lanes), 1 to 9 frames (a partial
workgroup, a full one, further ones), weighted and unweighted, peak_values given and NULL, frames where everything is
rejected, where exactly three peaks survive and where the survivors are collinear; guard bytes around all five results
and all inputs, bitwise repeats, no frames, error codes, a non-default stream.

Tolerance (lattice_ref.compare): selector bytes exactly 0 or 1 and equal, NaN pattern equal, zero, a, b and error
within eps32 |ref| + 16 kappa P eps64 max|refineds|.  tests/test_lattice_cpu.py establishes that no seeded position
lies within 1e-3 px of the tolerance and that the second term stays below eps32 / 16.
"""
import numpy as np
import pytest

import guarded
import lattice_ref as lr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SHAPES = {'zero': 2, 'a': 2, 'b': 2, 'error': 1}


class Call:
    """guarded inputs and five guarded result buffers of one case"""

    def __init__(self, c):
        r = c['refineds']
        self.n, self.k = r.shape[:2]
        n, k = self.n, self.k
        self.start, self.tol = c['start'], c['tol']
        self.inputs = {'refineds': guarded.Region(n, 2 * k, 2 * k, np.float32, init=r.reshape((n, 2 * k)), fill='nan'),
                       'indices': guarded.Region(1, 2 * k, 2 * k, np.int32, init=c['indices'].reshape((1, 2 * k)),
                                                 fill='max')}
        for name in ('weights', 'peak_values'):
            if c[name] is not None:
                self.inputs[name] = guarded.Region(n, k, k, np.float32, init=c[name], fill='nan')
        self.out = {name: guarded.Region(n, cols, cols, np.float32) for name, cols in SHAPES.items()}
        self.out['selector'] = guarded.Region(n, k, k, np.uint8)

    def ptr(self, name):
        return self.inputs[name].ptr if name in self.inputs else None

    def run(self, **kw):
        from libertem_amd import hip
        args = dict(device=0, refineds_ptr=self.ptr('refineds'), weights_ptr=self.ptr('weights'),
                    peak_values_ptr=self.ptr('peak_values'), n_frames=self.n, n_peaks=self.k,
                    indices_ptr=self.ptr('indices'), start=self.start, tolerance=self.tol,
                    zero_ptr=self.out['zero'].ptr, a_ptr=self.out['a'].ptr, b_ptr=self.out['b'].ptr,
                    selector_ptr=self.out['selector'].ptr, error_ptr=self.out['error'].ptr)
        args.update(kw)
        torch.cuda.synchronize()                            # (the uploads, whatever stream the call takes)
        hip.lattice_fit(**args)
        torch.cuda.synchronize()
        got = {}
        for name, region in self.out.items():
            guarded.unchanged_outside(region, name)
            got[name] = region.result()
        for name, region in self.inputs.items():
            guarded.unchanged(region, name)
        got['error'] = got['error'].reshape(-1)
        return got


def check(got, c, ref):
    assert set(np.unique(got['selector'])) <= {0, 1}
    return lr.compare(got, ref, c['refineds'])


@pytest.mark.parametrize('case', lr.KERNEL_CASES, ids=lambda c: c[0])
def test_kernel_vs_definition(case):
    from libertem_amd import hip
    c = lr.kernel_case(case)
    ref = lr.case_reference(c)
    call = Call(c)
    got = call.run()
    print(case[0], 'largest error / tolerance', check(got, c, ref))
    assert hip.lattice_last_kernel() == 'k_lattice_fit'
    # no atomics, a fixed order of the sums: a second call gives the same bytes
    again = call.run()
    for name in lr.NAMES:
        assert got[name].tobytes() == again[name].tobytes(), name


def test_no_frames_launches_nothing():
    from libertem_amd import hip
    c = lr.make_case('p7', 0, True, True, {}, 1)
    before = hip.lattice_last_kernel()
    got = Call(c).run()
    assert got['zero'].shape == (0, 2) and got['selector'].shape == (0, 7)
    assert hip.lattice_last_kernel() == before
    # no peaks: nothing is launched either, the results stay as they were
    c = lr.make_case('p7', 4, True, True, {}, 1)
    call = Call(c)
    image = {name: region.result() for name, region in call.out.items()}
    got = call.run(n_peaks=0)
    for name in ('zero', 'a', 'b', 'selector'):
        assert np.array_equal(got[name], image[name]), name


def test_error_codes():
    from libertem_amd import hip
    case = lr.KERNEL_CASES[4]
    c = lr.kernel_case(case)
    call = Call(c)
    for kw in (dict(n_frames=-1), dict(n_peaks=-1), dict(tolerance=-0.5), dict(tolerance=float('nan'))):
        with pytest.raises(ValueError, match=r'code -3'):
            call.run(**kw)
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            start = c['start'].copy()
            start[k] = bad
            with pytest.raises(ValueError, match=r'not finite.*code -3'):
                call.run(start=start)
    for name in ('refineds_ptr', 'indices_ptr', 'start', 'zero_ptr', 'a_ptr', 'b_ptr', 'selector_ptr', 'error_ptr'):
        with pytest.raises(ValueError, match=r'null.*code -1'):
            call.run(**{name: None})
    # nothing of that reached the results (their poison is intact), and a good call afterwards passes
    for name, region in call.out.items():
        guarded.unchanged(region, name)
    check(call.run(), c, lr.case_reference(c))
    assert hip.lattice_last_kernel() == 'k_lattice_fit'


def test_on_another_stream():
    c = lr.kernel_case(lr.KERNEL_CASES[6])
    call = Call(c)
    stream = torch.cuda.Stream()
    got = call.run(stream=stream)
    check(got, c, lr.case_reference(c))
    default = Call(c).run()
    for name in lr.NAMES:
        assert got[name].tobytes() == default[name].tobytes(), name
