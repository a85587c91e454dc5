"""
CepstrumUDF on the MI355X (Context.make_with('hip')) against the float64 restatement of tests/cepstrum_ref.py, within
its bound: an 8 x 8 scan of 32 x 32 uint16 frames of a strained lattice (`strained_lattice_scan`) transformed to
(16, 16) with the default Hann window; host and device-resident data, a region of interest, a cached second run, the
kernels the plan reports; `cepstrum_dataset` leaves the cepstra in HBM as a dataset, SumUDF runs on it, and `find_peaks`
on that sum finds the lattice vectors of an unstrained scan.
"""
import numpy as np
import pytest

import cepstrum_ref as cr

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SIG = (32, 32)
NAV = (8, 8)
OUT = (16, 16)
A, B = (5, 1), (-1, 4)
N = NAV[0] * NAV[1]
OFFSET, DC = 1.0, 3.5


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def scan():
    """64 uint16 frames of a lattice strained by up to 3 %, and the float64 restatement of their cepstra"""
    from libertem_amd.utils.generate import strained_lattice_scan
    rng = np.random.default_rng(11)
    frames = strained_lattice_scan(NAV, SIG, A, B, strain=rng.uniform(-0.03, 0.03, NAV + (2, 2)))[0]
    assert frames.dtype == np.uint16 and frames.shape == NAV + SIG
    flat = frames.reshape((N,) + SIG)
    return frames, flat, cr.reference(flat, OUT, OFFSET, None, DC)


def cepstra(res, raw=False):
    return np.asarray(res['cepstrum'].raw_data if raw else res['cepstrum'].data).reshape((-1,) + OUT)


def load(ctx, frames, resident, num_partitions=2):
    from libertem_amd.common.hiparray import HipArray
    return ctx.load('memory', data=HipArray.from_numpy(frames, 0) if resident else frames,
                    num_partitions=num_partitions, sig_dims=2)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_run_cepstrum_vs_restatement(ctx, scan, resident):
    from libertem_amd.udf import run_cepstrum
    frames, flat, ref = scan
    res = run_cepstrum(ctx, load(ctx, frames, resident), OUT, offset=OFFSET, dc_radius=DC)
    assert res['cepstrum'].data.shape == NAV + OUT and res['cepstrum'].data.dtype == np.float32
    got = cepstra(res)
    cr.compare(got, ref, flat, OFFSET, None, what='udf')
    assert np.all(got[:, cr.keep(OUT, DC) == 0] == 0)


@pytest.mark.parametrize('resident', [False, True], ids=['streamed', 'resident'])
def test_roi(ctx, scan, resident):
    from libertem_amd.udf import run_cepstrum
    frames, flat, ref = scan
    roi = np.zeros(NAV, bool)
    roi[0, 1] = roi[1, 0] = roi[3, 7] = roi[4, 0] = roi[7, 6] = roi[7, 7] = True
    rows = np.flatnonzero(roi.reshape(-1))
    got = cepstra(run_cepstrum(ctx, load(ctx, frames, resident, 3), OUT, offset=OFFSET, dc_radius=DC, roi=roi), raw=True)
    assert len(got) == len(rows) == 6
    cr.compare(got, ref[rows], flat[rows], OFFSET, None, what='roi')


def test_cached_plan_same_bytes_and_kernels(ctx, scan):
    from libertem_amd.udf import CepstrumUDF, cepstrum
    frames, flat, ref = scan
    ds = load(ctx, frames, True)
    u = CepstrumUDF(OUT, offset=OFFSET, dc_radius=DC)
    first = cepstra(ctx.run_udf(dataset=ds, udf=u))
    n_plans = len(cepstrum._PLANS)
    second = cepstra(ctx.run_udf(dataset=ds, udf=u))
    assert len(cepstrum._PLANS) == n_plans
    assert first.tobytes() == second.tobytes()
    plans = [p for key, p in cepstrum._PLANS.items() if key[1:5] == SIG + OUT]
    assert plans
    for name in ('k_ceps_load<uint16>', 'hipfft_r2c', 'k_ceps_store'):
        assert any(name in p.last_kernel() for p in plans), [p.last_kernel() for p in plans]


def test_cepstrum_dataset_is_device_resident_and_feeds_sum_udf(ctx, scan):
    from libertem_amd.common.hiparray import HipArray
    from libertem_amd.udf import cepstrum_dataset, run_cepstrum
    from libertem_amd.udf.sum import SumUDF
    frames, flat, ref = scan
    ds = load(ctx, frames, True)
    cds = cepstrum_dataset(ctx, ds, OUT, offset=OFFSET, dc_radius=DC)
    assert tuple(cds.shape) == NAV + OUT and tuple(cds.shape.sig) == OUT and cds.dtype == np.float32
    assert isinstance(cds._device_array, HipArray) and cds._data is None         # in HBM, and nowhere else
    downloaded = cepstra(run_cepstrum(ctx, ds, OUT, offset=OFFSET, dc_radius=DC))
    assert np.asarray(cds._device_array).reshape((N,) + OUT).tobytes() == downloaded.tobytes()
    total = np.asarray(ctx.run_udf(dataset=cds, udf=SumUDF())['intensity'].data)
    x = downloaded.astype(np.float64)
    err = np.abs(total.astype(np.float64) - x.sum(axis=0))
    tol = N * cr.EPS32 * np.abs(x).sum(axis=0)
    print(f"SumUDF on the cepstrum dataset: largest error / tolerance = {(err[tol > 0] / tol[tol > 0]).max():.4f}")
    assert total.shape == OUT and np.all(err <= tol)


def test_find_peaks_on_the_mean_cepstrum_of_an_unstrained_scan(ctx):
    from libertem_amd.udf import cepstrum_dataset, find_peaks
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.utils.generate import strained_lattice_scan
    frames, a_n, b_n = strained_lattice_scan(NAV, SIG, A, B)
    assert np.all(a_n == A) and np.all(b_n == B)
    cds = cepstrum_dataset(ctx, load(ctx, frames, False), OUT, dc_radius=3.5)
    total = np.asarray(ctx.run_udf(dataset=cds, udf=SumUDF())['intensity'].data)
    delta = np.zeros(OUT)
    delta[OUT[0] // 2, OUT[1] // 2] = 1                              # (correlation with it leaves the frame as it is)
    peaks = find_peaks(total, delta, num_peaks=4, min_distance=3)
    found = {(int(y) - OUT[0] // 2, int(x) - OUT[1] // 2) for y, x in peaks}
    assert found == {A, (-A[0], -A[1]), B, (-B[0], -B[1])}, peaks


def test_errors_on_device(ctx, scan):
    from libertem_amd.udf import CepstrumUDF
    ds = load(ctx, scan[0], False)
    with pytest.raises(ValueError, match='out_shape'):
        ctx.run_udf(dataset=ds, udf=CepstrumUDF((33, 9)))
    with pytest.raises(ValueError, match='offset'):
        ctx.run_udf(dataset=ds, udf=CepstrumUDF(OUT, offset=0.0))
