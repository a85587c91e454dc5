"""
run_pca without a GPU: the NumPy branches on the inline executor against the exact float64 SVD of tests/pca_ref.py
on the two mixed-phase scans of tests/pca_checks.py, and the generator itself.  tests/test_pca_gpu.py makes the same
assertions on the device.
"""
import numpy as np
import pytest

import pca_checks as pc
from libertem_amd.api import Context
from libertem_amd.udf.pca import run_pca
from libertem_amd.utils.generate import mixed_phase_scan


@pytest.fixture(scope='module')
def ctx():
    return Context.make_with('inline')


def _dataset(ctx, nav, sig):
    frames, roi = pc.make_case(nav, sig)
    return ctx.load('memory', data=frames, num_partitions=3, sig_dims=2), roi


@pytest.mark.parametrize('use_roi', [False, True], ids=['full', 'roi'])
@pytest.mark.parametrize('nav,sig', pc.CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_pca_matches_exact_svd(ctx, nav, sig, use_roi):
    ds, roi = _dataset(ctx, nav, sig)
    roi = roi if use_roi else None
    res = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi)
    assert res['components'].shape == (pc.N_COMPONENTS,) + sig
    assert res['scores'].shape == nav + (pc.N_COMPONENTS,)
    assert res['mean'].shape == sig
    assert set(res['timings']) == {'frame_passes', 'algebra'}
    pc.check_result(res, pc.exact(nav, sig, use_roi, True), roi, True, f"numpy {nav} x {sig} roi={use_roi}")


@pytest.mark.parametrize('nav,sig', pc.CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_pca_uncentred_matches_svd_of_the_frames(ctx, nav, sig):
    ds, _ = _dataset(ctx, nav, sig)
    res = run_pca(ctx, ds, pc.N_COMPONENTS, center=False)
    pc.check_result(res, pc.exact(nav, sig, False, False), None, False, f"numpy {nav} x {sig} uncentred")


def test_pca_seed_makes_runs_identical(ctx):
    nav, sig = pc.CASES[0]
    ds, roi = _dataset(ctx, nav, sig)
    a = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi, seed=3)
    b = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi, seed=3)
    c = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi, seed=4)
    for name in ('components', 'singular_values', 'explained_variance_ratio', 'scores', 'mean'):
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert not np.array_equal(a['components'], c['components'])


def test_pca_without_power_iterations_underestimates_the_tail(ctx):
    # why n_iter = 2 is the default: the plain sketch leaves the fourth singular value percents low
    nav, sig = pc.CASES[1]
    ds, _ = _dataset(ctx, nav, sig)
    ex = pc.exact(nav, sig, False, True)
    res = run_pca(ctx, ds, pc.N_COMPONENTS, n_iter=0)
    low = 1.0 - res['singular_values'] / ex['singular_values']
    assert (low > -1e-9).all() and 1e-3 < low[-1] < 0.3


def test_pca_value_errors(ctx):
    nav, sig = pc.CASES[0]
    ds, _ = _dataset(ctx, nav, sig)
    with pytest.raises(ValueError, match='exceeds'):
        run_pca(ctx, ds, 4, oversample=117)                 # 121 > 120 frames
    with pytest.raises(ValueError, match='exceeds'):
        run_pca(ctx, ds, 250, oversample=8)                 # 258 > 256 pixels (and > 120 frames)
    roi = np.zeros(nav, dtype=bool)
    roi[0, :10] = True
    with pytest.raises(ValueError, match='exceeds'):
        run_pca(ctx, ds, 4, roi=roi)                        # 12 > 10 selected frames
    with pytest.raises(ValueError):
        run_pca(ctx, ds, 0)


def test_mixed_phase_scan():
    nav, sig = (12, 10), (16, 16)
    frames, maps, patterns = mixed_phase_scan(nav, sig, n_phases=4, seed=0)
    again, _, _ = mixed_phase_scan(nav, sig, n_phases=4, seed=0)
    other, _, _ = mixed_phase_scan(nav, sig, n_phases=4, seed=1)
    assert frames.dtype == np.uint16 and frames.shape == nav + sig
    assert np.array_equal(frames, again) and not np.array_equal(frames, other)
    assert maps.shape == (4,) + nav and patterns.shape == (4,) + sig
    assert maps.min() >= 0.0 and maps.max() <= 1.0
    # smooth and mutually different abundance maps; sparse patterns on disjoint pixels; amplitudes fall 2.5 x
    c = np.corrcoef(maps.reshape((4, -1)))
    assert (np.abs(c - np.eye(4)) < 0.5).all()
    support = patterns.reshape((4, -1)) > 0
    assert (support.sum(axis=1) == 6).all() and (support.sum(axis=0) <= 1).all()
    peak = patterns.reshape((4, -1)).max(axis=1)
    assert np.allclose(peak[:-1] / peak[1:], 2.5, rtol=0.45)
    # the frames are Poisson draws about background + disk + sum_j map_j pattern_j
    # (defaults: 1 and 40): every pixel's scan average within six standard deviations of its Poisson mean
    yy, xx = np.mgrid[:16, :16]
    inside = (yy - 8) ** 2 + (xx - 8) ** 2 < (16 / 6) ** 2
    mean = 1.0 + 40.0 * inside + np.einsum('jyx,jhw->yxhw', maps, patterns).mean(axis=(0, 1))
    z = (frames.astype(np.float64).mean(axis=(0, 1)) - mean) / np.sqrt(mean / (nav[0] * nav[1]))
    assert np.abs(z).max() < 6.0
    assert mixed_phase_scan(nav, sig, dtype='float32')[0].dtype == np.float32
    with pytest.raises(ValueError):
        mixed_phase_scan(nav, (4, 4))
