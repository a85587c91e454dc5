"""
run_pca on the MI355X: StdDevUDF, ApplyMasksUDF and WeightedSumUDF on the device against the exact float64 SVD of
tests/pca_ref.py, with the assertions and the tolerance of tests/test_pca_cpu.py (tests/pca_checks.py).  `-m gpu` only.
"""
import numpy as np
import pytest

import pca_checks as pc
from libertem_amd.udf.pca import run_pca

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


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
    pc.check_result(res, pc.exact(nav, sig, use_roi, True), roi, True, f"hip {nav} x {sig} roi={use_roi}")


@pytest.mark.parametrize('nav,sig', pc.CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_pca_uncentred_matches_svd_of_the_frames(ctx, nav, sig):
    ds, _ = _dataset(ctx, nav, sig)
    res = run_pca(ctx, ds, pc.N_COMPONENTS, center=False)
    pc.check_result(res, pc.exact(nav, sig, False, False), None, False, f"hip {nav} x {sig} uncentred")


def test_pca_seed_makes_runs_identical(ctx):
    nav, sig = pc.CASES[0]
    ds, roi = _dataset(ctx, nav, sig)
    a = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi, seed=3)
    b = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi, seed=3)
    c = run_pca(ctx, ds, pc.N_COMPONENTS, roi=roi, seed=4)
    for name in ('components', 'singular_values', 'explained_variance_ratio', 'scores', 'mean'):
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert not np.array_equal(a['components'], c['components'])


def test_pca_value_errors(ctx):
    nav, sig = pc.CASES[0]
    ds, _ = _dataset(ctx, nav, sig)
    with pytest.raises(ValueError, match='exceeds'):
        run_pca(ctx, ds, 4, oversample=117)                 # 121 > 120 frames
    with pytest.raises(ValueError, match='exceeds'):
        run_pca(ctx, ds, 250, oversample=8)                 # 258 > 256 pixels
    roi = np.zeros(nav, dtype=bool)
    roi[0, :10] = True
    with pytest.raises(ValueError, match='exceeds'):
        run_pca(ctx, ds, 4, roi=roi)                        # 12 > 10 selected frames
