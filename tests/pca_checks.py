"""
What tests/test_pca_cpu.py and tests/test_pca_gpu.py share: the cases, the deviations of a `run_pca` result from
the exact float64 SVD of tests/pca_ref.py, and the tolerance both files assert.

The tolerance: per quantity, ten times the largest deviation of the NumPy branch from the exact SVD over all the
cases below (DESIGN.md section 4.6k has the measured values), and no looser than 1e-3 relative for the singular
values and 1 - 1e-4 for |<v, v_ref>|.  The deviation is that of the algorithm (two power iterations on a spectrum
whose fourth value is 1.6 - 2.7 times the fifth), not of the arithmetic: a device result outside the tolerance is a
finding.
"""
import numpy as np

import pca_ref

CASES = [((12, 10), (16, 16)), ((16, 16), (32, 32))]
N_COMPONENTS = 4

#: measured on the NumPy branch (n_iter = 2, all cases x roi x center): the largest deviation seen per quantity ...
MEASURED = {'singular_values': 2.42e-6, 'explained_variance_ratio': 4.83e-6, 'reconstruction': 7.79e-5,
            'dot': 2.88e-7}
#: ... and ten times that: relative for the singular values, the explained variance ratios and the rank-4
#: reconstruction (in its own norm); 1 - |<v, v_ref>| for every component
TOL = {name: 10.0 * seen for name, seen in MEASURED.items()}
assert max(TOL['singular_values'], TOL['explained_variance_ratio'], TOL['reconstruction']) <= 1e-3
assert TOL['dot'] <= 1e-4


def make_case(nav, sig):
    """-> (frames nav + sig uint16, roi nav bool): the same in every process"""
    from libertem_amd.utils.generate import mixed_phase_scan
    frames, _, _ = mixed_phase_scan(nav, sig, n_phases=N_COMPONENTS, seed=0)
    roi = np.random.default_rng(5).random(nav) > 0.3
    return frames, roi


_exact = {}


def exact(nav, sig, use_roi, center):
    """the exact PCA of a case, computed once per process; asserts that the case is well-posed"""
    key = (nav, sig, use_roi, center)
    if key not in _exact:
        frames, roi = make_case(nav, sig)
        x = frames.reshape((-1,) + sig)
        if use_roi:
            x = x[roi.reshape(-1)]
        ex = pca_ref.exact_pca(x, N_COMPONENTS, center=center)
        s = ex['all_singular_values']
        assert (s[:N_COMPONENTS] >= 1.3 * s[1:N_COMPONENTS + 1]).all(), s[:N_COMPONENTS + 1]
        _exact[key] = ex
    return _exact[key]


def deviations(res, ex, roi, center):
    """-> dict of the four deviations of a run_pca result from the exact one"""
    k = N_COMPONENTS
    sig = ex['mean'].shape
    comps = np.asarray(res['components'], dtype=np.float64).reshape((k, -1))
    ref = ex['components'].reshape((k, -1))
    scores = np.asarray(res['scores'], dtype=np.float64).reshape((-1, k))
    if roi is not None:
        outside = ~roi.reshape(-1)
        assert np.isnan(scores[outside]).all()
        scores = scores[~outside]
    assert np.isfinite(scores).all()
    recon = scores @ comps + (np.asarray(res['mean'], dtype=np.float64).reshape(-1)[None, :] if center else 0.0)
    trunc = ex['truncated'].reshape((scores.shape[0], -1))
    return {
        'singular_values': float(np.max(np.abs(res['singular_values'] - ex['singular_values'])
                                        / ex['singular_values'])),
        'dot': float(np.max(1.0 - np.abs((comps * ref).sum(axis=1)))),
        'explained_variance_ratio': float(np.max(np.abs(res['explained_variance_ratio']
                                                        - ex['explained_variance_ratio'])
                                                 / ex['explained_variance_ratio'])),
        'reconstruction': float(np.linalg.norm(recon - trunc) / np.linalg.norm(trunc)),
        'mean': float(np.max(np.abs(np.asarray(res['mean']).reshape(sig) - ex['mean']))),
    }


def check_result(res, ex, roi, center, what):
    """the assertions both files make on one result"""
    k = N_COMPONENTS
    dev = deviations(res, ex, roi, center)
    print(f"{what}: " + ', '.join(f"{name} {v:.3g}" for name, v in dev.items()))
    for name, tol in TOL.items():
        assert dev[name] <= tol, (what, name, dev)
    assert dev['mean'] <= 1e-9 * max(1.0, float(np.abs(ex['mean']).max())), (what, dev)
    comps = np.asarray(res['components'])
    assert comps.dtype == np.float32 and np.asarray(res['scores']).dtype == np.float32
    flat = comps.reshape((k, -1))
    # unit rows; the entry of largest magnitude positive, in the result and (by construction) in the reference
    assert np.allclose(np.linalg.norm(flat.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (flat[np.arange(k), np.argmax(np.abs(flat), axis=1)] > 0).all()
    # the scores carry the same sign as the reference's
    scores = np.asarray(res['scores'], dtype=np.float64).reshape((-1, k))
    scores = scores[roi.reshape(-1)] if roi is not None else scores
    assert ((scores * ex['scores']).sum(axis=0) > 0).all()
    return dev
