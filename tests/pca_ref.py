"""
Float64 restatements of WeightedSumUDF and run_pca for the tests, index-plain and without a call into the
package: the weighted sum as a loop over the frames, the exact PCA as the SVD of the (centred) frame matrix.
"""
import numpy as np


def weighted_sum(frames, weights):
    """frames (n, sy, sx), weights (n, k) -> (wsum (k, sy, sx), bound (k, sy, sx)): wsum[c] = sum_n w[n, c] x[n]
    and sum_n |w[n, c]| |x[n]|, both accumulated frame by frame in float64"""
    frames = np.asarray(frames)
    weights = np.asarray(weights, dtype=np.float64)
    n, k = weights.shape
    total = np.zeros((k,) + frames.shape[1:], dtype=np.float64)
    bound = np.zeros_like(total)
    for i in range(n):
        x = frames[i].astype(np.float64)
        for c in range(k):
            total[c] += weights[i, c] * x
            bound[c] += abs(weights[i, c]) * np.abs(x)
    return total, bound


def flip_signs(components, scores):
    """the entry of largest magnitude of every component positive, the scores flipped with it (in place)"""
    for c in range(components.shape[0]):
        flat = components[c].reshape(-1)
        if flat[np.argmax(np.abs(flat))] < 0:
            components[c] *= -1.0
            scores[:, c] *= -1.0
    return components, scores


def exact_pca(frames, n_components, center=True):
    """frames (n, sy, sx) -> dict of the exact PCA by np.linalg.svd of the float64 matrix (n, P), centred over the
    frames if `center`: 'components' (k, sy, sx), 'singular_values' (k,), 'all_singular_values',
    'explained_variance_ratio' (k,), 'scores' (n, k), 'mean' (sy, sx), 'truncated' (n, sy, sx): the rank-k part
    plus the mean"""
    frames = np.asarray(frames)
    n = frames.shape[0]
    sig = frames.shape[1:]
    x = frames.reshape((n, -1)).astype(np.float64)
    mean = x.mean(axis=0)
    xc = x - mean[None, :] if center else x
    u, s, vt = np.linalg.svd(xc, full_matrices=False)
    k = int(n_components)
    components = vt[:k].copy()
    scores = u[:, :k] * s[None, :k]
    flip_signs(components, scores)
    total = float((xc * xc).sum())
    truncated = scores @ components + (mean[None, :] if center else 0.0)
    return {
        'components': components.reshape((k,) + sig),
        'singular_values': s[:k].copy(),
        'all_singular_values': s,
        'explained_variance_ratio': s[:k] ** 2 / total,
        'scores': scores,
        'mean': mean.reshape(sig),
        'truncated': truncated.reshape((n,) + sig),
    }
