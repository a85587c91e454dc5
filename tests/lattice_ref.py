"""
Ground truth of the lattice-fit tests: the definition of LatticeRefineUDF's fit restated frame
by frame in float64 NumPy -- a least-squares call on sqrt(w)-scaled rows, sharing no code with
`libertem_amd.udf.lattice.fit_lattice` --, a seeded case maker, the case table of the kernel tests, the tolerance they
share and the scan of the UDF tests.

Definition, per frame, for positions r_k, weights w_k (1 if None), index pairs (i_k, j_k), start = (zero0, a0, b0), tol:
    p_k = zero0 + i_k a0 + j_k b0
    selector[k] = r_k finite, w_k finite, w_k > 0, |r_k - p_k|_2 <= tol (and peak_values[k] finite where given)
    a fit exists iff the selected index pairs are not collinear (exact, on the integers)
    zero, a, b = argmin sum_sel w_k |zero + i_k a + j_k b - r_k|^2;  error = sqrt(sum_sel w_k |res_k|^2 / sum_sel w_k)
    no fit: zero, a, b, error NaN
"""
import numpy as np

import correlation_ref as cr

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
NAMES = ('zero', 'a', 'b', 'selector', 'error')
START = np.array([24.3, 23.6, 0.4, 10.2, 9.8, -0.3])          # zero0, a0, b0 as (y, x)
TOL = 2.5


def reference(refineds, weights, peak_values, indices, start, tol):
    """-> dict: zero, a, b (n, 2), error (n,) float64, selector (n, P) bool; and what the tolerances are derived
    from: kappa (n,) = condition number of the weighted normal matrix M^T W M, G (n, 3, P) = (M^T W M)^-1 M^T W,
    H (n, 3, P) = (M^T W M)^-1 M^T (columns of unselected peaks 0), res (n,) = largest |res_k| of the frame;
    NaN / 0 where no fit exists."""
    r = np.asarray(refineds, dtype=np.float32).astype(np.float64)
    n, n_peaks = r.shape[:2]
    idx = [(int(i), int(j)) for i, j in np.asarray(indices)]
    start = np.asarray(start, dtype=np.float64)
    zero0, a0, b0 = start[0:2], start[2:4], start[4:6]
    out = {'zero': np.full((n, 2), np.nan), 'a': np.full((n, 2), np.nan), 'b': np.full((n, 2), np.nan),
           'error': np.full(n, np.nan), 'selector': np.zeros((n, n_peaks), bool), 'kappa': np.full(n, np.nan),
           'G': np.zeros((n, 3, n_peaks)), 'H': np.zeros((n, 3, n_peaks)), 'res': np.zeros(n),
           'dist': np.full((n, n_peaks), np.nan)}
    for f in range(n):
        w = np.ones(n_peaks)
        if weights is not None:
            w = np.asarray(weights[f], dtype=np.float32).astype(np.float64)
        chosen = []
        for k, (i, j) in enumerate(idx):
            p = zero0 + i * a0 + j * b0
            with np.errstate(all='ignore'):
                dist = float(np.sqrt(((r[f, k] - p) ** 2).sum()))
            out['dist'][f, k] = dist
            ok = bool(np.isfinite(r[f, k]).all() and np.isfinite(w[k]) and w[k] > 0 and dist <= tol)
            if peak_values is not None:
                ok = ok and bool(np.isfinite(peak_values[f][k]))
            if ok:
                chosen.append(k)
        out['selector'][f, chosen] = True
        if not chosen:
            continue
        i0, j0 = idx[chosen[0]]
        others = [k for k in chosen if idx[k] != (i0, j0)]
        if not others:
            continue
        i1, j1 = idx[others[0]][0] - i0, idx[others[0]][1] - j0
        if not any((idx[k][0] - i0) * j1 - (idx[k][1] - j0) * i1 != 0 for k in chosen):         # (Python integers)
            continue
        m = np.array([(1., idx[k][0], idx[k][1]) for k in chosen])
        wk, rk = w[chosen], r[f, chosen]
        sw = np.sqrt(wk)[:, None]
        x = np.linalg.lstsq(m * sw, rk * sw, rcond=None)[0]
        res = m @ x - rk
        out['zero'][f], out['a'][f], out['b'][f] = x
        out['error'][f] = np.sqrt((wk * (res ** 2).sum(axis=1)).sum() / wk.sum())
        normal = m.T @ (wk[:, None] * m)
        inv = np.linalg.inv(normal)
        out['kappa'][f] = np.linalg.cond(normal)
        out['H'][f][:, chosen] = inv @ m.T
        out['G'][f][:, chosen] = inv @ m.T * wk[None]
        out['res'][f] = np.sqrt((res ** 2).sum(axis=1)).max()
    return out


def largest(refineds):
    """max|refineds| over the finite ones"""
    r = np.abs(np.asarray(refineds, dtype=np.float64))
    return float(r[np.isfinite(r)].max())


def value_tolerance(ref, refineds):
    """per frame (n, 1): eps32 |ref| is added by the caller; this is 16 kappa P eps64 max|refineds| -- the float64
    solve, 16 the allowance for the constants of the elimination"""
    n_peaks = np.asarray(refineds).shape[1]
    return (16 * ref['kappa'] * n_peaks * EPS64 * largest(refineds))[:, None]


def compare(got, ref, refineds):
    """selector equal; NaN pattern equal; zero, a, b, error within eps32 |ref| + 16 kappa P eps64 max|refineds|.
    -> the largest error / tolerance"""
    assert np.array_equal(np.asarray(got['selector']).astype(bool), ref['selector'])
    solve = value_tolerance(ref, refineds)
    worst = 0.
    for name in ('zero', 'a', 'b', 'error'):
        g = np.asarray(got[name], dtype=np.float64).reshape((len(ref['kappa']), -1))
        e = ref[name].reshape(g.shape)
        assert np.array_equal(np.isnan(g), np.isnan(e)), name
        fit = ~np.isnan(e)
        lim = EPS32 * np.abs(e) + solve
        ratio = np.abs(g - e)[fit] / lim[fit]
        if ratio.size:
            print(f"lattice: largest {name} error / tolerance = {ratio.max():.3g}")
            assert ratio.max() <= 1, (name, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    return worst


# ---- the kernel cases ----------------------------------------------------------------------------------------------
def _grid(i_range, j_range):
    return np.array([(i, j) for i in range(*i_range) for j in range(*j_range)], dtype=np.int32)


INDEX_SETS = {
    'p1': np.array([(0, 0)], np.int32),
    'p2': np.array([(0, 0), (1, 0)], np.int32),
    'p3-line': np.array([(0, 0), (1, 1), (2, 2)], np.int32),
    'p3-span': np.array([(0, 0), (1, 0), (0, 1)], np.int32),
    'p7': _grid((-1, 2), (-1, 2))[:7],
    'p64': _grid((-4, 4), (-4, 4)),
    'p65': _grid((-6, 7), (-2, 3)),
    'p130': _grid((-6, 7), (-5, 5)),
}


def _spanning_three(idx):
    """the three peaks nearest the index origin that span the plane (a well-conditioned 3-point fit)"""
    order = sorted(range(len(idx)), key=lambda k: (abs(int(idx[k][0])) + abs(int(idx[k][1])), k))
    k0, k1 = order[0], order[1]
    d1 = idx[k1].astype(np.int64) - idx[k0]
    for k in order[2:]:
        d = idx[k].astype(np.int64) - idx[k0]
        if d[0] * d1[1] - d[1] * d1[0] != 0:
            return [k0, k1, k]
    raise ValueError("the index set is collinear")


def make_case(index_set, n_frames, weighted, with_values, special, seed):
    """-> dict(refineds (n, P, 2) f32, weights (n, P) f32 | None, peak_values (n, P) f32 | None, indices, start, tol).
    A true lattice per frame: the start lattice strained by up to 2 % (less for wide index sets: at most ~0.6 px at the
    farthest peak) and shifted by up to 0.5 px; positions with N(0, 0.05) noise; about one peak in ten an outlier
    moved by 3-6 px; weights uniform in [1, 20]; a few entries NaN, 0 or negative.  special: {frame: 'reject_all' |
    'three' (exactly the three spanning peaks nearest the origin survive) | 'collinear' (only one lattice row of
    three or more peaks survives)}."""
    rng = np.random.default_rng(seed)
    idx = INDEX_SETS[index_set]
    n_peaks = len(idx)
    zero0, a0, b0 = START[0:2], START[2:4], START[4:6]
    reach = max(1., float(np.abs(idx[:, :1] * a0[None] + idx[:, 1:] * b0[None]).sum(axis=1).max()))
    strain = min(0.02, 0.6 / reach)
    r = np.zeros((n_frames, n_peaks, 2))
    for f in range(n_frames):
        e = np.eye(2) + rng.uniform(-strain, strain, (2, 2))
        shift = rng.uniform(-0.5, 0.5, 2)
        r[f] = zero0 + shift + idx[:, :1] * (e @ a0)[None] + idx[:, 1:] * (e @ b0)[None]
    r += rng.normal(0., 0.05, r.shape)
    outlier = rng.random((n_frames, n_peaks)) < 0.1
    for f, what in special.items():
        if what == 'reject_all':
            outlier[f] = True
        elif what == 'three':
            outlier[f] = True
            outlier[f, _spanning_three(idx)] = False
        elif what == 'collinear':
            outlier[f] = idx[:, 1] != idx[0, 1]
            assert (~outlier[f]).sum() >= 3
    angle = rng.uniform(0, 2 * np.pi, (n_frames, n_peaks))
    length = np.where(outlier, rng.uniform(3., 6., (n_frames, n_peaks)), 0.)
    for f, what in special.items():
        length[f] = np.where(outlier[f], 8., 0.)               # (well outside the tolerance, whatever the direction)
    r += length[..., None] * np.stack([np.sin(angle), np.cos(angle)], axis=-1)
    r = r.astype(np.float32)
    weights = rng.uniform(1., 20., (n_frames, n_peaks)).astype(np.float32) if weighted else None
    values = rng.uniform(5., 50., (n_frames, n_peaks)).astype(np.float32) if with_values else None
    # a few damaged entries, away from the special frames (a set of three peaks or fewer keeps every second frame whole)
    plain = [f for f in range(n_frames) if f not in special and (n_peaks > 3 or f % 2)]
    for n_hit, f in enumerate(plain):
        k = (3 * n_hit + 1) % n_peaks
        r[f, k, n_hit % 2] = np.nan if n_hit % 3 else np.inf
        if weights is not None:
            weights[f, (k + 1) % n_peaks] = (np.nan, 0., -3.)[n_hit % 3]
            weights[f, (k + 2) % n_peaks] = np.inf if n_hit % 2 else -0.
        if values is not None:
            values[f, (k + 3) % n_peaks] = np.nan
    return dict(refineds=r, weights=weights, peak_values=values, indices=idx, start=START.copy(), tol=TOL)


# (id, index set, n_frames, weighted, peak_values given, special frames, seed): P in {1, 2, 3 collinear, 3 spanning, 7,
# 64, 65, 130} -- below, at and above one wave's 64 lanes --; 1, 4, 5 and 9 frames -- a partial workgroup of four waves,
# a full one, a second and a third one.  The seeds are picked so that no position lies within 1e-3 px of the
# tolerance: tests/test_lattice_cpu.py checks that, in float64, on the CPU.
KERNEL_CASES = [
    ('p1', 'p1', 1, True, False, {}, 1),
    ('p2', 'p2', 4, True, True, {}, 2),
    ('p3-line', 'p3-line', 5, False, True, {}, 3),
    ('p3-span', 'p3-span', 9, True, False, {}, 4),
    ('p7-weighted', 'p7', 5, True, True, {1: 'reject_all', 3: 'three'}, 5),
    ('p7-plain', 'p7', 4, False, False, {2: 'collinear'}, 6),
    ('p64', 'p64', 9, True, False, {0: 'three', 4: 'collinear', 8: 'reject_all'}, 7),
    ('p65', 'p65', 5, False, True, {1: 'collinear', 4: 'three'}, 8),
    ('p130', 'p130', 9, True, True, {2: 'three', 5: 'collinear', 7: 'reject_all'}, 9),
    ('p130-plain', 'p130', 1, False, False, {}, 10),
]


def kernel_case(case):
    _, index_set, n_frames, weighted, with_values, special, seed = case
    return make_case(index_set, n_frames, weighted, with_values, special, seed)


def case_reference(c):
    return reference(c['refineds'], c['weights'], c['peak_values'], c['indices'], c['start'], c['tol'])


# ---- the scan of the UDF tests -------------------------------------------------------------------------------------
SIG = (48, 48)
NAV = (4, 5)
ZERO, A, B = (24., 24.), (0., 10.), (10., 0.)
INDICES = np.concatenate([_grid((-1, 2), (-1, 2)), np.array([(2, -2)], np.int32)])     # (2, -2) -> (4, 44): clipped
R, Q = 4, 1
UDF_TOL = 2.4


def lattice_positions(zero, a, b, indices=INDICES):
    zero, a, b = (np.asarray(v, dtype=np.float64) for v in (zero, a, b))
    return zero[None] + indices[:, :1] * a[None] + indices[:, 1:] * b[None]


def make_scan(seed=1, dtype='uint16'):
    """20 frames of 48 x 48 from correlation_ref.make_frames, one call per frame: its disks sit at the integer
    positions of that frame's own lattice -- the start lattice shifted by up to 1.5 px and strained by up to 5 %
    (0.5 px at the nearest neighbours, 2 px at the far peak) -- with no per-peak shift (r = 1); every second frame is blurred by a common
    fractional shift.  -> frames (20, 48, 48), the per-frame true positions (20, P, 2).
    The seed is picked so that no (frame, peak) pair lies below the gap of correlation_ref.compare and no refined
    position within 0.05 px of UDF_TOL, which rejects 6 of the 200 pairs: tests/test_lattice_cpu.py checks both."""
    rng = np.random.default_rng(seed)
    frames, true = [], []
    for f in range(NAV[0] * NAV[1]):
        e = np.eye(2) + rng.uniform(-0.05, 0.05, (2, 2))
        shift = rng.uniform(-1.5, 1.5, 2)
        pos = lattice_positions(np.array(ZERO) + shift, e @ np.array(A), e @ np.array(B))
        peaks = np.clip(np.rint(pos), 0, np.array(SIG) - 1).astype(np.int64)
        fr, _, frac = cr.make_frames(SIG, peaks, 1, 1, seed=1000 * seed + f, dtype=dtype, n_blurred=f % 2)
        frames.append(fr[0])
        true.append(peaks + frac[0][None])
    return np.stack(frames), np.stack(true)
