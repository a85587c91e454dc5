"""
WeightedSumUDF without a GPU: the NumPy branch on the inline executor against the float64 loop of tests/pca_ref.py,
the ways to pass the weights, the ROI slicing of the weights, wide frames (float64, int64), a tileshape that cuts
the frames, merge == merge_all, and a gloo-sharded run (world size 2: 'wsum' merges by 'sum' across the ranks).
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import pca_ref
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.base import MergeAttrMapping
from libertem_amd.udf.weightedsum import WeightedSumUDF, nav_weights, run_weighted_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAV, SIG = (6, 7), (16, 16)


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


def _case(dtype, k, seed=21):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 4096, NAV + SIG).astype(dtype)
    return data, rng.standard_normal(NAV + (k,)).astype(np.float32)


def _check(got, data, w, roi=None):
    """the NumPy branch adds float64 tile products into the float32 buffer: one rounding per tile and merge"""
    x = data.reshape((-1,) + SIG)
    w = w.reshape((x.shape[0], -1))
    if roi is not None:
        x, w = x[roi.reshape(-1)], w[roi.reshape(-1)]
    ref, bound = pca_ref.weighted_sum(x, w)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert (np.abs(got.astype(np.float64) - ref) <= 1e-5 * bound + 1e-30).all()


@pytest.mark.parametrize('dtype', ['uint16', 'float32', 'float64', 'int64'])
@pytest.mark.parametrize('k', [1, 5, 70])
def test_wsum_numpy_against_the_loop(ctx, dtype, k):
    data, w = _case(dtype, k)
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    res = run_weighted_sum(ctx, ds, w)
    assert res['wsum'].data.shape == (k,) + SIG
    _check(res['wsum'].data, data, w)


def test_wsum_numpy_roi_slices_the_weights(ctx):
    data, w = _case('uint16', 4)
    roi = np.random.default_rng(22).random(NAV) > 0.4
    roi.reshape(-1)[14:28] = False                       # the second of three partitions is empty
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    _check(run_weighted_sum(ctx, ds, w, roi=roi)['wsum'].data, data, w, roi)
    aux = WeightedSumUDF.aux_data(w.reshape((-1, 4)), kind='nav', extra_shape=(4,), dtype='float32')
    as_aux = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(aux), roi=roi)['wsum'].data
    assert np.array_equal(as_aux, run_weighted_sum(ctx, ds, w, roi=roi)['wsum'].data)


def test_wsum_numpy_one_map_and_flat_weights(ctx):
    data, w = _case('uint16', 3)
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    one = run_weighted_sum(ctx, ds, w[..., 0])['wsum'].data
    assert one.shape == (1,) + SIG
    _check(one, data, w[..., :1])
    flat = run_weighted_sum(ctx, ds, w.reshape((-1, 3)))['wsum'].data
    assert np.array_equal(flat, run_weighted_sum(ctx, ds, w)['wsum'].data)
    aux1 = WeightedSumUDF.aux_data(w[..., 0].reshape(-1), kind='nav', dtype='float32')
    assert np.array_equal(ctx.run_udf(dataset=ds, udf=WeightedSumUDF(aux1))['wsum'].data, one)


def test_nav_weights_shapes():
    assert nav_weights(np.ones((6, 7)), (6, 7)).shape == (42, 1)
    assert nav_weights(np.ones(42), (6, 7)).shape == (42, 1)
    assert nav_weights(np.ones((6, 7, 3)), (6, 7)).shape == (42, 3)
    assert nav_weights(np.ones((42, 3), dtype=np.float64), (6, 7)).dtype == np.float32
    for bad in (np.ones((5, 7, 2)), np.ones((6, 7, 3, 1)), np.ones(41)):
        with pytest.raises(ValueError):
            nav_weights(bad, (6, 7))
    with pytest.raises(TypeError):
        nav_weights(np.ones((6, 7), dtype=np.complex64), (6, 7))


def test_wsum_refuses_complex_frames_and_cut_frames(ctx):
    w = _case('uint16', 2)[1]
    ds = ctx.load('memory', data=np.ones(NAV + SIG, dtype=np.complex64), num_partitions=3, sig_dims=2)
    with pytest.raises(NotImplementedError, match='complex64'):
        run_weighted_sum(ctx, ds, w)
    ds = ctx.load('memory', data=np.ones(NAV + SIG, dtype=np.uint16), num_partitions=3, sig_dims=2,
                  tileshape=(3, 4, 16))
    with pytest.raises(ValueError, match='whole frames'):
        run_weighted_sum(ctx, ds, w)


def test_wsum_merge_equals_merge_all():
    rng = np.random.default_rng(23)
    parts = {i: MergeAttrMapping({'wsum': rng.normal(100., 30., (3, 5, 6)).astype(np.float32)}) for i in range(7)}
    udf = WeightedSumUDF(np.ones((2, 2, 3), dtype=np.float32))
    dest = MergeAttrMapping({'wsum': np.zeros((3, 5, 6), np.float32)})
    for i in range(7):
        udf.merge(dest, parts[i])
    allm = udf.merge_all(parts)
    assert allm['wsum'].dtype == np.float32
    assert np.array_equal(dest.wsum, allm['wsum'])
    assert udf.get_dist_merge() == {'wsum': 'sum'}


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_gloo_sharded_wsum(tmp_path, ctx):
    world = 2
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           f'--nproc-per-node={world}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()),
           os.path.join(ROOT, 'tests', 'dist_worker_wsum.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    rng = np.random.default_rng(78)
    data = rng.integers(0, 3000, (7, 9, 12, 13)).astype(np.uint16)
    weights = rng.standard_normal((7, 9, 5)).astype(np.float32)
    roi = rng.random((7, 9)) > 0.5
    x = data.reshape((-1, 12, 13))
    for key, sel in (('wsum', slice(None)), ('roi_wsum', roi.reshape(-1))):
        ref, bound = pca_ref.weighted_sum(x[sel], weights.reshape((-1, 5))[sel])
        ranks = [np.load(os.path.join(tmp_path, f'rank{k}.npz'))[key] for k in range(world)]
        assert np.array_equal(ranks[0], ranks[1]), key           # every rank holds the merged result
        assert ranks[0].dtype == np.float32 and ranks[0].shape == ref.shape
        assert (np.abs(ranks[0].astype(np.float64) - ref) <= 1e-5 * bound + 1e-30).all(), key
