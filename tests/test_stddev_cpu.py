"""
StdDevUDF without a GPU: the NumPy branch on the CPU executor against the reference's results
(tests/golden/stddev.npz, generate_stddev_golden.py), merge == merge_all, run_stddev /
consolidate_result, SDAnalysis, the `libertem.udf.stddev` alias, and gloo-sharded runs.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import stddev_recipes
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.stddev import StdDevUDF, run_stddev, consolidate_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('sum', 'varsum', 'num_frames', 'var', 'std', 'mean')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'stddev.npz'))


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


def load_case(ctx, case):
    """-> (dataset, roi, corrections) of a golden case"""
    from libertem_amd.io.corrections import CorrectionSet
    data, roi, corr = stddev_recipes.make_stddev_case(case)
    ds = ctx.load('memory', data=data, num_partitions=case['num_partitions'], sig_dims=2,
                  tileshape=case.get('tileshape'), sync_offset=case.get('sync_offset', 0))
    corrections = None if corr is None else CorrectionSet(dark=corr[0], gain=corr[1])
    return ds, roi, corrections


def check_golden(res, golden, name, rtol=1e-12):
    for k in KEYS:
        got, exp = np.asarray(res[k].data), golden[f'{name}__{k}']
        assert got.dtype == exp.dtype, (k, got.dtype, exp.dtype)
        assert got.shape == exp.shape, (k, got.shape, exp.shape)
        if k == 'num_frames':
            assert np.array_equal(got, exp)
            continue
        # base dtype float32: the reference rounds every merge to float32 (and var / std / mean
        # inherit that)
        tol = 1e-5 if golden[f'{name}__varsum'].dtype == np.float32 else rtol
        scale = np.abs(exp).max()
        assert np.allclose(got, exp, rtol=tol, atol=tol * scale), (k, np.abs(got - exp).max(), scale)


@pytest.mark.parametrize('case', stddev_recipes.STDDEV_CASES, ids=lambda c: c['name'])
def test_numpy_branch_vs_golden(ctx, golden, case):
    data, _, _ = stddev_recipes.make_stddev_case(case)
    import hashlib
    assert hashlib.sha256(np.ascontiguousarray(data).tobytes()).digest() == \
        golden[case['name'] + '__sha_data'].tobytes()
    ds, roi, corrections = load_case(ctx, case)
    res = ctx.run_udf(dataset=ds, udf=StdDevUDF(**case.get('udf_kwargs', {})), roi=roi,
                      corrections=corrections)
    check_golden(res, golden, case['name'])


def test_sync_offset_counts_only_existing_frames(ctx):
    data = np.random.default_rng(3).integers(0, 500, (6, 6, 8, 8)).astype(np.uint16)
    flat = data.reshape((36, -1)).astype(np.float64)
    for off, sel in ((3, flat[3:]), (-3, flat[:33])):
        ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2, sync_offset=off)
        res = ctx.run_udf(dataset=ds, udf=StdDevUDF())
        assert res['num_frames'].data[0] == 33
        assert np.allclose(res['var'].data.reshape(-1), sel.var(axis=0), rtol=1e-12)
        assert np.allclose(res['mean'].data.reshape(-1), sel.mean(axis=0), rtol=1e-12)


def _part(n, s, v):
    from libertem_amd.udf.base import MergeAttrMapping
    return MergeAttrMapping({'num_frames': np.array([n], dtype=np.int64), 'sum': s, 'varsum': v})


def test_merge_equals_merge_all():
    rng = np.random.default_rng(11)
    frames = rng.normal(50., 3., (40, 5, 6))
    bounds = [0, 7, 7, 19, 33, 40]              # one empty partition
    parts = {}
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        chunk = frames[a:b]
        s = chunk.sum(axis=0) if b > a else np.zeros((5, 6))
        v = ((chunk - chunk.mean(axis=0)) ** 2).sum(axis=0) if b > a else np.zeros((5, 6))
        parts[i] = _part(b - a, s, v)
    udf = StdDevUDF()
    dest = _part(0, np.zeros((5, 6)), np.zeros((5, 6)))
    for p in parts.values():
        udf.merge(dest, p)
    allm = udf.merge_all(parts)
    assert int(dest.num_frames[0]) == allm['num_frames'] == 40
    assert np.array_equal(dest.sum, allm['sum'])
    assert np.array_equal(dest.varsum, allm['varsum'])
    assert np.allclose(allm['varsum'] / 40, frames.var(axis=0), rtol=1e-12)


def test_empty_partition_merges_as_identity():
    udf = StdDevUDF()
    s, v = np.arange(6.).reshape(2, 3), np.ones((2, 3))
    dest = _part(4, s.copy(), v.copy())
    udf.merge(dest, _part(0, np.full((2, 3), 99.), np.full((2, 3), 99.)))
    assert int(dest.num_frames[0]) == 4
    assert np.array_equal(dest.sum, s) and np.array_equal(dest.varsum, v)


def test_run_stddev_consolidate(ctx, golden):
    case = stddev_recipes.STDDEV_CASES[0]
    ds, _, _ = load_case(ctx, case)
    res = run_stddev(ctx, ds)
    assert set(res) == set(KEYS)
    assert res['num_frames'] == golden['u16__num_frames'][0]
    for k in ('sum', 'varsum', 'var', 'std', 'mean'):
        assert isinstance(res[k], np.ndarray)
        assert np.allclose(res[k], golden[f'u16__{k}'], rtol=1e-12)
    again = consolidate_result(ctx.run_udf(dataset=ds, udf=StdDevUDF(use_numba=False)))
    assert np.array_equal(again['var'], res['var'])


def test_reused_udf_object_restarts_counters(ctx):
    ds, _, _ = load_case(ctx, stddev_recipes.STDDEV_CASES[0])
    udf = StdDevUDF()
    r1 = ctx.run_udf(dataset=ds, udf=udf)
    r2 = ctx.run_udf(dataset=ds, udf=udf)
    assert r1['num_frames'].data[0] == r2['num_frames'].data[0] == 42
    assert np.array_equal(r1['varsum'].data, r2['varsum'].data)


def test_sd_analysis(ctx, golden):
    from libertem_amd.analysis import SDAnalysis
    ds, _, _ = load_case(ctx, stddev_recipes.STDDEV_CASES[0])
    res = ctx.run(SDAnalysis(dataset=ds, parameters={}))
    assert np.allclose(res.intensity.raw_data, golden['u16__std'], rtol=1e-12)
    assert np.allclose(res.intensity_lin.raw_data, golden['u16__std'], rtol=1e-12)
    # ROI from the analysis parameters (getroi.get_roi)
    from libertem_amd.analysis.getroi import get_roi
    params = {'roi': {'shape': 'rect', 'x': 1, 'y': 2, 'width': 3, 'height': 2}}
    roi_res = ctx.run(SDAnalysis(dataset=ds, parameters=params))
    roi = get_roi(params, ds.shape.nav)
    data, _, _ = stddev_recipes.make_stddev_case(stddev_recipes.STDDEV_CASES[0])
    sel = data[roi].reshape((int(roi.sum()), -1)).astype(np.float64)
    assert 0 < len(sel) < 42
    assert np.allclose(roi_res.intensity.raw_data.reshape(-1), sel.std(axis=0), rtol=1e-12)


def test_compat_alias():
    code = ("import libertem_amd.compat as c; c.install(); "
            "from libertem.udf.stddev import StdDevUDF, run_stddev, consolidate_result; "
            "import libertem_amd.udf.stddev as m; assert StdDevUDF is m.StdDevUDF; "
            "from libertem.analysis.sd import SDAnalysis; print('ok')")
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('world', [2, 3])
def test_gloo_sharded_stddev(tmp_path, ctx, world):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           f'--nproc-per-node={world}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()),
           os.path.join(ROOT, 'tests', 'dist_worker_stddev.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    # single-process result of the same run
    rng = np.random.default_rng(77)
    data = rng.integers(0, 3000, (7, 9, 12, 13)).astype(np.uint16)
    roi = rng.random((7, 9)) > 0.5
    ds = ctx.load('memory', data=data, num_partitions=7, sig_dims=2)
    single = ctx.run_udf(dataset=ds, udf=StdDevUDF())
    single_roi = ctx.run_udf(dataset=ds, udf=StdDevUDF(), roi=roi)
    for k in range(world):
        o = np.load(os.path.join(tmp_path, f'rank{k}.npz'))
        for key in KEYS:
            assert np.array_equal(o[key], np.asarray(single[key].data)), (k, key)
        for key in ('sum', 'varsum', 'num_frames'):
            assert np.array_equal(o['roi_' + key], np.asarray(single_roi[key].data)), (k, key)
