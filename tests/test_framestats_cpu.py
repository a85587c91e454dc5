"""
FEMUDF and LogsumUDF without a GPU: the NumPy branch on the CPU executor against the reference's results
(tests/golden/framestats.npz, generate_framestats_golden.py), the float conversion of full-range integers,
FEM's center convention, the complex-logsum TypeError, frame-cutting tileshapes, merge == merge_all,
FEMAnalysis, the `libertem.udf.FEM` / `libertem.udf.logsum` aliases, and gloo-sharded runs.
"""
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import framestats_recipes
from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.udf.FEM import FEMUDF, run_fem, ring_mask, ring_spans
from libertem_amd.udf.logsum import LogsumUDF, run_logsum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'framestats.npz'))


@pytest.fixture(scope='module')
def ctx():
    return Context(InlineJobExecutor())


def load_case(ctx, case, **kw):
    from libertem_amd.io.corrections import CorrectionSet
    data, roi, corr = framestats_recipes.make_case(case)
    ds = ctx.load('memory', data=data, num_partitions=case['num_partitions'], sig_dims=2,
                  sync_offset=case.get('sync_offset', 0), **kw)
    corrections = None if corr is None else CorrectionSet(dark=corr[0], gain=corr[1])
    return data, ds, roi, corrections


def check(got, exp, rtol):
    got = np.asarray(got)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, got.shape, exp.dtype, exp.shape)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    scale = np.abs(exp[ok]).max() if ok.any() else 0.
    assert np.allclose(got[ok], exp[ok], rtol=rtol, atol=rtol * scale), np.abs(got[ok] - exp[ok]).max()


def _sha_ok(case, golden):
    data, _, _ = framestats_recipes.make_case(case)
    return hashlib.sha256(np.ascontiguousarray(data).tobytes()).digest() == \
        golden[case['name'] + '__sha_data'].tobytes()


@pytest.mark.parametrize('case', framestats_recipes.FEM_CASES, ids=lambda c: c['name'])
def test_fem_numpy_vs_golden(ctx, golden, case):
    assert _sha_ok(case, golden)
    _, ds, roi, corrections = load_case(ctx, case)
    udf = FEMUDF(center=case['center'], rad_in=case['rad_in'], rad_out=case['rad_out'])
    res = ctx.run_udf(dataset=ds, udf=udf, roi=roi, corrections=corrections)
    check(res['intensity'].data, golden[case['name'] + '__intensity'], 1e-5)


@pytest.mark.parametrize('case', framestats_recipes.LOGSUM_CASES, ids=lambda c: c['name'])
def test_logsum_numpy_vs_golden(ctx, golden, case):
    assert _sha_ok(case, golden)
    _, ds, roi, corrections = load_case(ctx, case)
    res = ctx.run_udf(dataset=ds, udf=LogsumUDF(), roi=roi, corrections=corrections)
    check(res['logsum'].data, golden[case['name'] + '__logsum'], 1e-5)


@pytest.mark.parametrize('dtype', ['uint8', 'int8', 'uint16', 'int16'])
def test_logsum_full_range_integers_convert_first(ctx, dtype):
    # native integer arithmetic would wrap: max - min + 1 overflows to 0 (log -> -inf) or negative (NaN)
    info = np.iinfo(dtype)
    data = np.random.default_rng(5).integers(int(info.min), int(info.max) + 1, (3, 4, 8, 8)).astype(dtype)
    data[..., 0, 0] = info.min
    data[..., 7, 7] = info.max
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2)
    got = run_logsum(ctx, ds)['logsum'].data
    f = data.reshape((12, 8, 8)).astype(np.float32)
    exp = np.log(f - f.min(axis=(1, 2), keepdims=True) + np.float32(1)).astype(np.float64).sum(axis=0)
    assert np.all(np.isfinite(got))
    assert np.allclose(got, exp, rtol=1e-6)
    assert got[7, 7] == pytest.approx(12 * np.log(np.float32(info.max) - np.float32(info.min) + 1), rel=1e-6)


def test_fem_center_is_row_column(ctx):
    # non-square frame: center[0] is the row, center[1] the column (the reference's code, not its docstring)
    sig = (12, 30)
    mask = ring_mask((3, 22), 0, 2, sig)
    # rad_in = 0 takes out the centre pixel (`<=` in both masks)
    assert not mask[3, 22] and mask[1, 22] and mask[3, 24] and not mask[22 % 12, 3]
    assert np.count_nonzero(mask) == 12
    data = np.zeros((2, 3) + sig, dtype=np.float32)
    data[..., 1, 22] = 13.
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2)
    got = run_fem(ctx, ds, center=(3, 22), rad_in=0, rad_out=2)['intensity'].data
    vals = np.zeros(12, np.float32)
    vals[0] = 13.
    assert np.allclose(got, np.std(vals), rtol=1e-6)
    swapped = run_fem(ctx, ds, center=(22, 3), rad_in=0, rad_out=2)['intensity'].data
    assert np.all(np.isnan(swapped))           # (22, 3) lies outside a 12-row frame: empty ring


def test_ring_spans_cover_the_mask():
    mask = ring_mask((7.5, 9.2), 2.5, 6.1, (16, 20))
    spans = ring_spans(mask)
    rebuilt = np.zeros_like(mask)
    for r, x0, x1 in spans:
        assert x0 < x1
        rebuilt[r, x0:x1] = True
    assert np.array_equal(rebuilt, mask)
    assert len(ring_spans(np.zeros((4, 4), bool))) == 0


def test_logsum_complex_raises_typeerror(ctx):
    data = np.ones((2, 3, 8, 8), dtype=np.complex64)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2)
    with pytest.raises(TypeError):
        ctx.run_udf(dataset=ds, udf=LogsumUDF())


@pytest.mark.parametrize('make', [lambda: LogsumUDF(), lambda: FEMUDF(center=(8, 8), rad_in=2, rad_out=6)],
                         ids=['logsum', 'fem'])
def test_frame_cutting_tileshape_raises(ctx, make):
    data = np.ones((2, 3, 16, 16), dtype=np.float32)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, tileshape=(2, 8, 16))
    with pytest.raises(ValueError, match=r'tileshape \(2, 8, 16\)'):
        ctx.run_udf(dataset=ds, udf=make())


def test_whole_frame_tiles_without_a_forced_tileshape(ctx):
    # a tile-based UDF that sets WHOLE_FRAME_TILES sees whole frames even where the dataset's base shape
    # would cut them
    from libertem_amd.udf.base import UDF

    class Probe(UDF):
        WHOLE_FRAME_TILES = True

        def get_result_buffers(self):
            return {'n': self.buffer(kind='single', dtype='int64')}

        def process_tile(self, tile):
            assert tuple(tile.shape[1:]) == (64, 64), tile.shape
            self.results.n[:] += tile.shape[0]

        def merge(self, dest, src):
            dest.n[:] += src.n

    data = np.ones((4, 4, 64, 64), dtype=np.float32)
    ds = ctx.load('memory', data=data, num_partitions=2, sig_dims=2, base_shape=(1, 8, 8))
    assert ctx.run_udf(dataset=ds, udf=Probe())['n'].data[0] == 16


def _logsum_part(v):
    from libertem_amd.udf.base import MergeAttrMapping
    return MergeAttrMapping({'logsum': v})


def test_logsum_merge_equals_merge_all():
    rng = np.random.default_rng(13)
    parts = {i: _logsum_part(rng.normal(100., 30., (5, 6)).astype(np.float32)) for i in range(7)}
    udf = LogsumUDF()
    dest = _logsum_part(np.zeros((5, 6), np.float32))
    for p in parts.values():
        udf.merge(dest, p)
    allm = udf.merge_all(parts)
    assert allm['logsum'].dtype == np.float32
    assert np.array_equal(dest.logsum, allm['logsum'])


def test_parts1_equals_parts7(golden):
    for a, b in (('fem_parts1__intensity', 'fem_parts7__intensity'), ('log_parts1__logsum', 'log_parts7__logsum')):
        assert np.allclose(golden[a], golden[b], rtol=1e-5)


def test_fem_analysis(ctx, golden):
    from libertem_amd.analysis import FEMAnalysis
    case = framestats_recipes.FEM_CASES[0]
    _, ds, _, _ = load_case(ctx, case)
    cy, cx = case['center']
    res = ctx.run(FEMAnalysis(dataset=ds, parameters={'cx': cx, 'cy': cy, 'ri': case['rad_in'],
                                                      'ro': case['rad_out']}))
    check(res.intensity.raw_data, golden['fem_u16__intensity'], 1e-5)


def test_compat_alias():
    code = ("import libertem_amd.compat as c; c.install(); "
            "from libertem.udf.FEM import FEMUDF, run_fem; "
            "from libertem.udf.logsum import LogsumUDF, run_logsum; "
            "import libertem_amd.udf.FEM as m; import libertem_amd.udf.logsum as l; "
            "assert FEMUDF is m.FEMUDF and LogsumUDF is l.LogsumUDF; "
            "from libertem.analysis.fem import FEMAnalysis; from libertem.analysis import FEMAnalysis as F2; "
            "assert F2 is FEMAnalysis; print('ok')")
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


def test_gloo_sharded_framestats(tmp_path, ctx):
    world = 2
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           f'--nproc-per-node={world}', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()),
           os.path.join(ROOT, 'tests', 'dist_worker_framestats.py'), str(tmp_path)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    rng = np.random.default_rng(78)
    data = rng.integers(0, 3000, (7, 9, 12, 13)).astype(np.uint16)
    ds = ctx.load('memory', data=data, num_partitions=7, sig_dims=2)
    fem = ctx.run_udf(dataset=ds, udf=FEMUDF(center=(6, 6), rad_in=2, rad_out=5))
    logsum = ctx.run_udf(dataset=ds, udf=LogsumUDF())
    for k in range(world):
        o = np.load(os.path.join(tmp_path, f'rank{k}.npz'))
        assert np.array_equal(o['intensity'], np.asarray(fem['intensity'].data)), k
        # 'sum' buffers: the ranks' partial sums are added across ranks, not partition by partition
        assert np.allclose(o['logsum'], np.asarray(logsum['logsum'].data), rtol=1e-6), k
