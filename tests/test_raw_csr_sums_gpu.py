"""
SumUDF and SumSigUDF over raw_csr datasets on the GPU (`-m gpu`): both read the stored entries of the triple in
place (`k_csr_sum_frames`, `k_csr_sum_sig`) -- no dense window is allocated -- where the sum is a function of the
stored entries and exact or rounded once; float data in SumUDF and every other result dtype take the densified
frames and give the bits of a MemoryDataSet run.  Expected values: the reference's results in
tests/golden/raw_csr.npz, float64 NumPy sums, and the same UDF over a MemoryDataSet of the densified frames.
"""
import os

import numpy as np
import pytest

import raw_csr_recipes as recipes

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, 'golden', 'raw_csr.npz'))
CASES = {c['name']: c for c in recipes.CASES}
FLOAT_CASES = ('dtype_f4', 'nan_f4')
INT_CASES = tuple(sorted(set(CASES) - set(FLOAT_CASES)))


@pytest.fixture(scope='module')
def hip():
    from libertem_amd import hip as _hip
    _hip.lib()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _hip


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


def _load(ctx, tmp_path, case, inp):
    path = recipes.write_files(case, inp, str(tmp_path))
    return ctx.load('raw_csr', path=path, sync_offset=case['sync_offset'], num_partitions=case['num_partitions'])


def _memory(ctx, case, inp):
    return ctx.load('memory', data=recipes.dense_frames(inp).reshape(recipes.NAV + recipes.SIG), sig_dims=2,
                    num_partitions=case['num_partitions'], sync_offset=case['sync_offset'])


def _positioned(case, inp):
    """dense frames at their scan positions: frame g at position g - sync_offset, zeros elsewhere"""
    frames = recipes.dense_frames(inp)
    n, so = frames.shape[0], case['sync_offset']
    out = np.zeros_like(frames)
    for p in range(n):
        if 0 <= p + so < n:
            out[p] = frames[p + so]
    return out.reshape(recipes.NAV + recipes.SIG)


def _no_dense_window(ds):
    return ds._window.get('buf') is None


@pytest.mark.parametrize('name', sorted(CASES))
def test_sumsig_reads_the_stored_entries(ctx, hip, tmp_path, name):
    from libertem_amd.udf.sumsigudf import SumSigUDF
    case = CASES[name]
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    got = ctx.run_udf(dataset=ds, udf=SumSigUDF(), roi=inp['roi'])['intensity'].data
    assert _no_dense_window(ds)                                   # nothing was densified
    assert hip.csr_last_kernel().startswith('k_csr_sum_sig<')
    if inp['roi'] is not None:
        assert hip.csr_last_kernel().endswith(' rows')
    gold = GOLDEN[f'{name}__sumsig']
    assert got.shape == gold.shape and got.dtype == gold.dtype
    dense = _positioned(case, inp).astype(np.float64)
    roi = inp['roi'] if inp['roi'] is not None else np.ones(recipes.NAV, dtype=bool)
    ref = np.where(roi, dense.sum(axis=(2, 3)), np.nan)
    tol = 1e-5 * np.abs(np.nan_to_num(dense)).sum(axis=(2, 3))
    assert np.all(np.isnan(got[~roi]))
    assert np.array_equal(np.isnan(got), np.isnan(gold))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    assert np.all(np.abs(got - ref)[fin] <= tol[fin])
    if name == 'sync_m4_roi':
        # (the reference puts the per-frame rows of the first partition early: tests/test_raw_csr_cpu.py)
        assert np.all(np.abs(np.sort(got[roi]) - np.sort(gold[roi])) <= np.sort(tol[roi]).max())
    else:
        assert np.all(np.abs(got - gold)[fin] <= tol[fin])


@pytest.mark.parametrize('name', INT_CASES)
def test_sum_of_integer_frames_reads_the_stored_entries(ctx, hip, tmp_path, name):
    from libertem_amd.udf.sum import SumUDF
    case = CASES[name]
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    got = ctx.run_udf(dataset=ds, udf=SumUDF(), roi=inp['roi'])['intensity'].data
    assert _no_dense_window(ds)
    assert hip.csr_last_kernel().startswith('k_csr_sum_frames<')
    gold = GOLDEN[f'{name}__sum']
    assert got.shape == gold.shape
    dense = _positioned(case, inp).astype(np.float64)
    roi = inp['roi'] if inp['roi'] is not None else np.ones(recipes.NAV, dtype=bool)
    assert np.all(np.abs(got - gold) <= 1e-5 * np.abs(dense[roi]).sum(axis=0) + 1e-30)
    # at most 35 terms below 120 per pixel: far below 2^24, both routes are exact
    assert np.array_equal(got, dense[roi].sum(axis=0).astype(np.float32))
    mem = ctx.run_udf(dataset=_memory(ctx, case, inp), udf=SumUDF(), roi=inp['roi'])['intensity'].data
    assert got.dtype == mem.dtype and got.tobytes() == mem.tobytes()


@pytest.mark.parametrize('name', FLOAT_CASES)
def test_sum_of_float_frames_keeps_the_dense_route(ctx, tmp_path, name):
    from libertem_amd.udf.sum import SumUDF
    case = CASES[name]
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    got = ctx.run_udf(dataset=ds, udf=SumUDF(), roi=inp['roi'])['intensity'].data
    assert not _no_dense_window(ds)
    mem = ctx.run_udf(dataset=_memory(ctx, case, inp), udf=SumUDF(), roi=inp['roi'])['intensity'].data
    assert got.dtype == mem.dtype and got.shape == mem.shape
    assert np.array_equal(np.isnan(got), np.isnan(mem))
    assert got.tobytes() == mem.tobytes()


def test_sum_result_dtypes(ctx, hip, tmp_path):
    """float64 results take the stored entries; complex and integer results the densified frames"""
    from libertem_amd.udf.sum import SumUDF
    case = CASES['dtype_u2']
    inp = recipes.make_case(case)
    dense = recipes.dense_frames(inp)
    ds = _load(ctx, tmp_path, case, inp)
    got = ctx.run_udf(dataset=ds, udf=SumUDF(dtype='float64'))['intensity'].data
    assert _no_dense_window(ds) and hip.csr_last_kernel().startswith('k_csr_sum_frames<u16,f64>')
    assert got.dtype == np.float64 and np.array_equal(got, dense.astype(np.float64).sum(axis=0))
    for dtype in ('complex64', 'int64'):
        ds = _load(ctx, tmp_path, case, inp)
        before = hip.csr_last_kernel()
        got = ctx.run_udf(dataset=ds, udf=SumUDF(dtype=dtype))['intensity'].data
        assert not _no_dense_window(ds) and hip.csr_last_kernel() == before
        mem = ctx.run_udf(dataset=_memory(ctx, case, inp), udf=SumUDF(dtype=dtype))['intensity'].data
        assert got.dtype == mem.dtype == np.dtype(dtype) and got.tobytes() == mem.tobytes()
        assert np.array_equal(got, dense.sum(axis=0).astype(dtype))


def test_three_udfs_densify_nothing(ctx, tmp_path):
    from libertem_amd.udf.masks import ApplyMasksUDF
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    case = CASES['parts3']
    inp = recipes.make_case(case)
    masks = inp['masks']
    ds = _load(ctx, tmp_path, case, inp)
    udfs = [ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False), SumUDF(), SumSigUDF()]
    runs = []
    for _ in range(3):
        res = ctx.run_udf(dataset=ds, udf=udfs)
        runs.append(b''.join(r['intensity'].data.tobytes() for r in res))
    assert _no_dense_window(ds)
    assert runs[0] == runs[1] == runs[2]
    dense = recipes.dense_frames(inp).astype(np.float64)
    assert np.array_equal(res[1]['intensity'].data, dense.sum(axis=0).astype(np.float32))
    assert np.array_equal(res[2]['intensity'].data.reshape(-1), dense.sum(axis=(1, 2)).astype(np.float32))


def test_analyses_equal_the_udfs(ctx, tmp_path):
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    case = CASES['dtype_i2']
    inp = recipes.make_case(case)
    ds = _load(ctx, tmp_path, case, inp)
    a = ctx.run(ctx.create_sum_analysis(dataset=ds))
    b = ctx.run(ctx.create_sumsig_analysis(dataset=ds))
    assert _no_dense_window(ds)
    s = ctx.run_udf(dataset=ds, udf=SumUDF())['intensity'].data
    g = ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data
    assert np.array_equal(a['intensity_lin'].raw_data, s)
    assert np.array_equal(b['intensity'].raw_data, g)
