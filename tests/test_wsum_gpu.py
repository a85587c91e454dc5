"""
WeightedSumUDF through run_udf on the MI355X: (6, 7) x (16, 16) uint16 and float32 MemoryDataSets in 3 partitions
against the float64 loop of tests/pca_ref.py and against the NumPy branch on the inline executor.  `-m gpu` only.
"""
import numpy as np
import pytest

import pca_ref
from libertem_amd.udf.weightedsum import WeightedSumUDF, run_weighted_sum

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAV, SIG = (6, 7), (16, 16)


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def cpu_ctx():
    from libertem_amd.api import Context
    return Context.make_with('inline')


def _data(dtype):
    rng = np.random.default_rng(11)
    if np.dtype(dtype).kind == 'u':
        return rng.integers(0, 4096, NAV + SIG).astype(dtype)
    return (rng.standard_normal(NAV + SIG) * 50.0).astype(dtype)


def _weights(k, seed=12):
    return np.random.default_rng(seed).standard_normal(NAV + (k,)).astype(np.float32)


def _within_bound(got, frames, weights, roi=None):
    """|got - ref64| <= 1e-5 sum_n |w| |x| + 1e-30 per entry, against the loop over the frames"""
    x = frames.reshape((-1,) + SIG)
    w = weights.reshape((x.shape[0], -1))
    if roi is not None:
        x, w = x[roi.reshape(-1)], w[roi.reshape(-1)]
    ref, bound = pca_ref.weighted_sum(x, w)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 1e-5 * bound + 1e-30).all(), float((err / (1e-5 * bound + 1e-30)).max())


@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
@pytest.mark.parametrize('k', [1, 5, 70])
def test_wsum_against_the_loop_and_the_numpy_branch(ctx, cpu_ctx, dtype, k):
    """k = 70: two launches, 64 + 6 columns"""
    data, w = _data(dtype), _weights(k)
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    got = run_weighted_sum(ctx, ds, w)['wsum'].data
    assert got.shape == (k,) + SIG
    _within_bound(got, data, w)
    cpu = run_weighted_sum(cpu_ctx, cpu_ctx.load('memory', data=data, num_partitions=3, sig_dims=2), w)['wsum'].data
    _within_bound(cpu, data, w)
    # both are within the bound of the same reference: within twice the bound of each other
    _, bound = pca_ref.weighted_sum(data.reshape((-1,) + SIG), w.reshape((-1, k)))
    assert (np.abs(got.astype(np.float64) - cpu) <= 2e-5 * bound + 1e-30).all()


@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
def test_wsum_roi_that_empties_a_partition(ctx, cpu_ctx, dtype):
    data, w = _data(dtype), _weights(4)
    roi = np.random.default_rng(13).random(NAV) > 0.4
    roi.reshape(-1)[14:28] = False                       # the second of three partitions of 14 frames
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    got = run_weighted_sum(ctx, ds, w, roi=roi)['wsum'].data
    _within_bound(got, data, w, roi)
    cpu = run_weighted_sum(cpu_ctx, cpu_ctx.load('memory', data=data, num_partitions=3, sig_dims=2), w,
                           roi=roi)['wsum'].data
    _within_bound(cpu, data, w, roi)


def test_wsum_weights_as_aux_data_and_as_one_map(ctx):
    data = _data('uint16')
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    w = _weights(3)
    roi = np.random.default_rng(14).random(NAV) > 0.5
    as_array = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(w), roi=roi)['wsum'].data
    aux = WeightedSumUDF.aux_data(w.reshape((-1, 3)), kind='nav', extra_shape=(3,), dtype='float32')
    as_aux = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(aux), roi=roi)['wsum'].data
    assert np.array_equal(as_array, as_aux)
    _within_bound(as_aux, data, w, roi)
    # a map of the scan's shape is one component
    one = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(w[..., 0]))['wsum'].data
    assert one.shape == (1,) + SIG
    _within_bound(one, data, w[..., :1])
    with pytest.raises(ValueError):
        ctx.run_udf(dataset=ds, udf=WeightedSumUDF(np.ones((5, 7, 2), dtype=np.float32)))


@pytest.mark.parametrize('dtype', ['uint16', 'float32'])
def test_wsum_column_of_ones_is_the_sum(ctx, dtype):
    from libertem_amd.udf.sum import SumUDF
    data = _data(dtype)
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    w = _weights(3)
    w[..., 1] = 1.0
    got = run_weighted_sum(ctx, ds, w)['wsum'].data
    total = np.asarray(ctx.run_udf(dataset=ds, udf=SumUDF())['intensity'].data, dtype=np.float64)
    bound = np.abs(data.astype(np.float64)).sum(axis=(0, 1))
    assert (np.abs(got[1].astype(np.float64) - total) <= 2e-5 * bound + 1e-30).all()


def test_wsum_zero_one_weights_are_exact_on_uint16(ctx):
    data = _data('uint16')                               # 42 frames below 4096: every sum below 2^24
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    w = (np.random.default_rng(15).random(NAV + (6,)) > 0.5).astype(np.float32)
    got = run_weighted_sum(ctx, ds, w)['wsum'].data
    ref, _ = pca_ref.weighted_sum(data.reshape((-1,) + SIG), w.reshape((-1, 6)))
    assert np.array_equal(got.astype(np.float64), ref)


def test_wsum_result_stays_on_the_device(ctx):
    from libertem_amd.common.hiparray import HipArray
    data, w = _data('uint16'), _weights(2)
    ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
    res = ctx.run_udf(dataset=ds, udf=WeightedSumUDF(w), result_where='device')
    assert isinstance(res['wsum'].device_data, HipArray)
    _within_bound(res['wsum'].data, data, w)


def test_wsum_unsupported_dtypes_on_hip(ctx):
    for dtype in ('float64', 'complex64', 'int64'):
        data = np.ones(NAV + SIG, dtype=dtype)
        ds = ctx.load('memory', data=data, num_partitions=3, sig_dims=2)
        with pytest.raises(NotImplementedError, match=dtype):
            ctx.run_udf(dataset=ds, udf=WeightedSumUDF(_weights(2)))
