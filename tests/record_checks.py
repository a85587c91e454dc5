"""
What tests/test_record_cpu.py and tests/test_record_gpu.py share: the recipes of tests/golden/record_recipes.py run
through this package on a given Context and compared with the reference's checksums (tests/golden/record.npz).
"""
import os
import sys
import hashlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))

import record_recipes as recipes  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'record.npz'))


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).digest()


def assert_matches_golden(key, arr):
    """shape, dtype string and sha256 of the bytes of `arr` are the stored ones"""
    arr = np.ascontiguousarray(arr)
    assert tuple(arr.shape) == tuple(GOLDEN[f'{key}__shape'])
    assert arr.dtype.str == str(GOLDEN[f'{key}__dtype'])
    assert sha(arr) == GOLDEN[f'{key}__sha'].tobytes()


def write_recipe(ctx, recipe, tmp_path, data=None):
    """run RecordUDF (RECORD recipes) or convert_transposed (CONVERT recipes) over the recipe's MemoryDataSet ->
    the array of the written file.  `data`: the recipe's array as something else than a host array (a device
    tensor)."""
    from libertem_amd.udf.record import RecordUDF
    from libertem_amd.contrib.convert_transposed import convert_transposed
    kw = {}
    if data is None:
        data = recipes.make_data(recipe)
    else:
        kw['dtype'] = np.dtype(recipe['dtype'])
    ds = ctx.load('memory', data=data, sig_dims=recipe['sig_dims'], num_partitions=recipe['num_partitions'], **kw)
    path = os.path.join(str(tmp_path), recipe['name'] + '.npy')
    if recipe in recipes.CONVERT:
        convert_transposed(ctx, ds, path)
    else:
        ctx.run_udf(dataset=ds, udf=RecordUDF(path))
    return np.load(path)


def check_npy_case(ctx, case, paths):
    """load the .npy file of an NPY case and compare dataset and sums with the golden -> the two result arrays"""
    from libertem_amd.udf.sum import SumUDF
    from libertem_amd.udf.sumsigudf import SumSigUDF
    name = case['name']
    ds = ctx.load('npy', path=paths[case['file']], **case['kwargs'])
    assert tuple(ds.shape) == tuple(GOLDEN[f'{name}__ds_shape'])
    # the file's dtype; like the raw dataset this package reports it in native byte order (big-endian integers
    # are swapped per tile / on the device), the reference as it is stored
    assert np.dtype(ds.dtype) == np.dtype(str(GOLDEN[f'{name}__ds_dtype'])).newbyteorder('=')
    assert int(ds.meta.image_count) == int(GOLDEN[f'{name}__image_count'])
    roi = case.get('roi')
    got_sum = np.asarray(ctx.run_udf(dataset=ds, udf=SumUDF(), roi=roi)['intensity'].raw_data)
    got_sig = np.asarray(ctx.run_udf(dataset=ds, udf=SumSigUDF(), roi=roi)['intensity'].raw_data)
    if np.dtype(ds.dtype).kind == 'f':
        # float32 sums depend on their order: shape and dtype are the golden's, the values lie within
        # 1e-5 * sum |x| of the float64 sums of the recipe's array (the bound of tests/test_raw_csr_sums_cpu.py)
        frames = recipes.make_data(recipes.NPY_FILES[case['file']]).astype(np.float64)
        frames = frames.reshape((-1,) + tuple(ds.shape.sig))
        assert roi is None and not case['kwargs'].get('sync_offset')
        for key, got, want, mag in (
                ('sum', got_sum, frames.sum(axis=0), np.abs(frames).sum(axis=0)),
                ('sumsig', got_sig, frames.reshape(len(frames), -1).sum(axis=1),
                 np.abs(frames).reshape(len(frames), -1).sum(axis=1))):
            assert tuple(got.shape) == tuple(GOLDEN[f'{name}__{key}__shape'])
            assert got.dtype.str == str(GOLDEN[f'{name}__{key}__dtype'])
            assert np.all(np.abs(got.reshape(want.shape) - want) <= 1e-5 * mag)
    else:
        # whole numbers below 2**24: exact in float32 in any order, bit-equal
        assert_matches_golden(f'{name}__sum', got_sum)
        assert_matches_golden(f'{name}__sumsig', got_sig)
    return got_sum, got_sig
