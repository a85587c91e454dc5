"""
RecordUDF, the transposed-data converter and NPYDataSet on the GPU (-m gpu), on `Context.make_with('hip', gpus=0)`:
the recipes of tests/golden/record_recipes.py against the checksums the REAL reference's RecordUDF,
ConvertTransposedDatasetUDF and NPYDataSet gave (tests/golden/record.npz), from host arrays and from device tensors;
which transposition kernel a conversion launched; a recorded SEQ set with dark and gain side files against PickUDF;
the round trip convert -> load('npy') -> SumSigUDF; an npy file loaded twice.
"""
import os

import numpy as np
import pytest

import record_checks as checks
from record_checks import recipes

import records_recipes
import records_synth  # noqa: F401  (records_recipes writes its files with it)

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def npy_paths(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('npy')
    return {key: recipes.write_npy(key, tmp) for key in recipes.NPY_FILES}


def device_tensor(data):
    from libertem_amd.common.hiparray import HipArray
    return HipArray.from_numpy(data, 0).torch


@pytest.mark.parametrize('where', ('host', 'device'))
@pytest.mark.parametrize('name', [r['name'] for r in recipes.RECORD])
def test_record(ctx, tmp_path, name, where):
    recipe = recipes.case(name)
    data = device_tensor(recipes.make_data(recipe)) if where == 'device' else None
    checks.assert_matches_golden(name, checks.write_recipe(ctx, recipe, tmp_path, data=data))


@pytest.mark.parametrize('where', ('host', 'device'))
@pytest.mark.parametrize('name', [r['name'] for r in recipes.CONVERT])
def test_convert(ctx, tmp_path, name, where):
    from libertem_amd import hip
    recipe = recipes.case(name)
    other = 2 if np.dtype(recipe['dtype']).itemsize != 2 else 4
    scratch = torch.zeros(64, dtype=torch.uint8, device='cuda:0')
    hip.transpose2d(0, scratch.data_ptr(), 2, 2, 2, other, scratch.data_ptr() + 32, 2)
    assert hip.transpose_last_kernel() == f'k_transpose<{other}>'
    data = device_tensor(recipes.make_data(recipe)) if where == 'device' else None
    checks.assert_matches_golden(name, checks.write_recipe(ctx, recipe, tmp_path, data=data))
    # the device path ran, not the NumPy branch: the last launch of this thread is the item size's kernel
    assert hip.transpose_last_kernel() == f"k_transpose<{np.dtype(recipe['dtype']).itemsize}>"


def test_record_corrected_seq_equals_pick(ctx, tmp_path):
    """frames with the dataset's own dark frame and gain map applied: the file holds what PickUDF returns"""
    from libertem_amd.udf.raw import PickUDF
    from libertem_amd.udf.record import RecordUDF
    case = records_recipes.case('SEQ_A')
    fs = records_recipes.write_fileset(case['fileset'], str(tmp_path))
    assert fs['dark'] is not None and fs['gain'] is not None
    ds = ctx.load('seq', **records_recipes.load_kwargs(case, fs))
    path = str(tmp_path / 'seq.npy')
    ctx.run_udf(dataset=ds, udf=RecordUDF(path))
    picked = ctx.run_udf(dataset=ds, udf=PickUDF(), roi=np.ones(tuple(ds.shape.nav), dtype=bool))['intensity'].data
    picked = np.asarray(picked)
    written = np.load(path)
    assert written.shape == tuple(ds.shape)
    assert written.dtype == picked.dtype and written.dtype.kind == 'f'
    assert np.array_equal(written.reshape(picked.shape), picked)
    assert not np.array_equal(written.reshape((-1,) + fs['frames'].shape[1:]), fs['frames'])     # (corrected)


def test_round_trip(ctx, tmp_path):
    """convert a (sig, nav) array, load the file, sum the frames: the column sums of the source"""
    from libertem_amd.udf.sumsigudf import SumSigUDF
    recipe = recipes.case('CONV_u16')
    data = recipes.make_data(recipe)
    out = os.path.join(str(tmp_path), recipe['name'] + '.npy')
    checks.write_recipe(ctx, recipe, tmp_path)
    ds = ctx.load('npy', path=out)
    assert tuple(ds.shape) == (6, 7, 5, 13) and ds.dtype == np.uint16
    got = np.asarray(ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data)
    # whole numbers below 2**24 (65 values <= 4095 each): exact in float32
    want = data.reshape(65, 42).sum(axis=0, dtype=np.int64).reshape(6, 7)
    assert got.shape == (6, 7) and np.array_equal(got, want.astype(got.dtype))
    assert np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize('name', [c['name'] for c in recipes.NPY if not c.get('error')])
def test_npy_dataset(ctx, npy_paths, name):
    case = recipes.case(name)
    first = checks.check_npy_case(ctx, case, npy_paths)
    if name in ('NPY_plain', 'NPY_f4_sig1', 'NPY_m4_3'):
        # the file loaded again: identical result bytes
        second = checks.check_npy_case(ctx, case, npy_paths)
        for a, b in zip(first, second):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', [c['name'] for c in recipes.NPY if c.get('error')])
def test_npy_dataset_errors(ctx, npy_paths, name):
    from libertem_amd.io.dataset.base import DataSetException
    case = recipes.case(name)
    with pytest.raises(DataSetException):
        ctx.load('npy', path=npy_paths[case['file']], **case['kwargs'])
