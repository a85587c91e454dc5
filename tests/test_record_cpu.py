"""
CPU half of RecordUDF, the transposed-data converter and NPYDataSet: the two new library entries are declared in
include/ltmi.h with as many arguments as libertem_amd/hip.py binds, and on a CPU executor the three pieces give the
reference's files and results (tests/golden/record.npz, made by tests/golden/generate_record_golden.py).

Before these pieces existed every test here failed: `libertem_amd.udf.record`, `libertem_amd.contrib` and
`libertem_amd.io.dataset.npy` were a ModuleNotFoundError, `ctx.load('npy', ...)` answered "dataset type 'npy' is
not available", and the header had no ltmi_transpose2d.
"""
import os
import re

import numpy as np
import pytest

import record_checks as checks
from record_checks import recipes, GOLDEN

from libertem_amd.api import Context
from libertem_amd.executor.inline import InlineJobExecutor
from libertem_amd.io.dataset.base import DataSetException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'ltmi_transpose2d': 9, 'ltmi_transpose_last_kernel': 0}


@pytest.fixture(scope='module')
def ctx():
    ctx = Context(executor=InlineJobExecutor())
    yield ctx
    ctx.close()


@pytest.fixture(scope='module')
def npy_paths(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('npy')
    return {key: recipes.write_npy(key, tmp) for key in recipes.NPY_FILES}


def _declared_arguments(name):
    """number of parameters of `name` in the header text"""
    hdr = open(os.path.join(ROOT, 'include', 'ltmi.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, hdr)
    assert m, f"{name} is not declared in include/ltmi.h"
    args = m.group(1).strip()
    return 0 if args in ('', 'void') else len(args.split(','))


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_and_binding_agree(name):
    from libertem_amd import hip
    assert _declared_arguments(name) == ENTRIES[name]
    assert name in hip.EXPORTS
    fn = getattr(hip.lib(), name)
    assert len(fn.argtypes) == ENTRIES[name]


@pytest.mark.parametrize('name', [r['name'] for r in recipes.RECORD + recipes.CONVERT])
def test_written_file_is_the_references(ctx, tmp_path, name):
    recipe = recipes.case(name)
    written = checks.write_recipe(ctx, recipe, tmp_path)
    checks.assert_matches_golden(name, written)
    # (and what the checksum stands for: the frames themselves / their transposition)
    data = recipes.make_data(recipe)
    if recipe in recipes.CONVERT:
        n_sig = int(np.prod(data.shape[-recipe['sig_dims']:]))
        assert np.array_equal(written.reshape(n_sig, -1), data.reshape(-1, n_sig).T)
    else:
        assert np.array_equal(written, data)


def test_record_with_roi_raises(ctx, tmp_path):
    from libertem_amd.udf.record import RecordUDF
    from libertem_amd.contrib.convert_transposed import ConvertTransposedDatasetUDF
    recipe = recipes.case('REC_u16_p2')
    ds = ctx.load('memory', data=recipes.make_data(recipe), sig_dims=2, num_partitions=2)
    roi = np.zeros(tuple(ds.shape.nav), dtype=bool)
    roi[1, 2:5] = True
    for cls in (RecordUDF, ConvertTransposedDatasetUDF):
        with pytest.raises(RuntimeError, match='Recording with ROI is not supported.'):
            ctx.run_udf(dataset=ds, udf=cls(str(tmp_path / 'roi.npy')), roi=roi)


def test_convert_dm4_transposed_raises(ctx, tmp_path):
    from libertem_amd.contrib import convert_transposed as ct
    assert ct._convert_transposed_ds is ct.convert_transposed
    with pytest.raises(DataSetException, match='convert_transposed'):
        ct.convert_dm4_transposed(str(tmp_path / 'scan.dm4'), str(tmp_path / 'out.npy'), ctx=ctx)
    with pytest.raises(ValueError):
        ct.convert_dm4_transposed(str(tmp_path / 'scan.dm4'), str(tmp_path / 'out.npy'), ctx=ctx, num_cpus=2)


@pytest.mark.parametrize('name', [c['name'] for c in recipes.NPY if not c.get('error')])
def test_npy_dataset_gives_the_references_results(ctx, npy_paths, name):
    checks.check_npy_case(ctx, recipes.case(name), npy_paths)


@pytest.mark.parametrize('name', [c['name'] for c in recipes.NPY if c.get('error')])
def test_npy_dataset_errors(ctx, npy_paths, name):
    case = recipes.case(name)
    assert str(GOLDEN[f'{name}__error']) == 'DataSetException'
    with pytest.raises(DataSetException):
        ctx.load('npy', path=npy_paths[case['file']], **case['kwargs'])


def test_npy_dataset_interface(ctx, npy_paths):
    from libertem_amd.io.dataset import NPYDataSet
    import libertem_amd.io.dataset as dsmod
    assert 'NPYDataSet' in dsmod.__all__
    ds = ctx.load('NPY', path=npy_paths['u2'])
    assert isinstance(ds, NPYDataSet)
    assert ds.get_diagnostics() == [{"name": "dtype", "value": "uint16"}]
    assert ds.get_cache_key() == {"path": npy_paths['u2'], "shape": (4, 5, 6, 7), "dtype": "uint16",
                                  "sync_offset": 0}
    assert NPYDataSet.get_supported_extensions() == {"npy"}
    assert NPYDataSet.detect_params(npy_paths['u2'], InlineJobExecutor()) == {
        "parameters": {"path": npy_paths['u2'], "nav_shape": (4, 5), "sig_shape": (6, 7)},
        "info": {"image_count": 20, "native_sig_shape": (6, 7)}}
    assert NPYDataSet.detect_params(__file__, InlineJobExecutor()) is False
    with pytest.raises(ValueError):
        NPYDataSet(path=npy_paths['u2'], io_backend=object())
    with pytest.raises(DataSetException, match="'npy'"):
        ctx.load('no_such_type')


def test_reference_module_names_resolve():
    import libertem_amd.compat
    import libertem_amd.udf.record
    import libertem_amd.contrib.convert_transposed
    import libertem_amd.io.dataset.npy
    assert libertem_amd.compat.install()
    try:
        from libertem.udf.record import RecordUDF
        from libertem.contrib.convert_transposed import ConvertTransposedDatasetUDF, convert_dm4_transposed
        from libertem.io.dataset.npy import NPYDataSet
        from libertem.udf import RecordUDF as exported
    finally:
        libertem_amd.compat.uninstall()
    assert RecordUDF is libertem_amd.udf.record.RecordUDF is exported
    assert ConvertTransposedDatasetUDF is libertem_amd.contrib.convert_transposed.ConvertTransposedDatasetUDF
    assert convert_dm4_transposed is libertem_amd.contrib.convert_transposed.convert_dm4_transposed
    assert NPYDataSet is libertem_amd.io.dataset.npy.NPYDataSet
