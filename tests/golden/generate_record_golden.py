#!/usr/bin/env python
"""
Generate tests/golden/record.npz with the REAL Python reference's RecordUDF, ConvertTransposedDatasetUDF and
NPYDataSet + SumUDF + SumSigUDF (LiberTEM, /root/reference/src), through the same third-party stand-ins as the other
generators (`tests/golden/refshim/`).  The inputs are the seeded arrays and .npy files of record_recipes.py; stored
are, per written file and per UDF result over the npy datasets, shape, dtype string and the sha256 of the array
bytes, the image_count of every npy dataset, and for the loads that must fail the name of the exception class.

`libertem.contrib.convert_transposed` imports `libertem.api` (for a Dask context this generator never makes), which
needs packages that are not installed: an empty module stands in for it.

The UDFs run through `UDFRunner.run_for_dataset` on the InlineJobExecutor, as in the other generators.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_record_golden.py
"""
import io
import os
import sys
import types
import zipfile
import hashlib
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'

if not os.path.isdir(REF):
    print("reference not present, nothing to do")
    sys.exit(0)

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import record_recipes as recipes  # noqa: E402

sys.modules.setdefault('libertem.api', types.ModuleType('libertem.api'))

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.record import RecordUDF  # noqa: E402
from libertem.udf.sum import SumUDF  # noqa: E402
from libertem.udf.sumsigudf import SumSigUDF  # noqa: E402
from libertem.contrib.convert_transposed import ConvertTransposedDatasetUDF  # noqa: E402
from libertem.io.dataset.memory import MemoryDataSet  # noqa: E402
from libertem.io.dataset.npy import NPYDataSet  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)


def put(out, key, arr):
    arr = np.ascontiguousarray(arr)
    out[f"{key}__shape"] = np.array(arr.shape, dtype=np.int64)
    out[f"{key}__dtype"] = np.array(arr.dtype.str)
    out[f"{key}__sha"] = np.frombuffer(hashlib.sha256(arr.tobytes()).digest(), dtype=np.uint8)


def run_writer(recipe, udf_class, out, tmp):
    data = recipes.make_data(recipe)
    ds = MemoryDataSet(data=data, sig_dims=recipe['sig_dims'], num_partitions=recipe['num_partitions'])
    ds = ds.initialize(EX)
    path = os.path.join(tmp, recipe['name'] + '.npy')
    UDFRunner([udf_class(path)]).run_for_dataset(ds, EX)
    written = np.load(path)
    if udf_class is ConvertTransposedDatasetUDF:
        n_sig = int(np.prod(ds.shape.sig))
        assert np.array_equal(written.reshape(n_sig, -1), data.reshape(-1, n_sig).T)
    else:
        assert np.array_equal(written, data)
    put(out, recipe['name'], written)
    print(recipe['name'], written.shape, written.dtype.str, flush=True)


def run_npy(case, out, paths):
    name = case['name']
    try:
        ds = NPYDataSet(path=paths[case['file']], **case['kwargs'])
        ds = ds.initialize(EX)
        ds.check_valid()
    except Exception as e:                              # noqa: BLE001  (the class name is what is stored)
        assert case.get('error'), (name, e)
        out[f"{name}__error"] = np.array(type(e).__name__)
        print(name, type(e).__name__, e, flush=True)
        return
    assert not case.get('error'), name
    res = UDFRunner([SumUDF(), SumSigUDF()]).run_for_dataset(ds, EX, roi=case.get('roi')).buffers
    out[f"{name}__ds_shape"] = np.array(tuple(ds.shape), dtype=np.int64)
    out[f"{name}__ds_dtype"] = np.array(np.dtype(ds.dtype).str)
    out[f"{name}__image_count"] = np.int64(ds.meta.image_count)
    put(out, f"{name}__sum", res[0]['intensity'].raw_data)
    put(out, f"{name}__sumsig", res[1]['intensity'].raw_data)
    print(name, tuple(ds.shape), np.dtype(ds.dtype).str, int(ds.meta.image_count), flush=True)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for recipe in recipes.RECORD:
            run_writer(recipe, RecordUDF, out, tmp)
        for recipe in recipes.CONVERT:
            run_writer(recipe, ConvertTransposedDatasetUDF, out, tmp)
        paths = {key: recipes.write_npy(key, tmp) for key in recipes.NPY_FILES}
        for case in recipes.NPY:
            run_npy(case, out, paths)
    path = os.path.join(HERE, 'record.npz')
    # an .npz with fixed member times and order: the same bytes on every run
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
