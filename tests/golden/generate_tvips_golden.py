#!/usr/bin/env python
"""
Generate tests/golden/tvips.npz with the REAL Python reference's TVIPSDataSet + SumUDF + SumSigUDF + ApplyMasksUDF +
PickUDF (LiberTEM, /root/reference/src), through the same third-party stand-ins as the other generators
(`tests/golden/refshim/`).  The series come from the seeded recipes in tvips_recipes.py (written by
tests/tvips_synth.py) and are always named by their `_000` file; only small results are stored: the UDF results, the
sha256 and a crop of every picked raw frame, shape, dtype, raw dtype, image_count and the sync_offset the dataset
settled on, and per series what the reference's `detect_params` returned.

The file is written with fixed member times and order: the same bytes on every run.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_tvips_golden.py
"""
import io
import os
import sys
import hashlib
import tempfile
import warnings
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'

if not os.path.isdir(REF):
    print("reference not present, nothing to do")
    sys.exit(0)

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import tvips_recipes as recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.masks import ApplyMasksUDF  # noqa: E402
from libertem.udf.raw import PickUDF  # noqa: E402
from libertem.udf.sum import SumUDF  # noqa: E402
from libertem.udf.sumsigudf import SumSigUDF  # noqa: E402
from libertem.io.dataset.tvips import TVIPSDataSet  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def mask_udf(masks):
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


def run(case, out, paths):
    fileset, name = case['fileset'], case['name']
    ds = TVIPSDataSet(**recipes.load_kwargs(case, paths[fileset]))
    ds = ds.initialize(EX)
    ds.check_valid()
    sig = tuple(ds.shape.sig)
    # what the recipe says the dataset reports is what the reference reports
    assert tuple(ds.shape.nav) == tuple(case['nav']) and sig == recipes.sig_shape(case), (name, tuple(ds.shape))
    assert int(ds.meta.sync_offset) == case['sync_offset'], (name, ds.meta.sync_offset)
    roi = case['roi']
    masks = recipes.make_masks(case)
    pick_roi = roi if roi is not None else np.ones(tuple(ds.shape.nav), dtype=bool)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = UDFRunner([SumUDF(), SumSigUDF(), mask_udf(masks)]).run_for_dataset(ds, EX, roi=roi).buffers
        raw = UDFRunner([PickUDF()]).run_for_dataset(ds, EX, roi=pick_roi).buffers[0]
    raw = np.array(raw['intensity'].data).reshape((-1,) + sig)
    frames = raw.astype(recipes.stored_dtype(fileset))
    assert np.array_equal(frames, raw)
    out[f"{name}__sum"] = np.array(res[0]['intensity'].data)
    out[f"{name}__sumsig"] = np.array(res[1]['intensity'].data)
    out[f"{name}__masks"] = np.array(res[2]['intensity'].data)
    out[f"{name}__picked_dtype"] = np.array(raw.dtype.str)
    out[f"{name}__picked_sumsig"] = raw.reshape(len(raw), -1).sum(axis=1, dtype=np.float64)
    out[f"{name}__sha_frames"] = np.stack([sha(f) for f in frames])
    out[f"{name}__crops"] = np.stack([recipes.crop(fileset)(f) for f in frames])
    out[f"{name}__image_count"] = np.int64(ds.meta.image_count)
    out[f"{name}__sync_offset"] = np.int64(ds.meta.sync_offset)
    out[f"{name}__shape"] = np.array(tuple(ds.shape), dtype=np.int64)
    out[f"{name}__dtype"] = np.array(np.dtype(ds.dtype).str)
    out[f"{name}__raw_dtype"] = np.array(np.dtype(ds.meta.raw_dtype).str)
    print(name, tuple(ds.shape), np.dtype(ds.dtype), int(ds.meta.image_count), int(ds.meta.sync_offset),
          {k.split('__')[1]: (v.dtype.str, v.shape) for k, v in out.items() if k.startswith(name + '__')},
          flush=True)


def detect(fileset, out, paths):
    got = TVIPSDataSet.detect_params(paths[fileset]['path'], EX)
    params, info = got['parameters'], got['info']
    assert params['path'] == paths[fileset]['path'] and set(params) == {'path', 'nav_shape', 'sig_shape',
                                                                        'sync_offset'}
    assert set(info) == {'image_count', 'native_sig_shape'}
    assert (tuple(params['nav_shape']), int(params['sync_offset'])) == recipes.DETECTED[fileset], (fileset, params)
    out[f"{fileset}__detect_nav"] = np.array(tuple(params['nav_shape']), dtype=np.int64)
    out[f"{fileset}__detect_sig"] = np.array(tuple(params['sig_shape']), dtype=np.int64)
    out[f"{fileset}__detect_sync_offset"] = np.int64(params['sync_offset'])
    out[f"{fileset}__detect_image_count"] = np.int64(info['image_count'])
    out[f"{fileset}__detect_native_sig"] = np.array(tuple(info['native_sig_shape']), dtype=np.int64)
    print(fileset, got, flush=True)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {fs: recipes.write_fileset(fs, tmp) for fs in recipes.FILESETS}
        for case in recipes.CASES:
            run(case, out, paths)
        for fileset in recipes.FILESETS:
            detect(fileset, out, paths)
    path = os.path.join(HERE, 'tvips.npz')
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
