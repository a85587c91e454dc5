#!/usr/bin/env python
"""
Generate tests/golden/records.npz with the REAL Python reference's SEQDataSet, EMPADDataSet and BloDataSet +
SumUDF + SumSigUDF + ApplyMasksUDF + PickUDF (LiberTEM, /root/reference/src), through the same third-party
stand-ins as the other generators (`tests/golden/refshim/`, plus `defusedxml` and `ncempy.io.mrc`).  The files come
from the seeded recipes in records_recipes.py (written by tests/records_synth.py); only small results are stored:
the UDF results with the dataset's own corrections, the sha256 and a crop of every picked raw frame, shape, dtype,
raw dtype and image_count, and for SEQ the dark frame, the gain map and the coordinates of the excluded pixels as
the reference returned them.

As in generate_frms6_golden.py the UDFs run through `UDFRunner.run_for_dataset` with
`dataset.get_correction_data()` passed by hand (what `Context.run_udf` does for `corrections=None`); a dataset
without that method (EMPAD, BLO) runs without corrections.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_records_golden.py
"""
import os
import sys
import hashlib
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'

if not os.path.isdir(REF):
    print("reference not present, nothing to do")
    sys.exit(0)

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import records_recipes as recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.masks import ApplyMasksUDF  # noqa: E402
from libertem.udf.raw import PickUDF  # noqa: E402
from libertem.udf.sum import SumUDF  # noqa: E402
from libertem.udf.sumsigudf import SumSigUDF  # noqa: E402
from libertem.io.dataset.seq import SEQDataSet  # noqa: E402
from libertem.io.dataset.empad import EMPADDataSet  # noqa: E402
from libertem.io.dataset.blo import BloDataSet  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)
CLASSES = {'seq': SEQDataSet, 'empad': EMPADDataSet, 'blo': BloDataSet}


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def mask_udf(masks):
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


def run(case, out, paths):
    fileset = case['fileset']
    kind = recipes.FILESETS[fileset]['kind']
    ds = CLASSES[kind](**recipes.load_kwargs(case, paths[fileset]))
    ds = ds.initialize(EX)
    ds.check_valid()
    name = case['name']
    sig = tuple(ds.shape.sig)
    roi = case['roi']
    masks = recipes.make_masks(fileset)
    corr = ds.get_correction_data() if kind == 'seq' else None
    pick_roi = roi if roi is not None else np.ones(tuple(ds.shape.nav), dtype=bool)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = UDFRunner([SumUDF(), SumSigUDF(), mask_udf(masks)]).run_for_dataset(
            ds, EX, roi=roi, corrections=corr).buffers
        picked = UDFRunner([PickUDF()]).run_for_dataset(ds, EX, roi=pick_roi, corrections=corr).buffers[0]
        raw = UDFRunner([PickUDF()]).run_for_dataset(ds, EX, roi=pick_roi, corrections=None).buffers[0]
    raw = np.array(raw['intensity'].data).reshape((-1,) + sig)
    frames = raw.astype(recipes.stored_dtype(fileset))
    assert np.array_equal(frames, raw)
    out[f"{name}__sum"] = np.array(res[0]['intensity'].data)
    out[f"{name}__sumsig"] = np.array(res[1]['intensity'].data)
    out[f"{name}__masks"] = np.array(res[2]['intensity'].data)
    picked = np.array(picked['intensity'].data).reshape((-1,) + sig)
    out[f"{name}__picked_dtype"] = np.array(picked.dtype.str)
    out[f"{name}__picked_sumsig"] = picked.reshape(len(picked), -1).sum(axis=1, dtype=np.float64)
    if kind != 'empad':
        out[f"{name}__picked"] = picked
    out[f"{name}__sha_frames"] = np.stack([sha(f) for f in frames])
    out[f"{name}__crops"] = np.stack([recipes.crop(fileset)(f) for f in frames])
    out[f"{name}__image_count"] = np.int64(ds.meta.image_count)
    out[f"{name}__shape"] = np.array(tuple(ds.shape), dtype=np.int64)
    out[f"{name}__dtype"] = np.array(np.dtype(ds.dtype).str)
    out[f"{name}__raw_dtype"] = np.array(np.dtype(ds.meta.raw_dtype).str)
    if kind == 'seq':
        out[f"{name}__footer"] = np.int64(ds._footer_size)
        if corr.get_dark_frame() is not None:
            out[f"{name}__dark"] = np.array(corr.get_dark_frame())
        if corr.get_gain_map() is not None:
            out[f"{name}__gain"] = np.array(corr.get_gain_map())
        excluded = corr.get_excluded_pixels()
        if excluded is not None:
            # the map geometry of the recipe is one the reference's crop takes: a mask of the frame's own shape
            assert tuple(excluded.shape) == sig, (excluded.shape, sig)
            out[f"{name}__excluded"] = np.array(excluded.coords, dtype=np.int64)
    print(name, tuple(ds.shape), np.dtype(ds.dtype), int(ds.meta.image_count),
          {k.split('__')[1]: (v.dtype.str, v.shape) for k, v in out.items() if k.startswith(name + '__')},
          flush=True)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {fs: recipes.write_fileset(fs, tmp) for fs in recipes.FILESETS}
        for case in recipes.CASES:
            run(case, out, paths)
    path = os.path.join(HERE, 'records.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
