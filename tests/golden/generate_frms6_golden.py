#!/usr/bin/env python
"""
Generate tests/golden/frms6.npz with the REAL Python reference's FRMS6DataSet + SumUDF + SumSigUDF +
ApplyMasksUDF + PickUDF (LiberTEM, /root/reference/src), through the same third-party stand-ins as
generate_golden.py (`tests/golden/refshim/`).  The sets come from the seeded recipes in frms6_recipes.py
(written by tests/frms6_synth.py); only small results are stored: the UDF results with the dataset's own
corrections, the sha256 and a crop of every picked raw frame, the dark frame, the gain map as the reference
read it, shape, dtype and image_count.

Two things differ from `Context.run_udf` of the reference, neither changes what is computed:
  * the UDFs run through `UDFRunner.run_for_dataset`, as in the other generators; `Context.run_udf` would pass
    `dataset.get_correction_data()` when `corrections` is None (api.py), which is done by hand here.  The raw
    picks are the same run without corrections.
  * `get_correction_data()` of a set with neither a dark frame nor a gain map (set E) is an empty
    CorrectionSet; it is passed as it is.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_frms6_golden.py
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

import frms6_recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.masks import ApplyMasksUDF  # noqa: E402
from libertem.udf.raw import PickUDF  # noqa: E402
from libertem.udf.sum import SumUDF  # noqa: E402
from libertem.udf.sumsigudf import SumSigUDF  # noqa: E402
from libertem.io.dataset import frms6 as ref_frms6  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def mask_udf(masks):
    return ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                         mask_dtype=masks.dtype)


def run(case, out, paths):
    ds = ref_frms6.FRMS6DataSet(**frms6_recipes.load_kwargs(case, paths[case['fileset']]))
    ds = ds.initialize(EX)
    name = case['name']
    sig = tuple(ds.shape.sig)
    roi = case['roi']
    masks = frms6_recipes.make_masks(case['fileset'])
    corr = ds.get_correction_data()
    udfs = [SumUDF(), SumSigUDF(), mask_udf(masks)]
    if name == 'E':
        udfs.append(mask_udf(frms6_recipes.make_int_masks(case['fileset'])))
    pick_roi = roi if roi is not None else np.ones(tuple(ds.shape.nav), dtype=bool)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = UDFRunner(udfs).run_for_dataset(ds, EX, roi=roi, corrections=corr).buffers
        picked = UDFRunner([PickUDF()]).run_for_dataset(ds, EX, roi=pick_roi, corrections=corr).buffers[0]
        raw = UDFRunner([PickUDF()]).run_for_dataset(ds, EX, roi=pick_roi, corrections=None).buffers[0]
    raw = np.array(raw['intensity'].data).reshape((-1,) + sig)
    frames = raw.astype(np.uint16)          # (a set with offset correction reads into float32: exact here)
    assert np.array_equal(frames, raw)
    out[f"{name}__sum"] = np.array(res[0]['intensity'].data)
    out[f"{name}__sumsig"] = np.array(res[1]['intensity'].data)
    out[f"{name}__masks"] = np.array(res[2]['intensity'].data)
    if name == 'E':
        out[f"{name}__int_masks"] = np.array(res[3]['intensity'].data)
    out[f"{name}__picked"] = np.array(picked['intensity'].data).reshape((-1,) + sig)
    out[f"{name}__sha_frames"] = np.stack([sha(f) for f in frames])
    out[f"{name}__crops"] = np.stack([f[frms6_recipes.crop(case['fileset'])] for f in frames])
    out[f"{name}__image_count"] = np.int64(ds.meta.image_count)
    out[f"{name}__shape"] = np.array(tuple(ds.shape), dtype=np.int64)
    out[f"{name}__dtype"] = np.array(np.dtype(ds.dtype).str)
    out[f"{name}__raw_dtype"] = np.array(np.dtype(ds.meta.raw_dtype).str)
    if corr.get_dark_frame() is not None:
        out[f"{name}__dark"] = np.array(corr.get_dark_frame())
    if corr.get_gain_map() is not None:
        out[f"{name}__gain"] = np.array(corr.get_gain_map())
    print(name, tuple(ds.shape), np.dtype(ds.dtype), int(ds.meta.image_count),
          {k.split('__')[1]: (v.dtype.str, v.shape) for k, v in out.items() if k.startswith(name + '__')},
          flush=True)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {fs: frms6_recipes.write_fileset(fs, tmp) for fs in frms6_recipes.FILESETS}
        for case in frms6_recipes.CASES:
            run(case, out, paths)
    path = os.path.join(HERE, 'frms6.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
