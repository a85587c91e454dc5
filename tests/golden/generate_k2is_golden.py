#!/usr/bin/env python
"""
Generate tests/golden/k2is.npz with the REAL Python reference's K2ISDataSet + SumSigUDF + ApplyMasksUDF +
PickUDF (LiberTEM, /root/reference/src), through the same third-party stand-ins as generate_golden.py
(`tests/golden/refshim/`, here also one for `ncempy`: a .gtg without scan geometry).  The 8-file sets come from
the seeded recipes in k2is_recipes.py (written by tests/k2is_synth.py); only small results are stored: the UDF
results, the sha256 and a crop of every decoded frame, image_count, shape and the effective sync offset.

One thing differs from a stock run: `Sector.first_block_with_search` looks for the first shutter-active
block in steps of 32 * 8 * 50 blocks (400 frames) before it bisects, and reads past the end of a file of 4
frames; its step is set to 32 blocks (one frame) here.  The bisection itself is the reference's.

The reference decodes in interpreted Python under the numba stand-in: several minutes in all.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_k2is_golden.py
"""
import os
import sys
import hashlib
import tempfile
import functools
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

import k2is_recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.masks import ApplyMasksUDF  # noqa: E402
from libertem.udf.raw import PickUDF  # noqa: E402
from libertem.udf.sumsigudf import SumSigUDF  # noqa: E402
from libertem.io.dataset import k2is as ref_k2is  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

ref_k2is.Sector.first_block_with_search = functools.partialmethod(
    ref_k2is.Sector.first_block_with_search, step=ref_k2is.BLOCKS_PER_SECTOR_PER_FRAME)

EX = InlineJobExecutor(inline_threads=1)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def run(case, out, paths):
    ds = ref_k2is.K2ISDataSet(path=paths[case['fileset']], sync_offset=case['sync_offset'])
    ds = ds.initialize(EX)
    masks = k2is_recipes.make_masks()
    udfs = [SumSigUDF(), ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                                       mask_dtype=masks.dtype), PickUDF()]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = UDFRunner(udfs).run_for_dataset(ds, EX, roi=None).buffers
    name = case['name']
    picked = np.array(res[2]['intensity'].data).reshape((-1,) + tuple(ds.shape.sig))
    frames = picked.astype(np.uint16)       # (beside float32 UDFs the reference decodes into float32: exact here)
    assert np.array_equal(frames, picked)
    written = k2is_recipes.make_frames(case['fileset'])
    print(name, 'frames of the set at the scan positions:',
          [[g for g in range(len(written)) if np.array_equal(written[g], f)] or int(f.any()) for f in frames])
    out[f"{name}__sumsig"] = np.array(res[0]['intensity'].data)
    out[f"{name}__masks"] = np.array(res[1]['intensity'].data)
    out[f"{name}__sha_frames"] = np.stack([sha(f) for f in frames])
    out[f"{name}__crops"] = np.stack([f[k2is_recipes.CROP] for f in frames])
    out[f"{name}__image_count"] = np.int64(ds._image_count)
    out[f"{name}__shape"] = np.array(tuple(ds.shape), dtype=np.int64)
    out[f"{name}__sync_offset"] = np.int64(ds._sync_offset)
    out[f"{name}__first_offsets"] = np.array(ds._start_offsets, dtype=np.int64)
    out[f"{name}__last_offsets"] = np.array(ds._last_offsets, dtype=np.int64)
    print(name, tuple(ds.shape), int(ds._image_count), int(ds._sync_offset), out[f"{name}__sumsig"].dtype.str,
          out[f"{name}__masks"].dtype.str, out[f"{name}__sumsig"].ravel(), flush=True)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {fs: k2is_recipes.write_fileset(fs, tmp)[0] for fs in k2is_recipes.FILESETS}
        for case in k2is_recipes.CASES:
            run(case, out, paths)
    path = os.path.join(HERE, 'k2is.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
