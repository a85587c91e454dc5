#!/usr/bin/env python
"""
Generate tests/golden/raw_csr.npz with the REAL Python reference's RawCSRDataSet + ApplyMasksUDF + SumUDF +
SumSigUDF (LiberTEM, /root/reference/src), through the same third-party stand-ins as generate_golden.py
(`tests/golden/refshim/`).  Inputs come from the seeded recipes in raw_csr_recipes.py; only the results and
input checksums are stored.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_raw_csr_golden.py
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

import raw_csr_recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.masks import ApplyMasksUDF  # noqa: E402
from libertem.udf.sum import SumUDF  # noqa: E402
from libertem.udf.sumsigudf import SumSigUDF  # noqa: E402
from libertem.io.dataset.raw_csr import RawCSRDataSet  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def run(case, out, tmp):
    inp = raw_csr_recipes.make_case(case)
    path = raw_csr_recipes.write_files(case, inp, tmp, name=case['name'])
    ds = RawCSRDataSet(path=path, sync_offset=case['sync_offset'], num_partitions=case['num_partitions'])
    ds = ds.initialize(EX)
    masks = inp['masks']
    udfs = [ApplyMasksUDF(mask_factories=lambda: masks, use_sparse=False, mask_count=len(masks),
                          mask_dtype=masks.dtype), SumUDF(), SumSigUDF()]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = UDFRunner(udfs).run_for_dataset(ds, EX, roi=inp['roi']).buffers
    name = case['name']
    out[f"{name}__masks"] = np.array(res[0]['intensity'].data)
    out[f"{name}__sum"] = np.array(res[1]['intensity'].data)
    out[f"{name}__sumsig"] = np.array(res[2]['intensity'].data)
    for key in ('indptr', 'indices', 'data', 'masks'):
        out[f"{name}__sha_{key}"] = sha(inp[key])
    print(name, out[f"{name}__masks"].dtype.str, out[f"{name}__masks"].shape, out[f"{name}__sum"].dtype.str)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in raw_csr_recipes.CASES:
            run(case, out, tmp)
    path = os.path.join(HERE, 'raw_csr.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
