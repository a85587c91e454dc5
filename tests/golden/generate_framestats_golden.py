#!/usr/bin/env python
"""
Generate tests/golden/framestats.npz with the REAL Python reference's FEMUDF and LogsumUDF (LiberTEM,
/root/reference/src), through the same third-party stand-ins as generate_golden.py
(`tests/golden/refshim/`).  Inputs come from the seeded recipes in framestats_recipes.py; only the
results and an input checksum are stored.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_framestats_golden.py
"""
import os
import sys
import hashlib
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

import framestats_recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.FEM import FEMUDF  # noqa: E402
from libertem.udf.logsum import LogsumUDF  # noqa: E402
from libertem.io.dataset.memory import MemoryDataSet  # noqa: E402
from libertem.io.corrections import CorrectionSet  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def run(case, udf, key, out):
    data, roi, corr = framestats_recipes.make_case(case)
    ds = MemoryDataSet(data=data.copy(), num_partitions=case['num_partitions'], sig_dims=2,
                       sync_offset=case.get('sync_offset', 0))
    corrections = None if corr is None else CorrectionSet(dark=corr[0], gain=corr[1])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = UDFRunner([udf]).run_for_dataset(ds, EX, roi=roi, corrections=corrections).buffers[0]
    out[f"{case['name']}__{key}"] = np.array(res[key].data)
    out[f"{case['name']}__sha_data"] = sha(data)
    print(case['name'], res[key].data.dtype.str, res[key].data.shape)


def main():
    out = {}
    for case in framestats_recipes.FEM_CASES:
        run(case, FEMUDF(center=case['center'], rad_in=case['rad_in'], rad_out=case['rad_out']),
            'intensity', out)
    for case in framestats_recipes.LOGSUM_CASES:
        run(case, LogsumUDF(), 'logsum', out)
    path = os.path.join(HERE, 'framestats.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
