#!/usr/bin/env python
"""
Generate tests/golden/stddev.npz with the REAL Python reference's StdDevUDF (LiberTEM,
/root/reference/src), through the same third-party stand-ins as generate_golden.py
(`tests/golden/refshim/`).  Inputs come from the seeded recipes in stddev_recipes.py; only the
results and an input checksum are stored.

The reference runs with use_numba=False: under the stand-in `numba.njit` its numba loops run as
plain Python, where NumPy 2 promotion makes the tail loop of `process_tile` accumulate in float32
for float32 tiles.  The ndarray branch computes in the sum dtype throughout.

Skipped (exit 0) if /root/reference is absent.

Usage:  python tests/golden/generate_stddev_golden.py
"""
import os
import sys
import hashlib

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/src'

if not os.path.isdir(REF):
    print("reference not present, nothing to do")
    sys.exit(0)

sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import stddev_recipes  # noqa: E402

from libertem.udf.base import UDFRunner  # noqa: E402
from libertem.udf.stddev import StdDevUDF  # noqa: E402
from libertem.io.dataset.memory import MemoryDataSet  # noqa: E402
from libertem.io.corrections import CorrectionSet  # noqa: E402
from libertem.executor.inline import InlineJobExecutor  # noqa: E402

EX = InlineJobExecutor(inline_threads=1)
KEYS = ('sum', 'varsum', 'num_frames', 'var', 'std', 'mean')


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def main():
    out = {}
    for case in stddev_recipes.STDDEV_CASES:
        data, roi, corr = stddev_recipes.make_stddev_case(case)
        ds = MemoryDataSet(data=data.copy(), num_partitions=case['num_partitions'], sig_dims=2,
                           tileshape=case.get('tileshape'), sync_offset=case.get('sync_offset', 0))
        corrections = None if corr is None else CorrectionSet(dark=corr[0], gain=corr[1])
        udf = StdDevUDF(use_numba=False, **case.get('udf_kwargs', {}))
        res = UDFRunner([udf]).run_for_dataset(ds, EX, roi=roi, corrections=corrections).buffers[0]
        for k in KEYS:
            out[f"{case['name']}__{k}"] = np.array(res[k].data)
        out[f"{case['name']}__sha_data"] = sha(data)
        print(case['name'], {k: (res[k].data.dtype.str, res[k].data.shape) for k in KEYS})
    path = os.path.join(HERE, 'stddev.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == '__main__':
    main()
