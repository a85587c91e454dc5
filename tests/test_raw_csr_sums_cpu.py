"""
The sums on the stored entries of sparse frames, without a GPU: include/ltmi.h declares the entries and
libertem_amd/hip.py binds them with as many arguments, the two UDFs announce that they take sparse views, and on
a CPU executor they still give the reference's arrays (tests/golden/raw_csr.npz) over a raw_csr dataset.
"""
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))

import raw_csr_recipes as recipes  # noqa: E402

from libertem_amd.api import Context  # noqa: E402
from libertem_amd.executor.inline import InlineJobExecutor  # noqa: E402
from libertem_amd.udf.sum import SumUDF  # noqa: E402
from libertem_amd.udf.sumsigudf import SumSigUDF  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'raw_csr.npz'))
CASES = {c['name']: c for c in recipes.CASES}
ENTRIES = {'ltmi_csr_sum_sig': 13, 'ltmi_csr_sum_frames_workspace': 1, 'ltmi_csr_sum_frames': 14,
           'ltmi_csr_last_kernel': 0}


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


def test_python_wrappers():
    from libertem_amd import hip
    assert hip.csr_last_kernel() == '' or hip.csr_last_kernel().startswith('k_csr_sum_')
    # (the size is host arithmetic: splits x pixels x 8 bytes, at least one int64 per pixel)
    for n_px in (1, 117, 4096, 4097, 256 * 256, 512 * 512):
        nbytes = hip.csr_sum_frames_workspace(n_px)
        assert nbytes % (8 * n_px) == 0 and nbytes >= 8 * n_px
    assert hip.csr_sum_frames_workspace(0) == 0
    for fn, last in ((hip.csr_sum_sig, 'accumulate'), (hip.csr_sum_frames, 'workspace_ptr')):
        params = list(inspect.signature(fn).parameters)
        assert params[:9] == list(inspect.signature(hip.csr_densify).parameters)[:9]
        assert params[-2:] == [last, 'stream']


def test_udfs_take_sparse_views():
    from libertem_amd.udf.stddev import StdDevUDF
    from libertem_amd.udf.logsum import LogsumUDF
    assert SumUDF.ACCEPTS_CSR_VIEWS is True and SumSigUDF.ACCEPTS_CSR_VIEWS is True
    assert StdDevUDF.ACCEPTS_CSR_VIEWS is False and LogsumUDF.ACCEPTS_CSR_VIEWS is False


@pytest.mark.parametrize('name', ('dtype_u2', 'dtype_i4', 'dtype_f4', 'sync_p3_roi', 'sync_m4', 'parts3', 'nan_f4'))
def test_cpu_executor_gives_the_reference_arrays(tmp_path, name):
    case = CASES[name]
    inp = recipes.make_case(case)
    ctx = Context(executor=InlineJobExecutor())
    try:
        ds = ctx.load('raw_csr', path=recipes.write_files(case, inp, str(tmp_path)),
                      sync_offset=case['sync_offset'], num_partitions=case['num_partitions'])
        got_sum = ctx.run_udf(dataset=ds, udf=SumUDF(), roi=inp['roi'])['intensity'].data
        got_sig = ctx.run_udf(dataset=ds, udf=SumSigUDF(), roi=inp['roi'])['intensity'].data
    finally:
        ctx.close()
    frames = recipes.dense_frames(inp)
    n, so = frames.shape[0], case['sync_offset']
    dense = np.zeros(frames.shape, dtype=np.float64)
    for p in range(n):
        if 0 <= p + so < n:
            dense[p] = frames[p + so]
    dense = dense.reshape(recipes.NAV + recipes.SIG)
    roi = inp['roi'] if inp['roi'] is not None else np.ones(recipes.NAV, dtype=bool)
    # float32 sums of at most 35 terms per pixel / 117 per frame: 1e-5 relative to the sum of magnitudes
    mag = np.abs(np.nan_to_num(dense))
    for got, gold, tol in ((got_sum, GOLDEN[f'{name}__sum'], 1e-5 * mag[roi].sum(axis=0) + 1e-30),
                           (got_sig, GOLDEN[f'{name}__sumsig'], 1e-5 * mag.sum(axis=(2, 3)) + 1e-30)):
        assert got.shape == gold.shape
        assert np.array_equal(np.isnan(got), np.isnan(gold))
        fin = np.isfinite(gold)
        assert np.all(np.abs(got - gold)[fin] <= tol[fin])
