"""
bench.py without a GPU: what --dump-outputs writes (names, dtypes, the 64 MB cap) and the argument checks
that run before the GPU is touched.
"""
import os
import subprocess
import sys

import numpy as np

import bench
from libertem_amd.analysis.base import AnalysisResult, AnalysisResultSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Buffer:
    """what a UDF result maps a name to: an object with .data"""

    def __init__(self, data):
        self.data = data


def test_dump_of_a_udf_result(tmp_path):
    intensity = np.arange(24, dtype=np.float32).reshape((2, 3, 4))
    count = np.arange(6, dtype=np.uint32).reshape((2, 3))
    spec = (np.arange(4) + 1j * np.arange(4, 8)).astype(np.complex64)
    res = {'intensity': _Buffer(intensity), 'count': _Buffer(count), 'spec': _Buffer(spec)}
    bench.dump_outputs(bench.result_arrays(res), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['count.npy', 'intensity.npy', 'spec_imag.npy', 'spec_real.npy']
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert got['intensity'].dtype == np.float32 and np.array_equal(got['intensity'], intensity)
    assert got['count'].dtype == np.float64 and np.array_equal(got['count'], count)
    assert got['spec_real'].dtype == np.float32 and np.array_equal(got['spec_real'], spec.real)
    assert got['spec_imag'].dtype == np.float32 and np.array_equal(got['spec_imag'], spec.imag)


def test_dump_of_an_analysis_result(tmp_path):
    y = np.linspace(0, 1, 12).reshape((3, 4))
    raw = (np.ones((1, 2, 3, 4)) * (1 + 2j)).astype(np.complex128)
    res = AnalysisResultSet([AnalysisResult(y, key='y'), AnalysisResult(y.astype(np.float32), key='x')],
                            raw_results=raw)
    bench.dump_outputs(bench.result_arrays(res), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['raw_results_imag.npy', 'raw_results_real.npy', 'x.npy', 'y.npy']
    assert np.load(tmp_path / 'y.npy').dtype == np.float64 and np.load(tmp_path / 'x.npy').dtype == np.float32
    assert np.array_equal(np.load(tmp_path / 'raw_results_imag.npy'), raw.imag)
    assert np.load(tmp_path / 'raw_results_real.npy').dtype == np.float64


def test_dump_above_the_cap_is_a_fixed_sample_of_rows(tmp_path):
    big = np.random.default_rng(1).random((1000, 64))                # 512 000 bytes
    small = np.arange(2000, dtype=np.float32)                         # 8 000 bytes
    arrays = [('big', big), ('small', small)]
    for d in ('a', 'b'):
        bench.dump_outputs(arrays, str(tmp_path / d), limit=100_000)
    a, b = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'b' / 'big.npy')
    s = np.load(tmp_path / 'a' / 'small.npy')
    assert np.array_equal(a, b) and np.array_equal(s, np.load(tmp_path / 'b' / 'small.npy'))
    assert a.nbytes + s.nbytes <= 100_000 and a.shape[1] == 64 and len(a) > 100 and len(s) > 100
    # whole rows of the original, in their order; 1-D arrays: a sample of their elements
    rows = [int(np.flatnonzero((big == r).all(axis=1))[0]) for r in a]
    assert rows == sorted(set(rows))
    assert np.all(np.isin(s, small)) and np.all(np.diff(s) > 0)


def test_dump_below_the_cap_is_complete(tmp_path):
    big = np.random.default_rng(1).random((1000, 64))
    bench.dump_outputs([('big', big)], str(tmp_path))
    assert np.array_equal(np.load(tmp_path / 'big.npy'), big)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr
