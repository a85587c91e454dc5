"""
The dispatch overrides select the kernels they selected before they were given names (-m gpu).

tests/golden/dispatch_names.json was recorded by tests/golden/generate_dispatch_names.py on the commit before the
tuning record (csrc/ltmi_tuning.h) and the switch table (csrc/ltmi_switches.h): one `last_kernel()` string -- or the
error of a refused tuning triple -- per (stack, tile dtype, frames, row list, tuning triple, environment).  Every case
is replayed here: the same string, and a result equal to the float64 NumPy product within the bound of the route's own
kernel tests, in units of sum |a||b|: 2e-6 where the name shows exact float16 products (",f16"), k_scatter or
k_dense_split, 1e-5 for the other float32 results, 1e-12 for float64 results, integers bit for bit.  Where the name
cannot show an override (LTMI_KSPLIT_STRIDED: the order of the parts of a pixel split) the fixture holds a CRC of the
result, whose float32 rounding does.  The cases of one environment run in one fresh child process, since the library
caches some switches per process; one child at a time, each under a timeout, and none after a child that died.

The two tests of the fixture itself read JSON only and run without a GPU.
"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_generator():
    spec = importlib.util.spec_from_file_location('generate_dispatch_names',
                                                  os.path.join(HERE, 'golden', 'generate_dispatch_names.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_generator()
GROUPS = GEN.env_groups()
with open(os.path.join(HERE, 'golden', 'dispatch_names.json')) as _f:
    RECORDED = {e['id']: e for e in json.load(_f)['cases']}
_died = []            # the first child that ended abnormally: nothing more is started after it


def test_fixture_holds_the_generators_cases():
    assert sorted(RECORDED) == sorted(c['id'] for c in GEN.CASES)
    for c in GEN.CASES:
        e = RECORDED[c['id']]
        want = {k: c[k] for k in ('recipe', 'tile', 'frames', 'rows', 'env')}
        want['tuning'] = None if c['tuning'] is None else list(c['tuning'])
        assert {k: e[k] for k in want} == want, c['id']
        assert ('kernel' in e) != ('error' in e), c['id']
        assert e.get('note') == GEN.NOTES.get(c['recipe']), c['id']
        assert ('crc' in e) == bool(c.get('bits')), c['id']


def test_fixture_covers_every_route_and_override():
    names = [e['kernel'] for e in RECORDED.values() if 'kernel' in e]
    for part in ('k_dense_lds<', 'VALU columns', ',rows', 'k_dense_mfma<', 'column blocks', 'k_dense_split',
                 'k_dense_fold<', 'k_dense_fold16<', 'k_dense_generic', 'k_dense_lds64', 'k_dense_mfma_f64',
                 'k_sell_apply', 'k_bell_', 'k_scatter', 'banded', 'k_labels', ' +nf', ' exact-int'):
        assert any(part in n for n in names), part
    assert any('k_dense_lds<' in n and ',f16' in n for n in names)
    assert any('k_dense_lds<' in n and ',f16' not in n for n in names)
    assert not any('noDMA' in n or 'noMFMA' in n for n in names)
    codes = {e['tuning'][1] for e in RECORDED.values() if e['tuning'] and e['tuning'][0] == 0 and 'kernel' in e}
    assert codes >= {30, 33, 34, 35, 36, 37, 38, 40, 41, 42} and not codes & {31, 32}
    envs = {f"{k}={v}" for e in RECORDED.values() for k, v in e['env'].items()}
    assert envs >= {'LTMI_DENSE_F32_INSTR=1', 'LTMI_DENSE_F16=0', 'LTMI_BELL_F16=0', 'LTMI_SPARSE_SCATTER=0',
                    'LTMI_SPARSE_SCATTER=1', 'LTMI_SPARSE_BAND=0', 'LTMI_SPARSE_LABELS=1', 'LTMI_DENSE_FOLD=0',
                    'LTMI_DENSE_FOLD=2', 'LTMI_SPLIT=1', 'LTMI_ALIGNED_DMA_ONLY=1', 'LTMI_NONFINITE_GUARD=0',
                    'LTMI_MIB_WORDS=1', 'LTMI_FFT_FUSED=0'}
    # the order of the parts of a pixel split: unset, contiguous and in turn give one name and three roundings
    order = [e for e in RECORDED.values() if e.get('bits')]
    assert {e['env'].get('LTMI_KSPLIT_STRIDED') for e in order} == {None, '0', '1'}
    assert len({e['kernel'] for e in order}) == 1 and len({e['crc'] for e in order}) == 3
    assert not any('ABLATE' in v for v in envs)
    assert any('error' in e for e in RECORDED.values())


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(GROUPS)),
                         ids=[','.join(f'{k}={v}' for k, v in env.items()) or 'default' for env, _ in GROUPS])
def test_recorded_dispatch(index):
    pytest.importorskip("torch")
    assert not _died, f"not run: the child of {_died[0]} ended abnormally"
    env, members = GROUPS[index]
    results, rc, output = GEN.run_group(index)
    if results is None:
        _died.append(env or 'the default environment')
        pytest.fail(f"the child ended with {rc}:\n{output}")
    for c in members:
        want, got = RECORDED[c['id']], results[c['id']]
        print(c['id'], got)
        if 'error' in want:
            assert got.get('error') == want['error'], (c['id'], got)
            continue
        assert got.get('kernel') == want['kernel'], (c['id'], got, want['kernel'])
        assert got.get('crc') == want.get('crc'), (c['id'], got, want.get('crc'))
        if 'worst' in got:
            assert got['worst'] <= 1.0, (c['id'], got)
        else:
            assert got['kernel'] == '(no row-list kernel)', (c['id'], got)
