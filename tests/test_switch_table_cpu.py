"""
The dispatch overrides of the native library are declared once: the tuning record (csrc/ltmi_tuning.h) and the
LTMI_* environment switches (csrc/ltmi_switches.h).  Host only: a stand-alone program checks both headers under
AddressSanitizer / UBSan, and the sources are read as text for what must not come back.
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'libertem_amd', 'csrc')
ROW = re.compile(r'X\((LTMI_[A-Z0-9_]+), (once|every), (behaviour|measurement|garbage), "((?:[^"\\]|\\.)*)"\)')


def _read(path):
    with open(path) as f:
        return f.read()


def _header_rows():
    rows = ROW.findall(_read(os.path.join(CSRC, 'ltmi_switches.h')))
    assert len(rows) >= 30 and len({r[0] for r in rows}) == len(rows)
    return rows


def _doc_tables():
    """the rows of the two tables of INTEGRATION.md's "Environment switches": {name: (read, class, meaning)}"""
    doc = _read(os.path.join(ROOT, 'INTEGRATION.md'))
    section = doc[doc.index('## Environment switches'):doc.index('## Build / load contract')]
    native, python = section.split('### Python / bench only')
    assert '### Native library' in native

    def rows(text):
        out = {}
        for name, read, cls, meaning in re.findall(r'^\| `(LTMI_[A-Z0-9_]+)` \| ([^|]+) \| ([a-z]+) \| (.+) \|$', text,
                                                   flags=re.M):
            assert name not in out, name
            out[name] = (read.strip(), cls, meaning)
        return out
    return rows(native), rows(python)


def test_tuning_and_switch_tables_native(tmp_path):
    """tests/native/tuning_table.cpp: Tuning::set accepts exactly the documented triples, every predicate equals the
    written-out truth table, `every` switches follow the environment and `once` switches keep their first value"""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / 'tuning_table')
    build = subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-g', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=all', '-o', exe,
                            os.path.join(ROOT, 'tests', 'native', 'tuning_table.cpp')],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    env = {k: v for k, v in os.environ.items() if not k.startswith('LTMI_') and k != 'LD_PRELOAD'}
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert run.returncode == 0 and 'tuning_table: ok' in run.stdout, run.stdout


def test_environment_is_read_in_one_header():
    for path in sorted(glob.glob(os.path.join(CSRC, '*'))):
        if os.path.basename(path) != 'ltmi_switches.h':
            assert 'getenv(' not in _read(path), path
    assert _read(os.path.join(CSRC, 'ltmi_switches.h')).count('getenv(') == 2       # once / every, one accessor


def test_no_bare_variant_codes():
    """the launchers ask the tuning record by name: the misnamed field that held the codes is gone from every source, and
    no .hip file compares a tuning field with a literal 30..42"""
    sources = [p for pat in ('libertem_amd/**/*', 'include/*', 'tests/**/*.py', 'tests/native/*')
               for p in glob.glob(os.path.join(ROOT, pat), recursive=True)
               if os.path.isfile(p) and os.path.splitext(p)[1] in ('.hip', '.h', '.cpp', '.inc', '.py')]
    assert len(sources) > 100
    old_field = 'tune_ksplit' + '_ring'
    for path in sources:
        assert old_field not in _read(path), path
    code = r'(?:3[0-9]|4[0-2])\b'
    field = r'\btune\s*(?:\.|->)\s*(?:mt|waves|ksplit|variant)\b'
    compare = re.compile(rf'{field}\s*(?:==|!=|<=|>=|<|>)\s*{code}|\b{code}\s*(?:==|!=|<=|>=|<|>)\s*(?:\w+(?:\.|->))*{field[2:]}')
    hips = sorted(glob.glob(os.path.join(CSRC, '*.hip')))
    assert len(hips) >= 20
    for path in hips:
        for no, line in enumerate(_read(path).splitlines(), 1):
            assert not compare.search(line), f"{path}:{no}: {line.strip()}"
    assert compare.search('if (m->tune.variant == 37) return true;') and compare.search('x = 41 != m->tune.variant')
    assert not compare.search('if (m->tune.mt != 1 && m->n_px >= KC64)')


def test_switch_table_of_the_documentation():
    """INTEGRATION.md lists the native switches name for name and class for class (and read for read); its Python part
    has a row for every LTMI_* name in the package's Python sources"""
    header = {name: (read, cls, meaning) for name, read, cls, meaning in _header_rows()}
    native, python = _doc_tables()
    assert sorted(native) == sorted(header)
    for name, (read, cls, meaning) in header.items():
        assert native[name][:2] == (read, cls), name
        assert native[name][2] == meaning, name
    # (every switch the sources use through the accessors is one of the header's)
    used = set()
    for path in glob.glob(os.path.join(CSRC, '*')):
        used |= set(re.findall(r'switch_(?:text|set|int|is)<(?:ltmi::)?(LTMI_[A-Z0-9_]+)>', _read(path)))
    assert used == set(header), sorted(used ^ set(header))
    in_python = set()
    for path in glob.glob(os.path.join(ROOT, 'libertem_amd', '**', '*.py'), recursive=True):
        in_python |= set(re.findall(r'LTMI_[A-Z0-9_]+', _read(path)))
    assert len(in_python) >= 15
    assert not in_python - set(python), sorted(in_python - set(python))
    for name, (read, cls, meaning) in python.items():
        assert cls in ('behaviour', 'measurement', 'garbage'), name


def test_variant_enum_mirrors_the_header():
    from libertem_amd import hip
    hdr = _read(os.path.join(ROOT, 'include', 'ltmi.h'))
    body = hdr[hdr.index('enum ltmi_variant {'):]
    body = body[:body.index('};')]
    declared = {name: int(value) for name, value in re.findall(r'LTMI_VARIANT_([A-Z0-9_]+) = (\d+)', body)}
    assert len(declared) == 13
    assert {v.name: int(v) for v in hip.Variant} == declared
    assert hip.Variant.SPARSE_SELL == 41 and isinstance(hip.Variant.SPARSE_SELL, int)
