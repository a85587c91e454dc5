"""
The two .mib decode kernels of csrc/ltmi_mib.hip at their edges (-m gpu), through the C ABI:

  k_mib_decode    one 64-bit word per thread: every shape whose payload is not a whole number of 16-byte
                  chunks (or whose quad chip row is not), and every shape while LTMI_MIB_WORDS is set;
  k_mib_decode16  16 bytes of output per thread: the common shapes.

Every decode goes into the middle of a buffer filled with 0xCD whose guard bytes are checked afterwards,
from a source whose header size, frame stride and device address the test chooses, and is compared bit
for bit with the frames the encoder of tests/golden/recipes.py started from AND with the pixel-by-pixel
oracle (oracle/mib.py).  `hip.mib_last_kernel()` pins which kernel ran.  Integer work: bit-exact.
"""
import threading

import numpy as np
import pytest

import recipes

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

POISON = 0xCD
PAD = 0xA5
GUARD = 68          # bytes before the output: a multiple of every element size, not of 16
TAIL = 64           # guard bytes behind it
NAMES = {('u', 8): 'u8', ('u', 16): 'u16', ('u', 32): 'u32', ('r', 1): 'r1', ('r', 6): 'r6',
         ('r', 12): 'r12', ('r', 24): 'r24'}

# (frames, header bytes (None: 384 per chip, as written by the detector), stride padding, device offset)
GEOMETRIES = [
    (3, None, 0, 0),
    (1, 13, 5, 0),          # payloads at odd addresses, frames apart by an odd number of extra bytes
    (3, 13, 5, 0),
    (3, None, 5, 3),
    (1, None, 0, 3),
]


def _case(kind, bits, sig, quad=False, frames=3):
    name = f"{kind}{bits}{'_quad' if quad else ''}_{sig[0]}x{sig[1]}"
    seed = 7000 + bits * 131 + sig[0] * 17 + sig[1] + (5 if quad else 0)
    return dict(name=name, kind=kind, bits=bits, sig=tuple(sig), frames=(frames,), nav=(1, frames),
                quad=quad, seed=seed)


def _payload_bytes(case):
    h, w = case['sig']
    return h * w * case['bits'] // 8 if case['kind'] == 'u' else \
        h * w * {1: 1, 6: 8, 12: 16, 24: 32}[case['bits']] // 8


def _storage(case):
    if case['bits'] == 24:
        return np.dtype(np.float32)
    return np.dtype({1: np.uint8, 6: np.uint8, 8: np.uint8, 12: np.uint16, 16: np.uint16,
                     32: np.uint32}[case['bits']])


def kernel_name(case, wide, storage):
    mode = NAMES[(case['kind'], case['bits'])]
    if case['bits'] == 24 and np.dtype(storage) == np.float32:
        mode = 'r24f'
    quad = ',quad' if case.get('quad') and case['kind'] == 'r' else ''
    return f"k_mib_decode{'16' if wide else ''}<{mode}{quad}>"


_PREPARED = {}


def prepared(case):
    """-> (frames of the case's first file, their payloads, the oracle's decode of them): encoded and
    decoded on the host once per case, shared by every test, never written to"""
    got = _PREPARED.get(case['name'])
    if got is None:
        from oracle import mib as omib
        frames, files, _ = recipes.make_mib_case(case)
        blob = sorted(files.items())[0][1]
        n = case['frames'][0]
        chips = 4 if case.get('quad') else 1
        hdr, pay = 384 * chips, _payload_bytes(case)
        assert len(blob) == n * (hdr + pay)
        payloads = [blob[i * (hdr + pay) + hdr:(i + 1) * (hdr + pay)] for i in range(n)]
        # (handed to the oracle as they are: the header parser only takes square quad detectors)
        fields = dict(image_size=tuple(case['sig']), bits_per_pixel=case['bits'], mib_kind=case['kind'],
                      mib_dtype='u%02d' % case['bits'] if case['kind'] == 'u' else 'r64',
                      num_chips=chips, sensor_layout=(2, 2) if chips == 4 else (1, 1))
        ref = np.stack([omib.decode_frame(p, fields) for p in payloads])
        frames = frames[:n]
        frames.setflags(write=False)
        ref.setflags(write=False)
        assert np.array_equal(ref, frames.astype(np.uint32))          # the reference side itself
        got = _PREPARED[case['name']] = (frames, payloads, ref)
    return got


def decode_guarded(case, n, header, pad, offset, storage):
    """n frames of `case` re-laid at the given geometry -> (decoded (n, H, W) of `storage`, kernel name);
    asserts that no byte outside the output was written"""
    from libertem_amd import hip
    frames, payloads, _ = prepared(case)
    h, w = case['sig']
    chips = 4 if case.get('quad') else 1
    header = 384 * chips if header is None else header
    pay = _payload_bytes(case)
    stride = header + pay + pad
    host = np.full(offset + n * stride, PAD, dtype=np.uint8)
    for i in range(n):
        o = offset + i * stride
        host[o:o + header] = 0x5A
        host[o + header:o + header + pay] = np.frombuffer(payloads[i], dtype=np.uint8)
    src = torch.from_numpy(host).to('cuda:0')
    out_bytes = n * h * w * storage.itemsize
    assert GUARD % storage.itemsize == 0 and GUARD % 16 != 0
    buf = torch.full((GUARD + out_bytes + TAIL,), POISON, dtype=torch.uint8, device='cuda:0')
    hip.mib_decode(0, src.data_ptr() + offset, stride, header, case['kind'], case['bits'],
                   bool(case.get('quad')), n, h, w, buf.data_ptr() + GUARD, storage)
    torch.cuda.synchronize()
    back = buf.cpu().numpy()
    where = (case['name'], n, header, pad, offset, str(storage))
    assert np.all(back[:GUARD] == POISON), ('written before the output', where)
    assert np.all(back[GUARD + out_bytes:] == POISON), ('written behind the output', where)
    got = back[GUARD:GUARD + out_bytes].copy().view(storage).reshape(n, h, w)
    return got, hip.mib_last_kernel()


def check_case(case, wide, storages=None, geometries=GEOMETRIES):
    """every geometry: guards intact, decoded == encoder's frames == oracle, the expected kernel ran"""
    frames, _, ref = prepared(case)
    results = []
    for storage in (storages or [_storage(case)]):
        storage = np.dtype(storage)
        for n, header, pad, offset in geometries:
            n = min(n, len(frames))
            got, kernel = decode_guarded(case, n, header, pad, offset, storage)
            where = (case['name'], n, header, pad, offset, str(storage))
            assert kernel == kernel_name(case, wide, storage), where
            # (24 bit into float32: values below 2**24, exact)
            want = frames[:n].astype(storage)
            assert got.tobytes() == want.tobytes(), where
            assert np.array_equal(got.astype(np.uint32), ref[:n]), where
            results.append(got)
    return results


def _ids(cases):
    return [c['name'] for c in cases]


# ---- A. shapes that take the per-word kernel by default -------------------------------------------
WORD_CASES = [
    _case('u', 8, (5, 7)),              # 4 words + 3 bytes
    _case('u', 8, (3, 8)),              # whole words, 24 bytes
    _case('u', 8, (45, 47)),            # 265 words: two blocks, ragged, partial last word
    _case('u', 16, (5, 7)),             # 8 words + 6 bytes
    _case('u', 16, (3, 4)),             # whole words
    _case('u', 32, (5, 7)),             # 17 words + 4 bytes
    _case('u', 32, (3, 2)),             # whole words
    _case('r', 6, (3, 8)),
    _case('r', 6, (5, 24)),
    _case('r', 6, (33, 72)),            # 297 words: two blocks
    _case('r', 12, (3, 4)),
    _case('r', 12, (5, 12)),
    _case('r', 6, (4, 16), quad=True),  # chip rows of 8 and 24 pixels, not square
    _case('r', 6, (6, 48), quad=True),
    _case('r', 12, (4, 8), quad=True),  # chip rows of 4 and 12 pixels, not square
    _case('r', 12, (6, 24), quad=True),
    _case('r', 12, (90, 24), quad=True),    # 540 words: three blocks
]


@pytest.mark.parametrize('case', WORD_CASES, ids=_ids(WORD_CASES))
def test_per_word_kernel_by_shape(case, monkeypatch):
    monkeypatch.delenv('LTMI_MIB_WORDS', raising=False)
    check_case(case, wide=False)


# ---- B. the per-word kernel forced on shapes that take the wide kernel by default ----------------
def _first_file(case):
    return dict(case, frames=(case['frames'][0],))


# (the recipes' files hold up to 64 frames of 128 x 128: the whole file and its first frame, in the plain
# layout and with an odd header, a padded stride and an odd address)
FILE_GEOMETRIES = [(1 << 20, None, 0, 0), (1, 13, 5, 3), (1 << 20, 13, 5, 0)]
R24_STORAGES = [np.uint32, np.float32]
FORCED_CASES = [(_first_file(c), R24_STORAGES if c['bits'] == 24 else None, FILE_GEOMETRIES)
                for c in recipes.MIB_CASES] + [
    (_case('r', 1, (3, 64)), None, GEOMETRIES),
    (_case('r', 1, (2, 128), quad=True), None, GEOMETRIES),
    (_case('r', 1, (6, 256), quad=True), None, GEOMETRIES),
    (_case('r', 24, (3, 4)), R24_STORAGES, GEOMETRIES),
    (_case('r', 24, (5, 12)), R24_STORAGES, GEOMETRIES),
]


@pytest.mark.parametrize('case,storages,geometries', FORCED_CASES,
                         ids=[c['name'] for c, _, _ in FORCED_CASES])
def test_per_word_kernel_forced_equals_wide_kernel(case, storages, geometries, monkeypatch):
    monkeypatch.setenv('LTMI_MIB_WORDS', '1')
    forced = check_case(case, wide=False, storages=storages, geometries=geometries)
    monkeypatch.delenv('LTMI_MIB_WORDS')
    default = check_case(case, wide=True, storages=storages, geometries=geometries)
    assert len(forced) == len(default) > 0
    for a, b in zip(forced, default):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), case['name']


# ---- C. edges of the wide kernel -------------------------------------------------------------------
WIDE_CASES = [
    (_case('u', 16, (33, 72)), None),               # 297 chunks: two blocks, ragged
    (_case('u', 8, (4, 4)), None),                  # a single chunk
    (_case('r', 1, (3, 64)), None),
    (_case('r', 1, (2, 128), quad=True), None),
    (_case('r', 6, (4, 32), quad=True), None),      # one chunk per chip row, not square
    (_case('r', 12, (4, 16), quad=True), None),
    (_case('r', 24, (3, 4)), R24_STORAGES),
]


@pytest.mark.parametrize('case,storages', WIDE_CASES, ids=[c['name'] for c, _ in WIDE_CASES])
def test_wide_kernel_edges(case, storages, monkeypatch):
    monkeypatch.delenv('LTMI_MIB_WORDS', raising=False)
    check_case(case, wide=True, storages=storages)


# ---- D. argument checks ---------------------------------------------------------------------------
def test_refused_arguments_write_nothing_and_keep_the_kernel_name(monkeypatch):
    from libertem_amd import hip
    monkeypatch.delenv('LTMI_MIB_WORDS', raising=False)
    check_case(_case('u', 8, (4, 4)), wide=True, geometries=GEOMETRIES[:1])
    before = hip.mib_last_kernel()
    assert before == 'k_mib_decode16<u8>'
    raw = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda:0')
    out = torch.full((1 << 16,), POISON, dtype=torch.uint8, device='cuda:0')
    src, dst = raw.data_ptr(), out.data_ptr() + GUARD
    u8, u16, f32 = np.uint8, np.uint16, np.float32
    refused = [
        # stride, header, kind, bits, quad, frames, height, width, dst dtype, src, message
        (8192, 384, 'r', 24, True, 1, 8, 16, f32, src, '24-bit raw data of a quad'),
        (8192, 384, 'r', 24, True, 1, 8, 16, np.uint32, src, '24-bit raw data of a quad'),
        (8192, 384, 'r', 6, True, 1, 5, 16, u8, src, 'whole 64-bit words'),      # odd height
        (8192, 384, 'r', 12, True, 1, 5, 8, u16, src, 'whole 64-bit words'),
        (8192, 384, 'r', 6, True, 1, 4, 24, u8, src, 'chip width 12 is not a multiple of 8'),
        (8192, 384, 'u', 16, False, 1, 5, 7, u8, src, 'decode to uint16'),
        (8192, 384, 'u', 8, False, -1, 5, 7, u8, src, 'bad geometry'),
        (8192, 384, 'u', 8, False, 1, 0, 7, u8, src, 'bad geometry'),
        (8192, 384, 'u', 8, False, 1, 5, 7, u8, 0, 'null pointer'),
    ]
    for stride, header, kind, bits, quad, n, h, w, dt, s, message in refused:
        with pytest.raises(ValueError, match=message):
            hip.mib_decode(0, s, stride, header, kind, bits, quad, n, h, w, dst, dt)
        assert hip.mib_last_kernel() == before, message
    # no frames: fine, nothing launched
    hip.mib_decode(0, src, 8192, 384, 'r', 12, False, 0, 3, 4, dst, u16)
    assert hip.mib_last_kernel() == before
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_last_kernel_belongs_to_the_calling_thread(monkeypatch):
    """'' before a thread's first decode; a decode on another thread does not change this one's"""
    from libertem_amd import hip
    monkeypatch.delenv('LTMI_MIB_WORDS', raising=False)
    check_case(_case('u', 8, (4, 4)), wide=True, geometries=GEOMETRIES[:1])
    seen = []

    def other():
        try:
            seen.append(hip.mib_last_kernel())
            check_case(_case('r', 12, (3, 4)), wide=False, geometries=GEOMETRIES[:1])
            seen.append(hip.mib_last_kernel())
        except BaseException as e:                      # noqa: BLE001  (reported by the assert below)
            seen.append(e)

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == ['', 'k_mib_decode<r12>']
    assert hip.mib_last_kernel() == 'k_mib_decode16<u8>'


# ---- E. MIBDataSet on shapes that take the per-word kernel by default -------------------------------
@pytest.fixture(scope='module')
def ctx():
    from libertem_amd.api import Context
    assert torch.cuda.is_available()
    c = Context.make_with('hip', gpus=0)
    yield c
    c.close()


DATASET_CASES = [
    dict(name='ds_u16_5x7', kind='u', bits=16, sig=(5, 7), frames=(3, 2), nav=(1, 5), seed=7901),
    dict(name='ds_r12_quad_8x8', kind='r', bits=12, sig=(8, 8), frames=(4,), nav=(2, 2), quad=True,
         seed=7902),
    dict(name='ds_r6_quad_16x16', kind='r', bits=6, sig=(16, 16), frames=(2, 2), nav=(2, 2), quad=True,
         seed=7903),
]


def _write(tmp_path, case):
    frames, files, hdr = recipes.make_mib_case(case)
    d = tmp_path / case['name']
    d.mkdir()
    for fn, blob in files.items():
        (d / fn).write_bytes(blob)
    (d / (case['name'] + '.hdr')).write_text(hdr)
    return frames, str(d / (case['name'] + '.hdr'))


@pytest.mark.parametrize('case', DATASET_CASES, ids=_ids(DATASET_CASES))
def test_dataset_on_per_word_shapes(ctx, tmp_path, monkeypatch, case):
    from libertem_amd import hip
    from libertem_amd.io.dataset.mib import MIBDataSet
    from libertem_amd.udf.sumsigudf import SumSigUDF
    monkeypatch.delenv('LTMI_MIB_WORDS', raising=False)
    frames, hdr_path = _write(tmp_path, case)
    n = len(frames)
    want_sum = frames.reshape(n, -1).sum(axis=1).astype(np.float32)
    check_case(_case('u', 8, (4, 4)), wide=True, geometries=GEOMETRIES[:1])    # (another kernel's name)
    ds = ctx.load('mib', path=hdr_path)
    assert hip.mib_last_kernel().startswith('k_mib_decode<')
    assert tuple(ds.shape) == tuple(case['nav']) + tuple(case['sig']) and not ds.is_streamed
    got = ds.data.cpu().reshape(frames.shape)
    assert got.dtype == frames.dtype and np.array_equal(got, frames)
    s = ctx.run_udf(dataset=ds, udf=SumSigUDF())['intensity'].data
    assert np.array_equal(s.reshape(-1), want_sum)
    if case['name'] != 'ds_u16_5x7':
        return
    # the same series streamed: every partition decodes its window when its tiles are asked for
    frame_bytes = int(np.prod(case['sig'])) * frames.dtype.itemsize
    monkeypatch.setattr(MIBDataSet, 'MAX_RESIDENT_BYTES', 2 * frame_bytes)
    streamed = ctx.load('mib', path=hdr_path)
    monkeypatch.setattr(MIBDataSet, 'MAX_RESIDENT_BYTES', None)
    assert streamed.is_streamed and streamed.decode_bytes == 0
    check_case(_case('u', 8, (4, 4)), wide=True, geometries=GEOMETRIES[:1])
    s = ctx.run_udf(dataset=streamed, udf=SumSigUDF())['intensity'].data
    assert np.array_equal(s.reshape(-1), want_sum)
    assert streamed.decode_bytes > 0 and hip.mib_last_kernel() == 'k_mib_decode<u16>'
