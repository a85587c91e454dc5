"""
Which kernel every override of the dispatch selects: the characterization fixture tests/golden/dispatch_names.json.

    python tests/golden/generate_dispatch_names.py OUT.json      # needs a GPU; writes the fixture
    python tests/golden/generate_dispatch_names.py --group N     # (the child of one environment: JSON on stdout)

A case is (stack recipe, tile dtype, frame count, row list, tuning triple, environment) -> the `last_kernel()` string
of the call, or the error of a rejected tuning triple.  Tuning codes are plain numbers here, so the same file runs on a
tree from before `hip.Variant` existed: the committed fixture was recorded on the commit before the tuning record and
the switch table (csrc/ltmi_tuning.h, csrc/ltmi_switches.h) came in, and tests/test_dispatch_names_gpu.py replays it.

The cases of one environment run together in a fresh child process, started with no other LTMI_* variable set (but
LTMI_LIB): the library caches some switches per process.  Codes 31 / 32 and the *_ABLATE switches (garbage results by
design) are not launched.

Sizes: 32 x 32 detector pixels and 64 frames wherever the route is taken at that size.  Where it is not, NOTES below
says why, and the fixture repeats that as the `note` of every such case.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT_S = 240

F32, U16 = 'float32', 'uint16'


def _seed(*what):
    return zlib.crc32(repr(what).encode())


# ---- stack recipes: name -> dict(kind 'dense' | 'csr', masks, result dtype, sig or None) ---------------------------
def _dense(n_masks, n_px=1024, result=F32):
    rng = np.random.default_rng(_seed('dense', n_masks, n_px, result))
    rd = np.dtype(result)
    if rd.kind in 'iu':
        masks = rng.integers(0, 3, (n_masks, n_px)).astype(rd)
    elif rd.kind == 'c':
        masks = (rng.random((n_masks, n_px)) + 1j * rng.random((n_masks, n_px))).astype(rd)
    else:
        masks = (rng.integers(-8, 9, (n_masks, n_px)) / 8.0).astype(rd)      # few-bit weights: float16 images exist
    return dict(kind='dense', masks=masks, result=result, sig=None)


def _radial_dense(sig, n_bins, max_order):
    from libertem_amd import masks as pm
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    h, w = sig
    st = radial_mask_factory(h, w, w / 2, h / 2, 0, pm.bounding_radius(w / 2, h / 2, w, h), n_bins, max_order, False)()
    return dict(kind='dense', masks=np.ascontiguousarray(st.reshape(st.shape[0], -1)), result='complex64', sig=sig)


def _radial_sparse(sig, n_bins, max_order):
    from libertem_amd import masks as pm
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    h, w = sig
    st = radial_mask_factory(h, w, w / 2, h / 2, 0, pm.bounding_radius(w / 2, h / 2, w, h), n_bins, max_order, True)()
    return dict(kind='csr', masks=st.to_px_by_masks(dtype=np.complex64), result='complex64', sig=sig)


def _rings(result=F32):
    import scipy.sparse as sp
    sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]
    from oracle import masks as omasks
    rings = omasks.radial_bins(32, 32, 64, 64, n_bins=64, use_sparse=True, dtype=np.float32)
    m = sp.csr_matrix(rings.T.astype(np.float32))
    if np.dtype(result).kind in 'iu':
        m = sp.csr_matrix((np.ceil(np.abs(m.data) * 3).astype(result), m.indices, m.indptr), shape=m.shape)
    return dict(kind='csr', masks=m, result=result, sig=None)


def _scattered():
    import scipy.sparse as sp
    m = sp.random(4096, 512, density=0.002, format='csr', dtype=np.float32, random_state=np.random.RandomState(3))
    return dict(kind='csr', masks=m, result=F32, sig=None)


def _bins():
    from libertem_amd.masks import bin_masks
    return dict(kind='csr', masks=bin_masks((64, 64), 4).T.tocsr(), result=F32, sig=None)


RECIPES = {
    'dense3': lambda: _dense(3), 'dense16': lambda: _dense(16), 'dense17': lambda: _dense(17),
    'dense24': lambda: _dense(24), 'dense70': lambda: _dense(70), 'dense16_wide': lambda: _dense(16, n_px=4096),
    'dense16_f64': lambda: _dense(16, result='float64'), 'dense6_i32': lambda: _dense(6, result='int32'),
    'dense6_c128': lambda: _dense(6, result='complex128'),
    'fold25': lambda: _radial_dense((64, 128), 1, 24),         # 25 complex masks: 2 even + 2 odd groups
    'fold_even': lambda: _radial_dense((64, 128), 4, 0),       # 4 rings: a single column group, every column even
    'band': lambda: _radial_sparse((64, 128), 2, 7),           # 2 blocks of 8 complex masks
    'rings': _rings, 'rings_i32': lambda: _rings('int32'), 'scattered': _scattered, 'bins': _bins,
}


# why a recipe is larger than 32 x 32 pixels: goes into the fixture with every case of the recipe
NOTES = {
    'dense16_wide': '64 x 64 pixels: 16 mask slots of 256 pixels, so that a split into 8 parts has an order to choose',
    'fold25': '64 x 128 pixels: the smallest shape at which the tests of the row-mirror fold reach k_dense_fold and '
              'k_dense_fold16 (tests/guarded.py FOLD_SIGS)',
    'fold_even': '64 x 128 pixels, like fold25',
    'band': '64 x 128 pixels: the smallest shape at which the tests reach the banded image (tests/guarded.py BAND_SIGS)',
    'rings': '64 x 64 pixels, 64 masks: the scatter image is built for 64 columns and more, the blocked-ELL image by '
             'padding factor (tests/test_kernels_gpu.py test_sparse_dispatch_by_padding_factor)',
    'rings_i32': '64 x 64 pixels, 64 masks, like rings',
    'scattered': '64 x 64 pixels, 512 masks: the stack of test_sparse_dispatch_by_padding_factor that stays on k_sell_apply',
    'bins': '64 x 64 pixels in 4 x 4 bins: 256 masks, several chunks of the label image',
    'cryst': '128 x 128 pixels: the smallest shape of the fused crystallinity kernel',
}


# ---- the cases ------------------------------------------------------------------------------------------------------
def case(id, recipe, tile=F32, frames=64, rows=False, tuning=None, env=None, **extra):
    return dict(id=id, recipe=recipe, tile=tile, frames=frames, rows=rows, tuning=tuning, env=dict(env or {}), **extra)


CASES = [
    # k_dense_lds: float32 instruction, exact float16 products, and what switches the latter off
    case('lds-f32', 'dense16'),
    case('lds-u16-f16', 'dense16', U16),
    case('lds-u8-f16', 'dense16', 'uint8'),
    case('lds-u16-code37', 'dense16', U16, tuning=(0, 37, 0)),
    case('lds-u16-f32instr-env', 'dense16', U16, env={'LTMI_DENSE_F32_INSTR': '1'}),
    case('lds-u16-f16-off-env', 'dense16', U16, env={'LTMI_DENSE_F16': '0'}),
    case('lds-rows', 'dense16', rows=True),
    case('lds-u16-rows', 'dense16', U16, rows=True),
    case('lds-code30-ksplit3', 'dense16', tuning=(0, 30, 3)),
    case('lds-ksplit2', 'dense16', tuning=(0, 0, 2)),
    # (the name does not show the order of the 8 parts over the 16 mask slots, the float32 rounding of the sums does:
    # unset = runs of 4 slots in turn, 0 = a contiguous range each, 1 = single slots in turn -- `bits` records a CRC)
    case('lds-ksplit8-order-default', 'dense16_wide', tuning=(0, 30, 8), bits=True),
    case('lds-ksplit8-contiguous-env', 'dense16_wide', tuning=(0, 30, 8), bits=True, env={'LTMI_KSPLIT_STRIDED': '0'}),
    case('lds-ksplit8-in-turn-env', 'dense16_wide', tuning=(0, 30, 8), bits=True, env={'LTMI_KSPLIT_STRIDED': '1'}),
    case('lds-u16-code34-one-tile', 'dense16', U16, tuning=(0, 34, 0)),
    case('lds-u16-code34-rows', 'dense16', U16, rows=True, tuning=(0, 34, 0)),
    case('lds-f32-code34', 'dense16', tuning=(0, 34, 0)),
    case('lds-u16-code35-two-tiles', 'dense16', U16, tuning=(0, 35, 0)),
    # VALU columns and padded groups
    case('valu-3', 'dense3'),
    case('valu-3-u16', 'dense3', U16),
    case('valu-17', 'dense17'),
    case('valu-17-rows', 'dense17', rows=True),
    case('valu-17-code33-padded', 'dense17', tuning=(0, 33, 0)),
    case('valu-3-code33-padded', 'dense3', tuning=(0, 33, 0)),
    case('valu-17-code33-rows', 'dense17', rows=True, tuning=(0, 33, 0)),
    # the direct-load kernel
    case('mfma-1-4', 'dense16', tuning=(1, 4, 1)),
    case('mfma-2-8-u16', 'dense16', U16, tuning=(2, 8, 2)),
    case('mfma-unaligned-env', 'dense16', unaligned=True, env={'LTMI_ALIGNED_DMA_ONLY': '1'}),
    case('lds-unaligned', 'dense16', unaligned=True),
    # wide stacks
    case('blocks-70', 'dense70'),
    case('blocks-70-u16-rows', 'dense70', U16, rows=True),
    case('blocks-70-code33-one-image', 'dense70', tuning=(0, 33, 0)),
    case('blocks-70-mfma', 'dense70', tuning=(1, 4, 1)),
    # k_dense_split
    case('split-code36', 'dense24', tuning=(0, 36, 0)),
    case('split-env', 'dense24', env={'LTMI_SPLIT': '1'}),
    case('split-env-code30-off', 'dense24', tuning=(0, 30, 0), env={'LTMI_SPLIT': '1'}),
    case('split-env-code35-off', 'dense24', tuning=(0, 35, 0), env={'LTMI_SPLIT': '1'}),
    case('split-code36-rows', 'dense24', rows=True, tuning=(0, 36, 0)),
    case('split-not-default', 'dense24'),
    # row-mirror fold
    case('fold-f32', 'fold25'),
    case('fold-f32-code30-ksplit3', 'fold25', tuning=(0, 30, 3)),
    case('fold-f32-code38-unfolded', 'fold25', tuning=(0, 38, 0)),
    case('fold-u16-code37', 'fold25', U16, tuning=(0, 37, 0)),
    case('fold-u16', 'fold25', U16),
    case('fold-u16-code38', 'fold25', U16, tuning=(0, 38, 0)),
    case('fold-off-env', 'fold25', env={'LTMI_DENSE_FOLD': '0'}),
    case('fold-single-group', 'fold_even'),
    case('fold-single-group-env2', 'fold_even', env={'LTMI_DENSE_FOLD': '2'}),
    # float64 / integer / complex128 results
    case('f64-lds64', 'dense16_f64'),
    case('f64-lds64-rows', 'dense16_f64', rows=True),
    case('f64-mfma-mt1', 'dense16_f64', tuning=(1, 0, 0)),
    case('i32-exact-int', 'dense6_i32', 'int16'),
    case('generic-c128', 'dense6_c128', 'complex128', frames=9),
    # sparse stacks
    case('rings-u16', 'rings', U16, frames=32),
    case('rings-f32', 'rings', frames=32),
    case('rings-u16-code40', 'rings', U16, frames=32, tuning=(0, 40, 0)),
    case('rings-u16-code41-sell', 'rings', U16, frames=32, tuning=(0, 41, 0)),
    case('rings-f32-code41-sell', 'rings', frames=32, tuning=(0, 41, 0)),
    case('rings-f32-code42-no-scatter', 'rings', frames=32, tuning=(0, 42, 0)),
    case('rings-u16-rows', 'rings', U16, frames=32, rows=True),
    case('rings-u16-bell-f16-off-env', 'rings', U16, frames=32, env={'LTMI_BELL_F16': '0'}),
    case('rings-f32-scatter-off-env', 'rings', frames=32, env={'LTMI_SPARSE_SCATTER': '0'}),
    case('rings-u16-scatter-on-env', 'rings', U16, frames=32, env={'LTMI_SPARSE_SCATTER': '1'}),
    case('rings-u16-scatter-on-env-code42', 'rings', U16, frames=32, tuning=(0, 42, 0),
         env={'LTMI_SPARSE_SCATTER': '1'}),
    case('rings-i32-exact-int', 'rings_i32', 'int16', frames=32),
    case('rings-f32-nan', 'rings', frames=32, nan=True),
    case('rings-f32-code41-nan', 'rings', frames=32, tuning=(0, 41, 0), nan=True),
    case('rings-f32-nan-guard-off-env', 'rings', frames=32, nan=True, env={'LTMI_NONFINITE_GUARD': '0'}),
    case('scattered-u16', 'scattered', U16, frames=32),
    case('band-default', 'band', frames=40),
    case('band-on-env', 'band', frames=40, env={'LTMI_SPARSE_BAND': '1'}),
    case('band-on-env-u16', 'band', U16, frames=40, env={'LTMI_SPARSE_BAND': '1'}),
    case('band-on-env-code41', 'band', frames=40, tuning=(0, 41, 0), env={'LTMI_SPARSE_BAND': '1'}),
    case('band-on-env-code42', 'band', frames=40, tuning=(0, 42, 0), env={'LTMI_SPARSE_BAND': '1'}),
    case('band-off-env', 'band', frames=40, env={'LTMI_SPARSE_BAND': '0'}),
    case('bins-default', 'bins', frames=32),
    case('bins-labels-env', 'bins', frames=32, env={'LTMI_SPARSE_LABELS': '1'}),
    case('bins-labels-env-u16', 'bins', U16, frames=32, env={'LTMI_SPARSE_LABELS': '1'}),
    case('bins-labels-env-code41', 'bins', frames=32, tuning=(0, 41, 0), env={'LTMI_SPARSE_LABELS': '1'}),
    case('bins-labels-env-code42', 'bins', frames=32, tuning=(0, 42, 0), env={'LTMI_SPARSE_LABELS': '1'}),
    # tuning triples that are refused
    case('refused-code39', 'dense16', tuning=(0, 39, 0)),
    case('refused-code29', 'dense16', tuning=(0, 29, 0)),
    case('refused-code43', 'rings', U16, frames=32, tuning=(0, 43, 0)),
    case('refused-mt1-code37', 'dense16', tuning=(1, 37, 0)),
    case('refused-mt3', 'dense16', tuning=(3, 4, 0)),
    case('refused-waves2', 'dense16', tuning=(1, 2, 0)),
    case('refused-negative-ksplit', 'dense16', tuning=(1, 4, -1)),
    case('code30-negative-ksplit', 'dense16', tuning=(0, 30, -1)),
    # .mib decode and the crystallinity plan: kernels behind their own *_last_kernel
    case('mib-u16', 'mib', U16, frames=3),
    case('mib-u16-words-env', 'mib', U16, frames=3, env={'LTMI_MIB_WORDS': '1'}),
    case('cryst-fused', 'cryst', U16, frames=4),
    case('cryst-hipfft-env', 'cryst', U16, frames=4, env={'LTMI_FFT_FUSED': '0'}),
]
assert len({c['id'] for c in CASES}) == len(CASES)


def env_groups():
    """the distinct environments, in order of first use -> [(env, [cases])]"""
    groups = []
    for c in CASES:
        for env, members in groups:
            if env == c['env']:
                members.append(c)
                break
        else:
            groups.append((c['env'], [c]))
    return groups


# ---- running a case (in the child) ----------------------------------------------------------------------------------
def _dev(arr, extra_front=0):
    """device copy of a host array behind `extra_front` spare elements -> (tensor that owns it, pointer to the data)"""
    import torch
    flat = np.zeros(arr.size + extra_front, dtype=arr.dtype)
    flat[extra_front:] = arr.reshape(-1)
    t = torch.from_numpy(flat.view(np.uint8)).cuda()
    return t, t.data_ptr() + extra_front * arr.dtype.itemsize


def _frames(c, n_px):
    rng = np.random.default_rng(_seed('frames', c['recipe'], c['tile'], c['frames']))
    dt = np.dtype(c['tile'])
    n = c['frames']
    if dt.kind == 'f':
        x = rng.random((n, n_px)).astype(dt)
    elif dt.kind == 'c':
        x = (rng.random((n, n_px)) + 1j * rng.random((n, n_px))).astype(dt)
    else:
        x = rng.integers(max(np.iinfo(dt).min, -100), min(np.iinfo(dt).max, 4000), (n, n_px), endpoint=True).astype(dt)
    return x


def _worst(res, ref, scale, tol):
    """max of |res - ref| / (tol * scale) over the finite reference entries; the non-finite ones must agree in kind"""
    if np.iscomplexobj(ref):
        return max(_worst(res.real, ref.real, scale, tol), _worst(res.imag, ref.imag, scale, tol))
    fin = np.isfinite(ref)
    if not np.array_equal(np.isnan(res), np.isnan(ref)) or not np.array_equal(np.isinf(res), np.isinf(ref)):
        return float('inf')
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(res[fin].astype(np.float64) - ref[fin]) / (tol * scale[fin] + 1e-30)))


def run_masks(hip, c):
    import torch
    r = RECIPES[c['recipe']]()
    masks, rd = r['masks'], np.dtype(r['result'])
    if r['kind'] == 'dense':
        h = hip.MaskHandle.dense(0, masks, rd)
        dense = np.asarray(masks).T                                           # (n_px, n_masks)
    else:
        h = hip.MaskHandle.csr(0, masks, rd)
        dense = np.asarray(masks.todense())
    try:
        n_px, n_masks = dense.shape
        if r['sig'] is not None:
            h.set_sig_shape(*r['sig'])
        if c['tuning'] is not None:
            try:
                h.set_tuning(*c['tuning'])
            except ValueError as e:
                return dict(error='set_tuning: ' + str(e).rsplit('(code', 1)[1].strip(' )'))
        x = _frames(c, n_px)
        if c.get('nan'):
            stored = np.flatnonzero(np.abs(dense).sum(axis=1) > 0)
            x[1, stored[len(stored) // 2]] = np.nan
        rows = np.arange(c['frames'] - 1, -1, -3, dtype=np.int32) if c['rows'] else None
        n_out = c['frames'] if rows is None else len(rows)
        keep_x, x_ptr = _dev(x, extra_front=1 if c.get('unaligned') else 0)
        keep_o, o_ptr = _dev(np.full((n_out, n_masks), 7, dtype=rd))
        try:
            if rows is None:
                h.apply(x_ptr, x.dtype, c['frames'], n_px, o_ptr, n_masks, False)
            else:
                keep_r, r_ptr = _dev(rows)
                if not h.apply_rows(x_ptr, x.dtype, r_ptr, n_out, n_px, o_ptr, n_masks, False):
                    return dict(kernel='(no row-list kernel)')
        except (ValueError, hip.LtmiError) as e:
            return dict(error='apply: ' + str(e).rsplit('(code', 1)[1].strip(' )'))
        torch.cuda.synchronize()
        res = keep_o.cpu().numpy().view(rd).reshape(n_out, n_masks)
        kernel = h.last_kernel()
    finally:
        h.close()
    xs = x if rows is None else x[rows]
    if rd.kind in 'iu':
        ref = xs.astype(rd) @ dense.astype(rd)
        return dict(kernel=kernel, worst=0.0 if np.array_equal(res, ref) else float('inf'))
    wide = np.complex128 if (rd.kind == 'c' or xs.dtype.kind == 'c') else np.float64
    bad = ~np.isfinite(xs)
    with np.errstate(invalid='ignore'):
        ref = np.where(bad, 0, xs).astype(wide) @ dense.astype(wide)
        scale = np.abs(np.where(bad, 0, xs)).astype(np.float64) @ np.abs(dense).astype(np.float64)
    # a non-finite pixel reaches the masks that store it (sparse stacks multiply stored entries only)
    hit = bad.astype(np.float64) @ (dense != 0).astype(np.float64) > 0
    if c.get('nan') and c['env'].get('LTMI_NONFINITE_GUARD') == '0':
        res, ref, scale = res[~bad.any(axis=1)], ref[~bad.any(axis=1)], scale[~bad.any(axis=1)]    # the fast kernels' own patterns
    else:
        ref = np.where(hit, np.nan, ref)
        if np.iscomplexobj(ref):
            ref = np.where(hit, np.nan + 1j * np.nan, ref)
    # the bound of the route's own kernel tests, in units of sum |a||b|
    if rd.itemsize >= 8 and rd != np.complex64:
        tol = 1e-12
    elif any(part in kernel for part in (',f16', 'k_scatter', 'k_dense_split')):
        tol = 2e-6                              # exact float16 products, float32 FMAs per stored entry, bf16 x 3 pieces
    else:
        tol = 1e-5
    out = dict(kernel=kernel, worst=_worst(res, ref, scale, tol))
    if c.get('bits'):
        out['crc'] = zlib.crc32(np.ascontiguousarray(res).tobytes())
    return out


def run_mib(hip, c):
    """3 frames of 16 x 16 unsigned 16-bit pixels (big-endian payloads behind 384-byte headers)"""
    import torch
    n, h, w, header = c['frames'], 16, 16, 384
    rng = np.random.default_rng(_seed('mib'))
    frames = rng.integers(0, 65535, (n, h, w), endpoint=True).astype(np.uint16)
    stride = header + h * w * 2
    blob = np.full(n * stride, 0x5A, dtype=np.uint8)
    for i in range(n):
        blob[i * stride + header:(i + 1) * stride] = frames[i].astype('>u2').reshape(-1).view(np.uint8)
    src = torch.from_numpy(blob).cuda()
    dst = torch.zeros(n * h * w, dtype=torch.int16, device='cuda')
    hip.mib_decode(0, src.data_ptr(), stride, header, 'u', 16, False, n, h, w, dst.data_ptr(), np.dtype(np.uint16))
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint16).reshape(n, h, w)
    return dict(kernel=hip.mib_last_kernel(), worst=0.0 if np.array_equal(got, frames) else float('inf'))


def run_cryst(hip, c):
    """4 frames of 128 x 128 through ltmi_crystallinity, against the float64 expression of tests/cryst_ref.py"""
    sys.path[:0] = [p for p in (TESTS,) if p not in sys.path]
    from cryst_ref import F32_TOL, _cryst_reference, _cryst_run
    rng = np.random.default_rng(_seed('cryst'))
    frames = rng.integers(0, 4096, size=(c['frames'], 128, 128)).astype(np.uint16)
    ref, real_mask, half = _cryst_reference(frames, 8, 48, ((64, 64), 12))
    out, label = _cryst_run(hip, frames, real_mask, half, batch=4)
    return dict(kernel=label, worst=float(np.max(np.abs(out - ref)) / (F32_TOL * np.abs(ref).max())))


def run_case(hip, c):
    if c['recipe'] == 'mib':
        return run_mib(hip, c)
    if c['recipe'] == 'cryst':
        return run_cryst(hip, c)
    return run_masks(hip, c)


def run_group_here(index):
    """(the child) every case of environment `index` -> {id: result}"""
    sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]
    import torch                                                              # noqa: F401 (before the library)
    from libertem_amd import hip
    hip.lib()
    env, members = env_groups()[index]
    for k, v in env.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k))
    return {c['id']: run_case(hip, c) for c in members}


def run_group(index):
    """environment `index` in a fresh child process -> ({id: result} or None, the child's return code, its output)"""
    env, _ = env_groups()[index]
    clean = {k: v for k, v in os.environ.items() if not k.startswith('LTMI_') or k == 'LTMI_LIB'}
    clean.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--group', str(index)], env=clean, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        return None, 124, str(e.stdout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    if r.returncode != 0 or len(lines) != 1:
        return None, r.returncode, r.stdout
    return json.loads(lines[0][len('RESULT '):]), 0, r.stdout


def fixture_entry(c, result):
    e = {k: c[k] for k in ('id', 'recipe', 'tile', 'frames', 'rows', 'tuning', 'env')}
    for k in ('unaligned', 'nan', 'bits'):
        if c.get(k):
            e[k] = True
    if c['recipe'] in NOTES:
        e['note'] = NOTES[c['recipe']]
    if c.get('bits'):
        e['crc'] = result['crc']
    if 'error' in result:
        e['error'] = result['error']
    else:
        e['kernel'] = result['kernel']
    return e


def main(argv):
    if argv[:1] == ['--group']:
        print('RESULT ' + json.dumps(run_group_here(int(argv[1]))), flush=True)
        return 0
    out_path = argv[0]
    entries = []
    for i, (env, members) in enumerate(env_groups()):
        results, rc, output = run_group(i)
        if results is None:
            print(f"environment {env}: the child ended with {rc}\n{output}", file=sys.stderr)
            return 1                                                          # (nothing more is started on the GPU)
        for c in members:
            res = results[c['id']]
            print(f"{c['id']:42s} {res.get('kernel') or res.get('error')}  worst={res.get('worst')}", flush=True)
            if 'kernel' in res and 'worst' in res and not res['worst'] <= 1.0:
                print(f"{c['id']}: off the float64 product by {res['worst']} of the bound", file=sys.stderr)
                return 1
            entries.append(fixture_entry(c, res))
    with open(out_path, 'w') as f:
        json.dump({'cases': entries}, f, indent=1)
        f.write('\n')
    print(f"{len(entries)} cases -> {out_path}")
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
