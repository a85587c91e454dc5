"""
Guarded device buffers and the route table of tests/test_apply_bounds_gpu.py.

`Region` places an owned (rows, cols) rectangle at a leading dimension inside a larger device buffer whose every other
element holds a chosen fill: a byte poison around results (a stray store changes a byte that is compared afterwards),
quiet NaN / +Inf / 0 / the dtype's maximum around inputs (a stray load that meets a zero weight shows as 0 * NaN).  The
guard band of an input is 4 KiB on each side -- more than one 256-pixel float64 mask slot --, so a kernel that forgets
a bound reads the fill and not a foreign allocation.

`CASES` is the table of kernel routes behind `ltmi_apply_masks` / `ltmi_apply_masks_rows`, `FRAME_CSR_CASES` that of
`ltmi_apply_masks_csr`.  Everything here but `Region.upload` works without torch (tests/test_apply_bounds_cpu.py).
"""
import re
import zlib

import numpy as np

from libertem_amd.hip import Variant as V

OUT_GUARD = 256           # poison bytes in front of and behind a result; keeps the region's base 256-byte aligned
IN_GUARD = 4096           # fill bytes in front of and behind an input: one 256-pixel float64 mask slot is 2 KiB


def seed(*what):
    """a seed that is the same in every process (str hashes are salted per process)"""
    return zlib.crc32(repr(what).encode())


def poison(n):
    """n bytes, none of them zero, with a period (251) that no row length here shares"""
    return np.resize(((np.arange(251) * 151 + 7) % 251 + 1).astype(np.uint8), n)


def fill_value(dtype, fill):
    """what a non-owned element of an input holds"""
    dt = np.dtype(dtype)
    if fill == 'zero':
        return dt.type(0)
    if fill == 'max':
        assert dt.kind in 'iub', (dt, fill)
        return dt.type(True) if dt.kind == 'b' else dt.type(np.iinfo(dt).max)
    assert dt.kind in 'fc', (dt, fill)
    v = {'nan': np.nan, 'inf': np.inf}[fill]
    return dt.type(complex(v, v)) if dt.kind == 'c' else dt.type(v)        # (complex: both halves)


class Region:
    """(rows, cols) of `dtype` at leading dimension `ld` (elements) inside a larger device buffer; the region starts
    `shift` elements behind a 256-byte boundary, with a guard band in front and behind.  `init` fills the owned
    elements; `fill` says what every other element holds: 'poison' (bytes, for results), 'nan' / 'inf' / 'zero'
    (float inputs), 'max' / 'zero' (integer inputs)."""

    def __init__(self, rows, cols, ld, dtype, shift=0, init=None, fill='poison', upload=True):
        self.dt = np.dtype(dtype)
        self.rows, self.cols, self.ld, self.shift = int(rows), int(cols), int(ld), int(shift)
        assert self.ld >= self.cols and self.rows >= 0
        self.guard = OUT_GUARD if fill == 'poison' else IN_GUARD
        self.start = self.guard + self.shift * self.dt.itemsize
        self.nbytes = self.rows * self.ld * self.dt.itemsize
        self.total = self.start + self.nbytes + self.guard
        self.dev = None
        self.load(init, fill, upload=upload)

    def load(self, init=None, fill=None, upload=True):
        """a new image -- owned elements `init` (default: what they were), every other element `fill` -- in the SAME
        device buffer: the addresses of a second run are those of the first"""
        if fill is None:
            fill = self.fill
        if init is None and hasattr(self, 'host'):
            init = self.view(self.host).copy()
        self.fill = fill
        if fill == 'poison':
            host = poison(self.total)
        else:
            host = np.empty(self.total // self.dt.itemsize, dtype=self.dt)
            host[...] = fill_value(self.dt, fill)
            host = host.view(np.uint8)
        self.host = host
        if init is not None:
            self.view(host)[...] = init
        if upload:
            self.upload()

    def upload(self):
        import torch
        if self.dev is None:
            self.dev = torch.from_numpy(self.host).cuda()
            assert self.dev.data_ptr() % 256 == 0
        else:
            self.dev.copy_(torch.from_numpy(self.host))

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.start

    def view(self, image):
        """the owned elements inside a host image of the whole buffer"""
        flat = image[self.start:self.start + self.nbytes].view(self.dt)
        return flat.reshape(self.rows, self.ld)[:, :self.cols]

    def owned_mask(self):
        """bytes of the buffer that belong to the owned rectangle"""
        m = np.zeros(self.total, dtype=bool)
        rows = m[self.start:self.start + self.nbytes].reshape(self.rows, self.ld * self.dt.itemsize)
        rows[:, :self.cols * self.dt.itemsize] = True
        return m

    def download(self):
        import torch
        torch.cuda.synchronize()
        return self.dev.cpu().numpy()

    def result(self):
        """the owned elements as the device holds them now"""
        return self.view(self.download()).copy()


def where_is(region, byte):
    if byte < region.start:
        return 'front guard'
    if byte >= region.start + region.nbytes:
        return 'rear guard'
    r, c = divmod((byte - region.start) // region.dt.itemsize, region.ld)
    return f"row {r} column {c}" + (' (row padding)' if c >= region.cols else '')


def unchanged_outside(region, what=''):
    """every byte outside the owned rectangle is what the host image holds"""
    got = region.download()
    outside = ~region.owned_mask()
    bad = np.flatnonzero((got != region.host) & outside)
    assert bad.size == 0, f"{what}: {bad.size} bytes outside the owned rectangle changed, first at byte " \
                          f"{int(bad[0])}: {where_is(region, int(bad[0]))}"


def unchanged(region, what=''):
    """the whole buffer is what the host image holds (inputs)"""
    got = region.download()
    bad = np.flatnonzero(got != region.host)
    assert bad.size == 0, f"{what}: input buffer was written, first at byte {int(bad[0])}: " \
                          f"{where_is(region, int(bad[0]))}"


# ---- the route table ------------------------------------------------------------------------------------------------
FRAMES = (1, 17, 129)         # one frame, one more than a 16-frame tile, one more than a workgroup's 128 rows
                              # (LdsCfg::WG_ROWS, Lds64Cfg::WG_ROWS, FD_WG_ROWS, the split kernel's: all 128)
FRAMES_SMALL = (1, 17, 33, 65, 129)     # ... and of 32 and 64: k_bell_* (16 per frame tile, 1 or 2 tiles), k_scatter
                                        # (SC_FB = 64), k_dense_mfma / k_dense_mfma_f64 (16 MT per wave: 64, 128);
                                        # k_sell_apply has SP_F = 16


def px(slot, below=False, two=False):
    """one or two full mask slots plus a tail of 0, 1, 9, 33 pixels; 391 = 17 x 23 (odd rows); one count below a slot.
    two: the route takes rows of 256 pixels or more (lds_kernel_applies: a single column group, also the last column
    block), so the tails of 0 and 1 follow two slots of 128 as well"""
    first = 2 * slot if two else slot
    n = [first, first + 1, 2 * slot + 9, 2 * slot + 33, 391]
    if below:
        n.append(100)
    return tuple(sorted(set(n)))


def px_split(slot):
    """K splits: 3 full slots, 5 slots + 1 pixel, and 7 slots + a ragged one: 8 slots take a split into 8 parts whole
    (the parts of a launch are ceil(slots / ceil(slots / ksplit))), which are served in turn, in runs of 4 slots"""
    return (3 * slot, 5 * slot + 1, 7 * slot + 9)


class Case:
    """One kernel route.
    handle:  'dense' | 'fold' (dense + set_sig_shape, radial-Fourier stack) | 'csr' | 'band' (csr + set_sig_shape)
    result:  result dtype of the handle;  tuning: (mt, waves, ksplit) for set_tuning or None;  env: switches read when
             the handle is made;  expect: substrings `last_kernel()` must contain ('!x': must not contain x)
    tiles:   tile dtypes;  n_masks;  n_px: pixel counts, or sigs: ((h, w, (cy, cx) | None), ...) for 'fold' / 'band'
    rows:    ltmi_apply_masks_rows reports `handled` on this route
    aligned: the route only takes 16-byte aligned rows (the padded placement keeps rows and base 16-byte aligned)
    parts:   grid.y of the launch at the largest pixel count (K splits: the parts the pixel axis is cut into)
    whole_slots: the route only takes pixel counts that are a multiple of 128 (split_wanted in ltmi_split.hip)"""

    def __init__(self, id, handle, result, tuning, expect, tiles, n_masks, n_px=(), sigs=(), env=None, rows=True,
                 aligned=False, frames=FRAMES, radial=(1, 24), parts=None, whole_slots=False):
        self.id, self.handle, self.result, self.tuning, self.expect = id, handle, result, tuning, tuple(expect)
        self.tiles, self.n_masks, self.n_px, self.sigs = tuple(tiles), n_masks, tuple(n_px), tuple(sigs)
        self.env, self.rows, self.aligned, self.frames, self.radial = dict(env or {}), rows, aligned, frames, radial
        self.parts, self.whole_slots = parts, whole_slots

    def pixel_shapes(self):
        """[(n_px, sig | None, centre | None)]"""
        if self.sigs:
            return [(h * w, (h, w), c) for h, w, c in self.sigs]
        return [(n, None, None) for n in self.n_px]

    def sparse(self):
        return self.handle in ('csr', 'band')


F32, U16, U8, I16 = 'float32', 'uint16', 'uint8', 'int16'
NARROW = (U8, U16, I16)
FOLD_SIGS = ((64, 128, (32.5, 70.0)),      # rows y and 65 - y: rows 0 and 1 have their partner beyond the frame
             (96, 64, None))               # centre row 48: row 0 unpaired
BAND_SIGS = ((64, 128, None), (65, 64, None))     # (an odd number of rows: an unpaired row)

CASES = [
    # -- dense, float32 / complex64 results: direct loads
    Case('mfma-mt1', 'dense', F32, (1, 4, 1), ('k_dense_mfma<', 'MT=1', 'WAVES=4'), (F32, U16, U8, I16), 16,
         px(256, below=True), rows=False, frames=FRAMES_SMALL),
    Case('mfma-mt2', 'dense', F32, (2, 4, 1), ('k_dense_mfma<', 'MT=2', 'WAVES=4'), (F32, U16), 20,
         px(256, below=True), rows=False, frames=FRAMES_SMALL),
    Case('mfma-waves8', 'dense', F32, (1, 8, 1), ('k_dense_mfma<', 'WAVES=8'), (U16,), 16, px(256, below=True),
         rows=False, frames=FRAMES_SMALL),
    # -- k_dense_lds, float32 matrix instruction (integer frames: tuning 37)
    Case('lds-ng1', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=1,', '!,f16'), (F32,), 16, px(256)),
    Case('lds-ng2', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=2,', '!,f16'), (F32,), 24, px(128)),
    Case('lds-ng3', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=3,', '!,f16'), (F32,), 40, px(128)),
    Case('lds-ng4', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=4,', '!,f16'), (F32,), 64, px(128)),
    Case('lds-ng1+2valu', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=1+2 VALU'), (F32,), 17, px(128)),
    Case('lds-ng2+4valu', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=2+4 VALU'), (F32,), 35, px(128)),
    Case('lds-ng3+2valu', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=3+2 VALU'), (F32,), 50, px(128)),
    Case('lds-ng0+valu', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=0+'), (F32,), 3, px(128, two=True)),
    Case('lds-column-blocks', 'dense', F32, (0, V.DENSE_DEFAULT, 1), ('column blocks', 'k_dense_lds<'), (F32, U16), 70,
         px(128, two=True)),
    # -- exact float16 products (default dispatch) and the float32 instruction on the same frames
    Case('f16-ng1', 'dense', F32, None, ('k_dense_lds<', 'NG=1,', ',f16'), NARROW, 16, px(256)),
    Case('f16-ng2', 'dense', F32, None, ('k_dense_lds<', 'NG=2,', ',f16'), NARROW, 24, px(128)),
    Case('f16-ng3', 'dense', F32, None, ('k_dense_lds<', 'NG=3,', ',f16'), NARROW, 40, px(128)),
    Case('f16-ng4', 'dense', F32, None, ('k_dense_lds<', 'NG=4,', ',f16'), NARROW, 64, px(128)),
    Case('f32instr-ng1', 'dense', F32, (0, V.DENSE_F32_INSTR, 1), ('k_dense_lds<', 'NG=1,', '!,f16'), NARROW, 16, px(256)),
    Case('f32instr-ng3', 'dense', F32, (0, V.DENSE_F32_INSTR, 1), ('k_dense_lds<', 'NG=3,', '!,f16'), NARROW, 40, px(128)),
    Case('f32instr-ng4', 'dense', F32, (0, V.DENSE_F32_INSTR, 1), ('k_dense_lds<', 'NG=4,', '!,f16'), NARROW, 64, px(128)),
    # -- bf16 split (whole mask slots only: no ragged pixel counts on this route)
    Case('split-ng2', 'dense', F32, (0, V.DENSE_SPLIT_BF16, 1), ('k_dense_split',), (F32,), 24, (1024, 1152, 2048), rows=False,
         whole_slots=True),
    Case('split-ng4', 'dense', F32, (0, V.DENSE_SPLIT_BF16, 1), ('k_dense_split',), (F32,), 50, (1024, 1152, 2048), rows=False,
         whole_slots=True),
    # -- row-mirror fold
    Case('fold-f32', 'fold', 'complex64', (0, V.DENSE_DEFAULT, 1), ('k_dense_fold<f',), (F32,), 25, sigs=FOLD_SIGS, aligned=True),
    Case('fold-u16', 'fold', 'complex64', (0, V.DENSE_F32_INSTR, 1), ('k_dense_fold16<',), (U16,), 25, sigs=FOLD_SIGS[:1],
         aligned=True),
    # -- complex64 stacks
    Case('c64-8', 'dense', 'complex64', (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<', 'NG=1,'), (F32, U16), 8, px(256)),
    Case('c64-25', 'dense', 'complex64', (0, V.DENSE_DEFAULT, 1), ('k_dense_lds<',), (F32, U16), 25, px(128)),
    # -- K splits
    Case('lds-ng1-ksplit0', 'dense', F32, (0, V.DENSE_DEFAULT, 0), ('k_dense_lds<', 'NG=1,'), (F32, U16), 16, px_split(256)),
    Case('lds-ng1-ksplit3', 'dense', F32, (0, V.DENSE_DEFAULT, 3), ('k_dense_lds<', 'NG=1,'), (F32, U16), 16, px_split(256),
         parts=3),
    Case('lds-ng1-ksplit8', 'dense', F32, (0, V.DENSE_DEFAULT, 8), ('k_dense_lds<', 'NG=1,'), (F32, U16), 16, px_split(256),
         parts=8),
    Case('lds-ng4-ksplit0', 'dense', F32, (0, V.DENSE_DEFAULT, 0), ('k_dense_lds<', 'NG=4,'), (F32, U16), 64, px_split(128)),
    Case('lds-ng4-ksplit3', 'dense', F32, (0, V.DENSE_DEFAULT, 3), ('k_dense_lds<', 'NG=4,'), (F32, U16), 64, px_split(128),
         parts=3),
    Case('lds-ng4-ksplit8', 'dense', F32, (0, V.DENSE_DEFAULT, 8), ('k_dense_lds<', 'NG=4,'), (F32, U16), 64, px_split(128),
         parts=8),
    Case('fold-ksplit0', 'fold', 'complex64', (0, V.DENSE_DEFAULT, 0), ('k_dense_fold<f',), (F32,), 25, sigs=FOLD_SIGS[:1],
         aligned=True),
    Case('fold-ksplit3', 'fold', 'complex64', (0, V.DENSE_DEFAULT, 3), ('k_dense_fold<f',), (F32,), 25, sigs=FOLD_SIGS[:1],
         aligned=True),
    Case('fold-ksplit8', 'fold', 'complex64', (0, V.DENSE_DEFAULT, 8), ('k_dense_fold<f',), (F32,), 25, sigs=FOLD_SIGS[:1],
         aligned=True),
    # -- dense, float64 / complex128 / integer results
    Case('lds64', 'dense', 'float64', (0, 0, 1), ('k_dense_lds64',), ('float64', F32, 'int32', U16), 16, px(256)),
    Case('lds64-3groups', 'dense', 'float64', (0, 0, 1), ('k_dense_lds64',), ('float64', 'int64'), 37, px(256)),
    Case('lds64-ksplit0', 'dense', 'float64', (0, 0, 0), ('k_dense_lds64',), ('float64', 'int32'), 16,
         px_split(256)),
    Case('lds64-ksplit3', 'dense', 'float64', (0, 0, 3), ('k_dense_lds64',), ('float64', 'int32'), 16,
         px_split(256), parts=3),
    Case('mfma-f64-mt1', 'dense', 'float64', (1, 0, 1), ('k_dense_mfma_f64',), ('float64', F32, 'int32', U16), 16,
         px(256, below=True), rows=False, frames=FRAMES_SMALL),
    Case('mfma-f64-short-rows', 'dense', 'float64', (0, 0, 1), ('k_dense_mfma_f64',), ('float64', U16), 5,
         (100, 195, 255), rows=False, frames=FRAMES_SMALL),
    Case('mfma-f64-ksplit3', 'dense', 'float64', (1, 0, 3), ('k_dense_mfma_f64',), ('float64',), 16, px_split(256),
         rows=False, frames=FRAMES_SMALL),
    Case('c128', 'dense', 'complex128', (0, 0, 1), ('k_dense_lds64',), ('float64', 'int32'), 5, px(256)),
    Case('exact-int', 'dense', 'int32', (0, 0, 1), ('exact-int',), (I16, U16, 'int32'), 7, px(256)),
    Case('exact-int-short-rows', 'dense', 'int64', (0, 0, 1), ('exact-int',), ('int32', U8), 7, (100, 195),
         rows=False, frames=FRAMES_SMALL),
    Case('generic-c64', 'dense', 'complex64', None, ('k_dense_generic',), ('complex64',), 6, px(256, below=True),
         rows=False),
    Case('generic-i64', 'dense', 'int64', None, ('k_dense_generic',), ('int64',), 6, px(256, below=True),
         rows=False),
    # -- CSR handles
    Case('sell-f32', 'csr', F32, (0, V.SPARSE_SELL, 0), ('k_sell_apply<', '!f64'), (F32, U16, U8), 20, px(256, below=True),
         frames=FRAMES_SMALL),
    Case('sell-f64', 'csr', 'float64', (0, V.SPARSE_SELL, 0), ('k_sell_apply<', 'f64'), ('float64', F32, 'int32'), 20,
         px(256, below=True), frames=FRAMES_SMALL),
    Case('bell-apply', 'csr', F32, None, ('k_bell_apply',), (F32, U16, U8), 20, px(256, below=True),
         env={'LTMI_SPARSE_BELL': '1', 'LTMI_SPARSE_SCATTER': '0', 'LTMI_BELL_F16': '0'}, frames=FRAMES_SMALL),
    Case('bell-flat', 'csr', F32, None, ('k_bell_flat',), (U16, U8), 20, px(256, below=True),
         env={'LTMI_SPARSE_BELL': '1', 'LTMI_SPARSE_SCATTER': '0'}, frames=FRAMES_SMALL),
    Case('scatter', 'csr', F32, None, ('k_scatter',), (F32, U16), 20, px(256, below=True),
         env={'LTMI_SPARSE_BELL': '0', 'LTMI_SPARSE_SCATTER': '1'}, frames=FRAMES_SMALL),
    Case('band-f32', 'band', 'complex64', None, ('k_dense_fold<f', 'banded'), (F32,), 24, sigs=BAND_SIGS,
         env={'LTMI_SPARSE_BAND': '1'}, aligned=True, radial=(3, 7)),
    Case('band-u16', 'band', 'complex64', None, ('k_dense_fold16<', 'banded'), (U16,), 24, sigs=BAND_SIGS[:1],
         env={'LTMI_SPARSE_BAND': '1'}, aligned=True, radial=(3, 7)),
]

# ltmi_apply_masks_csr (k_apply_csr): (result dtype, n_masks)
FRAME_CSR_CASES = [(F32, 1), (F32, 3), (F32, 17), (F32, 64), ('float64', 1), ('float64', 3), ('float64', 64)]
FRAME_CSR_SHAPES = ((1, 300), (17, 391), (129, 257))          # (n_frames, n_px)


def case_params():
    """(case, tile dtype) pairs"""
    return [(c, t) for c in CASES for t in c.tiles]


def param_id(p):
    return f"{p[0].id}-{p[1]}"


# ---- inputs ---------------------------------------------------------------------------------------------------------
def radial_stack(sig, n_bins, max_order, centre=None):
    """the radial-Fourier stack (analysis/radialfourier.py), flattened: (n_bins (max_order + 1), h w) complex64"""
    from libertem_amd import masks as pm
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    h, w = sig
    cy, cx = (h / 2, w / 2) if centre is None else centre
    ro = pm.bounding_radius(cx, cy, w, h)
    st = radial_mask_factory(h, w, cx, cy, 0, ro, n_bins, max_order, False)()
    return np.ascontiguousarray(st.reshape(st.shape[0], -1))


def radial_sparse(sig, n_bins, max_order):
    """the same stack with several bins as CSR (n_px, n_masks) complex64: the masks of a bin share a support"""
    from libertem_amd import masks as pm
    from libertem_amd.analysis.radialfourier import radial_mask_factory
    h, w = sig
    cy, cx = h / 2, w / 2
    st = radial_mask_factory(h, w, cx, cy, 0, pm.bounding_radius(cx, cy, w, h), n_bins, max_order, True)()
    return st.to_px_by_masks(dtype=np.complex64)


def _round3(a):
    """integer weights in [-3, 3] from weights in [-1, 1]; rint is odd, so a mirror symmetry survives bit for bit"""
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        return (np.rint(3 * a.real) + 1j * np.rint(3 * a.imag)).astype(a.dtype)
    return np.rint(3 * a).astype(a.dtype)


def sparse_support(n_px, n_masks):
    """localised stack: mask k stores the pixels within `width` of its centre; the centres cover the whole frame but
    for pixels [44, 60), which no mask stores.  -> bool (n_px, n_masks)"""
    centre = (np.arange(n_masks) + 0.5) * n_px / n_masks
    width = 1.5 * n_px / n_masks
    sup = np.abs(np.arange(n_px)[:, None] - centre[None, :]) < width
    sup[44:60] = False
    return sup


def make_stack(case, n_px, sig=None, centre=None, integer=False):
    """the mask stack of a case: dense (n_masks, n_px) array, or scipy CSR (n_px, n_masks) for CSR handles.
    integer: weights in [-3, 3] (real and imaginary parts independently); otherwise fractional weights, about one
    in eight of them zero (a zero weight is where 0 * Inf shows)."""
    rd = np.dtype(case.result)
    rng = np.random.default_rng(seed('stack', case.id, n_px, integer))
    if case.handle == 'fold':
        st = radial_stack(sig, case.radial[0], case.radial[1], centre)
        return _round3(st) if integer else st
    if case.handle == 'band':
        csr = radial_sparse(sig, case.radial[0], case.radial[1])
        if integer:
            csr = csr.copy()
            csr.data = _round3(csr.data)              # (zeros stay stored: the supports are what they were)
        return csr
    n_masks = case.n_masks

    def weights(shape):
        if integer:
            return rng.integers(-3, 3, shape, endpoint=True).astype(np.float64)
        w = rng.random(shape) - 0.25
        w[rng.random(shape) < 0.125] = 0
        return w

    if case.handle == 'csr':
        import scipy.sparse as sps
        sup = sparse_support(n_px, n_masks)
        w = weights((n_px, n_masks))
        w[w == 0] = 1                                  # (every entry of the support is stored)
        return sps.csr_matrix((w * sup).astype(rd))
    w = weights((n_masks, n_px))
    if rd.kind == 'c':
        w = w + 1j * weights((n_masks, n_px))
    if rd.kind in 'iu':
        w = rng.integers(-3, 3, (n_masks, n_px), endpoint=True)
    return w.astype(rd)


def dense_of(stack):
    """(n_masks, n_px) array of a stack"""
    if hasattr(stack, 'toarray'):
        return np.ascontiguousarray(stack.toarray().T)
    return stack


def signed_pixels(tile_dtype):
    return np.dtype(tile_dtype).kind in 'ifc'


def int_frames(rng, tile_dtype, shape):
    """property E: integers in [0, 63], on the routes that take signed pixels in [-31, 31], stored in the tile dtype"""
    dt = np.dtype(tile_dtype)
    lo, hi = (-31, 31) if signed_pixels(dt) else (0, 63)
    a = rng.integers(lo, hi, shape, endpoint=True)
    if dt.kind == 'c':
        return (a + 1j * rng.integers(lo, hi, shape, endpoint=True)).astype(dt)
    return a.astype(dt)


def real_frames(rng, tile_dtype, shape):
    """finite frames with fractional values (floats) / a few thousand counts (integers)"""
    dt = np.dtype(tile_dtype)
    if dt.kind == 'b':
        return rng.integers(0, 2, shape).astype(dt)
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        return rng.integers(max(info.min, -2000), min(info.max, 4000), shape, endpoint=True).astype(dt)
    a = (rng.random(shape) - 0.3) * 50
    if dt.kind == 'c':
        a = a + 1j * (rng.random(shape) - 0.3) * 50
    return a.astype(dt)


def _parts(a):
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        return np.rint(a.real).astype(np.int64), np.rint(a.imag).astype(np.int64)
    return a.astype(np.int64), None


def int_product(x, w):
    """(x @ w.T in int64, real and imaginary parts; max of |x| @ |w|.T) for integer-valued x (n, n_px), w (k, n_px)"""
    xr, xi = _parts(x)
    wr, wi = _parts(w)
    re = xr @ wr.T
    im = None
    if xi is not None and wi is not None:
        re = re - xi @ wi.T
        im = xr @ wi.T + xi @ wr.T
    elif wi is not None:
        im = xr @ wi.T
    elif xi is not None:
        im = xi @ wr.T
    ax = np.abs(xr) + (0 if xi is None else np.abs(xi))
    aw = np.abs(wr) + (0 if wi is None else np.abs(wi))
    bound = int((ax @ aw.T).max()) if x.shape[0] else 0
    return re, im, bound


def exact_limit(result_dtype):
    """below this every partial sum of integers is exact, whatever the order"""
    rd = np.dtype(result_dtype)
    return 2 ** 24 if rd in (np.dtype('float32'), np.dtype('complex64')) else 2 ** 53


def as_result(re, im, result_dtype):
    rd = np.dtype(result_dtype)
    if rd.kind == 'c':
        return (re + 1j * (0 if im is None else im)).astype(rd)
    return re.astype(rd)                               # (integers wrap)


# ---- what properties B, C and D put where ---------------------------------------------------------------------------
def placements(case, n_px, itemsize):
    """(ld_tile, shift) of the tile: rows padded by 5 elements behind a base that is only element-aligned, and
    contiguous rows on a 256-byte boundary.  Routes that only take 16-byte aligned rows get 16 bytes of each."""
    if case.aligned:
        e = 16 // itemsize
        return [(n_px + e, e), (n_px, 0)]
    return [(n_px + 5, 1), (n_px, 0)]


def input_fills(tile_dtype):
    """property B: the surroundings of the tile, first the one the others are compared with"""
    return ('zero', 'nan', 'inf') if np.dtype(tile_dtype).kind in 'fc' else ('zero', 'max')


def bad_frames(n_frames):
    """property C: every third frame, the second of each three"""
    return np.arange(n_frames) % 3 == 1


def bad_pixels(n_px, whole):
    """property C: the first 40 and the last 40 pixels of a bad frame, or all of it"""
    m = np.zeros(n_px, dtype=bool)
    if whole:
        m[:] = True
    else:
        m[:40] = True
        m[-40:] = True
    return m


def c_shapes(case, slot=128):
    """property C: contiguous rows whose length is no multiple of a mask slot (nor of the 16-pixel blocks), two clean
    frames or more.  A route that takes whole slots only (k_dense_split) runs at its own pixel counts: frames can
    still reach each other through the 16-frame tiles and the frame-after-frame layout."""
    ragged = [(n, s, c) for n, s, c in case.pixel_shapes() if n % slot != 0 or case.sigs]
    return ragged if not case.whole_slots else case.pixel_shapes(), \
           [f for f in case.frames if int((~bad_frames(f)).sum()) >= 2]


def row_list(rng, n_named):
    """property D: `n_named` frames of a tile of 3 n_named, unsorted, one of them twice"""
    n_tile = 3 * n_named
    rows = rng.permutation(n_tile)[:n_named].astype(np.int32)
    if n_named >= 2:
        rows[n_named // 2] = rows[0]
    return n_tile, rows


def parts_in_turn(kern):
    """property D: does this launch of the frame-range kernel sum in another order than the row-list kernel?
    k_dense_lds cuts the pixel axis into grid.y parts.  With 8, 16, 32 or 64 parts (a power of two from 8 on:
    `ksplit_order` in ltmi_dense.hip) the parts of the frame-range kernel take the mask slots in turn, in runs of 4;
    the row-list kernel (`kstr` needs IND == 0 there) always gives each part a contiguous range.  The partial sums
    then hold other pixels, and the float32 results of the two kernels differ in their last bits by design."""
    grid = re.search(r'grid=\((\d+),(\d+)', kern)
    parts = int(grid.group(2)) if grid else 1
    return 'k_dense_lds<' in kern and ',rows' not in kern and parts >= 8 and parts & (parts - 1) == 0


def float64_product(data2d, masks2d):
    """(x @ w.T, |x| @ |w|.T) in float64 / complex128 for finite frames; the second is the scale of a tolerance"""
    x = np.asarray(data2d, dtype=np.float64)
    w = np.asarray(masks2d)
    w = w.astype(np.complex128 if w.dtype.kind == 'c' else np.float64)
    return x @ w.T, np.abs(x) @ np.abs(w).T


def stored_entries_ref(data2d, csr_px_by_masks):
    """the reference's sparse arithmetic in float64 / complex128: per mask, the stored entries only -- a non-finite
    pixel reaches exactly the masks that store it (copy of tests/test_kernels_gpu.py)"""
    csc = csr_px_by_masks.tocsc()
    csc.sort_indices()
    wide = np.complex128 if np.iscomplexobj(csc.data) else np.float64
    ref = np.zeros((data2d.shape[0], csc.shape[1]), dtype=wide)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(csc.shape[1]):
            idx = csc.indices[csc.indptr[k]:csc.indptr[k + 1]]
            val = csc.data[csc.indptr[k]:csc.indptr[k + 1]].astype(wide)
            if len(idx):
                ref[:, k] = (data2d[:, idx].astype(np.float64) * val[None, :]).sum(axis=1)
    return ref


def elementwise_ref(data2d, masks2d):
    """the dense product as an element-by-element float64 sum (no BLAS: its NaN handling is its own); real frames
    against complex masks are two real products.  0 * Inf = NaN, Inf - Inf = NaN, the infinity otherwise."""
    x = np.asarray(data2d, dtype=np.float64)
    w = np.asarray(masks2d)
    with np.errstate(invalid='ignore', over='ignore'):
        def one(wp):
            out = np.empty((x.shape[0], wp.shape[0]))
            for f in range(x.shape[0]):
                out[f] = (wp.astype(np.float64) * x[f][None, :]).sum(axis=1)
            return out
        if w.dtype.kind != 'c':
            return one(w)
        out = np.empty((x.shape[0], w.shape[0]), dtype=np.complex128)
        out.real = one(w.real)                  # (each part on its own: `a + 1j * b` would carry a non-finite b into
        out.imag = one(w.imag)                  # the real part as 0 * b = NaN)
        return out
