/*
 * ltmi.h -- C ABI of libltmi.so: MI355X (gfx950) kernels for LiberTEM's mask-application /
 * virtual-detector hot path.
 *
 * The reference (LiberTEM, pure Python) has no FFI for this path; its operator boundary is the
 * Python UDF interface (`process_tile` / `merge`, src/libertem/udf/base.py:1334-1608).  Each entry
 * point below replaces the array-library call the reference makes *inside* that interface and
 * cites it.  All pointers named `*_dev` / `tile` / `out` are DEVICE pointers owned by the caller
 * (torch-ROCm tensors' data_ptr()); the library never allocates user-visible memory.  It owns only
 * the opaque mask handles (prepared device images of the mask stack + a partial-sum workspace).
 *
 * Conventions
 *   - every function returns 0 (LTMI_OK) on success, a negative LTMI_E_* code for argument errors,
 *     or a positive code: a hipError_t, or LTMI_E_RCCL_BASE + ncclResult_t from the ltmi_comm_*
 *     functions; `ltmi_last_error()` returns a thread-local message.
 *   - nothing throws across the ABI.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); all work is enqueued on it and
 *     the call returns without synchronising.  A handle must be used on one stream at a time
 *     (its workspace is reused by consecutive calls).
 *   - `device` is the HIP device ordinal; handles remember theirs and every call on a handle
 *     switches to it (hipSetDevice) first.
 *   - tiles are row-major `(n_frames, n_px)` with `ld_tile` ELEMENTS between consecutive frames,
 *     i.e. exactly the flattened C-contiguous tile `tile.reshape((n, -1))` of
 *     src/libertem/udf/masks.py:79-83.
 */
#ifndef LTMI_H
#define LTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libltmi.so is built with -fvisibility=hidden: the functions declared between this push and the pop
 * at the end of the header are the WHOLE dynamic symbol table of the library (tests/test_runtime_cpu.py
 * compares `nm -D` with this header). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define LTMI_VERSION 1

#define LTMI_OK 0
#define LTMI_E_INVALID (-1)      /* bad argument (null pointer, negative size, ...) */
#define LTMI_E_DTYPE (-2)        /* dtype combination not supported */
#define LTMI_E_SHAPE (-3)        /* shapes do not match the handle */
#define LTMI_E_NOMEM (-4)        /* host allocation failed; a WDD filter or parallax store that does not fit */
#define LTMI_E_RCCL_BASE 10000   /* a failing RCCL call returns LTMI_E_RCCL_BASE + ncclResult_t */

/* dtype codes (numpy names) */
enum ltmi_dtype {
    LTMI_BOOL = 0, LTMI_U8 = 1, LTMI_I8 = 2, LTMI_U16 = 3, LTMI_I16 = 4, LTMI_U32 = 5,
    LTMI_I32 = 6, LTMI_U64 = 7, LTMI_I64 = 8, LTMI_F32 = 9, LTMI_F64 = 10, LTMI_C64 = 11,
    LTMI_C128 = 12
};

typedef struct ltmi_masks ltmi_masks;      /* opaque */

/* ---- misc ----------------------------------------------------------------------------- */
int ltmi_version(void);
const char *ltmi_last_error(void);
int ltmi_device_count(int *count);
/* name_out: at least 256 bytes. replaces libertem.utils.devices.detect() (utils/devices.py:31-60) */
int ltmi_device_info(int device, char *name_out, int *cu_count, int64_t *hbm_bytes, int *gfx_arch);

/* ---- mask stacks ------------------------------------------------------------------------
 * Dense stack.  Replaces MaskContainer.get_for_sig_slice(sig_slice, transpose=True) +
 * for_backend(m, backend).astype(dtype)  (src/libertem/common/container.py:74-94, :213-217):
 * `masks_host` is the HOST array of the sig-sliced, flattened stack, logical shape
 * (n_masks, n_px), C-contiguous ("mask-major", which is also the reference's physical layout),
 * already cast to `result_dtype` = np.result_type(input_dtype, mask_dtype)
 * (src/libertem/udf/masks.py:362).  The library converts it to its own device image
 * (see DESIGN.md "HBM layout") and keeps no reference to `masks_host`.
 */
int ltmi_masks_create_dense(int device, const void *masks_host, int result_dtype,
                            int64_t n_masks, int64_t n_px, ltmi_masks **out);

/* Sparse stack in CSR over pixels, exactly the matrix the reference builds in
 * _build_sparse (src/libertem/common/container.py:53-64): shape (n_px, n_masks),
 * indptr[n_px + 1], indices[nnz] (mask index), data[nnz] of `result_dtype`: float32, complex64,
 * float64, or -- for the integer result dtypes -- int64 values: ltmi_apply_masks then computes the
 * integer product with wrap-around (SciPy's integer matmul) through the float64 gather kernel and
 * fails with LTMI_E_DTYPE for a tile dtype whose sums could exceed 2^52 (bits of the tile dtype + bits
 * of the largest column sum of |values| > 52: densify and use ltmi_masks_create_dense).
 * complex128: pass (re, im) as two float64 columns (libertem_amd/hip.py MaskHandle.csr_complex128).
 * Host pointers; canonical format (sorted, no duplicates) is not required.
 * Two device images may be built: the sliced-ELL image of the gather kernel (always) and, for float32 /
 * complex64 stacks whose neighbouring masks share pixels (rings, radial bins), the blocked image that
 * runs on the matrix cores; ltmi_apply_masks picks the blocked one when it exists.  Environment (read here): LTMI_SPARSE_BELL=0 / 1 never / always builds the blocked image,
 * LTMI_BELL_MAX_RATIO moves the padding-factor threshold (default 8).
 * With LTMI_SPARSE_LABELS=1 a float32 stack that is a PARTITION -- no pixel is stored by two masks: the box masks of a
 * binned detector, a polar rebinning map, hard-edged rings -- and got neither the blocked nor the scatter image gets a
 * label image as well: a label and a weight per pixel, one multiply-add per labelled pixel (k_labels: uint8 / int8 /
 * uint16 / int16 / float32 tiles, row lists too); ltmi_masks_kind then reports 4.  Like the gather kernel it multiplies
 * stored entries only: an unlabelled non-finite pixel reaches no result, a stored zero weight times NaN is NaN.  Unset
 * or 0 the image is never built: the route is not the default because it is not yet faster than the gather kernel.
 * Both settings give valid results.
 */
int ltmi_masks_create_csr(int device, const int64_t *indptr, const int64_t *indices,
                          const void *data, int result_dtype, int64_t n_px, int64_t n_masks,
                          ltmi_masks **out);

/* Tells a float32 / complex64 handle the detector shape behind its n_px = sig_h * sig_w pixels (C order),
 * which the reference's MaskContainer knows from the mask arrays it stacks (common/container.py:260-314) and
 * flattens away before the product (udf/masks.py:79-83).  The library then looks for a mirror of the detector
 * rows, y -> c2 - y with c2 in {sig_h - 1, sig_h, sig_h + 1}, under which EVERY real column of the stack is even
 * or odd bit for bit -- radial-Fourier masks ring * exp(i o phi) (analysis/radialfourier.py:106-146), rings,
 * disks, centre-of-mass ramps built around the detector centre are -- and, when that saves matrix work (two or
 * more 16-column groups), keeps a folded image: float32 frames are then multiplied as
 * (x[y] + s x[c2 - y]) * w[y] over half of the rows with the stack's original weights (k_dense_fold).  Results
 * differ from the unfolded product by float32 round-off only; a stack without such a mirror is left as it is.
 * A CSR handle (ltmi_masks_create_csr, float32 / complex64) whose masks fall into blocks with ONE pixel support each
 * -- the orders of a bin in a radial-Fourier stack with several bins (n_bins > 1, use_sparse=True) -- and has such
 * a mirror gets a folded DENSE image per block over the 64-pixel stages that touch the block's support
 * (k_dense_fold / k_dense_fold16 over stage lists; float32 and 1- / 2-byte integer frames) when the cost estimate
 * favours it over the blocked sparse image; ltmi_masks_kind then reports 3.  The handle keeps a host copy of the
 * CSR arrays until this call or its first product.
 * Optional; LTMI_DENSE_FOLD=0 / LTMI_SPARSE_BAND=0 in the environment disable the searches (LTMI_SPARSE_BAND=1:
 * whatever the estimate says). */
int ltmi_masks_set_sig_shape(ltmi_masks *m, int sig_h, int sig_w);

/* Non-finite pixels (NaN / Inf in float32 / float64 frames): which zeros of a stack meet them.
 * The reference has two arithmetics.  A SPARSE stack is multiplied entry by stored entry
 * (`res_t[col, :] += left[:, row] * val`, src/libertem/common/numba/__init__.py:153-184; pydata path
 * src/libertem/udf/masks.py:71-74): a non-finite pixel reaches exactly the masks that store it.  A DENSE stack is
 * multiplied whole (`flat_tile @ masks` / torch.mm, src/libertem/udf/masks.py:59-66, :76-77): 0 * NaN = NaN, a
 * non-finite pixel reaches every mask.  Handles follow the arithmetic of the constructor that made them
 * (ltmi_masks_create_dense: dense, ltmi_masks_create_csr: sparse) on EVERY kernel route: where a fast kernel of a
 * CSR handle also multiplies padding zeros (blocked, scatter, banded images), ltmi_apply_masks[_rows] reads the
 * result rows of float frames, lists the frames with a non-finite result on the device and computes those again
 * on the gather kernel (stored entries only) -- one small extra kernel on clean data, no host synchronisation
 * (csrc/ltmi_guard.hip; LTMI_NONFINITE_GUARD=0 in the environment switches it off for timing comparisons).
 * The two calls below are for a caller that hands a stack to the OTHER constructor because that kernel is faster:
 *
 * ltmi_masks_set_sparse_origin: `m` (from ltmi_masks_create_dense) holds a stack that the reference multiplies
 * SPARSE -- a well-filled CSR stack that was densified; `gather` is the handle of ltmi_masks_create_csr for the same
 * stack (same device, n_px, result row: float32 / complex64 / float64, or float64 column pairs for a complex128
 * stack).  `m` takes ownership of `gather` (destroyed with it) and its products then follow the sparse arithmetic as
 * above, whichever dense kernel runs (LDS-DMA, folded, float64).
 *
 * ltmi_masks_set_dense_origin: `m` (from ltmi_masks_create_csr, float32 / complex64, fewer than 15 360 masks) holds
 * the non-zeros of a stack that the reference multiplies DENSE -- column blocks with a pixel support each, which
 * the banded image serves faster (ltmi_masks_set_sig_shape).  indptr / indices: the CSR arrays given to
 * ltmi_masks_create_csr (host; not kept).  Frames with a non-finite result or a non-finite pixel that no mask
 * stores are listed, and in their rows every mask that does not store ALL non-finite pixels of the frame
 * becomes NaN (a skipped 0 * NaN); masks that store them all keep the kernel's sums, which then equal the dense
 * product.  float32 frames only. */
int ltmi_masks_set_sparse_origin(ltmi_masks *m, ltmi_masks *gather);
/* ltmi_masks_create_csr with the gather kernel's image only (no blocked / scatter / banded images are tried): the
 * handle to pass as `gather` above.  Same arguments, same result dtypes. */
int ltmi_masks_create_csr_gather(int device, const int64_t *indptr, const int64_t *indices,
                                 const void *data, int result_dtype, int64_t n_px, int64_t n_masks,
                                 ltmi_masks **out);
int ltmi_masks_set_dense_origin(ltmi_masks *m, const int64_t *indptr, const int64_t *indices);
/* How many frames of the LAST product on this handle were listed for the redo / fix-up above (frames with a non-finite
 * result, or -- dense stack held as CSR -- a non-finite pixel no mask stores).  Diagnostic; SYNCHRONISES `stream` (the
 * stream of that product).  0 when the product was not checked (integer frames, a handle that is not guarded, the
 * gather kernel).  The reference has no counterpart: its NaNs simply appear in the result. */
int ltmi_masks_nonfinite_frames(ltmi_masks *m, void *stream, int64_t *count);

int ltmi_masks_destroy(ltmi_masks *m);
/* 0 = dense with float32 / complex64 results (f32 matrix cores), 1 = dense with any other result
 * dtype (float64, complex128 on real tiles, exactly representable integer sums: f64 matrix cores;
 * complex tiles and wider integers: VALU kernel), 2 = csr, 3 = csr with a banded dense image (see
 * ltmi_masks_set_sig_shape), 4 = csr with a label image (a partition stack, see ltmi_masks_create_csr).  3 and 4 say
 * which image the handle HOLDS, not what every product runs on: with kind 4, bool / 32- / 64-bit tiles, set_tuning 41 /
 * 42 and a handle with ltmi_masks_set_dense_origin stay on the gather kernel (ltmi_masks_last_kernel names the route) */
int ltmi_masks_kind(const ltmi_masks *m, int *kind);

/* ---- the hot call -----------------------------------------------------------------------
 * out[f, k] (+)= sum_p tile[f, p] * masks[k, p]
 * Replaces ApplyMasksEngine.process_flat (torch.mm / `flat_tile @ masks` / rmatmul:
 * src/libertem/udf/masks.py:59-77, src/libertem/common/numba/__init__.py:90-184) fused with the
 * dtype conversion of the tile (io/dataset/memory.py:102-105) and with the accumulation
 * `results.intensity[:] += ...` (src/libertem/udf/masks.py:389-392) when accumulate != 0.
 *   tile       device pointer, (n_frames, n_px) of `tile_dtype` (the dataset's NATIVE dtype --
 *              the astype(input_dtype) copy is fused), ld_tile elements between frames; element
 *              alignment is enough (rows of odd length: the 16-byte loads / LDS-DMA of gfx950 take
 *              any address; LTMI_ALIGNED_DMA_ONLY=1 in the environment keeps the vector paths to
 *              16-byte aligned rows)
 *   out        device pointer, (n_frames, n_masks) of the handle's result dtype, ld_out elements
 *   accumulate 0: out = product, 1: out += product
 */
int ltmi_apply_masks(ltmi_masks *m, const void *tile, int tile_dtype, int64_t n_frames,
                     int64_t ld_tile, void *out, int64_t ld_out, int accumulate, void *stream);

/* The same product for SELECTED frames of a tile, through a device list of frame numbers -- a region
 * of interest without the gathered copy of its frames (reference: the ROI is applied while reading,
 * frame by frame, io/dataset/memory.py:107-131; buffers are ROI-compressed, common/buffers.py:419-505):
 *   out[i, k] (+)= sum_p tile[rows[i], p] * masks[k, p],   0 <= i < n_rows
 * `rows`: DEVICE array of n_rows int32 frame numbers relative to `tile`.  *handled = 0 and nothing is
 * done when the handle / tile combination has no row-list kernel (then gather with ltmi_gather_rows and
 * call ltmi_apply_masks): row lists are served for dense float32 / complex64 stacks on uint8 / int8 /
 * uint16 / int16 / float32 tiles of at least one mask slot per frame, for dense float64 / complex128 /
 * exact-integer results of real tiles (>= 256 pixels per frame), and for sparse (CSR) stacks (both
 * sparse kernels, float32 / complex64 / float64 results).
 */
int ltmi_apply_masks_rows(ltmi_masks *m, const void *tile, int tile_dtype, const int32_t *rows,
                          int64_t n_rows, int64_t ld_tile, void *out, int64_t ld_out, int accumulate,
                          void *stream, int *handled);

/* Shifted masks: out[f, k] (+)= sum over the overlap of frame[f][y, x] * mask_k[y - dy_f, x - dx_f]
 * Replaces ApplyMasksEngine.process_frame_shifted (src/libertem/udf/masks.py:85-124), one call per
 * tile instead of one per frame.  Dense handles only.  `shifts` is a DEVICE array of n_frames
 * (dy, dx) int32 pairs; frames are (sig_h, sig_w) row-major, sig_h * sig_w == the handle's n_px.
 * A positive dy moves the mask down relative to the frame; no overlap contributes 0.  Any int32 pair
 * is a valid shift: |dy| >= sig_h or |dx| >= sig_w is "no overlap", however large.
 * Only pixels inside the overlap are read: a NaN / Inf pixel that the shift cuts off does not exist
 * for this product, one inside the overlap reaches every mask (0 * NaN = NaN), as in the reference.
 */
int ltmi_apply_masks_shifted(ltmi_masks *m, const void *tile, int tile_dtype, int64_t n_frames,
                             int64_t ld_tile, int sig_h, int sig_w, const int32_t *shifts,
                             void *out, int64_t ld_out, int accumulate, void *stream);

/* Same operation with the shifts on the HOST (n_frames (dy, dx) int32 pairs): lets the library
 * group the frames by shift and run them through the MFMA kernel against shifted copies of the
 * mask image (built on the device, cached in the handle, <= 4 GiB) -- one launch per tile at
 * close to the unshifted rate (float32 / complex64 results); float64 / complex128 / exact-integer
 * results: the f64 matrix-core kernel per group of frames with the same shift (one call for a tile
 * with a constant shift; up to 256 distinct shifts per tile, up to 4096 while a shift is shared by 8 frames on
 * average and the shifted images fit 4 GiB).  Falls back to the per-frame kernel
 * above (after uploading the shifts) for handles / tiles these paths do not take.
 * Non-finite pixels: the matrix-core routes multiply the WHOLE frame with an image that is zero
 * outside the overlap, which equals the product over the overlap for finite pixels only.  For
 * float32 / float64 frames the frames with a non-finite result row are therefore listed on the
 * device (no host synchronisation) and computed again by the per-frame kernel, so that the result
 * is the one documented above on every route; with `accumulate` the product of such a tile is
 * formed in a scratch buffer of the handle and added to `out` afterwards.  Integer frames run as
 * they are.  LTMI_NONFINITE_GUARD=0 in the environment switches this off (timing ablation): a
 * non-finite pixel anywhere in a frame then makes every result of that frame NaN on these routes. */
int ltmi_apply_masks_shifted_host(ltmi_masks *m, const void *tile, int tile_dtype, int64_t n_frames,
                                  int64_t ld_tile, int sig_h, int sig_w, const int32_t *shifts_host,
                                  void *out, int64_t ld_out, int accumulate, void *stream);

/* ---- reductions -------------------------------------------------------------------------
 * SumUDF.process_tile: out[p] (+)= sum_f tile[f, p]        (src/libertem/udf/sum.py:43-48)
 *   out: device (n_px,) of out_dtype; `workspace` device scratch of at least
 *   ltmi_sum_frames_workspace(n_frames, n_px, out_dtype) bytes (may be NULL if that is 0).
 *   out_dtype follows the reference's rule "result dtype = input dtype" (udf/sum.py:38-40):
 *   float32 / float64 for any real tile; complex64 / complex128 for complex (or real) tiles; an
 *   integer dtype for integer tiles (SumUDF(dtype=<integer>)): exact int64 accumulation, stored
 *   truncated = NumPy's wrap-around in the narrower type
 *   (reference tests/analysis/test_analysis_sum.py:157-163 `test_sum_complex`).
 */
int64_t ltmi_sum_frames_workspace(int64_t n_frames, int64_t n_px, int out_dtype);
int ltmi_sum_frames(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                    int64_t ld_tile, void *out, int out_dtype, int accumulate, void *workspace,
                    void *stream);
/* SumSigUDF.process_tile: out[f] (+)= sum_p tile[f, p]   (src/libertem/udf/sumsigudf.py:30-39);
 * out_dtype float32 / float64 for real tiles, complex64 / complex128 for complex tiles
 * (result_type(input, float32), udf/sumsigudf.py:23) */
int ltmi_sum_sig(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                 int64_t ld_tile, void *out, int out_dtype, int accumulate, void *stream);
/* StdDevUDF.process_tile: fold the n_frames frames of `tile` into running per-pixel moments
 * (src/libertem/udf/stddev.py:103-168 `process_tile`, :425-451 `StdDevUDF.process_tile`):
 *   sum[p]    = sum of the frames,  varsum[p] = sum over frames of |x - mean|^2,
 * both over the n_prev frames they already hold plus the tile's; n_prev == 0 overwrites them.
 * The tile's moments are computed per slab of frames in float64 about a shift (the slab's first
 * frame), the slabs and the running buffers are merged in a fixed order with the reference's
 * update (stddev.py:11-63): varsum += varsum_tile + n_tile |delta| |delta'| -- no atomics, the
 * results are bitwise repeatable.
 *   tile dtypes: uint8, int8, uint16, int16, uint32, int32, float32, float64, complex64, complex128;
 *   sum_dtype: float32 / float64 for real tiles, complex64 / complex128 for complex tiles;
 *   varsum_dtype: float32 / float64 (|x - mean|^2 of complex pixels).
 * Tile pixel p is element (p / cols) * ld_out + p % cols of `sum` and `varsum` (the strided
 * sub-rectangle of a partial-width sig slice; cols = ld_out = n_px: contiguous); n_px % cols == 0.
 * `workspace`: device scratch of ltmi_moments_workspace(n_frames, n_px, tile_dtype) bytes. */
int64_t ltmi_moments_workspace(int64_t n_frames, int64_t n_px, int tile_dtype);
int ltmi_moments_frames(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                        int64_t ld_tile, int64_t n_prev, void *sum, int sum_dtype, void *varsum,
                        int varsum_dtype, int64_t cols, int64_t ld_out, void *workspace, void *stream);
/* FEMUDF.process_frame: out[f] = np.std(frame_f[mask == 1])     (src/libertem/udf/FEM.py:65-66)
 * for the n_frames whole frames of `tile` (frame f at element f * ld_tile, pixel (r, x) at r * width + x;
 * complex pixels count as one element).  The ring is `spans`: device memory of n_spans int32 triples
 * (row, x0, x1), x0 < x1 <= width, row inside the frame, built on the host from the boolean mask
 * (FEM.py:44-63); n_ring = sum of x1 - x0.  Per frame float64 sums about the first ring pixel, reduced
 * in one workgroup in a fixed order (no atomics: bitwise repeatable); result sqrt(M2 / n) as float32,
 * ddof = 0, |x - mean|^2 for complex pixels.  An empty ring, or a NaN / inf pixel in it, gives NaN.
 *   tile dtypes: uint8, int8, uint16, int16, uint32, int32, float32, float64, complex64, complex128. */
int ltmi_ring_moments(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t width,
                      int64_t ld_tile, const void *spans, int n_spans, int64_t n_ring, void *out,
                      void *stream);
/* LogsumUDF.process_frame: out[p] += sum_f log(frame_f[p] - min(frame_f) + 1)
 * (src/libertem/udf/logsum.py:54-59) for the n_frames whole frames (n_px pixels) of `tile`.  Each term is
 * rounded in result_type(float32, tile dtype) (float for <= 16-bit integers and float32, double for
 * 32-bit integers and float64), the min propagates NaN (np.min); the terms are summed in float64 per
 * slab of frames and merged in a fixed order into the float32 `out` (no atomics: bitwise repeatable).
 *   tile dtypes: uint8, int8, uint16, int16, uint32, int32, float32, float64 (complex: LTMI_E_DTYPE).
 * Tile pixel p is element (p / cols) * ld_out + p % cols of `out`; n_px % cols == 0.
 * `workspace`: device scratch of ltmi_logsum_workspace(n_frames, n_px, tile_dtype) bytes. */
int64_t ltmi_logsum_workspace(int64_t n_frames, int64_t n_px, int tile_dtype);
int ltmi_logsum_frames(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                       int64_t ld_tile, void *out, int64_t cols, int64_t ld_out, void *workspace,
                       void *stream);
/* WeightedSumUDF.process_tile: out[c, p] (+)= sum_n weights[n, c] * frame_n[p] -- NumPy's
 * `weights.T @ tile.reshape((n, -1))`, the transposed mask product -- for the n_frames whole frames (n_px
 * pixels) of `tile` and 1 <= k <= 64 components (any other k: LTMI_E_SHAPE).  `weights`: float32
 * (n_frames, k) in device memory, ld_w >= k ELEMENTS between rows; `out`: float32, component c of tile pixel
 * p is element c * comp_stride + (p / cols) * ld_out + p % cols; n_px % cols == 0.  accumulate = 0
 * overwrites these elements, 1 adds to them; n_frames == 0 writes nothing either way.
 * Exact float32 FMAs on the matrix cores (v_mfma_f32_16x16x4_f32), one chain per slab of frames, the slabs
 * merged in float64 in a fixed order (no atomics: bitwise repeatable).  A NaN or inf pixel p of any frame
 * makes out[:, p] non-finite (0 * NaN, as in NumPy's dense product) and touches no other pixel.
 *   tile dtypes: bool, uint8, int8, uint16, int16, uint32, int32, float32 (others: LTMI_E_DTYPE); rows need
 *   not be 16-byte aligned.
 * `workspace`: device scratch of ltmi_wsum_workspace(n_frames, n_px, k) bytes -- the same for every tile
 * dtype, at most max(256 MiB, 4 k n_px). */
int64_t ltmi_wsum_workspace(int64_t n_frames, int64_t n_px, int k);
int ltmi_wsum_frames(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                     int64_t ld_tile, const void *weights, int k, int64_t ld_w, void *out, int64_t cols,
                     int64_t ld_out, int64_t comp_stride, int accumulate, void *workspace, void *stream);

/* merge for sig-kind buffers: dest[i] += src[i]         (src/libertem/udf/sum.py:50-52);
 * every dtype of enum ltmi_dtype but bool, integers wrap around like NumPy's `+=`.  LTMI_BOOL is
 * LTMI_E_DTYPE, also for ltmi_add2d: NumPy's `+=` on bool is a logical or and its `-=` an error. */
int ltmi_axpy(int device, void *dest, const void *src, int dtype, int64_t n, void *stream);
/* dest[r, c] (+|-)= src[r, c] for r < rows, c < cols; leading dimensions in ELEMENTS; ld_src == 0
 * broadcasts one row.  Replaces the NumPy in-place arithmetic around the kernels:
 *   `results.intensity[sig slice] += partial`  of a partial-width sig slice (src/libertem/udf/sum.py:43-48),
 *   the per-mask dark-frame constant of folded corrections (negate = 1, ld_src = 0;
 *   src/libertem/io/corrections/detector.py:315-338),
 *   `dest.intensity[:] += src.intensity`  (src/libertem/udf/sum.py:50-52). */
int ltmi_add2d(int device, void *dest, int64_t ld_dest, const void *src, int64_t ld_src, int dtype,
               int64_t rows, int64_t cols, int negate, void *stream);
/* dest[i, :] = src[idx[i], :]  -- the frames an ROI selects, gathered inside HBM (the reference
 * reads them frame by frame on the host, src/libertem/io/dataset/memory.py:107-131).
 * idx: DEVICE int64 (n_rows,); rows of row_bytes bytes, ld_src_bytes between source rows. */
int ltmi_gather_rows(int device, const void *src, int64_t ld_src_bytes, const int64_t *idx,
                     int64_t n_rows, int64_t row_bytes, void *dest, void *stream);

/* Host-to-host copy on `threads` threads (<= 0: a default from the core count, at most 16; capped at 64; at
 * least 1 MiB per thread): the staging copy of host-resident frames into page-locked bounce buffers, which has to keep
 * up with the H2D link.  Replaces, on the upload path of host datasets, the per-tile `astype` / slicing copies the
 * reference makes while reading (src/libertem/io/dataset/memory.py:102-131) -- here the bytes travel unconverted and
 * the dtype conversion happens in the kernels.  Plain memcpy semantics (no overlap); calls are serialised. */
int ltmi_host_copy(void *dst, const void *src, int64_t bytes, int threads);

/* Device address of page-locked host memory (hipHostMalloc / hipHostRegister): the place where the
 * kernels above may write small write-once result rows directly (`out` = this address), instead of
 * the reference's per-partition D2H export of device buffers (src/libertem/common/buffers.py:901-907). */
int ltmi_host_device_pointer(int device, void *host, void **dev_out);

/* ---- sparse frames (CSR) ---------------------------------------------------------------------
 * A scan whose frames are stored sparse -- the triple of the reference's RawCSRDataSet
 * (src/libertem/io/dataset/raw_csr.py:99-132, 410-431): row r of the CSR matrix is frame r, flattened;
 * `indptr` DEVICE int64 [n_rows + 1] starting at 0, `indices` DEVICE int32 [nnz] (flat pixel numbers),
 * `data` DEVICE [nnz] of the file's dtype.  The reference hands scipy.sparse tiles of it to the UDFs
 * (raw_csr.py:481-532); here the triple stays in HBM and the two kernels below read frames out of it.
 * Both assume CANONICAL rows -- indices strictly ascending, inside [0, n_px) -- which ltmi_csr_check
 * establishes once: no atomics, plain stores, bitwise repeatable results.  Frames are addressed as
 * `row0 + i` (rows == NULL) or `rows[i]` (DEVICE int32 list: a region of interest), 0 <= i < n_frames.
 *
 * ltmi_csr_check: *flags (DEVICE int, overwritten) = 0 for a canonical triple; bit 0: data that cannot be
 * used (an index outside [0, n_px), indptr decreasing, not starting at 0 or not ending at nnz -- rows with
 * a bad indptr are not read); bit 1: a row that is unsorted or stores a pixel twice (scipy's
 * sum_duplicates() on the host repairs those). */
int ltmi_csr_check(int device, const int64_t *indptr, const int32_t *indices, int64_t n_rows, int64_t n_px,
                   int64_t nnz, int *flags, void *stream);
/* out[i, p] = the dense frame: zero where nothing is stored.  Replaces `tile.toarray()` /
 * for_backend(tile, NUMPY) of the reference's UDF runner for UDFs that take dense tiles
 * (src/libertem/udf/base.py:2196-2206).  out: DEVICE (n_frames, n_px) of data_dtype (any 1 / 2 / 4 / 8 byte
 * dtype: the values are moved, not converted), ld_out >= n_px elements between frames; the elements
 * [n_px, ld_out) of a row are left as they are. */
int ltmi_csr_densify(int device, const int64_t *indptr, const int32_t *indices, const void *data,
                     int data_dtype, const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px,
                     void *out, int64_t ld_out, void *stream);
/* out[i, k] (+)= sum over the stored entries e of frame i of data[e] * masks[k, indices[e]]
 * Replaces ApplyMasksEngine.process_flat on a scipy.sparse CSR tile (`flat_tile @ masks`,
 * src/libertem/udf/masks.py:59-77) without densifying the frames.  `m`: a handle of
 * ltmi_masks_create_dense with float32 or float64 results and at most ltmi_csr_max_masks() masks; the
 * stack is kept a second time pixel-major ([n_px][masks padded to a power of two]), built on the first
 * call.  data dtypes: uint8, uint16, int16, uint32, int32, float32, converted to the result dtype and
 * accumulated in it.  A non-finite stored value reaches every mask of its frame (0 * NaN = NaN), as in the
 * dense product.  *handled = 0 and nothing is done for any other handle or data dtype (then densify and
 * call ltmi_apply_masks).  ltmi_masks_last_kernel reports "k_apply_csr<...>". */
int ltmi_apply_masks_csr(ltmi_masks *m, const int64_t *indptr, const int32_t *indices, const void *data,
                         int data_dtype, const int32_t *rows, int64_t row0, int64_t n_frames, void *out,
                         int64_t ld_out, int accumulate, void *stream, int *handled);
int ltmi_csr_max_masks(void);
/* The two sums that are functions of the stored entries alone, on the triple in place (no dense frames).  Both
 * rely on canonical rows, both skip a stored index outside [0, n_px) instead of following it, both are exact for
 * integer data and bitwise repeatable.  out_dtype: LTMI_F32 or LTMI_F64.  n_frames == 0 launches nothing.
 *
 * ltmi_csr_sum_sig: out[i] (+)= sum of the stored entries of frame i -- SumSigUDF on a sparse tile
 * (src/libertem/udf/sumsigudf.py:30-39 on a scipy.sparse tile).  out: DEVICE (n_frames,).  data dtypes uint8, uint16,
 * int16, uint32, int32 (summed in int64, converted once: the exact sum, correctly rounded) and float32 (summed in
 * float64, rounded once; a stored NaN makes its frame NaN).  A frame without entries gives 0. */
int ltmi_csr_sum_sig(int device, const int64_t *indptr, const int32_t *indices, const void *data, int data_dtype,
                     const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px, void *out, int out_dtype,
                     int accumulate, void *stream);
/* ltmi_csr_sum_frames: out[p] (+)= sum over the n_frames frames of their entry at pixel p -- SumUDF on a sparse
 * tile (src/libertem/udf/sum.py:43-48).  out: DEVICE (n_px,).  INTEGER data only (uint8, uint16, int16, uint32,
 * int32; float32 is LTMI_E_DTYPE: a float sum depends on its order, and the dense route's order is the one that is
 * pinned): every pixel is summed in int64 and converted once.  workspace: DEVICE, ltmi_csr_sum_frames_workspace(n_px)
 * bytes, 8-byte aligned, the caller's; its contents on entry do not matter and it can serve the next call. */
int64_t ltmi_csr_sum_frames_workspace(int64_t n_px);
int ltmi_csr_sum_frames(int device, const int64_t *indptr, const int32_t *indices, const void *data, int data_dtype,
                        const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px, void *out, int out_dtype,
                        int accumulate, void *workspace, void *stream);
/* Which kernel the calling thread's last ltmi_csr_sum_sig / ltmi_csr_sum_frames launched, e.g.
 * "k_csr_sum_sig<u16,f32>", "k_csr_sum_frames<i32,f64> rows" (" rows": a row list was passed); "" before the first.
 * A call that fails its argument checks or has n_frames == 0 launches nothing and leaves the string as it was. */
const char *ltmi_csr_last_kernel(void);

/* ---- detector corrections -------------------------------------------------------------------
 * Replaces CorrectionSet.apply -> detector.correct on a tile (src/libertem/io/corrections/
 * corrset.py:140-166, detector.py:17-101, called from io/dataset/base/backend.py:121-124) fused
 * with the astype(read_dtype) copy of io/dataset/memory.py:102-105:
 *   out[f, p] = ((double)tile[f, p] - dark[p]) * gain[p]      (dark / gain may be NULL)
 * `dark`, `gain`: DEVICE float64 arrays of n_px.  out: device (n_frames, n_px) of F32 or F64.
 */
int ltmi_correct(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                 int64_t ld_tile, const double *dark, const double *gain, void *out, int out_dtype,
                 int64_t ld_out, void *stream);
/* dead-pixel repair, in place: buf[f, excl[e]] = mean(buf[f, env[e][0..cnt[e])]) for all frames.
 * Tables as built by RepairDescriptor (detector.py:278-312): DEVICE int32 arrays excl[n_excl],
 * env[n_excl][max_env] (flat pixel indices of the good neighbours), cnt[n_excl]. */
int ltmi_repair_pixels(int device, void *buf, int dtype, int64_t n_frames, int64_t ld,
                       const int32_t *excl, const int32_t *env, const int32_t *cnt, int n_excl,
                       int max_env, void *stream);

/* Byte-order decode on the device: dst[i] = src[i] with its `itemsize` (1, 2, 4, 8) bytes reversed,
 * n_items items; src == dst (in place) is allowed.  Replaces the byte-swapping decoders of
 * DtypeConversionDecoder (src/libertem/io/dataset/base/decode.py:8-66, 74-100, 123-158), which run
 * on the host for every tile of a non-native-endian dataset; the dtype conversion those decoders
 * fuse (decode_swap_N) happens in the consuming kernels, which take every native dtype. */
int ltmi_byteswap(int device, const void *src, void *dst, int itemsize, int64_t n_items,
                  void *stream);

/* Merlin / Medipix .mib frames decoded on the device.  `src`: DEVICE copy of (part of) a .mib file starting
 * at a frame header; frame f = src + f * frame_stride: `header_bytes` of ASCII header, then the payload.
 * kind 'u' (bits 8 / 16 / 32): big-endian unsigned integers -> native LTMI_U8 / U16 / U32.
 * kind 'r' (bits 1 / 6 / 12 / 24, the detector's raw "R64" words): -> LTMI_U8 / U8 / U16 / U32 (24 bit
 * also LTMI_F32, exact); `quad` != 0: raw rows of a 2x2 detector ([chip 4 | chip 3 | chip 2 | chip 1],
 * chips 3 / 4 rotated by 180 degrees) assembled into height x width frames.  dst: (n_frames, height, width)
 * contiguous, `dst_dtype` must be the dtype named above.  Replaces MIBDecoder and its numba decoders
 * decode_r{1,6,12,24}_swap / decode_r{1,6,12}_swap_2x2 plus the per-row read ranges that feed them
 * (src/libertem/io/dataset/mib.py:224-398, 401-735), which the reference runs on the host per tile. */
int ltmi_mib_decode(int device, const void *src, int64_t frame_stride, int64_t header_bytes, int kind,
                    int bits, int quad, int64_t n_frames, int height, int width, void *dst,
                    int dst_dtype, void *stream);
/* Which of the two decode kernels the calling thread's last ltmi_mib_decode launched, e.g.
 * "k_mib_decode16<u16>" (16 bytes of output per thread: payloads of whole 16-byte chunks),
 * "k_mib_decode<r12,quad>" (one 64-bit word per thread: every other shape, and every shape while
 * LTMI_MIB_WORDS is set in the environment, which is read on every call), "k_mib_decode16<r24f>" (24 bit
 * into LTMI_F32).  "" before the first decode; a call that fails its argument checks or has n_frames == 0
 * launches nothing and leaves the string as it was.  Thread-local storage: valid until the thread's next
 * decode. */
const char *ltmi_mib_last_kernel(void);

/* Gatan K2 IS sector files decoded on the device.  `sector_src`: HOST array of 8 DEVICE pointers, one per
 * sector file (`*_1.bin` ... `*_8.bin`); pointer s is at the first block of the first frame of sector s in the
 * uploaded file bytes, frame f of the sector at sector_src[s] + f * 32 * 0x5758 (32 blocks of a 40-byte header
 * + 930 rows x 16 pixels, 12 bit little-endian: a = b0 | (b1 & 0x0F) << 8, b = b1 >> 4 | b2 << 4).  The 8
 * pointers are independent (the sectors need not start at the same file offset); each is a multiple of 8
 * bytes, which every block and payload row then is too.  Block k of a frame covers the rows
 * [930 (k / 16), +930) and the frame columns [256 s + 16 (15 - k % 16), +16).  dst: (n_frames, 1860, 2048)
 * contiguous, 16-byte aligned, `dst_dtype` must be LTMI_U16.  n_frames == 0 launches nothing.  Replaces
 * K2ISDecoder's decode_k2is / decode_uint12_le and the per-block read ranges that feed them
 * (src/libertem/io/dataset/k2is.py:82-164, 172-231), which the reference runs on the host per tile. */
int ltmi_k2is_decode(int device, const void *const sector_src[8], int64_t n_frames, void *dst,
                     int dst_dtype, void *stream);

/* PNDetector pnCCD .frms6 frames unfolded on the device.  `src`: DEVICE address of the first frame's payload in
 * a copy of (part of) a .frms6 file; the payload of frame f is at src + f * frame_stride (in a file: 64-byte
 * frame header + payload, so frame_stride = 64 + height * width * 2): `height` rows of `width` little-endian
 * uint16, folded.  With x = width / 2 the output frame is (2 * height * binning, x): output row y, binned index
 * yb = y / binning, is raw row yb, columns [0, x), in order for yb < height, and raw row 2 * height - 1 - yb,
 * columns [x, 2 x), reversed otherwise; binned rows are repeated, not rescaled.  dst: (n_frames,
 * 2 * height * binning, x) contiguous, `dst_dtype` must be LTMI_U16.  `width` is even, `binning` 1, 2 or 4, src and
 * frame_stride multiples of 2, height and width at most 65535.  Half rows of whole 16-byte pieces (x % 8 == 0)
 * with src, frame_stride and dst multiples of 16 take the kernel with 16-byte loads and stores, every other
 * geometry the one with a pixel per lane: chosen here, on the host.  n_frames == 0 (or an empty frame) launches
 * nothing.  Replaces the per-row read ranges and FRMS6Decoder's row-by-row decoders
 * (src/libertem/io/dataset/frms6.py:232-366), which the reference runs on the host per tile. */
int ltmi_frms6_decode(int device, const void *src, int64_t frame_stride, int64_t n_frames, int height,
                      int width, int binning, void *dst, int dst_dtype, void *stream);
/* Which kernel the calling thread's last ltmi_frms6_decode launched: "k_frms6_unfold16" or "k_frms6_unfold2";
 * "" before the first.  A call that launches nothing leaves the string as it was. */
const char *ltmi_frms6_last_kernel(void);

/* Frame records gathered on the device: the payloads of a file of fixed-size records [frame header | pixels |
 * frame footer] (Norpix .seq, EMPAD .raw, NanoMegas .blo) moved into one contiguous array.  `src`: DEVICE address of
 * the first frame's PAYLOAD in a copy of (part of) the file -- the caller has added the file header and the frame
 * header; the payload of frame i is the `payload_bytes` bytes at src + i * record_stride.  dst: DEVICE,
 * contiguous, frame i at dst + i * payload_bytes.  Bytes are moved, not converted.  No byte outside the payloads
 * is read and none outside [dst, dst + n_frames * payload_bytes) is written: the last record may end with its
 * payload, the first may start the buffer.  One kernel k_records<W>, a lane moving W bytes per access; W is the
 * largest of 16, 8, 4, 2, 1 that divides the address src, record_stride, payload_bytes and the address dst
 * (chosen here, on the host; no realignment that reads around a payload).  Frames are not a grid dimension and
 * all offsets are 64-bit: any number of frames, records any distance apart.  n_frames == 0 launches nothing.
 * n_frames < 0, payload_bytes < 1 and record_stride < payload_bytes: LTMI_E_SHAPE.  Replaces the per-tile read
 * ranges with which the reference strips frame headers and footers on the host
 * (src/libertem/io/dataset/base/tiling.py, decode.py). */
int ltmi_records_gather(int device, const void *src, int64_t record_stride, int64_t n_frames,
                        int64_t payload_bytes, void *dst, void *stream);
/* Which kernel the calling thread's last ltmi_records_gather launched: "k_records<16>" ... "k_records<1>"; ""
 * before the first.  A call that launches nothing leaves the string as it was. */
const char *ltmi_records_last_kernel(void);

/* Out-of-place transposition on the device: dst[c * ld_dst + r] = src[r * ld_src + c] for r < rows, c < cols.
 * src, dst: DEVICE, element-aligned (16-byte elements: 8), not overlapping; ld_src >= cols and ld_dst >= rows, in
 * elements.  Elements of item_bytes = 1, 2, 4, 8 or 16 bytes are moved, never interpreted (any dtype of that size,
 * complex128 included).  One kernel k_transpose<item_bytes>: a workgroup stages one tile (128 x 128 elements at 1
 * and 2 bytes, 64 x 64 at 4 and 8, 32 x 32 at 16) through an XOR-swizzled LDS image per step, so the global reads
 * run along the rows of src and the global writes along the rows of dst, 128 B to 512 B per row segment; edge tiles
 * are predicated.  Tiles are walked with a grid stride and all offsets are 64-bit: no grid dimension bounds rows or
 * cols.  No byte of dst outside the cols x rows rectangle is written (not the padding between rows and ld_dst
 * either) and none of src outside the rows x cols rectangle is read.  2 * rows * cols * item_bytes bytes of HBM
 * traffic.  rows == 0 or cols == 0 launches nothing.  Negative sizes and null pointers with work to do:
 * LTMI_E_INVALID; ld_src < cols, ld_dst < rows and sizes whose byte span does not fit int64: LTMI_E_SHAPE; any
 * other item_bytes: LTMI_E_DTYPE.  Replaces the `partition.T` assignment into the memory map of
 * ConvertTransposedDatasetUDF.process_partition (src/libertem/contrib/convert_transposed.py:28-40), which the
 * reference runs on one CPU thread per partition. */
int ltmi_transpose2d(int device, const void *src, int64_t ld_src, int64_t rows, int64_t cols, int item_bytes,
                     void *dst, int64_t ld_dst, void *stream);
/* Which kernel the calling thread's last ltmi_transpose2d launched: "k_transpose<1>" ... "k_transpose<16>"; ""
 * before the first.  A call that launches nothing leaves the string as it was.  (Names the instantiation behind
 * src/libertem/contrib/convert_transposed.py:28-40.) */
const char *ltmi_transpose_last_kernel(void);

/* Centre-of-mass post-processing on a 2D scan of ny x nx positions: from the rows (sum, sum*y, sum*x)
 * of the 3-mask product to the shift field and its derived maps, float64.  Replaces the NumPy chain
 * center_shifts -> apply_correction -> magnitude / divergence / curl_2d of src/libertem/udf/com.py:
 * 100-142 (run by COMAnalysis.get_generic_results, src/libertem/analysis/com.py:191-284):
 *   yc = (sum != 0 ? sum*y / sum : ref_y) - ref_y   (float32, like NumPy on float32 arrays), same for x;
 *   (y, x) = transform (2x2 row-major float64: rotation / flip, HOST pointer) . (yc, xc);
 *   magnitude = sqrt(y^2 + x^2); divergence = d y/dy + d x/dx; curl = d y/dx - d x/dy with
 *   np.gradient's stencils (central inside, one-sided at the edges, unit spacing).
 * raw: device float32, row i = scan position i, ld_raw floats between rows (>= 3); outputs: device
 * float64 (ny*nx each); out_mag / out_div / out_curl may be NULL. */
int ltmi_com_fields(int device, const float *raw, int64_t ld_raw, int ny, int nx, double ref_y,
                    double ref_x, const double *transform, double *out_y, double *out_x,
                    double *out_mag, double *out_div, double *out_curl, void *stream);

/* ---- Fourier-space operators (hipFFT) ----------------------------------------------------------
 * A plan owns a batched 2D real-to-complex hipFFT (frames of sig_h x sig_w float32, `max_batch`
 * per execution) and its workspace (f32 input + complex64 half spectra).
 */
typedef struct ltmi_fft_plan ltmi_fft_plan;   /* opaque */
int ltmi_fft_plan_create(int device, int sig_h, int sig_w, int max_batch, ltmi_fft_plan **out);
int ltmi_fft_plan_destroy(ltmi_fft_plan *p);
/* CrystallinityUDF.process_frame (src/libertem/udf/crystallinity.py:73-79) for a whole tile:
 *   out[f] (+)= sum( abs(rfft2(tile[f] * real_mask)) * half_mask )
 * tile: device (n_frames, sig_h*sig_w) of tile_dtype, ld_tile elements apart (native dtype, the
 * astype is fused); real_mask: device float32 (sig_h*sig_w) or NULL; half_mask: device float32
 * (sig_h, sig_w/2+1) = fftshift(ring)[:, :w/2+1] (crystallinity.py:64-65); its non-zeros lie in the
 * rows [0, row_lo) and [row_hi, sig_h) and in the columns [0, n_cols): only that box of the
 * spectrum is read (row_lo = row_hi = sig_h, n_cols = sig_w/2+1 reads everything);
 * out: device float32 (n_frames). */
int ltmi_crystallinity(ltmi_fft_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                       int64_t ld_tile, const float *real_mask, const float *half_mask, int row_lo,
                       int row_hi, int n_cols, float *out, int accumulate, void *stream);
/* The same on RAW frames with the detector corrections fused into the conversion pass (reference:
 * CorrectionSet.apply inside the tile read, src/libertem/io/corrections/detector.py:17-101, then
 * udf/crystallinity.py:73-79): v = (float)(((double)x - dark) * gain), every excluded pixel = mean
 * of its good neighbours' corrected values; no corrected copy of the tile is written.
 * dark / gain: device float64 (sig_h*sig_w) or NULL; excl (n_excl), env (n_excl, max_env),
 * cnt (n_excl): device int32 repair tables as for ltmi_repair_pixels (n_excl = 0: none).
 * 128 x 128 / 256 x 256 / 512 x 512 / 1024 x 1024 frames: the corrected float32 frames of a batch are written to the plan's workspace and
 * transformed by the fused kernel (see ltmi_fft_plan_last_kernel) instead of hipFFT. */
int ltmi_crystallinity_corrected(ltmi_fft_plan *p, const void *tile, int tile_dtype,
                                 int64_t n_frames, int64_t ld_tile, const double *dark,
                                 const double *gain, const int32_t *excl, const int32_t *env,
                                 const int32_t *cnt, int n_excl, int max_env,
                                 const float *real_mask, const float *half_mask, int row_lo,
                                 int row_hi, int n_cols, float *out, int accumulate, void *stream);
/* Which route the last ltmi_crystallinity* call of this plan took: "k_cryst_fused<...>" (256 x 256
 * frames, rings of up to 71 columns) / "k_cryst_fused128<...>" (128 x 128 frames, any ring): rows, columns
 * and the ring sum of a frame in the LDS of one workgroup; "k_cryst_rows<w><...> + k_cryst_cols<h>" (frames whose edges
 * are 256 / 512 / 1024 pixels in any combination -- 256 x 256 only for rings of more than 71 columns --, any ring: the ring's columns of the row transforms pass through the plan's workspace)
 * (csrc/ltmi_cryst.hip); or "hipfft_r2c<...>".  LTMI_FFT_FUSED=0 at plan creation keeps every
 * frame on hipFFT.  The string lives as long as the plan. */
const char *ltmi_fft_plan_last_kernel(const ltmi_fft_plan *p);

/* ---- template matching at given peaks (hipFFT) ---------------------------------------------------
 * A correlation plan owns a batched 2D real-to-complex and a complex-to-real hipFFT (frames of
 * sig_h x sig_w float32, `max_batch` per execution), their workspace (f32 frames + complex64 half
 * spectra of one batch) and the spectrum of ONE template.
 * template_host: HOST float32 (sig_h, sig_w), centred at (sig_h/2, sig_w/2); the plan stores
 * conj(rfft2(ifftshift(t))) / (sig_h sig_w) on the device, computed once with its own forward plan. */
typedef struct ltmi_corr_plan ltmi_corr_plan;   /* opaque */
int ltmi_corr_plan_create(int device, int sig_h, int sig_w, int max_batch, const float *template_host,
                          ltmi_corr_plan **out);
int ltmi_corr_plan_destroy(ltmi_corr_plan *p);
/* For every frame f of the tile and every peak k:
 *   corr = irfft2(rfft2((float)tile[f]) * conj(rfft2(ifftshift(t))))        (circular cross-correlation)
 *   W = corr[py-r .. py+r, px-r .. px+r], clipped to the frame (no wrap-around), r = crop_radius
 *   peak_values[f, k]     = max(W)
 *   centers[f, k]         = (y, x) of the first maximum of W in row-major order, frame coordinates
 *   refineds[f, k]        = centre of mass of N - min(N), N = the (2q+1)^2 neighbourhood of centers[f, k]
 *                           clipped to the frame, q = refine_radius; centers[f, k] if the weights sum to 0
 *   peak_elevations[f, k] = (max(W) - mean(W)) / std(W), ddof 0; 0 if std(W) is 0
 * A frame with a non-finite pixel gets peak_values = NaN for every peak (its other results are then the
 * window's first position and NaN); other frames are unaffected.
 * tile: device (n_frames, sig_h*sig_w) of tile_dtype (the dtypes ltmi_crystallinity takes), ld_tile
 * elements apart; peaks: device int32 (n_peaks, 2) of (py, px) inside the frame -- read back and checked
 * by every call, which therefore waits for the work already on `stream`; centers: device int32
 * (n_frames, n_peaks, 2); refineds: device float32 (n_frames, n_peaks, 2); peak_values, peak_elevations:
 * device float32 (n_frames, n_peaks).  No atomics: the results of a call repeat bit for bit.
 * A peak outside the frame, crop_radius < 1 or refine_radius < 1: LTMI_E_SHAPE. */
int ltmi_correlate_peaks(ltmi_corr_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                         int64_t ld_tile, const int32_t *peaks, int n_peaks, int crop_radius,
                         int refine_radius, int32_t *centers, float *refineds, float *peak_values,
                         float *peak_elevations, void *stream);
/* The kernels of the last ltmi_correlate_peaks call of this plan:
 * "k_corr_load<dtype> + hipfft_r2c + k_corr_mul + hipfft_c2r + k_corr_peaks batch=N" (csrc/ltmi_corr.hip).
 * The string lives as long as the plan. */
const char *ltmi_corr_plan_last_kernel(const ltmi_corr_plan *p);

/* ---- the strongest correlation maxima of every frame ---------------------
 * For every map c of (h, w) float32, with N = num_peaks, d = min_distance, b = border, q = refine_radius:
 *   1. p = (y, x) is a candidate iff, over every other p' with |y'-y| <= d and |x'-x| <= d inside the frame,
 *      c[p] > c[p'] where p' precedes p in row-major order and c[p] >= c[p'] where it follows;
 *   2. a candidate is eligible iff b <= y < h-b, b <= x < w-b and c[p] > threshold_abs;
 *   3. the eligible candidates by value descending, then index ascending; v0 the first value; if v0 > 0 those with
 *      c[p] < threshold_rel * v0 (one float32 multiply) go; the first N of the rest are kept: n_found[f];
 *   4. for k < n_found[f]: centers[f, k] = (y, x), and peak_values, refineds, peak_elevations as ltmi_correlate_peaks
 *      gives them for the peak centers[f, k] with crop_radius = d and refine_radius = q;
 *   5. for k >= n_found[f]: centers (-1, -1), the rest NaN;
 *   6. a map with a non-finite value has n_found = 0.
 * maps: DEVICE float32, map f at maps + f * ld_map (rows contiguous).  n_found: device int32 (n_frames); centers:
 * device int32 (n_frames, N, 2); refineds: device float32 (n_frames, N, 2); peak_values, peak_elevations: device
 * float32 (n_frames, N).  Limits: N <= 1024, w <= 8192, h w <= 2^31 - 1; any d (any number of cells per frame).
 * No atomics: the results of a call repeat bit for bit.  Nothing is read back and the stream is not drained; the
 * candidate scratch (16 bytes per (d+1)^2 cell and frame, at most 256 MiB at a time) belongs to the calling thread.
 * num_peaks outside [1, 1024], min_distance < 1, refine_radius < 1, border < 0 or 2 border >= min(h, w),
 * threshold_rel outside [0, 1], a NaN threshold, ld_map < h w, n_frames < 0: LTMI_E_SHAPE; a null pointer:
 * LTMI_E_INVALID.  n_frames == 0 launches nothing. */
int ltmi_find_peaks_maps(int device, const float *maps, int64_t n_frames, int h, int w, int64_t ld_map,
                         int num_peaks, int min_distance, int border, float threshold_abs, float threshold_rel,
                         int refine_radius, int32_t *n_found, int32_t *centers, float *refineds,
                         float *peak_values, float *peak_elevations, void *stream);
/* "k_pf_cells + k_pf_verify + k_pf_select + k_corr_found" after the first launching ltmi_find_peaks_maps call of
 * the calling thread, "" before. */
const char *ltmi_find_peaks_last_kernel(void);
/* The same search on the correlation maps of a tile: per batch the transforms of ltmi_correlate_peaks
 * (k_corr_load, R2C, k_corr_mul, C2R), then the search on the plan's workspace.  There is no peak list to check, so
 * nothing is read back and the stream is not drained.  ltmi_corr_plan_last_kernel then names
 * "k_corr_load<dtype> + hipfft_r2c + k_corr_mul + hipfft_c2r + k_pf_cells + k_pf_verify + k_pf_select +
 * k_corr_found batch=N".  Errors as above; an unsupported tile dtype: LTMI_E_DTYPE; ld_tile < h w: LTMI_E_SHAPE. */
int ltmi_correlate_find(ltmi_corr_plan *p, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                        int num_peaks, int min_distance, int border, float threshold_abs, float threshold_rel,
                        int refine_radius, int32_t *n_found, int32_t *centers, float *refineds, float *peak_values,
                        float *peak_elevations, void *stream);

/* ---- electron counting (csrc/ltmi_count.hip) --------------------------------
 * What an event is.  For every frame of (h, w) pixels, row-major pixel number p = y w + x, with the float32
 * thresholds t_bg (background) and t_x (x-ray; +inf switches it off):
 *   1. v[p] = float32(pixel[p]), rounded to nearest even like ndarray.astype(float32); with `dark`, v = v - dark[p],
 *      one float32 subtraction; with `gain`, v = v * gain[p], one float32 multiplication; subtract, then multiply;
 *   2. u[p] = v[p] if v[p] <= t_x, else 0: an x-ray hit is zeroed and does not count, NaN compares false and becomes
 *      0, +Inf with t_x = +inf stays and can be an event;
 *   3. p is an EVENT iff u[p] > t_bg and, over its up to 8 neighbours q inside the frame, u[p] > u[q] where q < p and
 *      u[p] >= u[q] where q > p: of equal neighbours the first in row-major order wins, no two events are adjacent;
 *   4. the events of a frame are listed by ascending p; an event's value is uint8(1) or u[p] as float32.
 * Every decision is an exact float32 comparison: the results are the bytes of the definition, and they repeat.
 * tile: DEVICE, frame f at tile + f * ld_tile pixels (rows contiguous, ld_tile >= h w), tile_dtype one of LTMI_U8,
 * LTMI_I8, LTMI_U16, LTMI_I16, LTMI_U32, LTMI_I32, LTMI_F32 (anything else: LTMI_E_DTYPE).  dark, gain: DEVICE
 * float32 (h w), or NULL.  Limits: h, w >= 1, h w <= 2^31 - 1, and w <= 4096 -- a strip of rows and its two halo
 * rows are staged in 48 KiB of LDS, which three rows of 4096 + 8 float32 fill.  n_frames < 0, a size outside the
 * limits, ld_tile < h w, a NaN threshold: LTMI_E_SHAPE; a null tile or output with work to do: LTMI_E_INVALID.
 * n_frames == 0 launches nothing.  Nothing is read back and the stream is not drained.
 *
 * n_events[f] = number of events of frame f (device int32, n_frames). */
int ltmi_count_events(int device, const void *tile, int tile_dtype, int64_t n_frames, int h, int w, int64_t ld_tile,
                      const float *dark, const float *gain, float t_bg, float t_x, int32_t *n_events, void *stream);
/* Writes frame f's events to indices_out[indptr[f] - base .. indptr[f + 1] - base), ascending, and their values to
 * the same places of values_out (values_dtype LTMI_U8: 1; LTMI_F32: u[p]; anything else: LTMI_E_DTYPE; values_out
 * NULL: indices only).  indptr: DEVICE int64 (n_frames + 1); indices_out, values_out: DEVICE, `capacity` elements
 * (capacity < 0: LTMI_E_SHAPE); status: DEVICE int32 (1), zeroed by the caller.  Writes go only to
 * [indptr[f] - base, indptr[f + 1] - base) intersected with [0, capacity).  *status becomes non-zero (an atomic or)
 * if the events of a frame do not number exactly indptr[f + 1] - indptr[f] or a range leaves [0, capacity); what
 * then stands inside the ranges is unspecified, nothing outside them is touched.  The order of the output needs no
 * sort and no atomic: a call's results repeat bit for bit. */
int ltmi_store_events(int device, const void *tile, int tile_dtype, int64_t n_frames, int h, int w, int64_t ld_tile,
                      const float *dark, const float *gain, float t_bg, float t_x, const int64_t *indptr,
                      int64_t base, int64_t capacity, int32_t *indices_out, void *values_out, int values_dtype,
                      int32_t *status, void *stream);
/* Rows of a strip for frames of (h, w): min(30, h, what fits the LDS budget); 0 for sizes outside the limits.  A
 * frame is walked in strips of this many rows (the last may be shorter). */
int ltmi_count_strip_rows(int h, int w);
/* "k_count_events" / "k_store_events" after the calling thread's last launching call, with " vec" where the pixels
 * were loaded 16 bytes per lane (w a multiple of 4); "" before the first. */
const char *ltmi_count_last_kernel(void);

/* ---- orientation matching in polar coordinates (csrc/ltmi_orient.hip) --------
 * Every frame against T templates at every in-plane rotation, reduced to the n_best best templates on the device.
 * Every float32 operation below is rounded on its own (no fused multiply-add), so everything but `norm_out` is the
 * bytes of the definition.  For a frame of (sig_h, sig_w) pixels:
 *   1. the sampling table gives every polar point (i, j), i < n_r, j < n_phi, four taps: pixel numbers
 *      tap_idx[i, j, 0..3] and float32 weights tap_w[i, j, 0..3] (bilinear: libertem_amd.udf.orientation.polar_table);
 *   2. P[i, j] = (w0 v0 + w1 v1) + (w2 v2 + w3 v3), v = float32(pixel at the tap): four float32 products, three
 *      float32 sums, in this association.  A tap of weight 0 is not read: its v is +0;
 *   3. template t holds the spots s in [indptr[t], indptr[t + 1]): (spot_r, spot_phi, spot_w);
 *   4. for a rotation k < n_phi: acc = +0, then over the spots in stored order
 *      acc = acc + spot_w[s] * P[spot_r[s], (spot_phi[s] + k) mod n_phi] (one float32 multiply, one float32 add);
 *      c[t] = the maximum of acc over k, rot[t] = the smallest k that reaches it; an empty template: c = 0, rot = 0;
 *   5. the templates by c descending, then t ascending: the first n_best fill template_out[f, :], rotation_out[f, :],
 *      correlation_out[f, :]; slots from min(n_best, T) on hold -1, -1, NaN;
 *   6. norm_out[f] = float32(sqrt(sum of float64(P[i, j])^2)), summed in float64 (a fixed order: it repeats);
 *   7. a frame with a non-finite pixel at a tap of non-zero weight: every slot -1, -1, NaN and norm_out NaN.
 * Frames whose P or scores overflow float32 are outside the definition.
 * A plan owns device copies of the table and the library.  tap_idx: HOST int32 (n_r, n_phi, 4), every entry in
 * [0, sig_h sig_w); tap_w: HOST float32 (n_r, n_phi, 4), finite; indptr: HOST int64 (n_templates + 1), from 0,
 * ascending; spot_r, spot_phi: HOST int32 in [0, n_r) and [0, n_phi); spot_w: HOST float32, finite -- all checked here.
 * Limits: 1 <= n_best <= 16, 1 <= n_phi <= 1024, n_r >= 1, n_r n_phi <= ltmi_orient_max_polar_words() (the polar
 * image and the kernel's other LDS share the 160 KiB of a CU), n_templates >= 1, sig_h sig_w <= 2^31 - 1; outside
 * them, or an entry out of range: LTMI_E_SHAPE, with the offending value in ltmi_last_error; a null pointer:
 * LTMI_E_INVALID. */
typedef struct ltmi_orient_plan ltmi_orient_plan;   /* opaque */
int ltmi_orient_plan_create(int device, int sig_h, int sig_w, int n_r, int n_phi, const int32_t *tap_idx,
                            const float *tap_w, int n_templates, const int64_t *indptr, const int32_t *spot_r,
                            const int32_t *spot_phi, const float *spot_w, int n_best, ltmi_orient_plan **out);
int ltmi_orient_plan_destroy(ltmi_orient_plan *p);
/* Steps 2 - 7 for n_frames frames.  tile: DEVICE, frame f at tile + f * ld_tile pixels (rows contiguous, ld_tile >=
 * sig_h sig_w), tile_dtype one of LTMI_U8, LTMI_I8, LTMI_U16, LTMI_I16, LTMI_U32, LTMI_I32, LTMI_F32 (anything else:
 * LTMI_E_DTYPE).  template_out, rotation_out: DEVICE int32 (n_frames, n_best); correlation_out: DEVICE float32
 * (n_frames, n_best); norm_out: DEVICE float32 (n_frames).  One workgroup per frame at a time; no atomics, a call's
 * results repeat bit for bit.  n_frames < 0 or ld_tile too small: LTMI_E_SHAPE; a null pointer with work to do:
 * LTMI_E_INVALID; n_frames == 0 launches nothing.  Nothing is read back and the stream is not drained. */
int ltmi_orient_match(ltmi_orient_plan *p, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                      int32_t *template_out, int32_t *rotation_out, float *correlation_out, float *norm_out,
                      void *stream);
/* Step 2 alone: P of frame f to polar_out + f * ld_polar (DEVICE float32, ld_polar >= n_r n_phi, else LTMI_E_SHAPE),
 * as computed -- non-finite taps propagate.  Arguments and errors as ltmi_orient_match. */
int ltmi_orient_polar(ltmi_orient_plan *p, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                      float *polar_out, int64_t ld_polar, void *stream);
/* "k_orient_match<dtype,NCH> grid=G lds=B" (NCH: the accumulators a lane holds, at least ceil(n_phi / 64)) or
 * "k_orient_polar<dtype>" after the plan's last launching call, "" before.  The string lives as long as the plan. */
const char *ltmi_orient_plan_last_kernel(const ltmi_orient_plan *p);
/* The largest n_r n_phi a plan takes, and the number of templates whose scores are selected from at a time. */
int ltmi_orient_max_polar_words(void);
int ltmi_orient_score_block(void);

/* ---- off-axis hologram reconstruction (hipFFT) -----------------------------
 * With s(i, n) = i for i <= (n-1)/2, else i - n (the signed frequency of index i, fftfreq order), for every frame:
 *   F = fft2((float)tile[f]) / (sig_h sig_w)
 *   G[u, v] = F[(sb_y + s(u, out_h)) mod sig_h, (sb_x + s(v, out_w)) mod sig_w] * aperture[u, v]
 *   wave = the unnormalised inverse DFT of G (= out_h out_w ifft2(G)), times ref_inv elementwise where given
 * A holography plan owns a batched 2D real-to-complex hipFFT of (sig_h, sig_w), a batched unnormalised
 * complex-to-complex backward hipFFT of (out_h, out_w), `max_batch` frames per execution, and their workspace: f32
 * frames, complex64 half spectra and complex64 outputs of one batch.
 * aperture_host: HOST float32 (out_h, out_w) in the unshifted layout, (0, 0) the sideband centre; stored on the device
 * as float32(aperture / (sig_h sig_w)), divided in float64.  ref_inv_host: HOST complex64 (out_h, out_w) as float
 * pairs, 1 / reference_wave, or NULL.
 * out_h > sig_h, out_w > sig_w, a non-positive shape, a sideband outside [0, sig_h) x [0, sig_w), a batch of more
 * than 2^31 - 1 pixels: LTMI_E_SHAPE; a null aperture or `out`, max_batch < 1: LTMI_E_INVALID. */
typedef struct ltmi_holo_plan ltmi_holo_plan;   /* opaque */
int ltmi_holo_plan_create(int device, int sig_h, int sig_w, int out_h, int out_w, int max_batch, int sb_y, int sb_x,
                          const float *aperture_host, const float *ref_inv_host, ltmi_holo_plan **out);
int ltmi_holo_plan_destroy(ltmi_holo_plan *p);
/* tile: device (n_frames, sig_h*sig_w) of tile_dtype (the dtypes ltmi_correlate_peaks takes), ld_tile elements apart;
 * out: device complex64 (n_frames, out_h*out_w), rows ld_out elements apart -- nothing between the rows and no row
 * from n_frames on is written.  Per batch: k_corr_load, R2C, k_holo_crop, C2C backward in place, k_holo_store
 * (csrc/ltmi_holo.hip).  A frame with a non-finite pixel has an unspecified wave; other frames are unaffected.  No
 * atomics: the results of a call repeat bit for bit.  Nothing is read back and the stream is not drained.
 * n_frames < 0, ld_tile < sig_h sig_w, ld_out < out_h out_w: LTMI_E_SHAPE; an unsupported tile dtype: LTMI_E_DTYPE;
 * a null pointer: LTMI_E_INVALID.  n_frames == 0 launches nothing. */
int ltmi_holo_reconstruct(ltmi_holo_plan *p, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                          void *out, int64_t ld_out, void *stream);
/* The kernels of the last launching ltmi_holo_reconstruct call of this plan:
 * "k_corr_load<dtype> + hipfft_r2c + k_holo_crop + hipfft_c2c + k_holo_store batch=N".  The string lives as long as
 * the plan. */
const char *ltmi_holo_plan_last_kernel(const ltmi_holo_plan *p);
/* Step 2 alone, on half spectra the caller supplies: spec is DEVICE complex64, frame f's (h, w/2 + 1) half spectrum
 * (what a real-to-complex transform of (h, w) stores) at spec + f * ld_spec elements.  Output element (u, v) reads
 * ky = (sb_y + s(u, out_h)) mod h, kx = (sb_x + s(v, out_w)) mod w: spec[ky, kx] for kx <= w/2, else
 * conj(spec[(h - ky) mod h, w - kx]); both components are multiplied by aperture_dev[u, v] (DEVICE float32
 * (out_h, out_w), used as it is) -- one float32 multiply each, so the result is defined bit for bit.  g_out: device
 * complex64, frame f at g_out + f * ld_g elements.  One launch of k_holo_crop.  Shape errors as for the plan, and
 * ld_spec < h (w/2 + 1), ld_g < out_h out_w, n_frames < 0: LTMI_E_SHAPE; a null pointer: LTMI_E_INVALID.
 * n_frames == 0 launches nothing. */
int ltmi_holo_crop(int device, const void *spec, int64_t n_frames, int h, int w, int64_t ld_spec, int out_h, int out_w,
                   int sb_y, int sb_x, const float *aperture_dev, void *g_out, int64_t ld_g, void *stream);

/* ---- exit-wave power cepstrum (hipFFT) --------------------------------------
 * For every frame, with y = (float)tile[f], all of it in float32:
 *   t = logf(max(y, 0) + offset) * window                       (sig_h, sig_w)
 *   C = |fft2(t)| / (sig_h sig_w)                               unshifted
 *   out[u, v] = C[(u - out_h/2) mod sig_h, (v - out_w/2) mod sig_w] * keep[u, v]
 * The output is centred like fftshift: quefrency (0, 0) at (out_h / 2, out_w / 2) (integer division); with
 * out_h == sig_h and out_w == sig_w it is fftshift(C), for even and odd sizes.  keep[u, v] = 0 where
 * hypot(u - out_h/2, v - out_w/2) < dc_radius (decided in float64 on the host), else 1.
 * A cepstrum plan owns a batched 2D real-to-complex hipFFT of (sig_h, sig_w), `max_batch` frames per execution, its
 * workspace (f32 frames and complex64 half spectra of one batch), the window (HOST float32 (sig_h, sig_w), copied) and
 * scale = float32(keep / (sig_h sig_w)), divided in float64.
 * out_h > sig_h, out_w > sig_w, a non-positive shape, a batch of more than 2^31 - 1 pixels: LTMI_E_SHAPE; a null
 * window or `out`, max_batch < 1, an offset that is not positive and finite, dc_radius < 0 or NaN: LTMI_E_INVALID. */
typedef struct ltmi_ceps_plan ltmi_ceps_plan;   /* opaque */
int ltmi_ceps_plan_create(int device, int sig_h, int sig_w, int out_h, int out_w, int max_batch, float offset,
                          const float *window_host, double dc_radius, ltmi_ceps_plan **out);
int ltmi_ceps_plan_destroy(ltmi_ceps_plan *p);
/* tile: device (n_frames, sig_h*sig_w) of tile_dtype (the dtypes ltmi_correlate_peaks takes), ld_tile elements apart;
 * out: device float32 (n_frames, out_h*out_w), rows ld_out elements apart -- nothing between the rows and no row from
 * n_frames on is written.  Per batch: k_ceps_load, R2C, k_ceps_store (csrc/ltmi_ceps.hip).  A frame with a non-finite
 * pixel has an unspecified result; other frames are unaffected.  Negative pixels count as 0.  No atomics: the results
 * of a call repeat bit for bit.  Nothing is read back and the stream is not drained.
 * n_frames < 0, ld_tile < sig_h sig_w, ld_out < out_h out_w: LTMI_E_SHAPE; an unsupported tile dtype: LTMI_E_DTYPE;
 * a null pointer: LTMI_E_INVALID.  n_frames == 0 launches nothing. */
int ltmi_ceps_transform(ltmi_ceps_plan *p, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                        float *out, int64_t ld_out, void *stream);
/* The kernels of the last launching ltmi_ceps_transform call of this plan:
 * "k_ceps_load<dtype> + hipfft_r2c + k_ceps_store batch=N".  The string lives as long as the plan. */
const char *ltmi_ceps_plan_last_kernel(const ltmi_ceps_plan *p);
/* Step 1 alone: out[f, p] = logf(max((float)tile[f, p], 0) + offset) * window_dev[p] for p < n_px; tile: device, frames
 * ld_tile elements apart; window_dev: DEVICE float32 (n_px); out: device float32 (n_frames, n_px), contiguous.  One
 * launch of k_ceps_load.  n_frames < 0, n_px < 1, ld_tile < n_px: LTMI_E_SHAPE; an unsupported tile dtype:
 * LTMI_E_DTYPE; an offset that is not positive and finite, a null pointer: LTMI_E_INVALID.  n_frames == 0 launches
 * nothing. */
int ltmi_ceps_load(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile, int64_t n_px,
                   float offset, const float *window_dev, float *out, void *stream);
/* Step 3 alone, on half spectra the caller supplies: spec is DEVICE complex64, frame f's (h, w/2 + 1) half spectrum at
 * spec + f * ld_spec elements.  Output element (u, v) reads ky = (u - out_h/2) mod h, kx = (v - out_w/2) mod w:
 * spec[ky, kx] for kx <= w/2, else spec[(h - ky) mod h, w - kx] (the magnitude needs no conjugate);
 * out = sqrt(re * re + im * im) * scale_dev[u, v] (DEVICE float32 (out_h, out_w), used as it is), every float32
 * operation rounded on its own and the square root correctly rounded, so the result is defined bit for bit.  out:
 * device float32, frame f at out + f * ld_out elements.  One launch of k_ceps_store.  Shape errors as for the plan, and
 * ld_spec < h (w/2 + 1), ld_out < out_h out_w, n_frames < 0: LTMI_E_SHAPE; a null pointer: LTMI_E_INVALID.
 * n_frames == 0 launches nothing. */
int ltmi_ceps_store(int device, const void *spec, int64_t n_frames, int h, int w, int64_t ld_spec, int out_h, int out_w,
                    const float *scale_dev, float *out, int64_t ld_out, void *stream);

/* ---- single-sideband ptychography (hipFFT) ---------------------------------
 * For a scan of (nav_y, nav_x) positions of real frames, P bright-field pixels K listed by their row-major frame
 * index idx[K] (pixel (y, x) = (idx / sig_w, idx % sig_w)), s(i, n) the signed frequency of index i as above, and the
 * geometry geom[LTMI_SSB_GEOM] = { lamb, dy, dx, semiconv, semiconv_pix, cy, cx, t00, t01, t10, t11 } (HOST doubles):
 *   G[K, iy, ix] = sum over the scan positions (ry, rx) of bf[ry nav_x + rx, K] exp(-2 pi i (s(iy) ry / nav_y +
 *                  s(ix) rx / nav_x))                          (the unnormalised DFT over the scan axes)
 *   for Q = (iy, ix) != (0, 0):
 *     qy = s(iy) / (nav_y dy), qx = s(ix) / (nav_x dx)
 *     d  = ((t00 qy + t01 qx) lamb semiconv_pix / semiconv, (t10 qy + t11 qx) lamb semiconv_pix / semiconv)
 *     in+(K) = (y - (cy + d_y))^2 + (x - (cx + d_x))^2 < semiconv_pix^2,   in-(K) the same with (cy - d_y, cx - d_x)
 *     pos = in+ and not in-, neg = in- and not in+, over the LISTED pixels (the caller lists the pixels of the disk
 *     (y - cy)^2 + (x - cx)^2 < semiconv_pix^2; the library does not test that)
 *     fourier[Q] = (sum_pos G[K, Q] / |pos| - sum_neg G[K, Q] / |neg|) / 2 if |pos| >= cutoff and |neg| >= cutoff,
 *                  else 0
 *   fourier[0, 0] = sum over all listed K of G[K, 0, 0] / P
 * The predicates are evaluated on the device in float64, every product, quotient and sum rounded on its own and in
 * the order written (products and quotients left to right): they agree with a NumPy float64 evaluation bit for bit.
 * The sums over K accumulate in float64 in a fixed order (thread, wave shuffle tree, waves in order, batches in
 * order), the quotients are float64, the result is cast to complex64 once.  No atomics: the results of a call repeat
 * bit for bit.  Every Q is computed from its own d; nothing is filled in by symmetry. */
#define LTMI_SSB_GEOM 11
/* The bright-field pixels of every frame: out[f, k] = (float)tile[f, idx[k]].  tile: device (n_frames, n_px) of
 * tile_dtype (the dtypes ltmi_correlate_peaks takes), ld_tile elements apart; idx_dev: DEVICE int32 (n_idx), frame
 * indices in any order -- an index outside [0, n_px) reads nothing and gives 0; out: device float32 (n_frames, n_idx),
 * rows ld_out elements apart -- nothing between the rows and no row from n_frames on is written.  One launch of
 * k_ssb_gather<dtype> (csrc/ltmi_ssb.hip), which converts in registers and walks the frames beyond 65535 grid rows in
 * a loop.  n_frames == 0 or n_idx == 0 launches nothing.  n_frames < 0, n_idx < 0, n_px < 1, ld_tile < n_px,
 * ld_out < n_idx: LTMI_E_SHAPE; an unsupported tile dtype: LTMI_E_DTYPE; a null pointer: LTMI_E_INVALID. */
int ltmi_ssb_gather(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile, int64_t n_px,
                    const int32_t *idx_dev, int n_idx, float *out, int64_t ld_out, void *stream);
/* A plan owns the list (idx_host: HOST int32 (n_idx), copied to the device), the geometry, one batched 2D
 * real-to-complex hipFFT of (nav_y, nav_x), min(max_batch, n_idx) bright-field pixels per execution, and its
 * workspace: per pixel of a batch the float32 scan image, its complex64 half spectrum (nav_y, nav_x/2 + 1) and the
 * transposed copy of that; plans of more than one batch also 40 bytes per Q for the sums so far.
 * A scan of one row or one column is transformed by a batched 1D hipFFT.
 * A non-positive scan or one of a single position, n_idx < 1, sig_w < 1, cutoff < 1, a non-finite geometry value, a
 * non-positive lamb, dy, dx, semiconv or semiconv_pix, a batch of more than 2^31 - 1 values: LTMI_E_SHAPE; a null
 * pointer, max_batch < 1: LTMI_E_INVALID. */
typedef struct ltmi_ssb_plan ltmi_ssb_plan;   /* opaque */
int ltmi_ssb_plan_create(int device, int nav_y, int nav_x, int sig_w, const int32_t *idx_host, int n_idx,
                         int max_batch, const double *geom, int cutoff, ltmi_ssb_plan **out);
int ltmi_ssb_plan_destroy(ltmi_ssb_plan *p);
/* bf: device float32 (nav_y nav_x, n_idx), rows ld_bf elements apart (what ltmi_ssb_gather wrote for the whole scan);
 * fourier_out: device complex64 (nav_y, nav_x), contiguous, the unshifted layout.  Per batch: ltmi_transpose2d (the
 * batch's columns of bf -> one scan image per pixel), R2C, ltmi_transpose2d (spectra -> (Q, pixel)), k_ssb_trotter.
 * Nothing is read back and the stream is not drained.  A pixel of bf that is not finite gives an unspecified result.
 * ld_bf < n_idx: LTMI_E_SHAPE; a null pointer: LTMI_E_INVALID. */
int ltmi_ssb_reconstruct(ltmi_ssb_plan *p, const float *bf, int64_t ld_bf, void *fourier_out, void *stream);
/* "k_transpose<4> + hipfft_r2c + k_transpose<8> + k_ssb_trotter batch=N" after the first ltmi_ssb_reconstruct call of
 * this plan, "" before.  The string lives as long as the plan. */
const char *ltmi_ssb_plan_last_kernel(const ltmi_ssb_plan *p);
/* The last step alone, on half spectra the caller supplies: spec is DEVICE complex64, element
 * spec[(iy (nav_x/2 + 1) + ix) ld_spec + K] = G[K, iy, ix] for ix <= nav_x / 2 (what a real-to-complex transform over
 * the scan axes of bf viewed as (nav_y, nav_x, P) stores); a Q with ix > nav_x / 2 reads the conjugate at
 * ((nav_y - iy) mod nav_y, nav_x - ix).  idx_dev: DEVICE int32 (n_idx) -- the indices give coordinates and never
 * address memory.  One launch of k_ssb_trotter, one workgroup per Q.  Errors as for the plan, and ld_spec < n_idx:
 * LTMI_E_SHAPE. */
int ltmi_ssb_trotter(int device, const void *spec, int64_t ld_spec, int nav_y, int nav_x, const int32_t *idx_dev,
                     int n_idx, int sig_w, const double *geom, int cutoff, void *fourier_out, void *stream);

/* ---- Wigner-distribution deconvolution ptychography (hipFFT) ---------------
 * The scan, s(i, n), d(Q), the geometry array and the float64 disk predicates are those of the single-sideband section
 * above.  window[LTMI_WDD_WINDOW] = { y0, x0, By, Bx } (HOST ints) names the detector pixels [y0, y0 + By) x
 * [x0, x0 + Bx); window pixel K = v Bx + u is detector pixel (y0 + v, x0 + u) -- the coordinates never address memory.
 * P = the window pixels with (y - cy)^2 + (x - cx)^2 < semiconv_pix^2 (the caller chooses a window that holds the whole
 * disk; the library does not test that).  For every Q = (iy, ix), the DC included:
 *   Gamma[K] = 1 where K lies in that disk and in the one centred at (cy, cx) - d(Q), else 0
 *   chi[rho] = sum_K Gamma[K] exp(+2 pi i (v rho_y / By + u rho_x / Bx))
 *   W[rho]   = conj(chi[rho]) / (|chi[rho]|^2 + epsilon P^2)
 *   F[Q, K]  = sum_rho W[rho] exp(+2 pi i (v rho_y / By + u rho_x / Bx))
 *   S[Q]     = sum_K G[K, Q] F[Q, K] / (By Bx)
 *   fourier[Q] = conj(S[(-iy) mod nav_y, (-ix) mod nav_x]) / |S[0, 0]|
 * chi and F come from an unnormalised backward complex64 hipFFT, W from a float64 quotient cast once; S accumulates in
 * float64 in a fixed order (thread, wave shuffle tree, waves in order, batches in order) and is cast to complex64 once.
 * A Q whose two disks share no window pixel has F = 0 and S = 0 exactly.  No atomics: a call repeats bit for bit.
 * All-zero data gives NaN (0 / 0). */
#define LTMI_WDD_WINDOW 4
/* F of the Qs q0 <= iy nav_x + ix < q0 + n_q -> filter_out, DEVICE complex64 (n_q, By Bx), contiguous.  q_batch Qs
 * per hipFFT execution (k_wdd_gamma, backward C2C, k_wdd_wiener, backward C2C).  The call owns its hipFFT plan and a
 * workspace of min(q_batch, n_q) windows and returns when the work on `stream` is done.  n_q == 0 launches nothing.
 * A non-positive scan or one of a single position, By < 1, Bx < 1, a non-positive or non-finite epsilon, a geometry
 * the single-sideband plan refuses, Qs outside the scan, P = 0, a batch of more than 2^31 - 1 values: LTMI_E_SHAPE; a
 * null pointer, q_batch < 1: LTMI_E_INVALID. */
int ltmi_wdd_filter(int device, int nav_y, int nav_x, const int *window, const double *geom, double epsilon,
                    int64_t q0, int64_t n_q, int q_batch, void *filter_out, void *stream);
/* acc[Q] (+)= sum over j < n_k of G[j, Q] filter[Q ld_filter + k0 + j] for every Q of the scan.  spec: DEVICE
 * complex64 half spectra laid out as ltmi_ssb_trotter takes them, spec[(iy (nav_x/2 + 1) + ix) ld_spec + j] = G[j, iy,
 * ix]; a Q with ix > nav_x / 2 reads the conjugate at ((nav_y - iy) mod nav_y, nav_x - ix).  acc: DEVICE float64
 * (nav_y nav_x, 2), real and imaginary part; first != 0: the sums start at zero, else at what acc holds.  One launch of
 * k_wdd_dot, one workgroup per Q.  A non-positive scan, k0 < 0, n_k < 1, ld_spec < n_k, ld_filter < k0 + n_k:
 * LTMI_E_SHAPE; a null pointer: LTMI_E_INVALID. */
int ltmi_wdd_dot(int device, const void *spec, int64_t ld_spec, int nav_y, int nav_x, const void *filter,
                 int64_t ld_filter, int k0, int n_k, double *acc, int first, void *stream);
/* fourier_out[Q] (DEVICE complex64 (nav_y, nav_x)) = conj(S[-Q]) / |S[0, 0]| with S = acc / n_window: one launch of
 * k_wdd_finish.  Errors as for ltmi_wdd_dot, and n_window < 1: LTMI_E_SHAPE. */
int ltmi_wdd_finish(int device, const double *acc, int nav_y, int nav_x, int n_window, void *fourier_out, void *stream);
/* A plan owns F for every Q (nav_y nav_x By Bx complex64, built at creation on the null stream), 16 bytes per Q for
 * the sums, one batched real-to-complex hipFFT of (nav_y, nav_x), min(max_batch, By Bx) window pixels per execution,
 * and the workspace of the single-sideband plan.  F that does not fit into the free device memory: LTMI_E_NOMEM, the
 * text gives the bytes needed.  The other errors as for ltmi_wdd_filter and ltmi_ssb_plan_create. */
typedef struct ltmi_wdd_plan ltmi_wdd_plan;   /* opaque */
int ltmi_wdd_plan_create(int device, int nav_y, int nav_x, const int *window, int max_batch, const double *geom,
                         double epsilon, ltmi_wdd_plan **out);
int ltmi_wdd_plan_destroy(ltmi_wdd_plan *p);
/* bf: device float32 (nav_y nav_x, By Bx), rows ld_bf elements apart (what ltmi_ssb_gather wrote for the window's
 * index list); fourier_out: device complex64 (nav_y, nav_x), contiguous, the unshifted layout.  Per batch the front
 * end of ltmi_ssb_reconstruct, then k_wdd_dot; k_wdd_finish after the last.  Nothing is read back and the stream is
 * not drained.  ld_bf < By Bx: LTMI_E_SHAPE; a null pointer: LTMI_E_INVALID. */
int ltmi_wdd_reconstruct(ltmi_wdd_plan *p, const float *bf, int64_t ld_bf, void *fourier_out, void *stream);
/* "k_transpose<4> + hipfft_r2c + k_transpose<8> + k_wdd_dot + k_wdd_finish batch=N" after the first
 * ltmi_wdd_reconstruct call of this plan, "" before.  The string lives as long as the plan. */
const char *ltmi_wdd_plan_last_kernel(const ltmi_wdd_plan *p);

/* ---- tilt-corrected bright-field imaging, "parallax" (hipFFT) ---------------
 * A scan (nav_y, nav_x) and P bright-field pixels K, each with a scan image I_K and a shift sh[K] = (y, x) in scan
 * pixels.  s(i, n) is the signed frequency of the single-sideband section, Nxc = nav_x / 2 + 1, Q = iy Nxc + ix:
 *   G[K, Q]  = the real-to-complex transform of I_K over the scan axes (numpy.fft.rfft2), pixel-major
 *   ey[K, iy] = exp(2 pi i (s(iy, nav_y) sh[K, 0] / nav_y)),  ex[K, ix] = exp(2 pi i (s(ix, nav_x) sh[K, 1] / nav_x))
 *   S[Q]     = (1 / P) sum_K G[K, Q] (ey[K, iy] ex[K, ix])          float64 sums in a fixed order, cast to complex64
 *   X[K, Q]  = G[K, Q] conj(R[Q]),  X[K, 0] = 0                      float32, every product rounded on its own
 *   C_K      = the unnormalised complex-to-real inverse transform of X[K]: C_K[t] = sum_r I_K(r + t) ref(r)
 *   peak     = the first maximum of C_K[ty mod nav_y, tx mod nav_x] over -m <= ty, tx <= m in row-major (ty, tx) order,
 *              plus per axis sub(c-, c0, c+) = clip((c- - c+) / (2 d), -0.5, 0.5) if d = c- - 2 c0 + c+ < 0, else 0,
 *              in float64 from the stored float32 neighbours (indices mod the axis)
 * A real inverse transform takes only the Hermitian part of the columns ix = 0 and ix = nav_x / 2 of a half spectrum;
 * the plan projects S onto it ((S[iy] + conj(S[-iy])) / 2, k_plx_herm), so that every inverse transform reads it alike.
 * No atomics: a call repeats bit for bit.  csrc/ltmi_parallax.hip. */
/* The ramps of n pixels: sh DEVICE float64 (n, 2) -> ey DEVICE complex128 (n, nav_y), ex DEVICE complex128 (n, Nxc).
 * One launch of k_plx_ramps, one sincos per value.  n == 0 launches nothing.  A non-positive scan, n < 0:
 * LTMI_E_SHAPE; a null pointer: LTMI_E_INVALID. */
int ltmi_plx_ramps(int device, const double *sh, int64_t n, int nav_y, int nav_x, void *ey_out, void *ex_out,
                   void *stream);
/* S of n pixels: spec DEVICE complex64 (n, nav_y Nxc), ey / ex as above -> s_out DEVICE complex64 (nav_y, Nxc).  One
 * launch of k_plx_sum: the lanes run along Q, wave w of a workgroup sums the pixels [w c, (w + 1) c), c = ceil(n / 4),
 * ascending, and the four partial sums are added in the order of the waves.  n < 1, a non-positive scan: LTMI_E_SHAPE;
 * a null pointer: LTMI_E_INVALID. */
int ltmi_plx_sum(int device, const void *spec, int n, int nav_y, int nav_x, const void *ey, const void *ex, void *s_out,
                 void *stream);
/* X of n pixels: spec DEVICE complex64 (n, nav_y Nxc), ref DEVICE complex64 (nav_y Nxc) -> x_out DEVICE complex64
 * (n, nav_y Nxc); re = g.re r.re + g.im r.im, im = g.im r.re - g.re r.im.  One launch of k_plx_mul.  Errors as for
 * ltmi_plx_ramps. */
int ltmi_plx_mul(int device, const void *spec, int64_t n, int nav_y, int nav_x, const void *ref, void *x_out,
                 void *stream);
/* The peaks of n correlation maps: maps DEVICE float32 (n, nav_y, nav_x), contiguous -> shifts_out DEVICE float64
 * (n, 2).  One launch of k_plx_peaks, one wave per map.  A map without a finite value gives an unspecified shift
 * inside the window.  max_shift < 1 or > 16383, an axis shorter than 2 max_shift + 1, n < 0: LTMI_E_SHAPE; a null
 * pointer: LTMI_E_INVALID. */
int ltmi_plx_peaks(int device, const float *maps, int64_t n, int nav_y, int nav_x, int max_shift, double *shifts_out,
                   void *stream);
/* A plan owns the store of all spectra (8 n_idx nav_y Nxc bytes), the ramps (16 n_idx (nav_y + Nxc) bytes), S, one
 * batched real-to-complex and one batched complex-to-real hipFFT of (nav_y, nav_x), min(max_batch, n_idx) pixels per
 * execution, and per pixel of a batch a float32 scan image / correlation map and a complex64 half spectrum.  A store
 * above store_limit_bytes or above the free device memory: LTMI_E_NOMEM, the text gives the bytes needed.  The shape
 * errors of ltmi_plx_peaks, n_idx < 1, a batch of more than 2^31 - 1 values: LTMI_E_SHAPE; a null pointer,
 * max_batch < 1: LTMI_E_INVALID. */
typedef struct ltmi_plx_plan ltmi_plx_plan;   /* opaque */
int ltmi_plx_plan_create(int device, int nav_y, int nav_x, int n_idx, int max_batch, int max_shift,
                         int64_t store_limit_bytes, ltmi_plx_plan **out);
int ltmi_plx_plan_destroy(ltmi_plx_plan *p);
/* bf: device float32 (nav_y nav_x, n_idx), rows ld_bf elements apart (what ltmi_ssb_gather wrote for the whole scan)
 * -> the store.  Per batch ltmi_transpose2d and the R2C transform.  ld_bf < n_idx: LTMI_E_SHAPE; a null pointer:
 * LTMI_E_INVALID. */
int ltmi_plx_plan_load(ltmi_plx_plan *p, const float *bf, int64_t ld_bf, void *stream);
/* One iteration: shifts DEVICE float64 (n_idx, 2), read (the shifts that align the reference R = S(shifts), R[0, 0] =
 * 0) and then overwritten with the measured ones.  k_plx_ramps, k_plx_sum, k_plx_herm, and per batch k_plx_mul, the C2R
 * transform and k_plx_peaks.  Nothing is read back and the stream is not drained.  Before ltmi_plx_plan_load, a null
 * pointer: LTMI_E_INVALID. */
int ltmi_plx_plan_iterate(ltmi_plx_plan *p, double *shifts, void *stream);
/* S(shifts), its self-paired columns Hermitian -> half_out DEVICE complex64 (nav_y, Nxc): numpy.fft.irfft2 of it is
 * the aligned mean image.  Errors as for ltmi_plx_plan_iterate. */
int ltmi_plx_plan_sum(ltmi_plx_plan *p, const double *shifts, void *half_out, void *stream);
/* What the plan's last call launched: "k_transpose<4> + hipfft_r2c batch=N" (load), "k_plx_ramps + k_plx_sum +
 * k_plx_herm + k_plx_mul + hipfft_c2r + k_plx_peaks batch=N" (iterate), "k_plx_ramps + k_plx_sum + k_plx_herm" (sum);
 * "" before the first.  The string lives as long as the plan. */
const char *ltmi_plx_plan_last_kernel(const ltmi_plx_plan *p);

/* ---- lattice fit to the matched peaks -------------------------------------------------------------
 * Per frame, for n_peaks peaks with positions r_k = refineds[f, k] (y, x), weights w_k = weights[f, k]
 * (1 where `weights` is NULL), integer lattice indices (i_k, j_k) = indices[k] (precondition |i|, |j| <= 2^20),
 * a start lattice zero0, a0, b0 = start[0..1], start[2..3], start[4..5] as (y, x) and tolerance tau >= 0 in
 * pixels; all arithmetic is float64, the results are cast once at the end:
 *   1. p_k = zero0 + i_k a0 + j_k b0
 *   2. selector[f, k] = 1 where r_k is finite in both components, w_k is finite, w_k > 0 and
 *      |r_k - p_k|_2 <= tau -- and, where `peak_values` is not NULL, peak_values[f, k] is finite --, else 0
 *   3. a fit EXISTS iff the index pairs of the selected peaks are not collinear, decided on the integers:
 *      k0 = the first selected k, k1 = the first selected k with another index pair; some selected k has
 *      (i_k - i_k0)(j_k1 - j_k0) - (j_k - j_k0)(i_k1 - i_k0) != 0 in int64.  (At least 3 peaks are then
 *      selected, and the weighted normal matrix is positive definite: no floating-point threshold.)
 *   4. if it exists: (zero, a, b)[f] minimises sum_sel w_k |zero + i_k a + j_k b - r_k|^2 -- the weight
 *      multiplies the SQUARED residual -- and error[f] = sqrt(sum_sel w_k |res_k|^2 / sum_sel w_k)
 *   5. otherwise zero, a, b and error of the frame are NaN; selector is as in step 2.
 * refineds: device float32 (n_frames, n_peaks, 2); weights, peak_values: device float32 (n_frames, n_peaks) or
 * NULL; indices: DEVICE int32 (n_peaks, 2); start: HOST, 6 doubles; zero, a, b: device float32 (n_frames, 2);
 * selector: device bytes (n_frames, n_peaks), each 0 or 1; error: device float32 (n_frames).
 * One launch of k_lattice_fit on `stream` (csrc/ltmi_lattice.hip: one wave per frame, float64 sums combined by a
 * fixed-order shuffle tree, no atomics: the results of a call repeat bit for bit).  The indices never address
 * memory, so nothing is read back and the stream is not drained.  n_frames == 0 or n_peaks == 0 launches nothing
 * (with n_peaks == 0 the outputs are left as they are: LatticeRefineUDF refuses an empty index list).
 * A null pointer other than weights / peak_values: LTMI_E_INVALID; n_frames < 0, n_peaks < 0, tolerance negative
 * or NaN, a non-finite start value: LTMI_E_SHAPE. */
int ltmi_lattice_fit(int device, const float *refineds, const float *weights, const float *peak_values,
                     int64_t n_frames, int n_peaks, const int32_t *indices, const double *start,
                     double tolerance, float *zero, float *a, float *b, uint8_t *selector, float *error,
                     void *stream);
/* "k_lattice_fit" after the first launch issued by the calling thread, "" before; unchanged by a call that
 * launches nothing. */
const char *ltmi_lattice_last_kernel(void);

/* ---- multi-GPU: RCCL (over xGMI) behind the C ABI ---------------------------------------------
 * One process per GPU; the path shards over scan positions, the ranks exchange per-partition nav-grid
 * results only.  Replaces, for a reference-side binding, the transport of partition results through
 * the executor (pickled over TCP, src/libertem/executor/dask.py:581-646) and the serial merge on the
 * main process (src/libertem/udf/base.py:2340-2358, udf/sum.py:50-52):
 *   'disjoint' nav buffers (ApplyMasksUDF, SumSigUDF, CoM) -> ltmi_comm_all_gather of equal row blocks,
 *   sig buffers (SumUDF)                                    -> ltmi_comm_all_reduce_sum.
 * The 128-byte id comes from ltmi_comm_unique_id on ONE rank and reaches the others through the
 * launcher's own channel (environment, file, torch.distributed store).  librccl is opened lazily. */
typedef struct ltmi_comm ltmi_comm;   /* opaque */
/* which librccl the ltmi_comm_* functions are bound to: file path (NUL-terminated, at most path_cap bytes),
 * ncclGetVersion() code, and whether that copy was already mapped by the process (a process that runs
 * torch.distributed binds to torch's bundled RCCL -- never a second one; otherwise LTMI_RCCL_LIB, the
 * loader path, /opt/rocm/lib).  Any of the output pointers may be NULL. */
int ltmi_comm_library_info(char *path_out, int64_t path_cap, int *version, int *was_loaded);
int ltmi_comm_unique_id(void *id_out /* 128 bytes */);
int ltmi_comm_create(int device, int rank, int world, const void *id /* 128 bytes */,
                     ltmi_comm **out);
int ltmi_comm_destroy(ltmi_comm *c);
/* recv[r * bytes_per_rank ...] = send of rank r, device pointers, on `stream` */
int ltmi_comm_all_gather(ltmi_comm *c, const void *send, void *recv, int64_t bytes_per_rank,
                         void *stream);
/* buf[i] = sum over ranks, in place; dtype: enum ltmi_dtype without the 16-bit integers */
int ltmi_comm_all_reduce_sum(ltmi_comm *c, void *buf, int dtype, int64_t n, void *stream);

/* ---- tuning / introspection (bench + tests) ------------------------------------------- */
/* the kernel-variant codes of ltmi_masks_set_tuning (passed as `waves` with mt = 0); the numbers are part of the ABI */
enum ltmi_variant {
    LTMI_VARIANT_NONE = 0,
    LTMI_VARIANT_DENSE_DEFAULT = 30,
    LTMI_VARIANT_DENSE_NO_DMA = 31,
    LTMI_VARIANT_DENSE_NO_MFMA = 32,
    LTMI_VARIANT_DENSE_PADDED_GROUPS = 33,
    LTMI_VARIANT_DENSE_ONE_TILE = 34,
    LTMI_VARIANT_DENSE_TWO_TILES = 35,
    LTMI_VARIANT_DENSE_SPLIT_BF16 = 36,
    LTMI_VARIANT_DENSE_F32_INSTR = 37,
    LTMI_VARIANT_DENSE_UNFOLDED = 38,
    LTMI_VARIANT_SPARSE_DEFAULT = 40,
    LTMI_VARIANT_SPARSE_SELL = 41,
    LTMI_VARIANT_SPARSE_NO_SCATTER = 42
};
/* force a kernel variant of a mask handle (bench / tests only; (0, 0, 0) = automatic).  Two forms:
 *   mt in {1,2}, waves in {4,8}: the direct-load kernel k_dense_mfma with that tile shape (8 waves: uint16 tiles
 *     only); mt = 1 on float64 results: the direct-load f64 kernel;
 *   mt = 0, waves = an ltmi_variant code (the handle then dispatches with mt = waves = 0):
 *     30  dense stacks as dispatched -- but not the same as 0: every code except 36 disables the bf16 split
 *         route, also where LTMI_SPLIT=1 asks for it
 *     31  k_dense_lds / k_dense_fold without the frame DMA: timing only, results are GARBAGE (uint16 tiles against
 *         one column group only, like 32 and 34)
 *     32  k_dense_lds / k_dense_fold without the matrix instruction: timing only, results are GARBAGE
 *     33  padded column groups instead of VALU columns; no column blocks for wide stacks; no row-list launch
 *     34  one 16-frame tile per wave (uint16 tiles, one column group, no row list)
 *     35  two 16-frame tiles per wave: 35 is the default shape, so it does what 30 does
 *     36  float32 tiles of stacks with 2 - 4 column groups on the bf16 x 3 split kernel (ltmi_split.hip)
 *     37  the float32 matrix instruction also for 1- / 2-byte integer tiles (by default those take exact
 *         float16-piece products, kernel names ending in ",f16"; LTMI_DENSE_F16=0 in the environment: never)
 *     38  the unfolded kernels for a stack that has a row-mirror image (ltmi_fold.hip)
 *     40  sparse stacks as dispatched
 *     41  the gather kernel k_sell_apply even if a banded, scatter, blocked or label image exists
 *     42  not the scatter kernel (nor the banded or label image): the blocked image or k_sell_apply
 *   ksplit: parts of the pixel split, 0 = auto.  Returns LTMI_E_INVALID for anything else. */
int ltmi_masks_set_tuning(ltmi_masks *m, int mt, int waves, int ksplit);
/* name of the kernel variant the last ltmi_apply_masks on this handle launched */
const char *ltmi_masks_last_kernel(const ltmi_masks *m);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* LTMI_H */
