// Shared host-side helpers for libltmi (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/ltmi.h"
#include "ltmi_switches.h"
#include "ltmi_tuning.h"

namespace ltmi {

void set_error(const char *fmt, ...);

#define LTMI_HIP(expr)                                                                   \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ltmi::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                            __FILE__, __LINE__);                                         \
            return (int)_e;                                                              \
        }                                                                                \
    } while (0)

#define LTMI_FAIL(code, ...)                                                             \
    do {                                                                                 \
        ltmi::set_error(__VA_ARGS__);                                                    \
        return (code);                                                                   \
    } while (0)

// gfx950 serves 16-byte vector loads and LDS-DMA loads from any element-aligned address at the speed
// of aligned ones (profiles/r02_unaligned.txt), so tiles whose rows are not 16-B aligned (odd pixel
// counts, e.g. 515 x 515 detectors) take the same vectorised kernels.  LTMI_ALIGNED_DMA_ONLY=1 in the
// environment restores the conservative dispatch (vector paths for 16-B aligned rows only).
static inline bool vector_loads_ok(const void *tile, int64_t ld_elems, size_t elem) {
    const bool aligned_only = switch_set<LTMI_ALIGNED_DMA_ONLY>();
    if ((((uintptr_t)tile) % 16 == 0) && ((ld_elems * (int64_t)elem) % 16 == 0)) return true;
    return !aligned_only && ((uintptr_t)tile) % elem == 0;
}

// Shifted masks: a shift of sig or more in either direction leaves no overlap, whatever its size.  Kernels and image
// builders clamp (dy, dx) to [-sig, sig] on entry, so that `sig + d`, `y1 - y0` and `y - d` stay inside int for every
// int32 shift.
__host__ __device__ static inline int clamp_shift(int d, int sig) { return d < -sig ? -sig : (d > sig ? sig : d); }

// K split of the LDS-DMA kernels (one workgroup per CU at a time, 256 CUs): `wgs` workgroups at
// ksplit = 1, each walking `n_slots` mask slots.  A split by ks makes ks x wgs workgroups of n_slots / ks
// slots; the launch takes ceil(ks wgs / 256) rounds of (n_slots / ks + start-up) plus, for ks > 1, the
// reduction of the partials.  Picks the ks with the shortest modelled time: fills the chip when there
// are fewer workgroups than CUs AND trims the last, partly filled round of awkward frame counts (313
// workgroups: 2 rounds unsplit = 2.0, ks = 4: 5 rounds of a quarter = 1.25 of one workgroup's time).
static inline int choose_ksplit(int64_t wgs, int n_slots) {
    const double START = 1.5, REDUCE = 6.0;             // in slot times (~3 us / ~14 us on C2)
    int max_ks = n_slots / 8 > 1 ? (n_slots / 8 < 64 ? n_slots / 8 : 64) : 1;
    if (wgs < 256) {
        // fewer workgroups than CUs: up to ~4 rounds' worth of workgroups
        max_ks = (int)std::min<int64_t>(max_ks, (1024 + wgs - 1) / wgs);
    } else {
        // whole rounds, or a last round that is at least 3/4 full: nothing to trim
        const int64_t tail = wgs % 256;
        if (tail == 0 || tail >= 192 || wgs > 4 * 256) return 1;
        max_ks = std::min(max_ks, 8);
    }
    double best = 1e300;
    int best_ks = 1;
    for (int ks = 1; ks <= max_ks; ++ks) {
        if (wgs * ks > 16384 && ks > 1) break;
        const double rounds = (double)((wgs * ks + 255) / 256);
        // (a launch of few rounds runs at the pace of its slowest CUs: ~8 % on a single round)
        const double t = rounds * ((double)n_slots / ks + START) * (1.0 + 0.08 / rounds) +
                         (ks > 1 ? REDUCE : 0.0);
        if (t < best * 0.98) {                          // a larger split has to be worth >= 2 %
            best = t;
            best_ks = ks;
        }
    }
    return best_ks;
}

// every part of a split of n slots into ksplit parts owns at least one slot: the smallest number of parts of the
// same size per part
static inline int clamp_ksplit(int ksplit, int n) {
    const int per = (n + ksplit - 1) / ksplit;
    return (n + per - 1) / per;
}

static inline int dtype_size(int dt) {
    switch (dt) {
        case LTMI_BOOL: case LTMI_U8: case LTMI_I8: return 1;
        case LTMI_U16: case LTMI_I16: return 2;
        case LTMI_U32: case LTMI_I32: case LTMI_F32: return 4;
        case LTMI_U64: case LTMI_I64: case LTMI_F64: case LTMI_C64: return 8;
        case LTMI_C128: return 16;
    }
    return 0;
}

static inline const char *dtype_name(int dt) {
    static const char *n[] = {"bool", "uint8", "int8", "uint16", "int16", "uint32", "int32",
                              "uint64", "int64", "float32", "float64", "complex64", "complex128"};
    return (dt >= 0 && dt <= LTMI_C128) ? n[dt] : "?";
}

// One hipMalloc allocation and its owner: freed by the destructor, move-only; reads as the raw pointer it replaces
// (kernel arguments, `if (buf)`, `buf + n`).  Counts are elements of T, bytes for DevBuf<void>.  The device of the
// allocation must be current when the buffer goes (ltmi_masks_destroy and plan_destroy of ltmi_fftshare.h see to it).
template <typename T>
class DevBuf {
    using E = typename std::conditional<std::is_void<T>::value, char, T>::type;
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DevBuf() { reset(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(E); }
    void reset() {
        if (p_) (void)hipFree((void *)p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // a fresh block of n elements (what the buffer held is freed first), ... zeroed, ... filled from the host
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc((void **)&p_, n * sizeof(E));
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    hipError_t alloc_zero(size_t n) {
        const hipError_t e = alloc(n);
        return e == hipSuccess ? hipMemset((void *)p_, 0, n * sizeof(E)) : e;
    }
    hipError_t upload(const E *host, size_t n) {
        const hipError_t e = alloc(n);
        return e == hipSuccess ? hipMemcpy((void *)p_, host, n * sizeof(E), hipMemcpyHostToDevice) : e;
    }
    // grow-only: room for n elements; a block that is too small is freed -- after the work on `stream`, which may
    // still read it -- BEFORE the larger one is made, so a growing run never holds both.  The contents are lost.
    int ensure(size_t n, hipStream_t stream) {
        if (n <= cap_) return LTMI_OK;
        if (p_) {
            LTMI_HIP(hipStreamSynchronize(stream));
            reset();
        }
        LTMI_HIP(alloc(n));
        return LTMI_OK;
    }
};

struct cfloat { float re, im; };
struct cdouble { double re, im; };

// one mask product: out[i, k] (+)= sum_p tile[i, p] * masks[k, p] for n_frames frames -- with `rows` (a device list,
// ltmi_apply_masks_rows) result row i is frame rows[i] of the tile
struct MaskCall {
    const void *tile;
    int tile_dtype;
    int64_t n_frames, ld_tile;
    void *out;
    int64_t ld_out;
    int accumulate;
    hipStream_t stream;
    const int32_t *rows = nullptr;
};

}  // namespace ltmi

struct ltmi_masks;
namespace ltmi {
int dense64_create(ltmi_masks *m);
// (img64: the handle's image or that of the shifted stack)
int dense64_apply(ltmi_masks *m, const double *img64, const MaskCall &call, bool *handled);
bool dense64_rows_ok(const ltmi_masks *m, const void *tile, int tile_dtype, int64_t ld);
size_t dense64_image_bytes(const ltmi_masks *m);
int dense64_build_shifted(ltmi_masks *m, int sig_h, int sig_w, int dy, int dx, double *img,
                          hipStream_t stream);
// blocked-ELL sparse image on the matrix cores (ltmi_bell.hip)
double bell_mac_ratio(const int64_t *indptr, const int64_t *indices, int nc, int64_t n_px,
                      int64_t n_masks);
void *bell_build(const int64_t *indptr, const int64_t *indices, const float *vals, int nc,
                 int64_t n_px, int64_t n_masks, int *err);
void bell_destroy(void *image);
// sparse stacks on the vector ALUs, one float32 FMA per stored entry (ltmi_scatter.hip)
double scat_fill(const int64_t *indptr, const int64_t *indices, int nc, int64_t n_px, int64_t n_masks);
void *scat_build(const int64_t *indptr, const int64_t *indices, const float *vals, int nc, int64_t n_px,
                 int64_t n_masks, int *err);
void scat_destroy(void *set);
int scat_apply(ltmi_masks *m, void *set, int cplx, const MaskCall &call, bool *handled);
// partition stacks (no pixel stored by two masks: binning, polar maps, hard rings) as a label and a weight per pixel
// (ltmi_labels.hip): float32 results, 1- / 2-byte integer and float32 frames
bool labels_qualifies(const int64_t *indptr, int64_t n_px, int64_t n_masks);
void *labels_build(const int64_t *indptr, const int64_t *indices, const float *vals, int64_t n_px, int64_t n_masks,
                   int *err);
void labels_destroy(void *image);
bool labels_takes(int tile_dtype);
int labels_apply(ltmi_masks *m, void *image, const MaskCall &call);
// float32 frames x multi-group float32 stacks on the bf16 matrix cores, float32-accurate (ltmi_split.hip)
bool split_selected(bool tuned);
bool split_wanted(int n_cols, int64_t n_px);
int split_create(int device, const float *gmasks, int64_t n_masks, int cpm, int64_t n_px, int n_cols,
                 void **image);
void split_destroy(void *image);
size_t split_image_bytes(const void *image);
int split_apply(ltmi_masks *m, void *image, const MaskCall &call);
// CrystallinityUDF for 256 x 256 frames in one kernel (ltmi_cryst.hip)
int cryst_fused_max_cols();
bool cryst_fused_shape(int h, int w);
bool cryst_fused_takes(int h, int w, int n_cols);
int64_t cryst_fused_workspace_floats(int h, int w);
bool cryst_fused_needs_gbuf(int h, int w, int n_cols);
int cryst_fused(const void *tile, int tile_dtype, int64_t n_frames, int64_t ld, int sig_h, int sig_w,
                const float *real_mask, const float *half_mask, int n_cols, float *mask_t, void *gbuf,
                int64_t gbuf_frames, float *out, int accumulate, int n_cu, hipStream_t stream, bool *handled);
// dense stacks folded about a mirror of the detector rows (ltmi_fold.hip)
int fold_create(ltmi_masks *m, int sig_h, int sig_w);
void fold_destroy(ltmi_masks *m);
bool fold_takes(const ltmi_masks *m, const float *tile, int64_t ld);
int launch_fold(ltmi_masks *m, const MaskCall &call);
// banded sparse stacks (column blocks with a common support each: radial Fourier with several bins) on k_dense_fold
struct KeptCsr;                                                             // host copy of a CSR stack, rows sorted
KeptCsr *band_keep_csr(const int64_t *indptr, const int64_t *indices, const float *vals, int nc, int64_t n_px,
                       int64_t n_masks);                                    // nullptr: not a candidate
void band_free_csr(KeptCsr *k);
void *band_build(const KeptCsr *k, int sig_h, int sig_w, double other_macs);    // nullptr: the other kernels serve
void band_destroy(void *band);
bool band_takes(void *band, const ltmi_masks *m, const void *tile, int tile_dtype, int64_t ld);   // float32, 1- / 2-byte integers
int band_apply(ltmi_masks *m, void *band, const MaskCall &call, int n_cols);
bool fold_takes16(ltmi_masks *m, const void *tile, int64_t ld, int px_bytes);   // 1- / 2-byte integer frames (image built on first use)
int launch_fold16(ltmi_masks *m, const MaskCall &call, int px_bytes, bool is_signed);
// the K-split workspace of a dense handle (ltmi_dense.hip)
int dense_ensure_partials(ltmi_masks *m, size_t need, hipStream_t stream);
float *dense_partial_sums(const ltmi_masks *m);
int dense_reduce_partials(ltmi_masks *m, int ksplit, int64_t n_frames, float *out, int64_t ld_out, int accumulate,
                          hipStream_t stream, int n_cols = -1);   // n_cols <= 0: the handle's
// ... on RAW frames with the detector corrections applied inside the row stage (256 x 256 frames)
int64_t cryst_corr_workspace_bytes(int h, int w, int64_t n_frames, int n_excl);
bool cryst_corr_takes(int h, int w, int n_cols, int tile_dtype, int n_excl);
int cryst_fused_corrected(const void *tile, int tile_dtype, int64_t n_frames, int64_t ld, int sig_h, int sig_w,
                          const double *dark, const double *gain, const int32_t *excl, const int32_t *env,
                          const int32_t *cnt, int n_excl, int max_env, const float *real_mask, const float *half_mask,
                          int n_cols, float *mask_t, void *gbuf, int64_t gbuf_frames, void *ws, float *out,
                          int accumulate, int n_cu, hipStream_t stream, bool *handled);
// non-finite pixels on sparse stacks (ltmi_guard.hip; the gather-kernel redo: ltmi_sparse.hip)
int csr_redo(ltmi_masks *m, const MaskCall &call, const int32_t *sel, const int *n_sel);   // call.n_frames: at most
bool csr_is_f64(const ltmi_masks *m);
bool guard_wanted(const ltmi_masks *m, int tile_dtype);
int guard_apply(ltmi_masks *m, const MaskCall &call);
void guard_destroy(ltmi_masks *m);
// the guard's pieces, for the shifted routes of ltmi_dense.hip: where the product goes, which result rows are
// non-finite (lists on the device), the product to its place
bool guard_wanted_shifted(const ltmi_masks *m, int tile_dtype);
int guard_target(ltmi_masks *m, int64_t n_frames, void *out, int64_t ld_out, int accumulate, hipStream_t stream,
                 void **target, int64_t *ld_target);
int guard_list_rows(ltmi_masks *m, const void *target, int64_t ld_target, int64_t n_frames, hipStream_t stream,
                    int **ctl, int32_t **list);
int guard_deliver(ltmi_masks *m, void *out, int64_t ld_out, int64_t n_frames, int accumulate, hipStream_t stream);
// ltmi_apply_masks without the guard (ltmi_dense.hip)
int apply_masks_unguarded(ltmi_masks *m, const MaskCall &call);
// the strongest local maxima of correlation maps (ltmi_peakfind.hip)
struct PeakFind {
    int n_peaks, d, border, q;             // d and q clamped to the frame's longer edge: the windows are clipped anyway
    float threshold_abs, threshold_rel;
};
int peakfind_params(const char *who, int h, int w, int num_peaks, int min_distance, int border, float threshold_abs,
                    float threshold_rel, int refine_radius, PeakFind *out);
const char *peakfind_kernels();            // "k_pf_cells + k_pf_verify + k_pf_select + k_corr_found"
// n_frames maps of (h, w) float32, ld_map elements apart -> the five results; `scratch` grows to two keys per cell
int peakfind_search(const float *maps, int64_t n_frames, int h, int w, int64_t ld_map, const PeakFind &pf,
                    DevBuf<uint64_t> &scratch, int32_t *n_found, int32_t *centers, float *refineds,
                    float *peak_values, float *peak_elevations, hipStream_t stream);
// ... its last step: the window statistics of the found peaks, on the code of k_corr_peaks (ltmi_corr.hip)
int corr_found_stats(const float *maps, int64_t n_frames, int h, int w, int64_t ld_map, const PeakFind &pf,
                     const int32_t *n_found, int32_t *centers, float *refineds, float *peak_values,
                     float *peak_elevations, hipStream_t stream);
// sparse frames against a dense stack (ltmi_csrframes.hip): the pixel-major image of the handle
int bell_apply(ltmi_masks *m, void *image, int cplx, const MaskCall &call, bool *handled);
}  // namespace ltmi

// The opaque handle behind `ltmi_masks*` (shared by ltmi_dense.hip and ltmi_sparse.hip).
struct ltmi_masks {
    int device = 0;
    int kind = 0;            // 0 dense/MFMA-f32, 1 dense/generic, 2 csr (SELL image; ltmi_masks_kind: 3 banded, 4 labels)
    int result_dtype = 0;
    int64_t n_masks = 0, n_px = 0;
    // kind 0
    int n_cols = 0;          // real f32 columns (2 per mask for complex64)
    int n_groups = 0;        // 16-column groups, padded to a multiple of ng
    int ng = 1;
    int n_chunks = 0;
    ltmi::DevBuf<float> img;
    ltmi::DevBuf<float> img2;   // slot-major image for k_dense_lds with ng > 1 (KB = 128)
    int n_slots2 = 0;
    ltmi::DevBuf<float> img3;   // ng3 groups + ne3 VALU columns (16 ng3 + 1..4 columns), slots of 128 px
    int n_slots3 = 0, ne3 = 0, ng3 = 0;   // ng3 full groups + ne3 VALU columns
    void *split = nullptr;   // bf16 x 3 image for float32 frames (ltmi_split.hip), stacks of >= 2 groups
    // float16 image of the standard (ng = 1) layout for unsigned 1- / 2-byte pixels (k_dense_lds X16):
    // w1 / w2 of the scaled weights in the two 16-byte units of a lane's 8 pixels; 1 / scale per column
    ltmi::DevBuf<float> img_h;
    ltmi::DevBuf<float> img2_h;  // ... of image 2 (ng > 1)
    ltmi::DevBuf<float> img3_h;  // ... of image 3 without VALU columns (3 groups)
    ltmi::DevBuf<float> inv_scale;
    // small weights that two float16 pieces do not carry to 2^-19 relative: left out of the float16
    // images; the epilogue of k_dense_lds X16 adds their float32 products
    ltmi::DevBuf<int32_t> tail_px, tail_col;
    ltmi::DevBuf<float> tail_val;
    int tail_n = 0;
    // float64 results on the f64 matrix cores (ltmi_dense64.hip)
    ltmi::DevBuf<double> img64;
    int n_groups64 = 0, n_chunks64 = 0;
    int cpm64 = 1;              // real columns per mask in the f64 image (2: complex128 masks)
    ltmi::DevBuf<double> ws64;    // partial sums of a K split
    ltmi::DevBuf<double> res64;   // f64 scratch result of the exact-integer path
    int mask_bits = 64;      // integer stacks: bits needed for max |mask value|
    void *shift_cache = nullptr;   // ltmi_dense.hip: images of the stack shifted by (dy, dx)
    void *fold = nullptr;          // ltmi_fold.hip: image folded about a mirror of the detector rows (ltmi_masks_set_sig_shape)
    ltmi::DevBuf<void> partials;  // arrival counters, then the partial sums of a K split (ltmi_dense.hip)
    ltmi::Tuning tune;       // ltmi_masks_set_tuning (ltmi_tuning.h)
    // kind 0 and 1
    ltmi::DevBuf<void> gmasks;    // (n_masks, n_px) of the accumulate type
    // ltmi_apply_masks_csr: the stack again pixel-major, [n_px][m_pad_px] of float / double, built on first use
    ltmi::DevBuf<void> img_px;
    int m_pad_px = 0;
    // kind 2 (ltmi_sparse.hip)
    void *csr = nullptr;
    // kind 0 with more than 64 real columns: the stack again as column blocks of <= 64 columns,
    // each with the tile width that fits it (ltmi_apply_masks walks them; tuning code 33 does not)
    std::vector<ltmi_masks *> blocks;
    std::vector<int64_t> block_first;        // first mask of every block
    // non-finite pixels (ltmi_guard.hip)
    ltmi_masks *sparse_origin = nullptr;   // a DENSE handle that stands for a sparse stack: the stack's gather image (owned)
    void *dense_origin = nullptr;          // a CSR handle that stands for a dense stack: its by-pixel tables
    void *guard = nullptr;                 // flagged-frame list + scratch of the guarded product
    bool last_exact = false;               // the last product ran on a kernel that multiplies stored entries only
    char last_kernel[128] = {0};
};

namespace ltmi {
// what a later stage did to the product of the kernel that `last_kernel` names: " +nf", " exact-int", " shifted, ..."
__attribute__((format(printf, 2, 3))) static inline void append_kernel_note(ltmi_masks *m, const char *fmt, ...) {
    const size_t len = strlen(m->last_kernel);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(m->last_kernel + len, sizeof(m->last_kernel) - len, fmt, ap);
    va_end(ap);
}
}  // namespace ltmi
