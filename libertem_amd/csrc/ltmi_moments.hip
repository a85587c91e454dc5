// Per-pixel moments over frames for StdDevUDF (gfx950).
//
//   ltmi_moments_frames : (sum, varsum)[p] <- merge((sum, varsum)[p] of n_prev frames,
//                                               moments of tile[:, p])
//                         (src/libertem/udf/stddev.py:103-168 process_tile / :11-100 merge)
//
// Two launches, no atomics (bitwise repeatable):
//   k_moments_slab : grid = (pixel blocks, frame slabs); a thread owns VEC consecutive real
//                    columns (16-byte loads) and walks its slab of frames.  It accumulates
//                    s = sum(x - K) and q = sum((x - K)^2) in float64, where the shift K is the
//                    column's value in the slab's first frame, and stores the slab's sum
//                    (s + n K) and M2 = q - s^2 / n (complex pixels: both parts, M2 summed).
//                    For integer frames x - K, s and q are exact (below 2^53).
//   k_moments_merge : one thread per pixel merges the slabs in order with the reference's
//                    pairwise update and folds the result into the running buffers:
//                      varsum += varsum_b + n_b |delta| |delta'|,
//                      delta = mean_b - mean_a, delta' = mean_b - mean_new.
#include "ltmi_tiles.h"

namespace ltmi {
namespace {

constexpr int MOM_BLOCK = 256;

// slabs: the frames of a tile in `fsplit` slabs of `per` frames (the last one may be shorter, none
// is empty)
struct Slabs {
    int fsplit;
    int64_t per;
};

Slabs moment_slabs(int64_t n_frames, int64_t n_px) {
    const int64_t want = frames_split(n_frames, n_px);
    Slabs s;
    s.per = (n_frames + want - 1) / want;
    s.fsplit = (int)((n_frames + s.per - 1) / s.per);       // no empty slab
    return s;
}

template <typename T> struct Diff {
    // (x - K) as float64; exact for every integer type here and for float32 pairs
    static __device__ __forceinline__ double of(T x, T k) { return (double)x - (double)k; }
};
template <> struct Diff<uint8_t> {
    static __device__ __forceinline__ double of(uint8_t x, uint8_t k) { return (double)((int)x - (int)k); }
};
template <> struct Diff<int8_t> {
    static __device__ __forceinline__ double of(int8_t x, int8_t k) { return (double)((int)x - (int)k); }
};
template <> struct Diff<uint16_t> {
    static __device__ __forceinline__ double of(uint16_t x, uint16_t k) { return (double)((int)x - (int)k); }
};
template <> struct Diff<int16_t> {
    static __device__ __forceinline__ double of(int16_t x, int16_t k) { return (double)((int)x - (int)k); }
};

// ws layout: for slab k and component c (0 .. L-1: the sum's real / imaginary part, L: M2),
// n_px doubles at ws + (k * (L + 1) + c) * n_px.  L = 1 for real, 2 for complex pixels.
template <typename T, int VEC, int L>
__global__ void __launch_bounds__(MOM_BLOCK)
k_moments_slab(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_cols,
               int64_t per, double *__restrict__ ws) {
    static_assert(VEC % L == 0, "a thread owns whole pixels");
    typedef tile_vec_t<T, VEC> vec_t;
    const int64_t c0 = ((int64_t)blockIdx.x * MOM_BLOCK + threadIdx.x) * VEC;
    if (c0 >= n_cols) return;
    const int64_t f0 = (int64_t)blockIdx.y * per;
    const int64_t f1 = min(n_frames, f0 + per);
    const int64_t n_px = n_cols / L;
    double s[VEC], q[VEC];
    T k[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s[e] = 0.0; q[e] = 0.0; }
    const bool full = (c0 + VEC <= n_cols);
    if (full) {
        const vec_t kv = *(const vec_t *)(tile + f0 * ld + c0);
#pragma unroll
        for (int e = 0; e < VEC; ++e) k[e] = kv[e];
        int64_t f = f0 + 1;
        for (; f + 3 < f1; f += 4) {
            vec_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = __builtin_nontemporal_load((const vec_t *)(tile + (f + u) * ld + c0));
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const double d = Diff<T>::of(v[u][e], k[e]);
                    s[e] += d;
                    q[e] = fma(d, d, q[e]);
                }
        }
        for (; f < f1; ++f) {
            const vec_t v = __builtin_nontemporal_load((const vec_t *)(tile + f * ld + c0));
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const double d = Diff<T>::of(v[e], k[e]);
                s[e] += d;
                q[e] = fma(d, d, q[e]);
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) k[e] = (c0 + e < n_cols) ? tile[f0 * ld + c0 + e] : (T)0;
        for (int64_t f = f0 + 1; f < f1; ++f)
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (c0 + e < n_cols) {
                    const double d = Diff<T>::of(tile[f * ld + c0 + e], k[e]);
                    s[e] += d;
                    q[e] = fma(d, d, q[e]);
                }
    }
    const double n = (double)(f1 - f0);
    double *slab = ws + (int64_t)blockIdx.y * (L + 1) * n_px;
#pragma unroll
    for (int i = 0; i < VEC / L; ++i) {
        const int64_t p = c0 / L + i;
        if (p >= n_px) break;
        double m2 = 0.0;
#pragma unroll
        for (int c = 0; c < L; ++c) {
            const int e = i * L + c;
            slab[c * n_px + p] = fma(n, (double)k[e], s[e]);     // sum = s + n K
            m2 += q[e] - s[e] * s[e] / n;
        }
        slab[L * n_px + p] = m2 < 0.0 ? 0.0 : m2;       // (rounding below 0 clamped; NaN passes)
    }
}

template <int L> __device__ __forceinline__ double cabs_(const double *v) {
    return L == 1 ? fabs(v[0]) : sqrt(v[0] * v[0] + v[1] * v[1]);
}

// (n_a, sum_a, m2_a) <- the union with (n_b, sum_b, m2_b); n_a > 0, n_b > 0 (stddev.py:11-63)
template <int L>
__device__ __forceinline__ void merge_into(double n_a, double *sum_a, double &m2_a, double n_b,
                                           const double *sum_b, double m2_b) {
    const double n = n_a + n_b;
    double delta[L], partial[L];
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const double mean_a = sum_a[c] / n_a, mean_b = sum_b[c] / n_b;
        delta[c] = mean_b - mean_a;
        const double mean = mean_a + (n_b * delta[c]) / n;
        partial[c] = mean_b - mean;
        sum_a[c] += sum_b[c];
    }
    m2_a = m2_a + m2_b + n_b * cabs_<L>(delta) * cabs_<L>(partial);
}

// S: the real type of the sum buffer (its L parts per pixel), V: the varsum type.  Pixel p of the
// tile is element (p / cols) * ld_out + p % cols of the output buffers.
template <int L, typename S, typename V>
__global__ void __launch_bounds__(MOM_BLOCK)
k_moments_merge(const double *__restrict__ ws, int fsplit, int64_t n_frames, int64_t per,
                int64_t n_px, int64_t n_prev, S *__restrict__ sum, V *__restrict__ varsum,
                int64_t cols, int64_t ld_out) {
    const int64_t p = (int64_t)blockIdx.x * MOM_BLOCK + threadIdx.x;
    if (p >= n_px) return;
    double acc[L], m2;
    double n_acc = (double)min(per, n_frames);
#pragma unroll
    for (int c = 0; c < L; ++c) acc[c] = ws[c * n_px + p];
    m2 = ws[L * n_px + p];
    for (int k = 1; k < fsplit; ++k) {
        const double *slab = ws + (int64_t)k * (L + 1) * n_px;
        const double n_b = (double)(min(n_frames, (k + 1) * per) - k * per);
        double sb[L];
#pragma unroll
        for (int c = 0; c < L; ++c) sb[c] = slab[c * n_px + p];
        merge_into<L>(n_acc, acc, m2, n_b, sb, slab[L * n_px + p]);
        n_acc += n_b;
    }
    const int64_t r = p / cols;
    const int64_t o = r * ld_out + (p - r * cols);
    if (n_prev > 0) {
        // the running moments are "a", the tile is "b" (stddev.py:135-168)
        double run[L];
#pragma unroll
        for (int c = 0; c < L; ++c) run[c] = (double)sum[o * L + c];
        double m2_run = (double)varsum[o];
        merge_into<L>((double)n_prev, run, m2_run, n_acc, acc, m2);
#pragma unroll
        for (int c = 0; c < L; ++c) acc[c] = run[c];
        m2 = m2_run;
    }
#pragma unroll
    for (int c = 0; c < L; ++c) sum[o * L + c] = (S)acc[c];
    varsum[o] = (V)m2;
}

template <typename T, int L>
int run_moments(const void *tile, int64_t n_frames, int64_t n_px, int64_t ld_tile, int64_t n_prev,
                void *sum, int sum_dtype, void *varsum, int varsum_dtype, int64_t cols, int64_t ld_out,
                void *ws, hipStream_t stream) {
    constexpr int VECA = (16 / (int)sizeof(T)) < L ? L : 16 / (int)sizeof(T);
    const Slabs sl = moment_slabs(n_frames, n_px);
    const int64_t n_cols = n_px * L;
    const int64_t ld = ld_tile * L;
    const bool vec_ok = vector_loads_ok(tile, ld, sizeof(T));
    const int vec = vec_ok ? VECA : L;
    const dim3 grid((unsigned)((n_cols + (int64_t)MOM_BLOCK * vec - 1) / ((int64_t)MOM_BLOCK * vec)),
                    (unsigned)sl.fsplit);
    if (vec_ok)
        hipLaunchKernelGGL((k_moments_slab<T, VECA, L>), grid, dim3(MOM_BLOCK), 0, stream,
                           (const T *)tile, ld, n_frames, n_cols, sl.per, (double *)ws);
    else
        hipLaunchKernelGGL((k_moments_slab<T, L, L>), grid, dim3(MOM_BLOCK), 0, stream,
                           (const T *)tile, ld, n_frames, n_cols, sl.per, (double *)ws);
    LTMI_HIP(hipGetLastError());
    const dim3 mgrid((unsigned)((n_px + MOM_BLOCK - 1) / MOM_BLOCK));
#define LTMI_MERGE(S, V)                                                                             \
    hipLaunchKernelGGL((k_moments_merge<L, S, V>), mgrid, dim3(MOM_BLOCK), 0, stream,                \
                       (const double *)ws, sl.fsplit, n_frames, sl.per, n_px, n_prev, (S *)sum,        \
                       (V *)varsum, cols, ld_out)
    const bool s64 = sum_dtype == LTMI_F64 || sum_dtype == LTMI_C128;
    const bool v64 = varsum_dtype == LTMI_F64;
    if (s64 && v64) LTMI_MERGE(double, double);
    else if (s64) LTMI_MERGE(double, float);
    else if (v64) LTMI_MERGE(float, double);
    else LTMI_MERGE(float, float);
#undef LTMI_MERGE
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

}  // namespace
}  // namespace ltmi

using namespace ltmi;

extern "C" int64_t ltmi_moments_workspace(int64_t n_frames, int64_t n_px, int tile_dtype) {
    if (n_frames <= 0 || n_px <= 0) return 0;
    const int L = dtype_in(tile_dtype, DT_CPLX) ? 2 : 1;
    const Slabs sl = moment_slabs(n_frames, n_px);
    return (int64_t)sl.fsplit * (L + 1) * n_px * (int64_t)sizeof(double);
}

extern "C" int ltmi_moments_frames(int device, const void *tile, int tile_dtype, int64_t n_frames,
                                   int64_t n_px, int64_t ld_tile, int64_t n_prev, void *sum,
                                   int sum_dtype, void *varsum, int varsum_dtype, int64_t cols,
                                   int64_t ld_out, void *workspace, void *stream_) {
    if (n_frames < 0 || n_px < 0 || ld_tile < n_px || n_prev < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_moments_frames: bad shape");
    if (int rc = check_sig_slice("ltmi_moments_frames", n_px, cols, ld_out)) return rc;
    if (n_frames == 0 || n_px == 0) return LTMI_OK;
    if (!tile || !sum || !varsum || !workspace)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_moments_frames: null pointer");
    const bool cplx_tile = dtype_in(tile_dtype, DT_CPLX);
    const bool cplx_sum = dtype_in(sum_dtype, DT_CPLX);
    const bool sum_ok = sum_dtype == LTMI_F32 || sum_dtype == LTMI_F64 || cplx_sum;
    const bool var_ok = varsum_dtype == LTMI_F32 || varsum_dtype == LTMI_F64;
    if (!sum_ok || !var_ok || cplx_tile != cplx_sum)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_moments_frames: unsupported dtypes tile=%s sum=%s varsum=%s",
                  dtype_name(tile_dtype), dtype_name(sum_dtype), dtype_name(varsum_dtype));
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    // 8- to 32-bit integers, floats and complex frames
    constexpr unsigned TILES = DT_INT8_32 | DT_FLOAT | DT_CPLX;
    if (!dtype_in(tile_dtype, TILES))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_moments_frames: unsupported tile dtype %s", dtype_name(tile_dtype));
    return dispatch_tile<TILES>(tile_dtype, [&](auto part) {
        return run_moments<LTMI_PART_T(part), LTMI_PART_L(part)>(
            tile, n_frames, n_px, ld_tile, n_prev, sum, sum_dtype, varsum, varsum_dtype, cols, ld_out,
            workspace, stream);
    });
}
