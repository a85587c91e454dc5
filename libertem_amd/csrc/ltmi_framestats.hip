// Per-frame statistics for FEMUDF and LogsumUDF (gfx950).
//
//   ltmi_ring_moments  : out[f] = std(frame_f[ring])                  (src/libertem/udf/FEM.py:65-66)
//   ltmi_logsum_frames : out[p] += sum_f log(frame_f[p] - min(frame_f) + 1)
//                                                                     (src/libertem/udf/logsum.py:54-59)
//
// k_ring        : one workgroup per frame.  Wave w walks spans w, w + 4, ... of the ring (row, x0, x1:
//                 taken from the exact boolean mask on the host), its lanes stride along the span, so
//                 only the 128-byte lines the ring touches are read.  Sums s = sum(x - K) and
//                 q = sum(|x - K|^2) in float64 about K, the frame's first ring pixel (as k_moments_slab;
//                 exact for <= 16-bit integers), reduced across the workgroup in a fixed order:
//                 std = sqrt((q - |s|^2 / n) / n).  No atomics: bitwise repeatable.
// logsum        : the tile is processed in chunks of frames that fit the Infinity Cache.  Per chunk
//   k_frame_min   one workgroup per frame: min in the compute dtype, NaN propagates (np.min);
//   k_logsum_slab grid (pixel blocks, frame slabs): a thread owns VEC consecutive pixels and adds the
//                 terms log((x - m) + 1), rounded in the compute dtype like the reference's float frame,
//                 in float64.  The chunk's second read is served from the cache;
//   k_logsum_merge one thread per pixel adds the slabs in order to a float64 accumulator and, after the
//                 last chunk, folds it into the float32 buffer.  No atomics: bitwise repeatable.
// The compute dtype is np.result_type(float32, stored dtype): float for <= 16-bit integers and float32,
// double for 32-bit integers and float64.
#include "ltmi_tiles.h"

namespace ltmi {
namespace {

constexpr int FS_BLOCK = 256;
constexpr int FS_WAVES = FS_BLOCK / 64;

template <typename T> __device__ __forceinline__ double as_f64(T x) { return (double)x; }

// ---- FEM: ring moments ------------------------------------------------------------------------------

// L = 1 (real pixels) or 2 (complex pixels: T is the part type)
template <typename T, int L>
__global__ void __launch_bounds__(FS_BLOCK)
k_ring(const T *__restrict__ tile, int64_t ld, int64_t width, const int32_t *__restrict__ spans,
       int n_spans, int64_t n_ring, float *__restrict__ out) {
    constexpr int UNR = 4;
    const int64_t f = blockIdx.x;
    if (n_spans == 0 || n_ring == 0) {
        if (threadIdx.x == 0) out[f] = __builtin_nanf("");
        return;
    }
    const T *fr = tile + f * ld * L;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    double k[L], s[L], q = 0.0;
    const int64_t first = ((int64_t)spans[0] * width + spans[1]) * L;
#pragma unroll
    for (int c = 0; c < L; ++c) {
        k[c] = as_f64(fr[first + c]);
        s[c] = 0.0;
    }
    // (measured on 256^2 uint16 frames: one pixel per lane beats 8-byte vectors per lane with four spans
    // in flight per wave, 2.8 vs 3.3 ms, and sixteen spans in flight, 7.7 ms)
    for (int sp = wave; sp < n_spans; sp += FS_WAVES) {
        const int64_t row = spans[3 * sp];
        const int x0 = spans[3 * sp + 1], x1 = spans[3 * sp + 2];
        const T *rp = fr + row * width * L;
        for (int x = x0 + lane; x < x1; x += 64 * UNR) {
            T v[UNR][L];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int c = 0; c < L; ++c)
                    v[u][c] = (x + 64 * u < x1) ? rp[(int64_t)(x + 64 * u) * L + c] : (T)0;
#pragma unroll
            for (int u = 0; u < UNR; ++u)
                if (x + 64 * u < x1)
#pragma unroll
                    for (int c = 0; c < L; ++c) {
                        const double d = as_f64(v[u][c]) - k[c];
                        s[c] += d;
                        q = fma(d, d, q);
                    }
        }
    }
    // wave reduction, then the waves in order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < L; ++c) s[c] += __shfl_down(s[c], off, 64);
        q += __shfl_down(q, off, 64);
    }
    __shared__ double red[FS_WAVES][L + 1];
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < L; ++c) red[wave][c] = s[c];
        red[wave][L] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts[L], tq = 0.0;
#pragma unroll
        for (int c = 0; c < L; ++c) ts[c] = 0.0;
        for (int w = 0; w < FS_WAVES; ++w) {
#pragma unroll
            for (int c = 0; c < L; ++c) ts[c] += red[w][c];
            tq += red[w][L];
        }
        const double n = (double)n_ring;
        double ss = 0.0;
#pragma unroll
        for (int c = 0; c < L; ++c) ss = fma(ts[c], ts[c], ss);
        double m2 = tq - ss / n;
        m2 = m2 < 0.0 ? 0.0 : m2;          // (rounding below 0 clamped; NaN passes)
        out[f] = (float)sqrt(m2 / n);
    }
}

template <typename T, int L>
int run_ring(const void *tile, int64_t n_frames, int64_t width, int64_t ld, const int32_t *spans,
             int n_spans, int64_t n_ring, float *out, hipStream_t stream) {
    hipLaunchKernelGGL((k_ring<T, L>), dim3((unsigned)n_frames), dim3(FS_BLOCK), 0, stream,
                       (const T *)tile, ld, width, spans, n_spans, n_ring, out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

// ---- logsum ----------------------------------------------------------------------------------------

// frames per chunk: both passes over a chunk stay within the 256 MiB Infinity Cache
constexpr int64_t LOGSUM_CHUNK_BYTES = 96ll << 20;
constexpr int LOGSUM_VEC_BYTES = 8;

struct LogsumPlan {
    int64_t chunk;       // frames per chunk
    int64_t px_blocks;   // workgroups along the pixels
    int fsplit;          // slabs per (full) chunk
};

LogsumPlan logsum_plan(int64_t n_frames, int64_t n_px, int elem) {
    LogsumPlan p;
    const int64_t frame_bytes = std::max<int64_t>(1, n_px * elem);
    p.chunk = std::max<int64_t>(1, std::min<int64_t>(n_frames, LOGSUM_CHUNK_BYTES / frame_bytes));
    const int vec = std::max(1, LOGSUM_VEC_BYTES / elem);
    p.px_blocks = (n_px + (int64_t)FS_BLOCK * vec - 1) / ((int64_t)FS_BLOCK * vec);
    int64_t want = (1024 + p.px_blocks - 1) / p.px_blocks;      // aim at >= 1024 workgroups
    // a slab of >= 32 frames: the float64 partials stay small next to the frames
    want = std::max<int64_t>(1, std::min<int64_t>(want, p.chunk / 32));
    p.fsplit = (int)std::min<int64_t>(want, 64);
    return p;
}

// x as the reference's float frame: result_type(float32, stored dtype)
template <typename T> struct Compute { typedef float type; };
template <> struct Compute<uint32_t> { typedef double type; };
template <> struct Compute<int32_t> { typedef double type; };
template <> struct Compute<double> { typedef double type; };

__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || a < b) ? a : ((b != b || b < a) ? b : a); }
__device__ __forceinline__ double min_nan(double a, double b) { return (a != a || a < b) ? a : ((b != b || b < a) ? b : a); }
__device__ __forceinline__ float shfl_down_ct(float v, int off) { return __shfl_down(v, off, 64); }
__device__ __forceinline__ double shfl_down_ct(double v, int off) { return __shfl_down(v, off, 64); }

template <typename T>
__global__ void __launch_bounds__(FS_BLOCK)
k_frame_min(const T *__restrict__ tile, int64_t ld, int64_t n_px,
            typename Compute<T>::type *__restrict__ mins) {
    typedef typename Compute<T>::type CT;
    constexpr int VEC = 16 / sizeof(T);
    typedef tile_vec_t<T, VEC> vec_t;
    const T *fr = tile + (int64_t)blockIdx.x * ld;
    CT m = __builtin_inf();
    const int64_t n_vec = n_px / VEC;
    int64_t i = threadIdx.x;
    for (; i + 3 * FS_BLOCK < n_vec; i += 4 * FS_BLOCK) {       // four loads in flight per thread
        vec_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const vec_t *)(fr + (i + u * FS_BLOCK) * VEC);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) m = min_nan(m, (CT)v[u][e]);
    }
    for (; i < n_vec; i += FS_BLOCK) {
        const vec_t v = *(const vec_t *)(fr + i * VEC);      // (plain load: k_logsum_slab reads it again)
#pragma unroll
        for (int e = 0; e < VEC; ++e) m = min_nan(m, (CT)v[e]);
    }
    for (int64_t i = n_vec * VEC + threadIdx.x; i < n_px; i += FS_BLOCK) m = min_nan(m, (CT)fr[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = min_nan(m, shfl_down_ct(m, off));
    __shared__ CT red[FS_WAVES];
    if (threadIdx.x % 64 == 0) red[threadIdx.x / 64] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        CT r = red[0];
        for (int w = 1; w < FS_WAVES; ++w) r = min_nan(r, red[w]);
        mins[blockIdx.x] = r;
    }
}

__device__ __forceinline__ float log_ct(float x) { return logf(x); }
__device__ __forceinline__ double log_ct(double x) { return log(x); }

// ws slab k: n_px doubles at ws + k * n_px; frames of slab k: [k * per, min(n, (k + 1) * per))
template <typename T, int VEC>
__global__ void __launch_bounds__(FS_BLOCK)
k_logsum_slab(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_px, int64_t per,
              const typename Compute<T>::type *__restrict__ mins, double *__restrict__ ws) {
    typedef typename Compute<T>::type CT;
    typedef tile_vec_t<T, VEC> vec_t;
    const int64_t p0 = ((int64_t)blockIdx.x * FS_BLOCK + threadIdx.x) * VEC;
    if (p0 >= n_px) return;
    const int64_t f0 = (int64_t)blockIdx.y * per;
    const int64_t f1 = min(n_frames, f0 + per);
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    if (p0 + VEC <= n_px) {
        int64_t f = f0;
        for (; f + 3 < f1; f += 4) {
            vec_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const vec_t *)(tile + (f + u) * ld + p0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const CT m = mins[f + u];
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += (double)log_ct(((CT)v[u][e] - m) + (CT)1);
            }
        }
        for (; f < f1; ++f) {
            const vec_t v = *(const vec_t *)(tile + f * ld + p0);
            const CT m = mins[f];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += (double)log_ct(((CT)v[e] - m) + (CT)1);
        }
    } else {
        for (int64_t f = f0; f < f1; ++f) {
            const CT m = mins[f];
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (p0 + e < n_px) acc[e] += (double)log_ct(((CT)tile[f * ld + p0 + e] - m) + (CT)1);
        }
    }
    double *slab = ws + (int64_t)blockIdx.y * n_px;
#pragma unroll
    for (int e = 0; e < VEC; ++e)
        if (p0 + e < n_px) slab[p0 + e] = acc[e];
}

// acc[p] = (first ? 0 : acc[p]) + slabs in order; last: out[(p / cols) * ld_out + p % cols] += acc[p]
__global__ void __launch_bounds__(FS_BLOCK)
k_logsum_merge(const double *__restrict__ ws, int fsplit, int64_t n_px, double *__restrict__ acc,
               int first, int last, float *__restrict__ out, int64_t cols, int64_t ld_out) {
    const int64_t p = (int64_t)blockIdx.x * FS_BLOCK + threadIdx.x;
    if (p >= n_px) return;
    double a = first ? 0.0 : acc[p];
    for (int k = 0; k < fsplit; ++k) a += ws[(int64_t)k * n_px + p];
    if (!last) {
        acc[p] = a;
        return;
    }
    const int64_t r = p / cols;
    const int64_t o = r * ld_out + (p - r * cols);
    out[o] = (float)((double)out[o] + a);
}

// workspace: [acc: n_px doubles][slabs: fsplit * n_px doubles][mins: chunk doubles]
int64_t logsum_ws_bytes(const LogsumPlan &p, int64_t n_px) {
    return ((int64_t)(1 + p.fsplit) * n_px + p.chunk) * (int64_t)sizeof(double);
}

template <typename T>
int run_logsum(const void *tile_, int64_t n_frames, int64_t n_px, int64_t ld, float *out, int64_t cols,
               int64_t ld_out, void *ws_, hipStream_t stream) {
    typedef typename Compute<T>::type CT;
    constexpr int VEC = LOGSUM_VEC_BYTES / (int)sizeof(T) > 0 ? LOGSUM_VEC_BYTES / (int)sizeof(T) : 1;
    const T *tile = (const T *)tile_;
    const LogsumPlan pl = logsum_plan(n_frames, n_px, (int)sizeof(T));
    double *acc = (double *)ws_;
    double *slabs = acc + n_px;
    CT *mins = (CT *)(slabs + (int64_t)pl.fsplit * n_px);
    const bool vec_ok = vector_loads_ok(tile, ld, sizeof(T));
    const dim3 mgrid((unsigned)((n_px + FS_BLOCK - 1) / FS_BLOCK));
    for (int64_t c0 = 0; c0 < n_frames; c0 += pl.chunk) {
        const int64_t nc = std::min<int64_t>(pl.chunk, n_frames - c0);
        const T *ct = tile + c0 * ld;
        hipLaunchKernelGGL((k_frame_min<T>), dim3((unsigned)nc), dim3(FS_BLOCK), 0, stream, ct, ld, n_px, mins);
        LTMI_HIP(hipGetLastError());
        // slabs of this chunk (a short last chunk gets fewer, none is empty)
        const int64_t per = (nc + pl.fsplit - 1) / pl.fsplit;
        const int fsplit = (int)((nc + per - 1) / per);
        if (vec_ok) {
            const dim3 grid((unsigned)((n_px + (int64_t)FS_BLOCK * VEC - 1) / ((int64_t)FS_BLOCK * VEC)),
                            (unsigned)fsplit);
            hipLaunchKernelGGL((k_logsum_slab<T, VEC>), grid, dim3(FS_BLOCK), 0, stream, ct, ld, nc, n_px,
                               per, (const CT *)mins, slabs);
        } else {
            const dim3 grid((unsigned)((n_px + FS_BLOCK - 1) / FS_BLOCK), (unsigned)fsplit);
            hipLaunchKernelGGL((k_logsum_slab<T, 1>), grid, dim3(FS_BLOCK), 0, stream, ct, ld, nc, n_px,
                               per, (const CT *)mins, slabs);
        }
        LTMI_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_logsum_merge, mgrid, dim3(FS_BLOCK), 0, stream, (const double *)slabs, fsplit,
                           n_px, acc, (int)(c0 == 0), (int)(c0 + nc >= n_frames), out, cols, ld_out);
        LTMI_HIP(hipGetLastError());
    }
    return LTMI_OK;
}

}  // namespace
}  // namespace ltmi

using namespace ltmi;

extern "C" int ltmi_ring_moments(int device, const void *tile, int tile_dtype, int64_t n_frames,
                                 int64_t width, int64_t ld_tile, const void *spans, int n_spans,
                                 int64_t n_ring, void *out, void *stream_) {
    if (n_frames < 0 || width <= 0 || n_spans < 0 || n_ring < 0 || ld_tile < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ring_moments: bad shape");
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !out || (n_spans > 0 && !spans))
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_ring_moments: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    const int32_t *sp = (const int32_t *)spans;
    constexpr unsigned TILES = DT_INT8_32 | DT_FLOAT | DT_CPLX;
    if (!dtype_in(tile_dtype, TILES))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_ring_moments: unsupported tile dtype %s", dtype_name(tile_dtype));
    return dispatch_tile<TILES>(tile_dtype, [&](auto part) {
        return run_ring<LTMI_PART_T(part), LTMI_PART_L(part)>(tile, n_frames, width, ld_tile, sp, n_spans,
                                                              n_ring, (float *)out, stream);
    });
}

// the frames logsum takes: no complex ones (the reference cannot cast their terms to float32 either)
constexpr unsigned LOGSUM_TILES = DT_INT8_32 | DT_FLOAT;

extern "C" int64_t ltmi_logsum_workspace(int64_t n_frames, int64_t n_px, int tile_dtype) {
    if (n_frames <= 0 || n_px <= 0 || !dtype_in(tile_dtype, LOGSUM_TILES)) return 0;
    return logsum_ws_bytes(logsum_plan(n_frames, n_px, dtype_size(tile_dtype)), n_px);
}

extern "C" int ltmi_logsum_frames(int device, const void *tile, int tile_dtype, int64_t n_frames,
                                  int64_t n_px, int64_t ld_tile, void *out, int64_t cols, int64_t ld_out,
                                  void *workspace, void *stream_) {
    if (n_frames < 0 || n_px < 0 || ld_tile < n_px)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_logsum_frames: bad shape");
    if (int rc = check_sig_slice("ltmi_logsum_frames", n_px, cols, ld_out)) return rc;
    if (!dtype_in(tile_dtype, LOGSUM_TILES))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_logsum_frames: unsupported tile dtype %s", dtype_name(tile_dtype));
    if (n_frames == 0 || n_px == 0) return LTMI_OK;
    if (!tile || !out || !workspace)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_logsum_frames: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    return dispatch_tile<LOGSUM_TILES>(tile_dtype, [&](auto part) {
        return run_logsum<LTMI_PART_T(part)>(tile, n_frames, n_px, ld_tile, (float *)out, cols, ld_out,
                                             workspace, stream);
    });
}
