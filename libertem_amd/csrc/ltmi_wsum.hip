// Weighted sums of the frames of a tile for WeightedSumUDF (gfx950): the transposed mask product
//
//   ltmi_wsum_frames : out[c, p] (+)= sum_n weights[n, c] * frame_n[p],   1 <= k <= 64 components c
//
// k_wsum_slab   grid (pixel blocks, frame slabs) of four waves.  A wave owns 16 chunks of VEC consecutive
//               pixels (VEC = 8 for 1- / 2-byte pixels, 4 for 4-byte ones) and all k components, and walks
//               its slab four frames at a time on v_mfma_f32_16x16x4_f32: lane l loads chunk l & 15 of
//               frame f + (l >> 4) with one vector load -- the frames as they lie in memory, no transpose,
//               no LDS -- and weights[f + (l >> 4), 16 g + (l & 15)] for each group g of 16 components.
//               Element e of the chunks is the B operand (B[frame][chunk]), the weights the A operand
//               (A[component][frame]) of MFMA (g, e): D[component][chunk] lands with the chunk on the lane,
//               so a lane ends up with VEC consecutive pixels of four components per group and stores them
//               as whole vectors.  The products are exact float32 FMAs, one chain per (component, pixel)
//               along the slab; a NaN or inf pixel reaches its own pixel of every component (0 * NaN) and
//               nothing else.  Components 16 g + i >= k carry zero weights and are not stored.
// k_wsum_merge  one thread per (component, pixel) adds the slabs in order in float64 and rounds once into
//               the float32 buffer (accumulate: after adding what it holds).  No atomics: bitwise repeatable.
//
// Slabs: wsum_plan() -- a function of (n_frames, n_px, k) only, so that the workspace query, which does not
// know the tile dtype, and the launch agree.  Enough slabs for >= 2048 workgroups and chains of <= 4096
// frames; at least max(32, 16 k) frames each, so that the partials (k floats per pixel and slab) stay small
// next to the frames read; at most 256; and no more than fit WSUM_WS_CAP bytes (one slab when even that
// does not fit: the workspace is max(cap, 4 k n_px) bytes at most).
#include "ltmi_tiles.h"

namespace ltmi {
namespace {

constexpr int WSUM_BLOCK = 256;
constexpr int WSUM_WAVES = WSUM_BLOCK / 64;
constexpr int WSUM_MAX_K = 64;
constexpr int64_t WSUM_PLAN_PX = 512;            // pixels per workgroup the plan reckons with
constexpr int64_t WSUM_MAX_CHAIN = 4096;         // frames per float32 chain
constexpr int64_t WSUM_WS_CAP = 256ll << 20;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WsumPlan {
    int64_t per;    // frames per slab, a multiple of 4
    int slabs;      // none is empty
};

WsumPlan wsum_plan(int64_t n_frames, int64_t n_px, int k) {
    const int64_t px_blocks = (n_px + WSUM_PLAN_PX - 1) / WSUM_PLAN_PX;
    int64_t want = (2048 + px_blocks - 1) / px_blocks;
    want = std::max<int64_t>(want, (n_frames + WSUM_MAX_CHAIN - 1) / WSUM_MAX_CHAIN);
    const int64_t min_per = std::max<int64_t>(32, 16 * (int64_t)k);
    want = std::min<int64_t>(want, std::max<int64_t>(1, n_frames / min_per));
    want = std::min<int64_t>(want, 256);
    const int64_t slab_bytes = (int64_t)k * n_px * (int64_t)sizeof(float);
    want = std::min<int64_t>(want, std::max<int64_t>(1, WSUM_WS_CAP / slab_bytes));
    WsumPlan p;
    p.per = ((n_frames + want - 1) / want + 3) / 4 * 4;
    p.slabs = (int)((n_frames + p.per - 1) / p.per);
    return p;
}

int64_t wsum_ws_bytes(const WsumPlan &p, int64_t n_px, int k) {
    return (int64_t)p.slabs * k * n_px * (int64_t)sizeof(float);
}

template <typename T> struct WsumVec { static constexpr int value = sizeof(T) == 4 ? 4 : 8; };

// the lane's VEC pixels from p0 of frame f as float; zero past the slab's last frame and past the frame's end
template <typename T, int VEC>
__device__ __forceinline__ void wsum_load_guarded(const T *__restrict__ tile, int64_t ld, int64_t f, int64_t f1,
                                                  int64_t p0, int64_t n_px, float (&x)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) x[e] = (f < f1 && p0 + e < n_px) ? (float)tile[f * ld + p0 + e] : 0.f;
}

// ws slab s: k rows of n_px floats at ws + s * k * n_px; frames of slab s: [s * per, min(n_frames, (s + 1) * per))
template <typename T, int G>
__global__ void __launch_bounds__(WSUM_BLOCK)
k_wsum_slab(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_px,
            const float *__restrict__ w, int k, int64_t ld_w, int64_t per, int vec_ok, float *__restrict__ ws) {
    constexpr int VEC = WsumVec<T>::value;
    constexpr int UNR = 4;                      // steps of four frames in flight
    typedef tile_vec_t<T, VEC> vec_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = lane & 15, quad = lane >> 4;
    const int64_t wave_p0 = ((int64_t)blockIdx.x * WSUM_WAVES + wave) * (16 * VEC);
    if (wave_p0 >= n_px) return;                // the whole wave: no barrier below
    const int64_t p0 = wave_p0 + (int64_t)chunk * VEC;
    const int64_t f0 = (int64_t)blockIdx.y * per;
    const int64_t f1 = min(n_frames, f0 + per);

    f32x4 acc[G][VEC];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[g][e] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the lane's weight column of every group; columns >= k read column k - 1 and count as zero
    int wcol[G];
    float wkeep[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int c = 16 * g + chunk;
        wcol[g] = c < k ? c : k - 1;
        wkeep[g] = c < k ? 1.f : 0.f;
    }

    int64_t f = f0;
    if (vec_ok && wave_p0 + 16 * VEC <= n_px) {
        // whole chunks, whole steps: nothing to guard
        for (; f + 4 * UNR <= f1; f += 4 * UNR) {
            vec_t v[UNR];
            float a[UNR][G];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int64_t fl = f + 4 * u + quad;
                v[u] = *(const vec_t *)(tile + fl * ld + p0);
#pragma unroll
                for (int g = 0; g < G; ++g) a[u][g] = w[fl * ld_w + wcol[g]];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    // (select, not multiply: a NaN or inf in column k - 1 must not reach the columns >= k)
                    const float ag = wkeep[g] != 0.f ? a[u][g] : 0.f;
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        acc[g][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag, (float)v[u][e], acc[g][e], 0, 0, 0);
                }
            }
        }
        for (; f + 4 <= f1; f += 4) {
            const int64_t fl = f + quad;
            const vec_t v = *(const vec_t *)(tile + fl * ld + p0);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float a = w[fl * ld_w + wcol[g]];
                const float ag = wkeep[g] != 0.f ? a : 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    acc[g][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag, (float)v[e], acc[g][e], 0, 0, 0);
            }
        }
    }
    // ragged chunks, rows that take no vector loads, and the last frames of the tile
    for (; f < f1; f += 4) {
        const int64_t fl = f + quad;
        float x[VEC];
        wsum_load_guarded<T, VEC>(tile, ld, fl, f1, p0, n_px, x);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float ag = (fl < f1 && wkeep[g] != 0.f) ? w[fl * ld_w + wcol[g]] : 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                acc[g][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag, x[e], acc[g][e], 0, 0, 0);
        }
    }

    // D[component 4 quad + r of the group][chunk]: this lane's own pixels p0 .. p0 + VEC - 1
    float *slab = ws + (int64_t)blockIdx.y * k * n_px;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * g + 4 * quad + r;
            if (c >= k) continue;
            float *row = slab + (int64_t)c * n_px + p0;
            if (p0 + VEC <= n_px) {
#pragma unroll
                for (int e0 = 0; e0 < VEC; e0 += 4) {
                    tile_vec_t<float, 4> o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = acc[g][e0 + e][r];
                    *(tile_vec_t<float, 4> *)(row + e0) = o;
                }
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (p0 + e < n_px) row[e] = acc[g][e][r];
            }
        }
}

// out[c * comp_stride + (p / cols) * ld_out + p % cols] (+)= the slabs of (c, p) in order; grid (pixel blocks, k)
__global__ void __launch_bounds__(WSUM_BLOCK)
k_wsum_merge(const float *__restrict__ ws, int slabs, int k, int64_t n_px, float *__restrict__ out, int64_t cols,
             int64_t ld_out, int64_t comp_stride, int accumulate) {
    const int64_t p = (int64_t)blockIdx.x * WSUM_BLOCK + threadIdx.x;
    if (p >= n_px) return;
    const int c = blockIdx.y;
    double a = 0.0;
    for (int s = 0; s < slabs; ++s) a += (double)ws[((int64_t)s * k + c) * n_px + p];
    const int64_t r = p / cols;
    const int64_t o = (int64_t)c * comp_stride + r * ld_out + (p - r * cols);
    out[o] = accumulate ? (float)((double)out[o] + a) : (float)a;
}

template <typename T>
int run_wsum(const void *tile_, int64_t n_frames, int64_t n_px, int64_t ld, const float *w, int k, int64_t ld_w,
             float *out, int64_t cols, int64_t ld_out, int64_t comp_stride, int accumulate, void *ws_,
             hipStream_t stream) {
    constexpr int VEC = WsumVec<T>::value;
    const T *tile = (const T *)tile_;
    float *ws = (float *)ws_;
    const WsumPlan pl = wsum_plan(n_frames, n_px, k);              // matches the workspace query
    const int vec_ok = vector_loads_ok(tile, ld, sizeof(T)) ? 1 : 0;
    const int64_t wg_px = (int64_t)WSUM_WAVES * 16 * VEC;
    const dim3 grid((unsigned)((n_px + wg_px - 1) / wg_px), (unsigned)pl.slabs);
#define LTMI_WSUM_LAUNCH(G)                                                                                  \
    hipLaunchKernelGGL((k_wsum_slab<T, G>), grid, dim3(WSUM_BLOCK), 0, stream, tile, ld, n_frames, n_px, w, k, \
                       ld_w, pl.per, vec_ok, ws)
    switch ((k + 15) / 16) {
        case 1: LTMI_WSUM_LAUNCH(1); break;
        case 2: LTMI_WSUM_LAUNCH(2); break;
        case 3: LTMI_WSUM_LAUNCH(3); break;
        default: LTMI_WSUM_LAUNCH(4); break;
    }
#undef LTMI_WSUM_LAUNCH
    LTMI_HIP(hipGetLastError());
    const dim3 mgrid((unsigned)((n_px + WSUM_BLOCK - 1) / WSUM_BLOCK), (unsigned)k);
    hipLaunchKernelGGL(k_wsum_merge, mgrid, dim3(WSUM_BLOCK), 0, stream, (const float *)ws, pl.slabs, k, n_px, out,
                       cols, ld_out, comp_stride, accumulate);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

// bool (read as uint8), 1- / 2- / 4-byte integers and float32
constexpr unsigned WSUM_TILES = DT_BOOL | DT_INT8_32 | dtype_bit(LTMI_F32);

}  // namespace
}  // namespace ltmi

using namespace ltmi;

extern "C" int64_t ltmi_wsum_workspace(int64_t n_frames, int64_t n_px, int k) {
    if (n_frames <= 0 || n_px <= 0 || k < 1 || k > WSUM_MAX_K) return 0;
    return wsum_ws_bytes(wsum_plan(n_frames, n_px, k), n_px, k);
}

extern "C" int ltmi_wsum_frames(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t n_px,
                                int64_t ld_tile, const void *weights, int k, int64_t ld_w, void *out, int64_t cols,
                                int64_t ld_out, int64_t comp_stride, int accumulate, void *workspace,
                                void *stream_) {
    if (n_frames < 0 || n_px < 0 || ld_tile < n_px)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wsum_frames: bad shape");
    if (k < 1 || k > WSUM_MAX_K)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wsum_frames: k = %d is outside 1 .. %d", k, WSUM_MAX_K);
    if (ld_w < k)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wsum_frames: ld_w %lld is below k = %d", (long long)ld_w, k);
    if (int rc = check_sig_slice("ltmi_wsum_frames", n_px, cols, ld_out)) return rc;
    if (n_px > 0 && k > 1 && comp_stride < (n_px / cols - 1) * ld_out + cols)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wsum_frames: comp_stride %lld is shorter than one component",
                  (long long)comp_stride);
    if (!dtype_in(tile_dtype, WSUM_TILES))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_wsum_frames: unsupported tile dtype %s", dtype_name(tile_dtype));
    if (n_frames == 0 || n_px == 0) return LTMI_OK;
    if (!tile || !weights || !out || !workspace)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_wsum_frames: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    return dispatch_tile<WSUM_TILES>(tile_dtype, [&](auto part) {
        return run_wsum<LTMI_PART_T(part)>(tile, n_frames, n_px, ld_tile, (const float *)weights, k, ld_w,
                                           (float *)out, cols, ld_out, comp_stride, accumulate ? 1 : 0, workspace,
                                           stream);
    });
}
