// ltmi_orient.hip -- orientation matching in polar coordinates: every frame against a library of templates at every
// in-plane rotation, reduced to the best few templates on the device (the definition:
// include/ltmi.h).
//
// One workgroup of ORI_THREADS threads (16 waves: 4 per SIMD, what 4-byte LDS reads need to reach their rate) takes one
// frame at a time, grid-strided over the frames.
//   stage 1  the frame is resampled to the polar image P (n_r, n_phi) in LDS: a sampling point per thread and step,
//            its four taps gathered from global memory (the table is read by every workgroup and stays in L2), the
//            pixels converted in registers, four float32 products and three float32 sums, none contracted.  The
//            non-finite flag and the float64 sum of squares are reduced over the workgroup in a fixed order.
//   stage 2  a wave takes a template, its lanes the rotations: lane l keeps the accumulators of the rotations
//            k = 64 c + l, c < NCH = ceil(n_phi / 64).  A spot is 8 bytes -- (row offset << 10 | phi, weight) -- at a
//            wave-uniform address, loaded once and used for every chunk; the lanes of a chunk read consecutive words of
//            P's row.  The wrap at n_phi is min_u32(phi + k, phi + k - n_phi): the polar image of the largest shapes
//            (64 x 360 float32 = 90 KiB) does not fit LDS twice, so no row is stored doubled.  The template's maximum
//            and the lowest rotation that reaches it are a wave reduction.
//   stage 3  the scores of a block of ORI_BLOCK templates sit in LDS; wave 0 merges each block into the running list
//            of the n_best best, which lane j keeps for slot j: slot after slot, the best candidate behind the one
//            picked last in the order (score descending, template ascending).  No atomics, one fixed order.
// Weak case: fewer frames than CUs -- a frame is one workgroup's, the rest of the chip idles.
#include "ltmi_tiles.h"
#include <cmath>
#include <new>

// the definition rounds every product and every sum on its own: no fused multiply-add in this file.  (The products
// and sums below are plain operators: __fmul_rn / __fadd_rn are inline functions of a header compiled with
// contraction on, and the two fuse after inlining.)
#pragma clang fp contract(off)

namespace ltmi {
namespace {

constexpr int ORI_THREADS = 1024, ORI_WAVES = ORI_THREADS / 64;
constexpr int ORI_BLOCK = 1024;                             // templates whose scores sit in LDS at a time
constexpr int ORI_MAX_PHI = 1024, ORI_MAX_BEST = 16;
static_assert(ORI_MAX_PHI == 16 * 64, "ltmi_orient_match instantiates 1 to 16 accumulators per lane");
constexpr int ORI_LDS_TOTAL = 160 * 1024;
// behind P: scores and rotations of a block, the waves' sums of squares, their flags
constexpr int ORI_LDS_OTHER = ORI_BLOCK * 8 + ORI_WAVES * 8 + ORI_WAVES * 4;
constexpr int ORI_MAX_WORDS = (ORI_LDS_TOTAL - ORI_LDS_OTHER) / 4;
constexpr unsigned ORI_DTYPES = DT_INT8_32 | dtype_bit(LTMI_F32);
constexpr int ORI_GRID = 1024;

struct Spot {
    uint32_t at;                                            // (spot_r * n_phi) << 10 | spot_phi
    float w;
};

struct OrientArgs {
    const void *tile;
    int64_t n_frames, ld_tile;
    int n_points, n_phi;                                    // n_points = n_r * n_phi
    const int4 *tap_idx;
    const float4 *tap_w;
};

struct LibArgs {
    int n_templates, n_best;
};

__device__ __forceinline__ bool ori_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// P of one sampling point; a tap of weight 0 is not read.  -> bad: a tap of non-zero weight is not finite
template <typename T>
__device__ __forceinline__ float ori_sample(const T *__restrict__ src, int4 at, float4 w, bool *bad) {
    const float v0 = w.x != 0.f ? (float)src[at.x] : 0.f;
    const float v1 = w.y != 0.f ? (float)src[at.y] : 0.f;
    const float v2 = w.z != 0.f ? (float)src[at.z] : 0.f;
    const float v3 = w.w != 0.f ? (float)src[at.w] : 0.f;
    // (an all-ones exponent: infinity or NaN; integer pixels are finite)
    *bad = std::is_same<T, float>::value &&
           (ori_nonfinite(v0) || ori_nonfinite(v1) || ori_nonfinite(v2) || ori_nonfinite(v3));
    return (w.x * v0 + w.y * v1) + (w.z * v2 + w.w * v3);
}

template <typename T>
__global__ void __launch_bounds__(256)
k_orient_polar(OrientArgs a, float *__restrict__ polar_out, int64_t ld_polar) {
    for (int64_t f = blockIdx.x; f < a.n_frames; f += gridDim.x) {
        const T *src = (const T *)a.tile + f * a.ld_tile;
        float *dst = polar_out + f * ld_polar;
        for (int i = threadIdx.x; i < a.n_points; i += 256) {
            bool bad;
            dst[i] = ori_sample<T>(src, a.tap_idx[i], a.tap_w[i], &bad);
        }
    }
}

// (value, rotation) of two lanes: the larger value, of equal values the lower rotation
__device__ __forceinline__ void ori_wave_best(float &v, int &k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int ok = __shfl_xor(k, off, 64);
        if (ov > v || (ov == v && ok < k)) v = ov, k = ok;
    }
}

template <typename T, int NCH>
__global__ void __launch_bounds__(ORI_THREADS)
k_orient_match(OrientArgs a, LibArgs lib, const int32_t *__restrict__ indptr, const Spot *__restrict__ spots,
               int32_t *__restrict__ template_out, int32_t *__restrict__ rotation_out,
               float *__restrict__ correlation_out, float *__restrict__ norm_out) {
    extern __shared__ __align__(16) unsigned char ori_smem[];
    float *P = (float *)ori_smem;
    // (n_points rounded up to even: the doubles behind stay 8-byte aligned)
    double *sh_ss = (double *)(P + ((a.n_points + 1) & ~1));
    float *sh_score = (float *)(sh_ss + ORI_WAVES);
    int *sh_rot = (int *)(sh_score + ORI_BLOCK);
    int *sh_bad = sh_rot + ORI_BLOCK;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_phi = a.n_phi;                              // NCH = ceil(n_phi / 64)
    // this lane's rotations; a lane past n_phi scores rotation 0 again and stays out of the reduction
    unsigned kc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) kc[c] = c * 64 + lane < n_phi ? c * 64 + lane : 0;
    const float NAN_F = __builtin_nanf("");

    for (int64_t f = blockIdx.x; f < a.n_frames; f += gridDim.x) {
        // ---- stage 1
        const T *src = (const T *)a.tile + f * a.ld_tile;
        bool bad = false;
        double ss = 0.;
        for (int i = tid; i < a.n_points; i += ORI_THREADS) {
            bool b;
            const float p = ori_sample<T>(src, a.tap_idx[i], a.tap_w[i], &b);
            bad |= b;
            ss += (double)p * (double)p;
            P[i] = p;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
        const bool wave_bad = __any(bad);
        if (lane == 0) sh_ss[wave] = ss, sh_bad[wave] = wave_bad ? 1 : 0;
        __syncthreads();
        double total = 0.;
        int any_bad = 0;
        for (int j = 0; j < ORI_WAVES; ++j) total += sh_ss[j], any_bad |= sh_bad[j];
        if (any_bad) {                                      // (uniform over the workgroup)
            if (tid < lib.n_best) {
                template_out[f * lib.n_best + tid] = -1;
                rotation_out[f * lib.n_best + tid] = -1;
                correlation_out[f * lib.n_best + tid] = NAN_F;
            }
            if (tid == 0) norm_out[f] = NAN_F;
            __syncthreads();                                // sh_ss and sh_bad are read before the next frame's
            continue;
        }
        // wave 0, lane j: slot j of the running list
        float my_c = NAN_F;
        int my_t = -1, my_r = -1, n_have = 0;
        for (int t0 = 0; t0 < lib.n_templates; t0 += ORI_BLOCK) {
            const int nb = min(ORI_BLOCK, lib.n_templates - t0);
            // ---- stage 2
            for (int b = wave; b < nb; b += ORI_WAVES) {
                const int s0 = indptr[t0 + b], s1 = indptr[t0 + b + 1];
                float acc[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = 0.f;
                for (int s = s0; s < s1; ++s) {
                    const Spot sp = spots[s];
                    const unsigned phi = sp.at & 1023u, row = sp.at >> 10;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        const unsigned x = kc[c] + phi;
                        acc[c] = acc[c] + sp.w * P[row + min(x, x - (unsigned)n_phi)];
                    }
                }
                float v = acc[0];
                int k = lane;
#pragma unroll
                for (int c = 1; c < NCH; ++c)
                    if (acc[c] > v) v = acc[c], k = c * 64 + lane;
                if (lane >= n_phi) k = 0;                   // (only in chunk 0: its value is rotation 0's)
                ori_wave_best(v, k);
                if (lane == 0) sh_score[b] = v, sh_rot[b] = k;
            }
            __syncthreads();
            // ---- stage 3
            if (wave == 0) {
                float new_c = NAN_F, prev_c = __builtin_huge_valf();
                int new_t = -1, new_r = -1, prev_t = -1, n_new = 0;
                for (int j = 0; j < lib.n_best; ++j) {
                    // the best candidate behind (prev_c, prev_t): of the list's slots, then of the block
                    bool found = false;
                    float bc = 0.f;
                    int bt = 0, br = 0;
                    if (lane < n_have && (my_c < prev_c || (my_c == prev_c && my_t > prev_t)))
                        found = true, bc = my_c, bt = my_t, br = my_r;
                    for (int b = lane; b < nb; b += 64) {
                        const float c = sh_score[b];
                        const int t = t0 + b;
                        if ((c < prev_c || (c == prev_c && t > prev_t)) && (!found || c > bc || (c == bc && t < bt)))
                            found = true, bc = c, bt = t, br = sh_rot[b];
                    }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const bool of = __shfl_xor((int)found, off, 64) != 0;
                        const float oc = __shfl_xor(bc, off, 64);
                        const int ot = __shfl_xor(bt, off, 64), orot = __shfl_xor(br, off, 64);
                        if (of && (!found || oc > bc || (oc == bc && ot < bt)))
                            found = true, bc = oc, bt = ot, br = orot;
                    }
                    if (!found) break;                      // (the same in every lane)
                    if (lane == j) new_c = bc, new_t = bt, new_r = br;
                    prev_c = bc, prev_t = bt;
                    ++n_new;
                }
                my_c = new_c, my_t = new_t, my_r = new_r, n_have = n_new;
            }
            __syncthreads();
        }
        if (wave == 0 && lane < lib.n_best) {
            template_out[f * lib.n_best + lane] = my_t;
            rotation_out[f * lib.n_best + lane] = my_r;
            correlation_out[f * lib.n_best + lane] = my_c;
        }
        if (tid == 0) norm_out[f] = (float)sqrt(total);
    }
}

template <typename T, int NCH>
int launch_match(int device, unsigned grid, size_t smem, hipStream_t stream, const OrientArgs &a, const LibArgs &lib,
                 const int32_t *indptr, const Spot *spots, int32_t *template_out, int32_t *rotation_out,
                 float *correlation_out, float *norm_out) {
    static bool set[16] = {false};
    if (!set[device & 15]) {
        LTMI_HIP(hipFuncSetAttribute((const void *)k_orient_match<T, NCH>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     ORI_LDS_TOTAL));
        set[device & 15] = true;
    }
    hipLaunchKernelGGL((k_orient_match<T, NCH>), dim3(grid), dim3(ORI_THREADS), smem, stream, a, lib, indptr, spots,
                       template_out, rotation_out, correlation_out, norm_out);
    return LTMI_OK;
}

}  // namespace
}  // namespace ltmi

using namespace ltmi;

struct ltmi_orient_plan {
    int device = 0;
    int sig_h = 0, sig_w = 0, n_r = 0, n_phi = 0, n_templates = 0, n_best = 0;
    DevBuf<int4> tap_idx;
    DevBuf<float4> tap_w;
    DevBuf<int32_t> indptr;
    DevBuf<Spot> spots;
    char last_kernel[96] = {0};
};

extern "C" int ltmi_orient_max_polar_words(void) { return ORI_MAX_WORDS; }

extern "C" int ltmi_orient_score_block(void) { return ORI_BLOCK; }

extern "C" int ltmi_orient_plan_create(int device, int sig_h, int sig_w, int n_r, int n_phi, const int32_t *tap_idx,
                                       const float *tap_w, int n_templates, const int64_t *indptr,
                                       const int32_t *spot_r, const int32_t *spot_phi, const float *spot_w, int n_best,
                                       ltmi_orient_plan **out) {
    const char *who = "ltmi_orient_plan_create";
    if (!out) LTMI_FAIL(LTMI_E_INVALID, "%s: null output pointer", who);
    *out = nullptr;
    if (sig_h < 1 || sig_w < 1 || (int64_t)sig_h * sig_w > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: frames of %d x %d (1 to 2^31 - 1 pixels each)", who, sig_h, sig_w);
    if (n_best < 1 || n_best > ORI_MAX_BEST)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: n_best %d must lie in [1, %d]", who, n_best, ORI_MAX_BEST);
    if (n_phi < 1 || n_phi > ORI_MAX_PHI)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: n_phi %d must lie in [1, %d]", who, n_phi, ORI_MAX_PHI);
    if (n_r < 1) LTMI_FAIL(LTMI_E_SHAPE, "%s: n_r %d must be at least 1", who, n_r);
    if ((int64_t)n_r * n_phi > ORI_MAX_WORDS)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: a polar image of n_r %d x n_phi %d = %lld values, LDS holds at most %d", who, n_r,
                  n_phi, (long long)n_r * n_phi, ORI_MAX_WORDS);
    if (n_templates < 1) LTMI_FAIL(LTMI_E_SHAPE, "%s: n_templates %d must be at least 1", who, n_templates);
    if (!tap_idx || !tap_w || !indptr) LTMI_FAIL(LTMI_E_INVALID, "%s: null pointer", who);
    const int n_points = n_r * n_phi, n_px = sig_h * sig_w;
    for (int64_t i = 0; i < (int64_t)n_points * 4; ++i) {
        if (tap_idx[i] < 0 || tap_idx[i] >= n_px)
            LTMI_FAIL(LTMI_E_SHAPE, "%s: tap_idx[%lld] = %d lies outside the %d pixels of a frame", who, (long long)i,
                      tap_idx[i], n_px);
        if (!std::isfinite(tap_w[i]))
            LTMI_FAIL(LTMI_E_SHAPE, "%s: tap_w[%lld] = %g is not finite", who, (long long)i, (double)tap_w[i]);
    }
    if (indptr[0] != 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: indptr[0] = %lld, not 0", who, (long long)indptr[0]);
    for (int t = 0; t < n_templates; ++t)
        if (indptr[t + 1] < indptr[t] || indptr[t + 1] > INT32_MAX)
            LTMI_FAIL(LTMI_E_SHAPE, "%s: indptr[%d] = %lld after %lld", who, t + 1, (long long)indptr[t + 1],
                      (long long)indptr[t]);
    const int64_t n_spots = indptr[n_templates];
    if (n_spots > 0 && (!spot_r || !spot_phi || !spot_w)) LTMI_FAIL(LTMI_E_INVALID, "%s: null pointer", who);
    ltmi_orient_plan *p = nullptr;
    try {
        std::vector<Spot> packed((size_t)n_spots);
        std::vector<int32_t> ptr32((size_t)n_templates + 1);
        for (int t = 0; t <= n_templates; ++t) ptr32[(size_t)t] = (int32_t)indptr[t];
        for (int64_t s = 0; s < n_spots; ++s) {
            if (spot_r[s] < 0 || spot_r[s] >= n_r)
                LTMI_FAIL(LTMI_E_SHAPE, "%s: spot_r[%lld] = %d lies outside [0, %d)", who, (long long)s, spot_r[s],
                          n_r);
            if (spot_phi[s] < 0 || spot_phi[s] >= n_phi)
                LTMI_FAIL(LTMI_E_SHAPE, "%s: spot_phi[%lld] = %d lies outside [0, %d)", who, (long long)s, spot_phi[s],
                          n_phi);
            if (!std::isfinite(spot_w[s]))
                LTMI_FAIL(LTMI_E_SHAPE, "%s: spot_w[%lld] = %g is not finite", who, (long long)s, (double)spot_w[s]);
            // (spot_r n_phi < 2^16 and spot_phi < 2^10: 26 bits)
            packed[(size_t)s] = Spot{((uint32_t)(spot_r[s] * n_phi) << 10) | (uint32_t)spot_phi[s], spot_w[s]};
        }
        LTMI_HIP(hipSetDevice(device));
        p = new ltmi_orient_plan();
        p->device = device;
        p->sig_h = sig_h, p->sig_w = sig_w, p->n_r = n_r, p->n_phi = n_phi;
        p->n_templates = n_templates, p->n_best = n_best;
        hipError_t e = p->tap_idx.upload((const int4 *)tap_idx, (size_t)n_points);
        if (e == hipSuccess) e = p->tap_w.upload((const float4 *)tap_w, (size_t)n_points);
        if (e == hipSuccess) e = p->indptr.upload(ptr32.data(), ptr32.size());
        // (an empty library still gets a block: the kernels take the pointer)
        if (e == hipSuccess) e = n_spots ? p->spots.upload(packed.data(), packed.size()) : p->spots.alloc_zero(1);
        if (e != hipSuccess) {
            delete p;
            LTMI_FAIL((int)e, "%s: uploading the tables failed: %s", who, hipGetErrorString(e));
        }
    } catch (const std::bad_alloc &) {
        delete p;
        LTMI_FAIL(LTMI_E_NOMEM, "%s: out of host memory", who);
    }
    *out = p;
    return LTMI_OK;
}

extern "C" int ltmi_orient_plan_destroy(ltmi_orient_plan *p) {
    if (!p) return LTMI_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return LTMI_OK;
}

extern "C" const char *ltmi_orient_plan_last_kernel(const ltmi_orient_plan *p) { return p ? p->last_kernel : ""; }

static int orient_args(const char *who, const ltmi_orient_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                       int64_t ld_tile, OrientArgs *a) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "%s: null plan", who);
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: n_frames is %lld", who, (long long)n_frames);
    if (ld_tile < (int64_t)p->sig_h * p->sig_w)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: ld_tile %lld < frame size %d", who, (long long)ld_tile, p->sig_h * p->sig_w);
    if (!dtype_in(tile_dtype, ORI_DTYPES))
        LTMI_FAIL(LTMI_E_DTYPE, "%s: tile dtype %s is not supported", who, dtype_name(tile_dtype));
    *a = OrientArgs{tile, n_frames, ld_tile, p->n_r * p->n_phi, p->n_phi, p->tap_idx.get(), p->tap_w.get()};
    return LTMI_OK;
}

extern "C" int ltmi_orient_polar(ltmi_orient_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                                 int64_t ld_tile, float *polar_out, int64_t ld_polar, void *stream_) {
    const char *who = "ltmi_orient_polar";
    OrientArgs a;
    const int rc = orient_args(who, p, tile, tile_dtype, n_frames, ld_tile, &a);
    if (rc != LTMI_OK) return rc;
    if (ld_polar < a.n_points)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: ld_polar %lld < polar image size %d", who, (long long)ld_polar, a.n_points);
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !polar_out) LTMI_FAIL(LTMI_E_INVALID, "%s: null pointer", who);
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned grid = (unsigned)std::min<int64_t>(n_frames, 8 * ORI_GRID);
    const int rd = dispatch_tile<ORI_DTYPES>(tile_dtype, [&](auto part) {
        typedef LTMI_PART_T(part) T;
        hipLaunchKernelGGL((k_orient_polar<T>), dim3(grid), dim3(256), 0, stream, a, polar_out, ld_polar);
        return LTMI_OK;
    });
    if (rd != LTMI_OK) return rd;
    LTMI_HIP(hipGetLastError());
    snprintf(p->last_kernel, sizeof(p->last_kernel), "k_orient_polar<%s>", dtype_name(tile_dtype));
    return LTMI_OK;
}

extern "C" int ltmi_orient_match(ltmi_orient_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                                 int64_t ld_tile, int32_t *template_out, int32_t *rotation_out, float *correlation_out,
                                 float *norm_out, void *stream_) {
    const char *who = "ltmi_orient_match";
    OrientArgs a;
    const int rc = orient_args(who, p, tile, tile_dtype, n_frames, ld_tile, &a);
    if (rc != LTMI_OK) return rc;
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !template_out || !rotation_out || !correlation_out || !norm_out)
        LTMI_FAIL(LTMI_E_INVALID, "%s: null pointer", who);
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const LibArgs lib{p->n_templates, p->n_best};
    const size_t smem = (size_t)((a.n_points + 1) & ~1) * 4 + ORI_LDS_OTHER;
    const unsigned grid = (unsigned)std::min<int64_t>(n_frames, ORI_GRID);
    const int nch = (p->n_phi + 63) / 64;
    const int rd = dispatch_tile<ORI_DTYPES>(tile_dtype, [&](auto part) {
        typedef LTMI_PART_T(part) T;
        switch (nch) {
#define LTMI_ORI_CASE(N)                                                                                         \
    case N:                                                                                                      \
        return launch_match<T, N>(p->device, grid, smem, stream, a, lib, p->indptr.get(), p->spots.get(),       \
                                  template_out, rotation_out, correlation_out, norm_out);
            LTMI_ORI_CASE(1) LTMI_ORI_CASE(2) LTMI_ORI_CASE(3) LTMI_ORI_CASE(4) LTMI_ORI_CASE(5) LTMI_ORI_CASE(6)
            LTMI_ORI_CASE(7) LTMI_ORI_CASE(8) LTMI_ORI_CASE(9) LTMI_ORI_CASE(10) LTMI_ORI_CASE(11) LTMI_ORI_CASE(12)
            LTMI_ORI_CASE(13) LTMI_ORI_CASE(14) LTMI_ORI_CASE(15) LTMI_ORI_CASE(16)
#undef LTMI_ORI_CASE
        }
        return (int)LTMI_E_SHAPE;
    });
    if (rd != LTMI_OK) return rd;
    LTMI_HIP(hipGetLastError());
    snprintf(p->last_kernel, sizeof(p->last_kernel), "k_orient_match<%s,%d> grid=%u lds=%zu", dtype_name(tile_dtype),
             nch, grid, smem);
    return LTMI_OK;
}
