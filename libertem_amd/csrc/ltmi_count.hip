// ltmi_count.hip -- electron events of dense frames: count them, then write them as CSR rows.
//
// Per frame of (h, w) pixels, p = y w + x, with float32 thresholds t_bg and t_x:
//   1. v[p] = float32(pixel[p]) (round to nearest even), then v - dark[p], then v * gain[p] (one float32 operation
//      each, where the array is given);
//   2. u[p] = v[p] if v[p] <= t_x, else 0 (NaN compares false and becomes 0);
//   3. p is an EVENT iff u[p] > t_bg and, over its up to 8 neighbours q inside the frame, u[p] > u[q] where q < p and
//      u[p] >= u[q] where q > p (of equal neighbours the first wins; no two events are adjacent);
//   4. the events of a frame in ascending p; their value is uint8(1) or u[p].
//
// One workgroup of 256 threads walks a frame in strips of up to CNT_MAX_STRIP rows.  A strip and its two halo rows are
// staged in LDS as float32 u, so steps 1 - 2 happen once per pixel (halo rows twice); the rows are CNT pitch floats
// apart with the pixels from column 4 on, and the cells around the frame -- column 3, column 4 + w, the row above the
// first and below the last -- hold -inf: u[p] > -inf fails only where u[p] = -inf, which is no event for any t_bg,
// and u[p] >= -inf always holds (u has no NaN), so the 3 x 3 test needs no edge cases.
//   stage   16 bytes of pixels per lane (the strip's rows are one contiguous run of the frame) where w is a multiple
//           of 4, written to LDS as float4; a pixel per lane otherwise (515 x 515 sensors).
//   test    a wave takes 64 columns of CNT_RUN rows at a time and slides down them: 3 LDS reads per pixel and step,
//           consecutive lanes on consecutive banks, and the maximum of each row's three cells is kept for the two
//           steps that need it (3 maxima and 2 comparisons per pixel).  The ballot of a row's 64 flags is one word
//           of the strip's event bitmap.
//   count   k_count_events only adds the popcounts: a sum per wave, one LDS reduction per frame.
//   store   k_store_events keeps the bitmap (rows x ceil(w / 64) words) in LDS, scans the popcounts of the words over
//           the workgroup, and then every set bit knows its rank: offset of the frame so far + prefix of its word +
//           set bits below it.  Indices come out ascending with no sort and no atomics on the data path; all-zero
//           words are skipped by whole waves.
// A frame's writes are confined to [indptr[f] - base, indptr[f + 1] - base) and [0, capacity); a frame whose events
// do not number indptr[f + 1] - indptr[f], or whose range leaves [0, capacity), ORs 1 into *status (a global atomic).
#include "ltmi_tiles.h"

namespace ltmi {
namespace {

constexpr int CNT_MAX_W = 4096;                               // three rows of the widest frame fit the LDS budget
constexpr int CNT_MAX_STRIP = 30;                             // rows per strip: halo traffic 2 / 30; with the halo, a
                                                              // strip of a 256-wide uint16 frame is 4 loads per lane
constexpr int CNT_BATCH = 4;                                  // pixel loads a lane has in flight while staging
constexpr int CNT_RUN = 8;                                    // rows a wave slides down per 64-column block
constexpr int cnt_pitch(int w) { return (w + 5 + 3) & ~3; }   // 4 cells in front (3 of them unused), 1 behind
constexpr int CNT_LDS_FLOATS = 3 * cnt_pitch(CNT_MAX_W);      // 48 KiB
constexpr unsigned CNT_DTYPES = DT_INT8_32 | dtype_bit(LTMI_F32);

struct CountArgs {
    const void *tile;
    int64_t n_frames, ld_tile;
    int h, w, strip, vec;
    const float *dark, *gain;
    float t_bg, t_x;
};

struct StoreArgs {
    const int64_t *indptr;
    int64_t base, capacity;
    int32_t *indices;
    void *values;
    int values_f32;
    int32_t *status;
};

__device__ __forceinline__ float cnt_u(float v, const float *dark, const float *gain, int p, float t_x) {
    if (dark) v = __fsub_rn(v, dark[p]);
    if (gain) v = __fmul_rn(v, gain[p]);
    return v <= t_x ? v : 0.f;
}

// rows [y0 - 1, y0 + rows + 1) of the frame `src` into LDS rows 0 .. rows + 1; rows outside the frame become -inf
template <typename T, int VEC>
__device__ __forceinline__ void cnt_stage(const T *__restrict__ src, const CountArgs &a, int y0, int rows, int pitch,
                                          float *__restrict__ lds) {
    const int w = a.w, tid = threadIdx.x;
    const float NEG = -__builtin_huge_valf();
    const int ya = max(y0 - 1, 0), yb = min(y0 + rows + 1, a.h);   // frame rows to load
    if (y0 == 0)
        for (int x = tid; x < w; x += 256) lds[4 + x] = NEG;
    if (y0 + rows == a.h)
        for (int x = tid; x < w; x += 256) lds[(rows + 1) * pitch + 4 + x] = NEG;
    const int first = ya * w, count = (yb - ya) * w;              // one contiguous run of the frame
    const int r_off = ya - (y0 - 1);                              // LDS row of frame row ya
    if (a.vec) {
        // w is a multiple of 4: a group of 4 pixels lies inside one row and on a 16-byte boundary of LDS
        typedef tile_vec_t<T, VEC> vec_t;
        typedef tile_vec_t<float, 4> f4_t;
        // (row, column) of a lane's first group by one division, of the next ones by adding the step's.  CNT_BATCH
        // pixel loads are issued before the first is used: a strip of a 256-wide frame is one batch per lane.
        constexpr int STEP = 256 * VEC, Q = VEC / 4;
        const int step_r = STEP / w, step_x = STEP - step_r * w;
        int r = tid * VEC / w, x = tid * VEC - r * w;
        for (int j0 = tid * VEC; j0 < count; j0 += CNT_BATCH * STEP) {
            vec_t v[CNT_BATCH];
#pragma unroll
            for (int b = 0; b < CNT_BATCH; ++b)
                if (j0 + b * STEP + VEC <= count) v[b] = *(const vec_t *)(src + first + j0 + b * STEP);
#pragma unroll
            for (int b = 0; b < CNT_BATCH; ++b) {
                const int j = j0 + b * STEP;
                if (j >= count) break;
                f4_t d[Q], g[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (a.dark && j + 4 * q < count) d[q] = *(const f4_t *)(a.dark + first + j + 4 * q);
                    if (a.gain && j + 4 * q < count) g[q] = *(const f4_t *)(a.gain + first + j + 4 * q);
                }
                T px[VEC];
                if (j + VEC <= count) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) px[k] = v[b][k];
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) px[k] = j + k < count ? src[first + j + k] : T(0);
                }
                int rq = r, xq = x;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    if (j + 4 * q >= count) break;
                    float4 u = make_float4((float)px[4 * q], (float)px[4 * q + 1], (float)px[4 * q + 2],
                                           (float)px[4 * q + 3]);
                    if (a.dark) {
                        u.x = __fsub_rn(u.x, d[q][0]);
                        u.y = __fsub_rn(u.y, d[q][1]);
                        u.z = __fsub_rn(u.z, d[q][2]);
                        u.w = __fsub_rn(u.w, d[q][3]);
                    }
                    if (a.gain) {
                        u.x = __fmul_rn(u.x, g[q][0]);
                        u.y = __fmul_rn(u.y, g[q][1]);
                        u.z = __fmul_rn(u.z, g[q][2]);
                        u.w = __fmul_rn(u.w, g[q][3]);
                    }
                    u.x = u.x <= a.t_x ? u.x : 0.f;
                    u.y = u.y <= a.t_x ? u.y : 0.f;
                    u.z = u.z <= a.t_x ? u.z : 0.f;
                    u.w = u.w <= a.t_x ? u.w : 0.f;
                    *(float4 *)(lds + (rq + r_off) * pitch + 4 + xq) = u;
                    xq += 4;                                    // (x and w are multiples of 4: at most w)
                    if (xq == w) xq = 0, ++rq;
                }
                r += step_r, x += step_x;
                if (x >= w) x -= w, ++r;
            }
        }
    } else {
        for (int j = tid; j < count; j += 256) {
            const int r = j / w, x = j - r * w;
            lds[(r + r_off) * pitch + 4 + x] = cnt_u((float)src[first + j], a.dark, a.gain, first + j, a.t_x);
        }
    }
}

// the 3 x 3 test on the staged strip: -> this wave's events; with STORE, bitmap word (row, 64-column block) = ballot
template <bool STORE>
__device__ __forceinline__ int cnt_test(const float *__restrict__ lds, int rows, int w, int pitch, int wpr, float t_bg,
                                        uint64_t *__restrict__ words) {
    // (the wave's number as a scalar: the loops over its items and rows are uniform, their counters and the row
    //  offsets live in scalar registers)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_runs = (rows + CNT_RUN - 1) / CNT_RUN;
    int found = 0;
    for (int item = wave; item < n_runs * wpr; item += 4) {
        const int g = item / wpr, c = item - g * wpr;
        const int i0 = g * CNT_RUN, i1 = min(rows, i0 + CNT_RUN);
        const int x = c * 64 + lane;
        const bool active = x < w;
        const float *col = lds + 4 + (active ? x : 0);            // (idle lanes read column 0: inside the strip)
        // ha, hb: the largest of the three cells above / beside-and-at the pixel's column, row by row (u has no NaN,
        // so the maxima are exact): the pixel beats its earlier neighbours iff it exceeds max(ha, left), and the later
        // ones iff it reaches max(right, the three below)
        float ha = fmaxf(fmaxf(col[i0 * pitch - 1], col[i0 * pitch]), col[i0 * pitch + 1]);
        float b0 = col[(i0 + 1) * pitch - 1], b1 = col[(i0 + 1) * pitch], b2 = col[(i0 + 1) * pitch + 1];
        float hb = fmaxf(fmaxf(b0, b1), b2);
        for (int i = i0; i < i1; ++i) {
            const float *below = col + (i + 2) * pitch;
            const float c0 = below[-1], c1 = below[0], c2 = below[1];
            const float hc = fmaxf(fmaxf(c0, c1), c2);
            const float before = fmaxf(fmaxf(ha, b0), t_bg), after = fmaxf(hc, b2);
            const bool ev = active && b1 > before && b1 >= after;
            const unsigned long long m = __ballot(ev);
            found += __popcll(m);
            if (STORE && lane == 0) words[i * wpr + c] = m;
            ha = hb, hb = hc;
            b0 = c0, b1 = c1, b2 = c2;
        }
    }
    return found;
}

// the -inf columns left and right of the frame: written once, no strip overwrites them
__device__ __forceinline__ void cnt_pad_columns(float *lds, int strip, int w, int pitch) {
    const float NEG = -__builtin_huge_valf();
    for (int r = threadIdx.x; r < strip + 2; r += 256) {
        lds[r * pitch + 3] = NEG;
        lds[r * pitch + 4 + w] = NEG;
    }
}

template <typename T, int VEC>
__global__ void __launch_bounds__(256)
k_count_events(CountArgs a, int32_t *__restrict__ n_events) {
    extern __shared__ __align__(16) unsigned char cnt_smem[];      // all of the kernel's LDS: the base stays 16-byte aligned
    float *lds = (float *)cnt_smem;
    const int pitch = cnt_pitch(a.w), wpr = (a.w + 63) / 64;
    int *sh_found = (int *)(lds + (a.strip + 2) * pitch);
    cnt_pad_columns(lds, a.strip, a.w, pitch);
    for (int64_t f = blockIdx.x; f < a.n_frames; f += gridDim.x) {
        const T *src = (const T *)a.tile + f * a.ld_tile;
        int found = 0;
        for (int y0 = 0; y0 < a.h; y0 += a.strip) {
            const int rows = min(a.strip, a.h - y0);
            __syncthreads();                                    // the last strip's test is done with LDS
            cnt_stage<T, VEC>(src, a, y0, rows, pitch, lds);
            __syncthreads();
            found += cnt_test<false>(lds, rows, a.w, pitch, wpr, a.t_bg, nullptr);
        }
        if ((threadIdx.x & 63) == 0) sh_found[threadIdx.x >> 6] = found;
        __syncthreads();
        if (threadIdx.x == 0) n_events[f] = sh_found[0] + sh_found[1] + sh_found[2] + sh_found[3];
        // (sh_found is rewritten after the two barriers of the next frame's first strip)
    }
}

template <typename T, int VEC>
__global__ void __launch_bounds__(256)
k_store_events(CountArgs a, StoreArgs s, int n_words_max) {
    extern __shared__ __align__(16) unsigned char cnt_smem[];
    const int pitch = cnt_pitch(a.w), wpr = (a.w + 63) / 64;
    float *lds = (float *)cnt_smem;
    uint64_t *words = (uint64_t *)(lds + (a.strip + 2) * pitch);      // (pitch is a multiple of 4: 16-byte aligned)
    int *prefix = (int *)(words + n_words_max);
    int *sh_sum = prefix + n_words_max;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    cnt_pad_columns(lds, a.strip, a.w, pitch);
    for (int64_t f = blockIdx.x; f < a.n_frames; f += gridDim.x) {
        const T *src = (const T *)a.tile + f * a.ld_tile;
        // this frame's range of the outputs: rank k goes to lo + k where that lies in [wlo, whi), the part of
        // [indptr[f] - base, indptr[f + 1] - base) inside [0, capacity)
        const int64_t p0 = s.indptr[f], p1 = s.indptr[f + 1];
        int64_t lo = 0, hi = 0, claimed = 0;
        const bool ovf = __builtin_sub_overflow(p0, s.base, &lo) || __builtin_sub_overflow(p1, s.base, &hi) ||
                         __builtin_sub_overflow(p1, p0, &claimed);
        const bool bad = ovf || hi < lo || lo < 0 || hi > s.capacity;
        int64_t wlo = 0, whi = 0;
        if (!ovf && hi >= lo && lo < s.capacity) {              // (lo < capacity <= 2^60: lo + k cannot overflow)
            wlo = lo > 0 ? lo : 0;
            whi = hi < s.capacity ? hi : s.capacity;
        } else {
            lo = 0;
        }
        int done = 0;                                           // events of the strips before this one
        for (int y0 = 0; y0 < a.h; y0 += a.strip) {
            const int rows = min(a.strip, a.h - y0);
            __syncthreads();                                    // the last strip's writers are done with LDS
            cnt_stage<T, VEC>(src, a, y0, rows, pitch, lds);
            __syncthreads();
            cnt_test<true>(lds, rows, a.w, pitch, wpr, a.t_bg, words);
            __syncthreads();
            // exclusive scan of the words' popcounts, 256 words at a time
            const int n_words = rows * wpr;
            int carry = 0;
            for (int t0 = 0; t0 < n_words; t0 += 256) {
                const int t = t0 + tid;
                const int mine = t < n_words ? __popcll(words[t]) : 0;
                int incl = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                if (lane == 63) sh_sum[wave] = incl;
                __syncthreads();
                int before = carry;
                for (int j = 0; j < wave; ++j) before += sh_sum[j];
                if (t < n_words) prefix[t] = before + incl - mine;
                carry += sh_sum[0] + sh_sum[1] + sh_sum[2] + sh_sum[3];
                __syncthreads();
            }
            // every set bit to its place
            for (int t0 = wave * 64; t0 < n_words; t0 += 256) {
                // a word per lane, then the wave walks the words that hold an event
                unsigned long long busy = __ballot(t0 + lane < n_words && words[t0 + lane] != 0);
                while (busy) {
                    const int t = t0 + __ffsll((long long)busy) - 1;
                    busy &= busy - 1;
                    const unsigned long long m = words[t];
                    if ((m >> lane) & 1) {
                        const int r = t / wpr, x = (t - r * wpr) * 64 + lane;
                        const int64_t rank = (int64_t)done + prefix[t] + __popcll(m & ((1ull << lane) - 1));
                        const int64_t at = lo + rank;
                        if (at >= wlo && at < whi) {
                            s.indices[at] = (y0 + r) * a.w + x;
                            if (s.values) {
                                if (s.values_f32) ((float *)s.values)[at] = lds[(r + 1) * pitch + 4 + x];
                                else ((uint8_t *)s.values)[at] = 1;
                            }
                        }
                    }
                }
            }
            done += carry;
        }
        if (tid == 0 && (bad || (int64_t)done != claimed)) atomicOr(s.status, 1);
    }
}

thread_local const char *t_last_kernel = "";

int count_args(const char *who, const void *tile, int tile_dtype, int64_t n_frames, int h, int w, int64_t ld_tile,
               const float *dark, const float *gain, float t_bg, float t_x, CountArgs *a) {
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: n_frames is %lld", who, (long long)n_frames);
    if (h < 1 || w < 1 || (int64_t)h * w > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: frames of %d x %d (1 to 2^31 - 1 pixels each)", who, h, w);
    if (w > CNT_MAX_W) LTMI_FAIL(LTMI_E_SHAPE, "%s: frames of %d columns, counting takes at most %d", who, w, CNT_MAX_W);
    if (ld_tile < (int64_t)h * w) LTMI_FAIL(LTMI_E_SHAPE, "%s: ld_tile < frame size", who);
    if (t_bg != t_bg || t_x != t_x) LTMI_FAIL(LTMI_E_SHAPE, "%s: a threshold is NaN", who);
    if (!dtype_in(tile_dtype, CNT_DTYPES))
        LTMI_FAIL(LTMI_E_DTYPE, "%s: tile dtype %s is not supported", who, dtype_name(tile_dtype));
    const int strip = std::max(1, std::min({CNT_MAX_STRIP, h, CNT_LDS_FLOATS / cnt_pitch(w) - 2}));
    const size_t elem = (size_t)dtype_size(tile_dtype);
    const bool vec = w % 4 == 0 && vector_loads_ok(tile, ld_tile, elem) && (!dark || vector_loads_ok(dark, 4, 4)) &&
                     (!gain || vector_loads_ok(gain, 4, 4));
    *a = CountArgs{tile, n_frames, ld_tile, h, w, strip, vec ? 1 : 0, dark, gain, t_bg, t_x};
    return LTMI_OK;
}

unsigned count_grid(int64_t n_frames) { return (unsigned)std::min<int64_t>(n_frames, 1 << 20); }

}  // namespace
}  // namespace ltmi

using namespace ltmi;

extern "C" int ltmi_count_strip_rows(int h, int w) {
    if (h < 1 || w < 1 || w > CNT_MAX_W) return 0;
    return std::max(1, std::min({CNT_MAX_STRIP, h, CNT_LDS_FLOATS / cnt_pitch(w) - 2}));
}

extern "C" const char *ltmi_count_last_kernel(void) { return t_last_kernel; }

extern "C" int ltmi_count_events(int device, const void *tile, int tile_dtype, int64_t n_frames, int h, int w,
                                 int64_t ld_tile, const float *dark, const float *gain, float t_bg, float t_x,
                                 int32_t *n_events, void *stream_) {
    CountArgs a;
    const int rc = count_args("ltmi_count_events", tile, tile_dtype, n_frames, h, w, ld_tile, dark, gain, t_bg, t_x, &a);
    if (rc != LTMI_OK) return rc;
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !n_events) LTMI_FAIL(LTMI_E_INVALID, "ltmi_count_events: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    const size_t smem = (size_t)(a.strip + 2) * cnt_pitch(w) * sizeof(float) + 4 * sizeof(int);
    const int rd = dispatch_tile<CNT_DTYPES>(tile_dtype, [&](auto part) {
        typedef LTMI_PART_T(part) T;
        constexpr int VEC = sizeof(T) == 1 ? 8 : 16 / (int)sizeof(T);     // (8 pixels of a byte each: the registers of 16)
        hipLaunchKernelGGL((k_count_events<T, VEC>), dim3(count_grid(n_frames)), dim3(256), smem, stream, a, n_events);
        return LTMI_OK;
    });
    if (rd != LTMI_OK) return rd;
    LTMI_HIP(hipGetLastError());
    t_last_kernel = a.vec ? "k_count_events vec" : "k_count_events";
    return LTMI_OK;
}

extern "C" int ltmi_store_events(int device, const void *tile, int tile_dtype, int64_t n_frames, int h, int w,
                                 int64_t ld_tile, const float *dark, const float *gain, float t_bg, float t_x,
                                 const int64_t *indptr, int64_t base, int64_t capacity, int32_t *indices_out,
                                 void *values_out, int values_dtype, int32_t *status, void *stream_) {
    CountArgs a;
    const int rc = count_args("ltmi_store_events", tile, tile_dtype, n_frames, h, w, ld_tile, dark, gain, t_bg, t_x, &a);
    if (rc != LTMI_OK) return rc;
    if (capacity < 0 || capacity > INT64_MAX / 8)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_store_events: capacity %lld", (long long)capacity);
    if (values_dtype != LTMI_U8 && values_dtype != LTMI_F32)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_store_events: values of dtype %s (uint8 or float32)", dtype_name(values_dtype));
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !indptr || !indices_out || !status) LTMI_FAIL(LTMI_E_INVALID, "ltmi_store_events: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    const int n_words = a.strip * ((w + 63) / 64);
    const size_t smem = (size_t)(a.strip + 2) * cnt_pitch(w) * sizeof(float) + (size_t)n_words * (8 + 4) + 4 * sizeof(int);
    if (smem > 64 * 1024) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_store_events: %zu bytes of LDS for frames of %d columns", smem, w);
    const StoreArgs s{indptr, base, capacity, indices_out, values_out, values_dtype == LTMI_F32 ? 1 : 0, status};
    const int rd = dispatch_tile<CNT_DTYPES>(tile_dtype, [&](auto part) {
        typedef LTMI_PART_T(part) T;
        constexpr int VEC = sizeof(T) == 1 ? 8 : 16 / (int)sizeof(T);     // (8 pixels of a byte each: the registers of 16)
        hipLaunchKernelGGL((k_store_events<T, VEC>), dim3(count_grid(n_frames)), dim3(256), smem, stream, a, s, n_words);
        return LTMI_OK;
    });
    if (rd != LTMI_OK) return rd;
    LTMI_HIP(hipGetLastError());
    t_last_kernel = a.vec ? "k_store_events vec" : "k_store_events";
    return LTMI_OK;
}
