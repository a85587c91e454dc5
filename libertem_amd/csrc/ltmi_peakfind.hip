// ltmi_peakfind.hip -- the strongest local maxima of correlation maps.
//
// Per map c of (h, w) float32, with N = num_peaks, d = min_distance, b = border:
//   1. p is a CANDIDATE iff it beats every other pixel p' of its (2d+1)^2 neighbourhood clipped to the frame:
//      c[p] > c[p'] where p' precedes p in row-major order, c[p] >= c[p'] where it follows;
//   2. a candidate is ELIGIBLE iff b <= y < h - b, b <= x < w - b and c[p] > threshold_abs;
//   3. the eligible candidates ordered by value descending, then index ascending; with v0 the first value and
//      v0 > 0, those with c[p] < float32(threshold_rel) * v0 go; the first N of the rest are kept;
//   4. / 5. their window statistics by k_corr_found (ltmi_corr.hip), (-1, -1) and NaN in the other slots;
//   6. a map with a non-finite value keeps nothing.
//
// Everything is decided on ONE 64-bit key per pixel: the order-preserving bits of the value (-0 as +0) above the
// complement of the row-major index.  "p' beats p" is key(p') > key(p), and a larger key comes first in step 3.  The
// key of a non-finite value is all ones ("poison"): it wins every maximum and so reaches the selection by itself.
//
// The frame is cut into aligned (d+1) x (d+1) cells.  Two candidates are more than d apart, so a cell holds at most
// one -- its maximum key --, and every cell owns a slot: no atomics, no compaction of unknown size.
//   k_pf_cells   a workgroup per run of cell rows: column maxima of the keys into LDS (each value is read once,
//                coalesced, 16 bytes per lane where the rows allow), then one thread per cell takes the maximum of
//                its d+1 columns.
//   k_pf_verify  eight lanes per cell, one per neighbouring cell: a neighbour whose maximum is smaller cannot beat the
//                cell's maximum p; one whose maximum is larger AND within d of p beats it; only a larger maximum
//                farther than d away makes the eight lanes scan the part of that cell inside p's neighbourhood.
//                Survivors keep their key, the others get 0.
//   k_pf_select  a workgroup per frame: largest eligible key -> v0 and the relative threshold; the keys that pass are
//                packed into LDS by ballot prefix sums and each is ranked by counting the larger ones; rank < N is
//                its slot.  Where more than PF_CAP keys pass, the N-th largest key is first found by bisection on
//                the key's 64 bits (keys are distinct, so exactly N remain).
// The results of a call repeat bit for bit.
#include "ltmi_common.h"

namespace ltmi {

constexpr int PF_CAP = 4096;            // keys ranked in LDS (32 KiB)
constexpr int PF_MAX_PEAKS = 1024;      // <= PF_CAP: what the bisection leaves must fit
constexpr int PF_MAX_W = 8192;          // column keys of one cell row in LDS (64 KiB)
constexpr int PF_LPC = 8;               // lanes per cell of k_pf_verify
constexpr uint64_t PF_POISON = ~0ull;

__device__ __forceinline__ uint64_t pf_key(float v, uint32_t idx) {
    if (!(fabsf(v) <= 3.402823466e+38f)) return PF_POISON;
    v = v == 0.f ? 0.f : v;
    uint32_t u = __float_as_uint(v);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
    return ((uint64_t)u << 32) | (uint32_t)~idx;
}

__device__ __forceinline__ float pf_value(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u >> 31) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ uint32_t pf_index(uint64_t key) { return ~(uint32_t)key; }

// rows_per_wg cell rows per workgroup, their column maxima in LDS: (rows_per_wg, w) keys.  A work item is one column of
// one cell row -- or, with `vec`, four columns read as one 16-byte load per pixel row (w a multiple of 4, maps and
// ld_map 16-byte aligned) --, so that a narrow frame still fills the workgroup.
__global__ void __launch_bounds__(256)
k_pf_cells(const float *__restrict__ maps, int64_t ld_map, int h, int w, int d1, int ncy, int ncx, int rows_per_wg,
           int vec, uint64_t *__restrict__ cellmax) {
    extern __shared__ __align__(16) unsigned char pf_smem[];
    uint64_t *col = (uint64_t *)pf_smem;                     // (rows_per_wg, w)
    const float *c = maps + (int64_t)blockIdx.y * ld_map;
    uint64_t *out = cellmax + (int64_t)blockIdx.y * ncy * ncx;
    const int cr0 = (int)blockIdx.x * rows_per_wg;
    const int n_cr = min(ncy - cr0, rows_per_wg);
    const int per_row = vec ? w / 4 : w;
    for (int item = threadIdx.x; item < n_cr * per_row; item += 256) {
        const int r = item / per_row, xi = item - r * per_row;
        const int y0 = (cr0 + r) * d1, y1 = min(h, y0 + d1);
        if (vec) {
            const int x = 4 * xi;
            uint64_t k0 = 0, k1 = 0, k2 = 0, k3 = 0;
            for (int y = y0; y < y1; ++y) {
                const uint32_t i = (uint32_t)y * (uint32_t)w + (uint32_t)x;
                const float4 v = *(const float4 *)(c + i);
                const uint64_t a0 = pf_key(v.x, i), a1 = pf_key(v.y, i + 1), a2 = pf_key(v.z, i + 2),
                               a3 = pf_key(v.w, i + 3);
                k0 = a0 > k0 ? a0 : k0;
                k1 = a1 > k1 ? a1 : k1;
                k2 = a2 > k2 ? a2 : k2;
                k3 = a3 > k3 ? a3 : k3;
            }
            uint64_t *dst = col + (int64_t)r * w + x;
            dst[0] = k0;
            dst[1] = k1;
            dst[2] = k2;
            dst[3] = k3;
        } else {
            uint64_t k = 0;
            for (int y = y0; y < y1; ++y) {
                const uint32_t i = (uint32_t)y * (uint32_t)w + (uint32_t)xi;
                const uint64_t ki = pf_key(c[i], i);
                k = ki > k ? ki : k;
            }
            col[(int64_t)r * w + xi] = k;
        }
    }
    __syncthreads();
    for (int item = threadIdx.x; item < n_cr * ncx; item += 256) {
        const int r = item / ncx, cx = item - r * ncx;
        const int x0 = cx * d1, x1 = min(w, x0 + d1);
        const uint64_t *src = col + (int64_t)r * w;
        uint64_t k = 0;
        for (int x = x0; x < x1; ++x) k = src[x] > k ? src[x] : k;
        out[(int64_t)(cr0 + r) * ncx + cx] = k;
    }
}

// Eight lanes per cell.  Lane j first looks at neighbouring cell j alone (see the head of the file) and either settles
// it or asks for a scan; unless one of them has found the cell's maximum beaten already, the eight lanes then scan
// every asked-for part together, a pixel per lane and step, with no exit inside a part, so that the loads of a scan
// are in flight together.
__global__ void __launch_bounds__(256)
k_pf_verify(const float *__restrict__ maps, int64_t ld_map, int h, int w, int d, int ncy, int ncx,
            const uint64_t *__restrict__ cellmax, uint64_t *__restrict__ cand) {
    __shared__ unsigned char verdict[256];                  // 1: beaten, 2: poison
    const int64_t n_cells = (int64_t)ncy * ncx;
    const int64_t ci = (int64_t)blockIdx.x * (256 / PF_LPC) + threadIdx.x / PF_LPC;
    const int l = threadIdx.x % PF_LPC;
    const bool active = ci < n_cells;
    const float *c = maps + (int64_t)blockIdx.y * ld_map;
    const uint64_t *cm = cellmax + (int64_t)blockIdx.y * n_cells;
    const int d1 = d + 1;
    int v = 0, scan = 0, py = 0, px = 0, cy = 0, cx = 0;
    uint64_t kp = 0;
    if (active) {
        kp = cm[ci];
        if (kp == PF_POISON) {
            v = 2;
        } else {
            const int pi = (int)pf_index(kp);
            py = pi / w;
            px = pi - py * w;
            cy = (int)(ci / ncx);
            cx = (int)(ci - (int64_t)cy * ncx);
            const int j = l + (l >= 4);                     // 0..8 without the cell itself
            const int ny = cy + j / 3 - 1, nx = cx + j % 3 - 1;
            if (ny >= 0 && ny < ncy && nx >= 0 && nx < ncx) {
                const uint64_t km = cm[(int64_t)ny * ncx + nx];
                if (km == PF_POISON) {
                    v = 2;
                } else if (km > kp) {
                    const int mi = (int)pf_index(km), my = mi / w, mx = mi - my * w;
                    if (abs(my - py) <= d && abs(mx - px) <= d) v = 1;
                    else scan = 1;
                }
            }
        }
    }
    // (every lane of the wave is here: the ballots are taken outside the branches)
    const int shift = threadIdx.x & 63 & ~(PF_LPC - 1);
    const unsigned group = (1u << PF_LPC) - 1;
    const unsigned long long asked = __ballot(scan), settled = __ballot(v != 0);
    // a cell that one of its lanes has settled already needs no scan
    unsigned todo = ((unsigned)(settled >> shift) & group) ? 0u : (unsigned)(asked >> shift) & group;
    while (todo) {
        const int lj = __ffs(todo) - 1;
        todo &= todo - 1;
        const int j = lj + (lj >= 4);
        const int ny = cy + j / 3 - 1, nx = cx + j % 3 - 1;
        // the part of the neighbouring cell inside p's neighbourhood
        const int ya = max(ny * d1, py - d), yb = min(min(ny * d1 + d, h - 1), py + d);
        const int xa = max(nx * d1, px - d), xb = min(min(nx * d1 + d, w - 1), px + d);
        if (ya > yb || xa > xb) continue;
        const int ww = xb - xa + 1, cnt = ww * (yb - ya + 1);
        for (int i = l; i < cnt; i += PF_LPC) {
            const int yy = i / ww;
            const uint32_t at = (uint32_t)(ya + yy) * (uint32_t)w + (uint32_t)(xa + i - yy * ww);
            v |= pf_key(c[at], at) > kp;
        }
        // (the lanes of a cell run this loop together; those of other cells that have left it count as 0)
        if ((unsigned)(__ballot(v != 0) >> shift) & group) break;
    }
    verdict[threadIdx.x] = (unsigned char)v;
    __syncthreads();
    if (active && l == 0) {
        int any = 0;
#pragma unroll
        for (int i = 0; i < PF_LPC; ++i) any |= verdict[threadIdx.x + i];
        cand[(int64_t)blockIdx.y * n_cells + ci] = (any & 2) ? PF_POISON : (any ? 0ull : kp);
    }
}

__device__ __forceinline__ uint64_t pf_block_max(uint64_t v, uint64_t *sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint64_t a = sh[0] > sh[1] ? sh[0] : sh[1], b = sh[2] > sh[3] ? sh[2] : sh[3];
    __syncthreads();
    return a > b ? a : b;
}

__device__ __forceinline__ int pf_block_sum(int v, int *sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(256)
k_pf_select(const uint64_t *__restrict__ cand, int64_t n_cells, int h, int w, int n_peaks, int b, float thr_abs,
            float thr_rel, int32_t *__restrict__ n_found, int32_t *__restrict__ centers) {
    __shared__ uint64_t list[PF_CAP];
    __shared__ uint64_t sh_k[4];
    __shared__ int sh_i[4];
    const int64_t f = blockIdx.x;
    const uint64_t *keys = cand + f * n_cells;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto eligible = [&](uint64_t k) {
        if (k == 0) return false;
        const int i = (int)pf_index(k), y = i / w, x = i - y * w;
        return y >= b && y < h - b && x >= b && x < w - b && pf_value(k) > thr_abs;
    };
    uint64_t best = 0;
    for (int64_t i = tid; i < n_cells; i += 256) {
        const uint64_t k = keys[i];
        if (k == PF_POISON || (eligible(k) && k > best)) best = k;
    }
    best = pf_block_max(best, sh_k);
    if (best == PF_POISON || best == 0) {                   // a non-finite value, or nothing eligible
        if (tid == 0) n_found[f] = 0;
        return;
    }
    const float v0 = pf_value(best);
    const bool rel = v0 > 0.f;
    const float t = thr_rel * v0;
    auto passes = [&](uint64_t k) { return eligible(k) && !(rel && pf_value(k) < t); };
    int cnt = 0;
    for (int64_t i = tid; i < n_cells; i += 256) cnt += passes(keys[i]);
    const int n_pass = pf_block_sum(cnt, sh_i);
    uint64_t floor_key = 0;
    if (n_pass > PF_CAP) {
        // the N-th largest passing key, bit by bit from the top: the largest value that N keys reach
        for (int bit = 63; bit >= 0; --bit) {
            const uint64_t trial = floor_key | (1ull << bit);
            cnt = 0;
            for (int64_t i = tid; i < n_cells; i += 256) {
                const uint64_t k = keys[i];
                cnt += k >= trial && passes(k);
            }
            if (pf_block_sum(cnt, sh_i) >= n_peaks) floor_key = trial;
        }
    }
    int n_list = 0;
    for (int64_t i0 = 0; i0 < n_cells; i0 += 256) {
        const int64_t i = i0 + tid;
        const uint64_t k = i < n_cells ? keys[i] : 0;
        const bool take = k >= floor_key && passes(k);
        const unsigned long long m = __ballot(take);
        if (lane == 0) sh_i[wave] = __popcll(m);
        __syncthreads();
        int at = n_list + __popcll(m & ((1ull << lane) - 1));
        for (int j = 0; j < wave; ++j) at += sh_i[j];
        if (take && at < PF_CAP) list[at] = k;
        n_list += sh_i[0] + sh_i[1] + sh_i[2] + sh_i[3];
        __syncthreads();
    }
    n_list = min(n_list, PF_CAP);
    for (int i = tid; i < n_list; i += 256) {
        const uint64_t me = list[i];
        int rank = 0;
        for (int j = 0; j < n_list; ++j) rank += list[j] > me;
        if (rank < n_peaks) {
            const int p = (int)pf_index(me), y = p / w;
            centers[2 * (f * n_peaks + rank)] = y;
            centers[2 * (f * n_peaks + rank) + 1] = p - y * w;
        }
    }
    if (tid == 0) n_found[f] = min(n_list, n_peaks);
}

namespace {
thread_local const char *t_last_kernel = "";
// the scratch of ltmi_find_peaks_maps: per calling thread, for the device and the stream of its last call
struct MapsScratch {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf<uint64_t> keys;
};
thread_local MapsScratch t_scratch;
}  // namespace

const char *peakfind_kernels() { return "k_pf_cells + k_pf_verify + k_pf_select + k_corr_found"; }

int peakfind_params(const char *who, int h, int w, int num_peaks, int min_distance, int border, float threshold_abs,
                    float threshold_rel, int refine_radius, PeakFind *out) {
    if (h <= 0 || w <= 0 || (int64_t)h * w > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: maps of %d x %d (at most 2^31 - 1 values each)", who, h, w);
    if (w > PF_MAX_W) LTMI_FAIL(LTMI_E_SHAPE, "%s: maps of %d columns, the search takes at most %d", who, w, PF_MAX_W);
    if (num_peaks < 1 || num_peaks > PF_MAX_PEAKS)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: num_peaks %d must lie in [1, %d]", who, num_peaks, PF_MAX_PEAKS);
    if (min_distance < 1 || refine_radius < 1)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: min_distance %d and refine_radius %d must be at least 1", who, min_distance,
                  refine_radius);
    if (border < 0 || 2 * (int64_t)border >= std::min(h, w))
        LTMI_FAIL(LTMI_E_SHAPE, "%s: border %d must be at least 0 and leave a pixel of %d x %d", who, border, h, w);
    if (!(threshold_rel >= 0.f && threshold_rel <= 1.f))
        LTMI_FAIL(LTMI_E_SHAPE, "%s: threshold_rel %g must lie in [0, 1]", who, (double)threshold_rel);
    if (threshold_abs != threshold_abs) LTMI_FAIL(LTMI_E_SHAPE, "%s: threshold_abs is NaN", who);
    // (neighbourhoods and windows are clipped to the frame: a radius beyond its longer edge changes nothing)
    out->n_peaks = num_peaks;
    out->d = std::min(min_distance, std::max(h, w));
    out->border = border;
    out->q = std::min(refine_radius, std::max(h, w));
    out->threshold_abs = threshold_abs;
    out->threshold_rel = threshold_rel;
    return LTMI_OK;
}

int peakfind_search(const float *maps, int64_t n_frames, int h, int w, int64_t ld_map, const PeakFind &pf,
                    DevBuf<uint64_t> &scratch, int32_t *n_found, int32_t *centers, float *refineds,
                    float *peak_values, float *peak_elevations, hipStream_t stream) {
    const int d1 = pf.d + 1;
    const int ncy = (h + d1 - 1) / d1, ncx = (w + d1 - 1) / d1;
    const int64_t n_cells = (int64_t)ncy * ncx;
    // 16-byte loads where every pixel row of every map starts on a 16-byte boundary
    const int vec = w % 4 == 0 && ld_map % 4 == 0 && (uintptr_t)maps % 16 == 0;
    // cell rows per workgroup: enough work items for its 256 threads, what fits 64 KiB of column keys
    const int per_row = vec ? w / 4 : w;
    const int rows_per_wg = std::max(1, std::min({(256 + per_row - 1) / per_row, PF_MAX_W / w, ncy}));
    // frames per launch: grid.y, and at most 2^24 cells (256 MiB of keys) at a time
    const int64_t chunk =
        std::min<int64_t>(std::min<int64_t>(n_frames, 32768), std::max<int64_t>(1, (1 << 24) / n_cells));
    const int rc = scratch.ensure((size_t)(2 * chunk * n_cells), stream);
    if (rc != LTMI_OK) return rc;
    uint64_t *cellmax = scratch, *cand = scratch + chunk * n_cells;
    const int64_t N = pf.n_peaks;
    for (int64_t f0 = 0; f0 < n_frames; f0 += chunk) {
        const int64_t n = std::min(chunk, n_frames - f0);
        const float *m = maps + f0 * ld_map;
        hipLaunchKernelGGL(k_pf_cells, dim3((unsigned)((ncy + rows_per_wg - 1) / rows_per_wg), (unsigned)n), dim3(256),
                           (size_t)rows_per_wg * w * sizeof(uint64_t), stream, m, ld_map, h, w, d1, ncy, ncx,
                           rows_per_wg, vec, cellmax);
        LTMI_HIP(hipGetLastError());
        const int64_t per_wg = 256 / PF_LPC;
        hipLaunchKernelGGL(k_pf_verify, dim3((unsigned)((n_cells + per_wg - 1) / per_wg), (unsigned)n), dim3(256), 0,
                           stream, m, ld_map, h, w, pf.d, ncy, ncx, (const uint64_t *)cellmax, cand);
        LTMI_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_pf_select, dim3((unsigned)n), dim3(256), 0, stream, (const uint64_t *)cand, n_cells, h, w,
                           pf.n_peaks, pf.border, pf.threshold_abs, pf.threshold_rel, n_found + f0,
                           centers + 2 * f0 * N);
        LTMI_HIP(hipGetLastError());
        const int rs = corr_found_stats(m, n, h, w, ld_map, pf, n_found + f0, centers + 2 * f0 * N,
                                        refineds + 2 * f0 * N, peak_values + f0 * N, peak_elevations + f0 * N, stream);
        if (rs != LTMI_OK) return rs;
    }
    return LTMI_OK;
}

}  // namespace ltmi

using namespace ltmi;

extern "C" int ltmi_find_peaks_maps(int device, const float *maps, int64_t n_frames, int h, int w, int64_t ld_map,
                                    int num_peaks, int min_distance, int border, float threshold_abs,
                                    float threshold_rel, int refine_radius, int32_t *n_found, int32_t *centers,
                                    float *refineds, float *peak_values, float *peak_elevations, void *stream_) {
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_find_peaks_maps: negative frame count");
    PeakFind pf;
    const int rc = peakfind_params("ltmi_find_peaks_maps", h, w, num_peaks, min_distance, border, threshold_abs,
                                   threshold_rel, refine_radius, &pf);
    if (rc != LTMI_OK) return rc;
    if (ld_map < (int64_t)h * w) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_find_peaks_maps: ld_map < map size");
    if (n_frames == 0) return LTMI_OK;
    if (!maps || !n_found || !centers || !refineds || !peak_values || !peak_elevations)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_find_peaks_maps: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    MapsScratch &s = t_scratch;
    if (s.keys && (s.device != device || s.stream != stream)) {
        // the launches of the last call may still use the keys: wait for them, and free on the device that owns them
        LTMI_HIP(hipSetDevice(s.device));
        LTMI_HIP(hipDeviceSynchronize());
        if (s.device != device) s.keys.reset();
        LTMI_HIP(hipSetDevice(device));
    }
    s.device = device;
    s.stream = stream;
    t_last_kernel = peakfind_kernels();
    return peakfind_search(maps, n_frames, h, w, ld_map, pf, s.keys, n_found, centers, refineds, peak_values,
                           peak_elevations, stream);
}

extern "C" const char *ltmi_find_peaks_last_kernel(void) { return t_last_kernel; }
