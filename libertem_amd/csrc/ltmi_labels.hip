// Partition stacks for gfx950 (MI355X):  out[f, k] (+)= sum_{p : label[p] = k} w[p] * tile[f, p]
//
// A sparse stack in which every pixel is stored by at most one mask -- the box masks of a binned detector
// (reference: examples/binning.ipynb), a polar rebinning map, hard-edged rings -- is a label per pixel and a
// weight per pixel: one multiply-add per labelled pixel, nothing for the others.  The stack has thousands of columns
// with one entry per pixel, which pads the blocked image 16 x and leaves k_sell_apply with one LDS gather per entry
// and 16 frames per workgroup.  Here the data movement follows the frames instead:
//
//   * a workgroup owns LB_F = 64 frames, one per LANE, and walks the chunks of LB_P = 512 consecutive pixels that hold
//     a labelled pixel (the others are never read).  A chunk of the 64 frames is read once, in address order (16-byte
//     loads, four lanes per 64 bytes of a frame row), and staged in LDS in the tile's own type, pixel-major:
//     slab[p][64 frames], written as 32-bit words (a lane loads the same 8 pixels of 4 / 2 / 1 frames of 1- / 2- /
//     4-byte pixels), 64 bytes of padding behind every 8 pixel rows so that, by the address arithmetic, the four
//     lanes that share a frame row write to different banks (not checked with counters).  The next chunk's loads are issued before the sums of this one (registers), so the
//     HBM stream does not stop for the LDS phase.
//   * the host sorts the labelled pixels of a chunk by label: a SEGMENT is the run of one label inside one chunk, its
//     RECORDS (local pixel, weight) in pixel order.  A wave takes a run of segments; the records are wave-uniform
//     (one coalesced load of 64 records, then v_readlane), every lane adds w * slab[p][its frame]: the LDS read is
//     one row (64 consecutive elements), and the label data is read once per 64 frames.
//   * the sums of 32 segments x 64 frames (a TURN) are turned in LDS and written with the lanes along the labels;
//     the tables of a turn are indexed by the turn alone and fetched one turn ahead, like the values in `out` that a
//     turn adds to, so no load waits for another between the barriers.  A label that
//     spans several chunks (a bin over several detector rows, a ring) is added to `out` chunk by chunk by the ONE
//     workgroup that owns its frames, in chunk order: no atomics, the same bits on every run.  The chunk list is cut
//     for more workgroups only where no label crosses the cut (every few detector rows for box bins, never for
//     rings), so a label still has one owner.
//
// Only stored entries are multiplied (a stored 0 times NaN is NaN, an unlabelled NaN reaches nothing): the arithmetic
// of the reference's CSR loop (common/numba/__init__.py:153-184) without a second pass.
// NOT THE DEFAULT ROUTE: the image is built only with LTMI_SPARSE_LABELS=1.  Measured (DESIGN.md 4.3c,
// profiles/bench_label_stacks.txt) the kernel is ahead of k_sell_apply on uint16 bins of 8 only, and a stack whose labels
// span the frame (rings, polar maps) is ONE group: one workgroup per 64 frames, far too few for the tiles of a UDF run.
// Why it is slow is a conjecture (the time hardly changed with the instructions per record: probably the frame read,
// 1 - 2 KiB per frame row at a time), not a counter measurement.
#include "ltmi_common.h"
#include "ltmi_tiles.h"
#include <cstring>
#include <new>
#include <typeinfo>

namespace ltmi {

constexpr int LB_F = 64;        // frames per workgroup (one per lane)
constexpr int LB_P = 512;       // pixels per chunk
constexpr int LB_NT = 512;      // threads per workgroup (8 waves)
constexpr int LB_NW = LB_NT / 64;
constexpr int LB_SB = 32;       // segments per turn of the result stage
constexpr int LB_SW = LB_SB / LB_NW;   // ... per wave
constexpr int LB_RS = 66;       // floats per segment in the result stage (even: the two frames of a lane pair differ in bank)
constexpr int LB_IT = LB_P * LB_F / 8 / LB_NT;   // 8-pixel loads per thread and chunk
constexpr int LB_PAD = 64;      // bytes behind every 8 pixel rows of the slab: the 4 lanes of a frame row write 4 x 64 banks
static_assert(LB_IT == 8 && LB_NW == 8, "the loader's lane roles");

__host__ __device__ constexpr size_t lb_slab_bytes(size_t elem) { return (size_t)(LB_P / 8) * (8 * LB_F * elem + LB_PAD); }

// A TURN is up to LB_SB segments of one chunk: what the waves sum between two barriers.  Everything a turn needs is
// indexed by the turn alone, so the kernel fetches it one turn ahead with independent loads.
struct LabelImage {
    int n_active = 0, n_segs = 0, n_groups = 0, n_empty = 0, n_turns = 0;
    size_t n_rec = 0;
    DevBuf<int> t_info;         // [n_turns][4] pixel chunk, segments | first turn of its chunk << 8, the next active
                                //              chunk, the first turn of that chunk
    DevBuf<int> t_rec;          // [n_turns][LB_NW + 1] first record of every wave's segments, end of the last
    DevBuf<int> t_end;          // [n_turns][LB_SB] end of a segment's records
    DevBuf<int> t_label;        // [n_turns][LB_SB] label k; -(k + 2): an earlier chunk holds it too (add to `out`); -1: none
    DevBuf<uint16_t> rec_pix;   // [n_rec + 64] pixel inside the chunk
    DevBuf<float> rec_w;        // [n_rec + 64]
    DevBuf<int> group_toff;     // [n_groups + 1] first turn of the runs of active chunks that no label leaves
    DevBuf<int> empty_cols;     // [n_empty] columns without a stored entry
};

template <typename T>
__global__ void __launch_bounds__(LB_NT)
k_labels(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_px, const int4 *__restrict__ t_info,
         const int *__restrict__ t_rec, const int *__restrict__ t_end, const int *__restrict__ t_label,
         const uint16_t *__restrict__ rec_pix, const float *__restrict__ rec_w, const int *__restrict__ group_toff,
         int n_groups, int groups_per_wg, float *out, int64_t ld_out, int accumulate, int vec_ok,
         const int32_t *__restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lb_lds[];
    constexpr int K = 4 / (int)sizeof(T);                 // frames per 32-bit word of the slab
    constexpr int ROWB = LB_F * (int)sizeof(T);           // bytes of a pixel row
    float *res = (float *)(lb_lds + lb_slab_bytes(sizeof(T)));          // [LB_SB][LB_RS]
    typedef typename TileVec<T, 8>::vec_a vec8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t f0 = (int64_t)blockIdx.x * LB_F;
    const int g0 = (int)blockIdx.y * groups_per_wg;
    const int g1 = g0 + groups_per_wg < n_groups ? g0 + groups_per_wg : n_groups;
    if (g0 >= g1) return;
    const int b0 = group_toff[g0], b1 = group_toff[g1];

    // loader role: lanes 4 i .. 4 i + 3 read 4 x 8 consecutive pixels of K frames each (16 K frames per load group,
    // 4 / K groups for the 64); the K frames of a pixel go to the slab as one 32-bit word
    const int lg = lane & 3, lfs = lane >> 2;
    const T *rowp[4];                                     // frame (q / K) * 16 K + lfs * K + q % K
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int64_t frame = f0 + (q / K) * 16 * K + lfs * K + q % K;
        if (frame > n_frames - 1) frame = n_frames - 1;
        if (rows) frame = rows[frame];                    // a region of interest: result row i = frame rows[i]
        rowp[q] = tile + frame * ld;
    }
    vec8 x[LB_IT];                                        // load group g = it / K: frame block g % (4 / K), pixel half g / (4 / K)
    auto load_chunk = [&](int px_chunk) {
        const int64_t pbase = (int64_t)px_chunk * LB_P;
#pragma unroll
        for (int it = 0; it < LB_IT; ++it) {
            const int g = it / K;
            const int64_t p = pbase + (wave * 8 + (g / (4 / K)) * 4 + lg) * 8;
            const T *row = rowp[(g % (4 / K)) * K + it % K];
            if (vec_ok && p + 8 <= n_px) {
                x[it] = __builtin_nontemporal_load((const tile_vec_t<T, 8> *)(row + p));
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[it][j] = p + j < n_px ? row[p + j] : (T)0;
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int g = 0; g < LB_IT / K; ++g) {
            const int pg = wave * 8 + (g / (4 / K)) * 4 + lg;            // 8-pixel group: LB_PAD bytes behind each
            unsigned char *dst = lb_lds + pg * (8 * ROWB + LB_PAD) + (g % (4 / K)) * 64 + lfs * 4;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t word = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const T v = x[g * K + k][j];
                    if constexpr (sizeof(T) == 4) word = __float_as_uint(v);
                    else if constexpr (sizeof(T) == 2) word |= (uint32_t)(uint16_t)v << (16 * k);
                    else word |= (uint32_t)(uint8_t)v << (8 * k);
                }
                *(uint32_t *)(dst + j * ROWB) = word;
            }
        }
    };
    const unsigned char *mine = lb_lds + lane * (int)sizeof(T);          // this lane's frame in pixel row 0

    struct Turn { int4 info; int r0, r1, endv, code; };
    auto fetch_turn = [&](int b) {
        Turn t;
        t.info = t_info[b];
        t.r0 = t_rec[b * (LB_NW + 1) + wave];
        t.r1 = t_rec[b * (LB_NW + 1) + wave + 1];
        t.endv = t_end[b * LB_SB + wave * LB_SW + (lane & (LB_SW - 1))];   // lane i < LB_SW: end of the wave's segment i
        t.code = t_label[b * LB_SB + (tid & (LB_SB - 1))];
        return t;
    };

    Turn cur = fetch_turn(b0);
    load_chunk(cur.info.x);
    // the first 64 records of the wave's segments (the arrays are padded by 64)
    int pv0 = rec_pix[cur.r0 + lane], wv0 = __float_as_int(rec_w[cur.r0 + lane]);
    for (int b = b0; b < b1; ++b) {
        const int n_seg = cur.info.y & 0xff;
        if (cur.info.y >> 8) {                            // the first turn of a chunk
            store_chunk();                                // (the slab is free: a barrier ended the previous turn)
            __syncthreads();
            if (cur.info.w < b1) load_chunk(cur.info.z);  // the next chunk: in flight during the sums
        }
        // where this thread's sums of the turn go (lanes along the segments = ascending labels), and what is there
        // if they are added: the sums of earlier chunks are in `out`, a barrier ended their turn
        const int code = cur.code;
        const bool add = accumulate || code < -1;
        const int label = code < -1 ? -code - 2 : code;
        float old[LB_F * LB_SB / LB_NT];
#pragma unroll
        for (int i = 0; i < LB_F * LB_SB / LB_NT; ++i) {
            const int f = (tid / LB_SB) + (LB_NT / LB_SB) * i;
            old[i] = (code != -1 && add && f0 + f < n_frames) ? out[(f0 + f) * ld_out + label] : 0.f;
        }
        Turn nxt = cur;
        if (b + 1 < b1) nxt = fetch_turn(b + 1);
        // this wave's segments of the turn and their records, which lie one after the other
        const int ns = n_seg - wave * LB_SW < LB_SW ? n_seg - wave * LB_SW : LB_SW;
        if (ns > 0) {
            const int r0 = __builtin_amdgcn_readfirstlane(cur.r0), r1 = __builtin_amdgcn_readfirstlane(cur.r1);
            int s = 0, seg_end = __builtin_amdgcn_readlane(cur.endv, 0);
            float acc = 0.f;
            for (int rb = r0; rb < r1; rb += 64) {
                if (rb != r0) {
                    pv0 = rec_pix[rb + lane];
                    wv0 = __float_as_int(rec_w[rb + lane]);
                }
                // 64 records, one per lane; pixels as byte offsets of their slab rows
                const int n = r1 - rb < 64 ? r1 - rb : 64;
                const int pv = pv0 * ROWB + (pv0 >> 3) * LB_PAD, wv = wv0;
                int j = 0;
                while (j < n) {
                    const int e = seg_end - rb < n ? seg_end - rb : n;   // (> j: a segment holds a record)
                    // one fixed order per label: its pixels ascending (4 LDS reads in flight)
                    for (; j + 4 <= e; j += 4) {
                        float xs[4], ws[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            ws[u] = __int_as_float(__builtin_amdgcn_readlane(wv, j + u));
                            xs[u] = (float)*(const T *)(mine + __builtin_amdgcn_readlane(pv, j + u));
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc = fmaf(ws[u], xs[u], acc);
                    }
                    for (; j < e; ++j) {
                        const float w = __int_as_float(__builtin_amdgcn_readlane(wv, j));
                        acc = fmaf(w, (float)*(const T *)(mine + __builtin_amdgcn_readlane(pv, j)), acc);
                    }
                    if (rb + j == seg_end) {
                        res[(wave * LB_SW + s) * LB_RS + lane] = acc;
                        acc = 0.f;
                        if (++s < ns) seg_end = __builtin_amdgcn_readlane(cur.endv, s);
                    }
                }
            }
        }
        if (b + 1 < b1) {                                 // the next turn's records: in flight during the write
            pv0 = rec_pix[nxt.r0 + lane];
            wv0 = __float_as_int(rec_w[nxt.r0 + lane]);
        }
        __syncthreads();
        if (code != -1) {
#pragma unroll
            for (int i = 0; i < LB_F * LB_SB / LB_NT; ++i) {
                const int f = (tid / LB_SB) + (LB_NT / LB_SB) * i;
                if (f0 + f < n_frames) {
                    const float v = res[(tid & (LB_SB - 1)) * LB_RS + f];
                    out[(f0 + f) * ld_out + label] = add ? old[i] + v : v;
                }
            }
        }
        __syncthreads();                                  // the stage is free; the turn's sums are in `out`
        cur = nxt;
    }
}

// a plain product gives 0 in the columns that store nothing
__global__ void __launch_bounds__(256)
k_labels_zero_cols(float *__restrict__ out, int64_t ld_out, int64_t n_frames, const int *__restrict__ cols,
                   int n_cols) {
    const int64_t total = n_frames * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        out[(i / n_cols) * ld_out + cols[i % n_cols]] = 0.f;
}

// Is the stack a partition?  No pixel stored twice, at least one entry (masks.is_label_stack is the host-side twin);
// records, segments and turns are counted in int.
bool labels_qualifies(const int64_t *indptr, int64_t n_px, int64_t n_masks) {
    const int64_t nnz = indptr[n_px];
    if (nnz <= 0 || n_masks >= (1ll << 31) || n_px >= (1ll << 31)) return false;
    for (int64_t p = 0; p < n_px; ++p)
        if (indptr[p + 1] - indptr[p] > 1) return false;
    return true;
}

void labels_destroy(void *image) { delete (LabelImage *)image; }

void *labels_build(const int64_t *indptr, const int64_t *indices, const float *vals, int64_t n_px, int64_t n_masks,
                   int *err) {
    *err = LTMI_OK;
    LabelImage *im = new (std::nothrow) LabelImage();
    if (!im) {
        *err = LTMI_E_NOMEM;
        set_error("out of host memory");
        return nullptr;
    }
    try {
        const int64_t n_chunks = (n_px + LB_P - 1) / LB_P;
        // the last chunk that holds a label: where the chunk list may be cut
        std::vector<int64_t> last_chunk((size_t)n_masks, -1);
        for (int64_t p = 0; p < n_px; ++p)
            if (indptr[p + 1] > indptr[p]) last_chunk[(size_t)indices[indptr[p]]] = p / LB_P;
        std::vector<int> chunk, seg_off(1, 0), seg_label, seg_rec(1, 0), group_off(1, 0), empty_cols;
        std::vector<uint8_t> seg_later, seen((size_t)n_masks, 0);
        std::vector<uint16_t> rec_pix;
        std::vector<float> rec_w;
        std::vector<std::pair<int64_t, int>> px;          // (label, local pixel) of one chunk
        int64_t reach = -1;                               // last chunk of the labels met so far
        for (int64_t ch = 0; ch < n_chunks; ++ch) {
            px.clear();
            const int64_t p1 = std::min<int64_t>((ch + 1) * LB_P, n_px);
            for (int64_t p = ch * LB_P; p < p1; ++p)
                if (indptr[p + 1] > indptr[p]) px.emplace_back(indices[indptr[p]], (int)(p - ch * LB_P));
            if (px.empty()) continue;
            std::sort(px.begin(), px.end());              // by label, a label's pixels ascending
            chunk.push_back((int)ch);
            for (size_t i = 0; i < px.size(); ++i) {
                const int64_t k = px[i].first;
                if (i == 0 || k != px[i - 1].first) {
                    if (i) seg_rec.push_back((int)rec_pix.size());
                    seg_label.push_back((int)k);
                    seg_later.push_back(seen[(size_t)k]);
                    seen[(size_t)k] = 1;
                    reach = std::max(reach, last_chunk[(size_t)k]);
                }
                rec_pix.push_back((uint16_t)px[i].second);
                rec_w.push_back(vals[indptr[ch * LB_P + px[i].second]]);
            }
            seg_rec.push_back((int)rec_pix.size());
            seg_off.push_back((int)seg_label.size());
            if (reach <= ch) group_off.push_back((int)chunk.size());
        }
        for (int64_t k = 0; k < n_masks; ++k)
            if (!seen[(size_t)k]) empty_cols.push_back((int)k);
        // the turns: up to LB_SB segments of one chunk each
        std::vector<int> t_info, t_rec, t_end, t_label, first_turn(chunk.size() + 1, 0), group_toff;
        for (size_t ai = 0; ai < chunk.size(); ++ai) {
            first_turn[ai] = (int)(t_info.size() / 4);
            for (int sb = seg_off[ai]; sb < seg_off[ai + 1]; sb += LB_SB) {
                const int n = std::min(LB_SB, seg_off[ai + 1] - sb);
                t_info.push_back(chunk[ai]);
                t_info.push_back(n | ((sb == seg_off[ai]) << 8));
                t_info.push_back(ai + 1 < chunk.size() ? chunk[ai + 1] : 0);
                t_info.push_back((int)ai + 1);            // (the chunk: its first turn below)
                for (int w = 0; w <= LB_NW; ++w) t_rec.push_back(seg_rec[sb + std::min(w * LB_SW, n)]);
                for (int i = 0; i < LB_SB; ++i) {
                    t_end.push_back(seg_rec[sb + std::min(i + 1, n)]);
                    t_label.push_back(i < n ? (seg_later[sb + i] ? -(seg_label[sb + i] + 2) : seg_label[sb + i]) : -1);
                }
            }
        }
        const int n_turns = (int)(t_info.size() / 4);
        first_turn[chunk.size()] = n_turns;
        for (int t = 0; t < n_turns; ++t) t_info[4 * t + 3] = first_turn[t_info[4 * t + 3]];
        for (int g : group_off) group_toff.push_back(first_turn[g]);
        im->n_active = (int)chunk.size();
        im->n_segs = (int)seg_label.size();
        im->n_groups = (int)group_off.size() - 1;
        im->n_empty = (int)empty_cols.size();
        im->n_turns = n_turns;
        im->n_rec = rec_pix.size();
        rec_pix.resize(rec_pix.size() + 64, 0);           // a wave loads whole pieces of 64 records
        rec_w.resize(rec_w.size() + 64, 0.f);
        hipError_t e = im->t_info.upload(t_info.data(), t_info.size());
        if (e == hipSuccess) e = im->t_rec.upload(t_rec.data(), t_rec.size());
        if (e == hipSuccess) e = im->t_end.upload(t_end.data(), t_end.size());
        if (e == hipSuccess) e = im->t_label.upload(t_label.data(), t_label.size());
        if (e == hipSuccess) e = im->rec_pix.upload(rec_pix.data(), rec_pix.size());
        if (e == hipSuccess) e = im->rec_w.upload(rec_w.data(), rec_w.size());
        if (e == hipSuccess) e = im->group_toff.upload(group_toff.data(), group_toff.size());
        if (e == hipSuccess && im->n_empty) e = im->empty_cols.upload(empty_cols.data(), empty_cols.size());
        if (e != hipSuccess) {
            delete im;
            *err = (int)e;
            set_error("uploading the label image failed: %s", hipGetErrorString(e));
            return nullptr;
        }
    } catch (const std::bad_alloc &) {
        delete im;
        *err = LTMI_E_NOMEM;
        set_error("out of host memory while packing the label image");
        return nullptr;
    }
    return im;
}

bool labels_takes(int tile_dtype) {
    switch (tile_dtype) {
        case LTMI_U8: case LTMI_I8: case LTMI_U16: case LTMI_I16: case LTMI_F32: return true;
    }
    return false;
}

template <typename T>
static int launch_labels(ltmi_masks *m, const LabelImage *im, const MaskCall &call) {
    const T *tile = (const T *)call.tile;
    float *out = (float *)call.out;
    const int vec_ok = vector_loads_ok(tile, call.ld_tile, sizeof(T)) ? 1 : 0;
    const size_t lds = lb_slab_bytes(sizeof(T)) + (size_t)LB_SB * LB_RS * sizeof(float);
    static bool set[16] = {false};
    if (!set[m->device & 15]) {
        LTMI_HIP(hipFuncSetAttribute((const void *)k_labels<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        set[m->device & 15] = true;
    }
    if (im->n_empty && !call.accumulate) {
        const int64_t total = call.n_frames * im->n_empty;
        hipLaunchKernelGGL(k_labels_zero_cols, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0,
                           call.stream, out, call.ld_out, call.n_frames, (const int *)im->empty_cols, im->n_empty);
        LTMI_HIP(hipGetLastError());
    }
    // more workgroups than frame groups: the chunk list cut where no label crosses (aim: 4 workgroups per CU)
    const int64_t n_fg = (call.n_frames + LB_F - 1) / LB_F;
    const int want = (int)std::min<int64_t>((1024 + n_fg - 1) / n_fg, im->n_groups);
    const int n_split = clamp_ksplit(std::max(want, 1), im->n_groups);
    const int per = (im->n_groups + n_split - 1) / n_split;
    const dim3 grid((unsigned)n_fg, (unsigned)n_split);
    hipLaunchKernelGGL(k_labels<T>, grid, dim3(LB_NT), lds, call.stream, tile, call.ld_tile, call.n_frames, m->n_px,
                       (const int4 *)im->t_info.get(), (const int *)im->t_rec, (const int *)im->t_end,
                       (const int *)im->t_label, (const uint16_t *)im->rec_pix, (const float *)im->rec_w,
                       (const int *)im->group_toff, im->n_groups, per, out, call.ld_out, call.accumulate, vec_ok,
                       call.rows);
    LTMI_HIP(hipGetLastError());
    m->last_exact = true;                                 // only stored entries were multiplied
    snprintf(m->last_kernel, sizeof(m->last_kernel), "k_labels<%s%s> grid=(%u,%u) chunks=%d segs=%d",
             typeid(T).name(), call.rows ? ",rows" : "", grid.x, grid.y, im->n_active, im->n_segs);
    return LTMI_OK;
}

int labels_apply(ltmi_masks *m, void *image, const MaskCall &call) {
    const LabelImage *im = (const LabelImage *)image;
    if (call.n_frames >= (1ll << 31) * LB_F)
        LTMI_FAIL(LTMI_E_SHAPE, "label stacks: too many frames in one call");
    switch (call.tile_dtype) {
        case LTMI_U8: return launch_labels<uint8_t>(m, im, call);
        case LTMI_I8: return launch_labels<int8_t>(m, im, call);
        case LTMI_U16: return launch_labels<uint16_t>(m, im, call);
        case LTMI_I16: return launch_labels<int16_t>(m, im, call);
        case LTMI_F32: return launch_labels<float>(m, im, call);
    }
    LTMI_FAIL(LTMI_E_DTYPE, "label stacks: tile dtype %s is not supported", dtype_name(call.tile_dtype));
}

}  // namespace ltmi
