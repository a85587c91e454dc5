// Out-of-place transposition of a 2D array in HBM (gfx950): dst[c * ld_dst + r] = src[r * ld_src + c] for r < rows,
// c < cols, elements of 1, 2, 4, 8 or 16 bytes that are moved, never interpreted.  Replaces the `partition.T`
// assignment into the memory map with which the reference turns a (sig, nav) dataset into (nav, sig) on one CPU
// thread (src/libertem/contrib/convert_transposed.py:28-40).
//
// Pure byte movement, bound by HBM: 2 * rows * cols * item_bytes bytes, each element read once and written once.
// A workgroup (256 lanes) stages one T x T tile through LDS per step, so the global reads run along the rows of
// src and the global writes along the rows of dst; it walks the flat list of tiles with a grid stride (no grid
// dimension counts rows or columns, all offsets are 64-bit).  Edge tiles are predicated, per unit and, where a
// unit straddles the edge, per element.
//
// A lane moves one UNIT per access: the element itself at 4, 8 and 16 bytes, 4 bytes = E elements at 1 and 2 bytes
// (E = 4, 2), from any element-aligned address (gfx950 serves those at the speed of aligned ones):
//
//   item bytes   unit   E    T     row of the tile   LDS     wave-instruction, global read / global write
//        1        4 B   4   128    32 units          16 KB   2 x 128 B / 2 x 128 B
//        2        4 B   2   128    64 units          32 KB   256 B / 256 B
//        4        4 B   1    64    64 units          16 KB   256 B / 256 B
//        8        8 B   1    64    64 units          32 KB   512 B / 512 B
//       16       16 B   1    32    32 units          16 KB   2 x 512 B / 2 x 512 B
//
// LDS image: row-major [T rows][T / E units], unpadded, unit j of row r stored at unit j ^ ((r / E) % 32) of its
// row (XOR swizzle; the row is 32 or 64 units, so the unit stays in it).  In the write pass lane l stores unit
// l % UR of a row; in the read pass lane l of a dst row (tile column cc) takes rows l * E ... l * E + E - 1 at
// column cc, i.e. unit (cc / E) ^ (l % 32) of each: one whole unit at E = 1, one element from each of E rows
// (ds_read_u8 / ds_read_u16) at E > 1, packed into the unit that is stored.  Rows are a multiple of 128 B long, so
// the bank of an access is set by its unit index alone.  Conflict degree by the bank rules of the instructions
// (writes and 1-, 2-, 4-byte reads: bank = (a / 4) % 32; ds_read_b64 / _b128: (a / 4) % 64):
//
//   item bytes   write pass                                      read pass
//        1       ds_write_b32, 32-lane halves: one row each,     ds_read_u8, halves: lanes 0..31 of a column,
//                units j ^ s, all distinct: 1-way                banks (cc / 4) ^ l, all distinct: 1-way
//        2       ds_write_b32: a half holds 32 consecutive j,    ds_read_u16: banks ((cc / 2) ^ (l % 32)) % 32 per
//                (j ^ s) % 32 distinct: 1-way                    half, distinct: 1-way
//        4       as at 2 bytes: 1-way                            ds_read_b32: banks (cc ^ (l % 32)) % 32: 1-way
//        8       ds_write_b64, groups of 16 consecutive lanes,   ds_read_b64, halves, a lane covers banks
//                2 banks a lane, (j ^ s) % 16 distinct: 1-way    2 u, 2 u + 1 with u = cc ^ (l % 32), u % 32
//                                                                distinct: 1-way
//       16       ds_write_b128, groups of 8 consecutive lanes,   ds_read_b128, 16-lane groups {0-3, 12-15, 20-27},
//                4 banks a lane, (j ^ s) % 8 distinct: 1-way     {4-11, 16-19, 28-31} (+32): l % 16 distinct within
//                                                                a group, 16-B slots (cc ^ l) % 16 distinct: 1-way
//
// The loads of a tile are all issued before its LDS stores (up to 32 units in flight per lane).
#include "ltmi_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// U: the unit in LDS; G: the same unit at a global address that is only element-aligned; EL: the element (E > 1)
template <int IB> struct cfg;
template <> struct cfg<1> {
    typedef uint32_t U; typedef uint32_t G __attribute__((aligned(1))); typedef uint8_t EL;
    static constexpr int E = 4, T = 128;
};
template <> struct cfg<2> {
    typedef uint32_t U; typedef uint32_t G __attribute__((aligned(2))); typedef uint16_t EL;
    static constexpr int E = 2, T = 128;
};
template <> struct cfg<4> {
    typedef uint32_t U; typedef uint32_t G; typedef uint32_t EL;
    static constexpr int E = 1, T = 64;
};
template <> struct cfg<8> {
    typedef uint64_t U; typedef uint64_t G; typedef uint64_t EL;
    static constexpr int E = 1, T = 64;
};
template <> struct cfg<16> {
    typedef u32x4 U; typedef u32x4 G __attribute__((aligned(8))); typedef u32x4 EL;   // (complex128: 8-byte aligned)
    static constexpr int E = 1, T = 32;
};

constexpr int THREADS = 256;
constexpr int64_t MAX_BLOCKS = 256 * 8;                                 // 8 blocks on each of the 256 CUs

// grid: (min(items, MAX_BLOCKS)).  tiles_c = ceil(cols / T), items = ceil(rows / T) * tiles_c.
template <int IB>
__global__ void __launch_bounds__(THREADS)
k_transpose(const unsigned char *__restrict__ src, int64_t ld_src, int64_t rows, int64_t cols,
            unsigned char *__restrict__ dst, int64_t ld_dst, int64_t tiles_c, int64_t items) {
    typedef cfg<IB> C;
    typedef typename C::U U;
    typedef typename C::G G;
    typedef typename C::EL EL;
    constexpr int E = C::E, T = C::T, UR = T / E, N = T * UR / THREADS;
    __shared__ U tile[T * UR];
    const int tid = threadIdx.x;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tr = item / tiles_c, tc = item - tr * tiles_c;
        const int64_t r0 = tr * T, c0 = tc * T;
        U v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int idx = k * THREADS + tid, row = idx / UR, j = idx % UR;
            const int64_t r = r0 + row, c = c0 + (int64_t)j * E;
            v[k] = U{};
            if (r < rows && c < cols) {
                const unsigned char *p = src + (r * ld_src + c) * IB;
                if constexpr (E == 1) {
                    v[k] = *(const G *)p;
                } else {
                    if (c + E <= cols) {
                        v[k] = *(const G *)p;
                    } else {                                            // the unit straddles the last column
                        uint32_t w = 0;
#pragma unroll
                        for (int e = 0; e < E - 1; ++e)
                            if (c + e < cols) w |= (uint32_t)((const EL *)p)[e] << (8 * IB * e);
                        v[k] = w;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int idx = k * THREADS + tid, row = idx / UR, j = idx % UR;
            tile[row * UR + (j ^ ((row / E) & 31))] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int idx = k * THREADS + tid, cc = idx / UR, l = idx % UR;
            const int64_t dr = c0 + cc, dc = r0 + (int64_t)l * E;       // row and first column in dst
            if (dr < cols && dc < rows) {
                unsigned char *q = dst + (dr * ld_dst + dc) * IB;
                if constexpr (E == 1) {
                    *(G *)q = tile[l * UR + (cc ^ (l & 31))];
                } else {
                    const EL *t = (const EL *)tile;
                    EL el[E];
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        el[e] = t[((l * E + e) * UR + ((cc / E) ^ (l & 31))) * E + cc % E];
                    if (dc + E <= rows) {
                        uint32_t w = 0;
#pragma unroll
                        for (int e = 0; e < E; ++e) w |= (uint32_t)el[e] << (8 * IB * e);
                        *(G *)q = w;
                    } else {                                            // the unit straddles the last row of src
#pragma unroll
                        for (int e = 0; e < E - 1; ++e)
                            if (dc + e < rows) ((EL *)q)[e] = el[e];
                    }
                }
            }
        }
        __syncthreads();                                                // the next tile overwrites the image
    }
}

template <int IB>
void launch(const void *src, int64_t ld_src, int64_t rows, int64_t cols, void *dst, int64_t ld_dst,
            hipStream_t stream) {
    constexpr int T = cfg<IB>::T;
    const int64_t tiles_r = (rows + T - 1) / T, tiles_c = (cols + T - 1) / T, items = tiles_r * tiles_c;
    const unsigned blocks = (unsigned)std::min<int64_t>(items, MAX_BLOCKS);
    hipLaunchKernelGGL(k_transpose<IB>, dim3(blocks), dim3(THREADS), 0, stream, (const unsigned char *)src, ld_src,
                       rows, cols, (unsigned char *)dst, ld_dst, tiles_c, items);
}

// the kernel of the last launch issued by this thread ("" before the first): ltmi_transpose_last_kernel
thread_local const char *t_last_kernel = "";

}  // namespace

extern "C" const char *ltmi_transpose_last_kernel(void) { return t_last_kernel; }

extern "C" int ltmi_transpose2d(int device, const void *src, int64_t ld_src, int64_t rows, int64_t cols,
                                int item_bytes, void *dst, int64_t ld_dst, void *stream_) {
    if (rows < 0 || cols < 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_transpose2d: %lld x %lld elements", (long long)rows, (long long)cols);
    if (ld_src < cols)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_transpose2d: source rows %lld elements apart cannot hold %lld columns",
                  (long long)ld_src, (long long)cols);
    if (ld_dst < rows)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_transpose2d: destination rows %lld elements apart cannot hold %lld columns",
                  (long long)ld_dst, (long long)rows);
    if (item_bytes != 1 && item_bytes != 2 && item_bytes != 4 && item_bytes != 8 && item_bytes != 16)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_transpose2d: elements of %d bytes (1, 2, 4, 8 or 16)", item_bytes);
    // the byte spans of both arrays, with a tile of slack for the kernel's r0 + row and c0 + column sums
    const int64_t slack = 256;
    int64_t a, b, ra, ca;
    if (__builtin_add_overflow(rows, slack, &ra) || __builtin_add_overflow(cols, slack, &ca) ||
        __builtin_mul_overflow(ra, ld_src, &a) || __builtin_mul_overflow(a, (int64_t)item_bytes, &a) ||
        __builtin_mul_overflow(ca, ld_dst, &b) || __builtin_mul_overflow(b, (int64_t)item_bytes, &b))
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_transpose2d: %lld x %lld elements of %d bytes, rows %lld and %lld elements "
                  "apart, do not fit 64-bit offsets", (long long)rows, (long long)cols, item_bytes,
                  (long long)ld_src, (long long)ld_dst);
    if (rows == 0 || cols == 0) return LTMI_OK;
    if (!src || !dst) LTMI_FAIL(LTMI_E_INVALID, "ltmi_transpose2d: null pointer");
    if (((uintptr_t)src | (uintptr_t)dst) % (item_bytes == 16 ? 8 : item_bytes))
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_transpose2d: src and dst must be aligned to the element");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    switch (item_bytes) {
        case 1: launch<1>(src, ld_src, rows, cols, dst, ld_dst, stream); break;
        case 2: launch<2>(src, ld_src, rows, cols, dst, ld_dst, stream); break;
        case 4: launch<4>(src, ld_src, rows, cols, dst, ld_dst, stream); break;
        case 8: launch<8>(src, ld_src, rows, cols, dst, ld_dst, stream); break;
        default: launch<16>(src, ld_src, rows, cols, dst, ld_dst, stream); break;
    }
    LTMI_HIP(hipGetLastError());
    static const char *const names[] = {"k_transpose<1>", "k_transpose<2>", "k_transpose<4>", "k_transpose<8>",
                                        "k_transpose<16>"};
    t_last_kernel = names[item_bytes == 16 ? 4 : item_bytes == 8 ? 3 : item_bytes == 4 ? 2 : item_bytes == 2 ? 1 : 0];
    return LTMI_OK;
}
