// Gatan K2 IS sector files decoded on the device (gfx950): block headers stripped, 12-bit little-endian pixel
// pairs unpacked, the mirrored 930 x 16 blocks of the 8 sectors laid out as (1860, 2048) uint16 frames.
// Replaces decode_k2is / decode_uint12_le and the per-block read ranges that feed them
// (src/libertem/io/dataset/k2is.py:82-164, 172-231), which the reference runs on the host for every tile.
//
// The layout is a transposition: consecutive source bytes are consecutive ROWS of one 16-pixel column strip
// (24 bytes per row), consecutive destination bytes run ACROSS the 16 strips of a sector (512 bytes per row).
// One workgroup takes K2_ROWS rows of all 16 blocks of one (frame, sector, half):
//   load:  16 runs of K2_ROWS * 24 contiguous bytes, one per block, 8 bytes per lane (block starts and rows
//          are multiples of 8 bytes) -> LDS, as they come (the LDS image is a linear copy: lane w writes
//          8-byte word w);
//   store: one lane per 8 pixels = 12 bytes of LDS (three dwords) -> one 16-byte store; the 32 lanes of half
//          a wave write the 512 bytes of one row of the sector, a wave two such rows.
// LDS reads: lane (strip j, half-strip h) of a row reads dword 186 (15 - j) + 3 h + 6 r + d; 186 = 26 mod 32
// and h adds 3, so the 32 lanes of a group hit 32 different banks (even for h = 0, odd for h = 1).
// Pure byte shuffling: 5.72 MB in, 7.62 MB out per frame, bound by HBM.
#include "ltmi_common.h"

namespace {

constexpr int K2_HEADER = 40, K2_BLOCK = 0x5758, K2_BLOCKS_PER_FRAME = 32, K2_SECTORS = 8;
constexpr int K2_BLOCK_ROWS = 930, K2_ROW_BYTES = 24, K2_H = 1860, K2_W = 2048;
constexpr int K2_ROWS = 31;                                     // rows of a block per workgroup
constexpr int K2_STRIPS = K2_BLOCK_ROWS / K2_ROWS;              // 30 workgroups per (frame, sector, half)
constexpr int K2_RUN_WORDS = K2_ROWS * K2_ROW_BYTES / 8;        // 93 8-byte words per block and workgroup
constexpr int K2_WORDS = 16 * K2_RUN_WORDS;                     // 1488
constexpr int K2_UNITS = K2_ROWS * 32;                          // 16-byte stores per workgroup
static_assert(K2_STRIPS * K2_ROWS == K2_BLOCK_ROWS, "whole strips");
static_assert((K2_ROWS * K2_ROW_BYTES) % 8 == 0, "runs of whole 8-byte words");
static_assert(K2_BLOCK % 8 == 0 && K2_HEADER % 8 == 0, "8-byte aligned payload rows");

struct K2Sources { const unsigned char *p[K2_SECTORS]; };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256)
k_k2is_decode(K2Sources src, unsigned char *__restrict__ dst) {
    __shared__ uint64_t raw[K2_WORDS];
    const int strip = blockIdx.x, sector = blockIdx.y >> 1, half = blockIdx.y & 1;
    const int64_t frame = blockIdx.z;
    const unsigned char *in = src.p[sector] + (frame * K2_BLOCKS_PER_FRAME + half * 16) * (int64_t)K2_BLOCK
                              + K2_HEADER + strip * (K2_ROWS * K2_ROW_BYTES);
    for (int w = threadIdx.x; w < K2_WORDS; w += 256) {
        const int kk = w / K2_RUN_WORDS, j = w - kk * K2_RUN_WORDS;
        raw[w] = *(const uint64_t *)(in + (int64_t)kk * K2_BLOCK + j * 8);
    }
    __syncthreads();
    const uint32_t *words = (const uint32_t *)raw;
    const int64_t row0 = frame * K2_H + half * K2_BLOCK_ROWS + strip * K2_ROWS;
    unsigned char *out = dst + (row0 * K2_W + sector * 256) * 2;
    for (int u = threadIdx.x; u < K2_UNITS; u += 256) {
        const int r = u >> 5, c = u & 31;                        // row of the strip, 8-pixel column of the sector
        const int kk = 15 - (c >> 1);                            // the x order of the blocks is mirrored
        const uint32_t *t = words + kk * (K2_RUN_WORDS * 2) + r * 6 + (c & 1) * 3;
        const uint32_t d0 = t[0], d1 = t[1], d2 = t[2];
        // four 24-bit groups = four pixel pairs: a = low 12 bits, b = high 12 bits
        const uint32_t v0 = d0 & 0xFFFFFFu, v1 = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
        const uint32_t v2 = (d1 >> 16) | ((d2 & 0xFFu) << 16), v3 = d2 >> 8;
        u32x4 o;
        o[0] = (v0 & 0xFFFu) | ((v0 >> 12) << 16);
        o[1] = (v1 & 0xFFFu) | ((v1 >> 12) << 16);
        o[2] = (v2 & 0xFFFu) | ((v2 >> 12) << 16);
        o[3] = (v3 & 0xFFFu) | ((v3 >> 12) << 16);
        *(u32x4 *)(out + (int64_t)r * (K2_W * 2) + c * 16) = o;
    }
}

}  // namespace

extern "C" int ltmi_k2is_decode(int device, const void *const sector_src[8], int64_t n_frames, void *dst,
                                int dst_dtype, void *stream_) {
    if (dst_dtype != LTMI_U16)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_k2is_decode: 12-bit pixels decode to %s, not %s",
                  ltmi::dtype_name(LTMI_U16), ltmi::dtype_name(dst_dtype));
    if (n_frames < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_k2is_decode: bad geometry (frames=%lld)", (long long)n_frames);
    if (!sector_src || !dst) LTMI_FAIL(LTMI_E_INVALID, "ltmi_k2is_decode: null pointer");
    K2Sources src;
    for (int s = 0; s < K2_SECTORS; ++s) {
        src.p[s] = (const unsigned char *)sector_src[s];
        if (!src.p[s]) LTMI_FAIL(LTMI_E_INVALID, "ltmi_k2is_decode: null pointer (sector %d)", s);
        if ((uintptr_t)src.p[s] % 8 != 0)
            LTMI_FAIL(LTMI_E_INVALID, "ltmi_k2is_decode: the blocks of sector %d do not start at a multiple "
                                      "of 8 bytes (%p)", s, sector_src[s]);
    }
    if ((uintptr_t)dst % 16 != 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_k2is_decode: dst is not 16-byte aligned (%p)", dst);
    if (n_frames == 0) return LTMI_OK;
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t frame_in = (int64_t)K2_BLOCKS_PER_FRAME * K2_BLOCK, frame_out = (int64_t)K2_H * K2_W * 2;
    const int64_t max_frames = 65535;                           // gridDim.z
    for (int64_t f0 = 0; f0 < n_frames; f0 += max_frames) {
        const int64_t nf = std::min(max_frames, n_frames - f0);
        K2Sources part;
        for (int s = 0; s < K2_SECTORS; ++s) part.p[s] = src.p[s] + f0 * frame_in;
        hipLaunchKernelGGL(k_k2is_decode, dim3(K2_STRIPS, 2 * K2_SECTORS, (unsigned)nf), dim3(256), 0, stream,
                           part, (unsigned char *)dst + f0 * frame_out);
        LTMI_HIP(hipGetLastError());
    }
    return LTMI_OK;
}
