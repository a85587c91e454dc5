// PNDetector pnCCD .frms6 frames unfolded on the device (gfx950): a stored frame of `height` rows of
// `width` = 2 x uint16 is folded; raw row r holds output row r (its columns [0, x), in order) and output row
// 2 height - 1 - r (its columns [x, 2 x), reversed).  With a binned readout every output row is written
// `binning` times, not rescaled.  Replaces the per-row read ranges and the row-by-row numba decoder of the
// reference (src/libertem/io/dataset/frms6.py:232-366), which run on the host for every tile.
//
// Pure byte movement, bound by HBM: every raw pixel is read once and written `binning` times.
//
// No LDS.  A linear copy through LDS would pay only if the reversed half did not coalesce, and it does: the
// work unit is one 16-byte piece (8 pixels) of a raw row and consecutive lanes take consecutive pieces, so a
// wave LOADS 1 KiB of contiguous raw bytes, whichever half they belong to.  The reversal is done where it is
// free: the 8 pixels of a piece are turned round in registers (4 dwords swapped, their halves rotated), and the
// piece goes to the mirrored piece of the output row (lane index -> x / 8 - 1 - piece).  The lanes of a wave
// that hold pieces of a reversed half row STORE one contiguous span of that output row as well, only in
// descending lane order: the same cache lines, each written whole by one wave-instruction.
//
// k_frms6_unfold16: the vector path; half rows of whole 16-byte pieces (x % 8 == 0) and 16-byte aligned
//     payloads, strides and destination -- the real detector (132 x 528 raw, 528-byte half rows, records a
//     multiple of 64 bytes apart).
// k_frms6_unfold2: one pixel per lane for every other geometry (windowed readouts: any even width, half rows
//     that start at any 2-byte boundary).  The host picks the kernel from the geometry and the addresses;
//     nothing is faulted into.
#include "ltmi_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t swap_halves(uint32_t v) { return (v >> 16) | (v << 16); }

// grid: (pieces of a frame / 256, 1, frames).  half_pieces = x / 8; a raw row is 2 * half_pieces pieces.
__global__ void __launch_bounds__(256)
k_frms6_unfold16(const unsigned char *__restrict__ src, int64_t frame_stride, int height, int half_pieces,
                 int binning, unsigned char *__restrict__ dst) {
    const int64_t piece = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int row_pieces = 2 * half_pieces;
    if (piece >= (int64_t)height * row_pieces) return;
    const int r = (int)(piece / row_pieces), u = (int)(piece - (int64_t)r * row_pieces);
    const int64_t frame = blockIdx.z;
    u32x4 v = *(const u32x4 *)(src + frame * frame_stride + piece * 16);
    int yb = r, c = u;
    if (u >= half_pieces) {
        yb = 2 * height - 1 - r;
        c = row_pieces - 1 - u;
        u32x4 t;
        t[0] = swap_halves(v[3]);
        t[1] = swap_halves(v[2]);
        t[2] = swap_halves(v[1]);
        t[3] = swap_halves(v[0]);
        v = t;
    }
    const int64_t row_bytes = (int64_t)half_pieces * 16;
    unsigned char *out = dst + ((frame * 2 * height + yb) * binning) * row_bytes + (int64_t)c * 16;
    for (int k = 0; k < binning; ++k) *(u32x4 *)(out + k * row_bytes) = v;
}

// grid: (pixels of a frame / 256, 1, frames)
__global__ void __launch_bounds__(256)
k_frms6_unfold2(const unsigned char *__restrict__ src, int64_t frame_stride, int height, int x, int binning,
                uint16_t *__restrict__ dst) {
    const int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int width = 2 * x;
    if (px >= (int64_t)height * width) return;
    const int r = (int)(px / width), col = (int)(px - (int64_t)r * width);
    const int64_t frame = blockIdx.z;
    const uint16_t v = *(const uint16_t *)(src + frame * frame_stride + px * 2);
    const int yb = col < x ? r : 2 * height - 1 - r;
    const int c = col < x ? col : width - 1 - col;
    uint16_t *out = dst + ((frame * 2 * height + yb) * binning) * (int64_t)x + c;
    for (int k = 0; k < binning; ++k) out[(int64_t)k * x] = v;
}

// the kernel of the last launch issued by this thread ("" before the first): ltmi_frms6_last_kernel
thread_local const char *t_last_kernel = "";

}  // namespace

extern "C" const char *ltmi_frms6_last_kernel(void) { return t_last_kernel; }

extern "C" int ltmi_frms6_decode(int device, const void *src, int64_t frame_stride, int64_t n_frames,
                                 int height, int width, int binning, void *dst, int dst_dtype, void *stream_) {
    if (dst_dtype != LTMI_U16)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_frms6_decode: 16-bit pixels decode to %s, not %s",
                  ltmi::dtype_name(LTMI_U16), ltmi::dtype_name(dst_dtype));
    // (height and width are 16-bit fields of the file header)
    if (n_frames < 0 || height < 0 || width < 0 || height > 65535 || width > 65535 || frame_stride < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_frms6_decode: bad geometry (frames=%lld, height=%d, width=%d, stride=%lld)",
                  (long long)n_frames, height, width, (long long)frame_stride);
    if (width % 2 != 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_frms6_decode: a folded frame has an even width, not %d", width);
    if (binning != 1 && binning != 2 && binning != 4)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_frms6_decode: binning is 1, 2 or 4, not %d", binning);
    if (!src || !dst) LTMI_FAIL(LTMI_E_INVALID, "ltmi_frms6_decode: null pointer");
    if ((uintptr_t)src % 2 != 0 || frame_stride % 2 != 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_frms6_decode: the payloads do not start at multiples of 2 bytes "
                                  "(%p, stride %lld)", src, (long long)frame_stride);
    if ((uintptr_t)dst % 2 != 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_frms6_decode: dst is not 2-byte aligned (%p)", dst);
    if (n_frames == 0 || height == 0 || width == 0) return LTMI_OK;
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    const int x = width / 2;
    const bool vec = x % 8 == 0 && (uintptr_t)src % 16 == 0 && frame_stride % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const int64_t frame_out = (int64_t)2 * height * binning * x * 2;        // bytes
    const int64_t units = vec ? (int64_t)height * (width / 8) : (int64_t)height * width;
    const unsigned blocks = (unsigned)((units + 255) / 256);                // < 2^24
    const int64_t max_frames = 65535;                                       // gridDim.z
    for (int64_t f0 = 0; f0 < n_frames; f0 += max_frames) {
        const int64_t nf = std::min(max_frames, n_frames - f0);
        const unsigned char *in = (const unsigned char *)src + f0 * frame_stride;
        unsigned char *out = (unsigned char *)dst + f0 * frame_out;
        if (vec)
            hipLaunchKernelGGL(k_frms6_unfold16, dim3(blocks, 1, (unsigned)nf), dim3(256), 0, stream, in,
                               frame_stride, height, x / 8, binning, out);
        else
            hipLaunchKernelGGL(k_frms6_unfold2, dim3(blocks, 1, (unsigned)nf), dim3(256), 0, stream, in,
                               frame_stride, height, x, binning, (uint16_t *)out);
        LTMI_HIP(hipGetLastError());
    }
    t_last_kernel = vec ? "k_frms6_unfold16" : "k_frms6_unfold2";
    return LTMI_OK;
}
