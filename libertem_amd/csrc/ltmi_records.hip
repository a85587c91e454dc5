// Frame records gathered on the device (gfx950): a file of fixed-size records [frame header | pixels | frame
// footer] (Norpix .seq, EMPAD .raw, NanoMegas .blo) is uploaded as it is, and the payloads -- `payload_bytes`
// every `record_stride` bytes -- are moved into one contiguous array.  Replaces the per-tile read ranges with which
// the reference strips headers and footers on the host for every run (src/libertem/io/dataset/base/tiling.py,
// decode.py).
//
// Pure byte movement, bound by HBM: every payload byte is read once and written once, nothing is converted.
// A lane moves W bytes per access, W in {1, 2, 4, 8, 16}: the host picks the largest W that divides the address of
// the first payload, the record stride, the payload size and the address of the destination, so every access of
// every frame is naturally aligned and none reaches outside a payload -- no aligned-load-and-shift realignment
// that would read the framing (or past the end of a buffer whose last record ends with its payload).
//
// Work is dealt in pieces of one frame: 256 lanes x UNROLL accesses, consecutive lanes on consecutive units (a
// wave-instruction loads / stores 64 W contiguous bytes, 1 KiB at W = 16).  A block walks the flat list of
// (frame, piece) pairs with a grid stride: the frame of a piece is one scalar division per piece, not one per
// lane, no grid dimension counts frames, and all offsets are 64-bit.  The loads of a piece are issued before its
// stores (UNROLL independent loads in flight per lane).
#include "ltmi_common.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int W> struct unit;
template <> struct unit<1> { typedef uint8_t type; };
template <> struct unit<2> { typedef uint16_t type; };
template <> struct unit<4> { typedef uint32_t type; };
template <> struct unit<8> { typedef uint64_t type; };
template <> struct unit<16> { typedef u32x4 type; };

constexpr int THREADS = 256, UNROLL = 4, PIECE = THREADS * UNROLL;      // units of W bytes per piece
constexpr int64_t MAX_BLOCKS = 256 * 8;                                 // 8 blocks on each of the 256 CUs

// grid: (min(n_frames * pieces, MAX_BLOCKS)).  per = payload_bytes / W, pieces = ceil(per / PIECE).
template <int W>
__global__ void __launch_bounds__(THREADS)
k_records(const unsigned char *__restrict__ src, int64_t record_stride, int64_t n_frames, int64_t per,
          int64_t pieces, unsigned char *__restrict__ dst) {
    typedef typename unit<W>::type T;
    const int64_t items = n_frames * pieces;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t frame = item / pieces, piece = item - frame * pieces;
        const T *in = (const T *)(src + frame * record_stride);
        T *out = (T *)(dst + frame * per * W);
        const int64_t u0 = piece * PIECE + threadIdx.x;
        T v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k)
            if (u0 + k * THREADS < per) v[k] = in[u0 + k * THREADS];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k)
            if (u0 + k * THREADS < per) out[u0 + k * THREADS] = v[k];
    }
}

template <int W>
void launch(const void *src, int64_t record_stride, int64_t n_frames, int64_t payload_bytes, void *dst,
            hipStream_t stream) {
    const int64_t per = payload_bytes / W, pieces = (per + PIECE - 1) / PIECE;
    const unsigned blocks = (unsigned)std::min<int64_t>(n_frames * pieces, MAX_BLOCKS);
    hipLaunchKernelGGL(k_records<W>, dim3(blocks), dim3(THREADS), 0, stream, (const unsigned char *)src,
                       record_stride, n_frames, per, pieces, (unsigned char *)dst);
}

// the kernel of the last launch issued by this thread ("" before the first): ltmi_records_last_kernel
thread_local const char *t_last_kernel = "";

}  // namespace

extern "C" const char *ltmi_records_last_kernel(void) { return t_last_kernel; }

extern "C" int ltmi_records_gather(int device, const void *src, int64_t record_stride, int64_t n_frames,
                                   int64_t payload_bytes, void *dst, void *stream_) {
    if (n_frames < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_records_gather: n_frames is %lld", (long long)n_frames);
    if (payload_bytes < 1)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_records_gather: a payload of %lld bytes", (long long)payload_bytes);
    if (record_stride < payload_bytes)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_records_gather: records %lld bytes apart cannot hold payloads of %lld bytes",
                  (long long)record_stride, (long long)payload_bytes);
    int64_t span, total;
    if (__builtin_mul_overflow(n_frames, record_stride, &span) ||
        __builtin_mul_overflow(n_frames, payload_bytes + PIECE, &total))
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_records_gather: %lld records %lld bytes apart do not fit 64-bit offsets",
                  (long long)n_frames, (long long)record_stride);
    if (n_frames == 0) return LTMI_OK;
    if (!src || !dst) LTMI_FAIL(LTMI_E_INVALID, "ltmi_records_gather: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    // the largest W that divides all four: the lowest set bit of their union, 16 at most
    const uint64_t bits = (uint64_t)(uintptr_t)src | (uint64_t)record_stride | (uint64_t)payload_bytes |
                          (uint64_t)(uintptr_t)dst | 16u;
    const int w = (int)(bits & (~bits + 1));
    switch (w) {
        case 16: launch<16>(src, record_stride, n_frames, payload_bytes, dst, stream); break;
        case 8: launch<8>(src, record_stride, n_frames, payload_bytes, dst, stream); break;
        case 4: launch<4>(src, record_stride, n_frames, payload_bytes, dst, stream); break;
        case 2: launch<2>(src, record_stride, n_frames, payload_bytes, dst, stream); break;
        default: launch<1>(src, record_stride, n_frames, payload_bytes, dst, stream); break;
    }
    LTMI_HIP(hipGetLastError());
    static const char *const names[] = {"k_records<1>", "k_records<2>", "k_records<4>", "k_records<8>",
                                        "k_records<16>"};
    t_last_kernel = names[w == 16 ? 4 : w == 8 ? 3 : w == 4 ? 2 : w == 2 ? 1 : 0];
    return LTMI_OK;
}
