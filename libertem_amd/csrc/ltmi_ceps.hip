// ltmi_ceps.hip -- exit-wave power cepstrum of every frame.
//
// For every frame of a tile: z = log(max(y, 0) + offset) * window; C = |fft2(z)| / (h w); the (oh, ow) quefrencies
// around the origin are cut out of C, centred like fftshift -- quefrency (0, 0) at (oh / 2, ow / 2) -- and multiplied by
// `keep`, which clears a disk around the origin.  Per batch of frames: k_ceps_load (native pixels -> windowed logarithm,
// f32), hipFFT R2C, k_ceps_store (the gather from the half spectrum with wrap-around and Hermitian mirroring, the
// magnitude, keep / (h w)).  No atomics: a second call gives the same bytes.
#include "ltmi_fftshare.h"
#include <algorithm>
#include <cmath>
#include <vector>

struct ltmi_ceps_plan {
    int device = 0;
    int h = 0, w = 0, wc = 0;           // frame shape, complex columns w/2+1
    int oh = 0, ow = 0;                 // output shape
    int batch = 0;                      // frames per hipFFT execution
    float offset = 1.f;                 // added before the logarithm
    ltmi::DevBuf<float> real_buf;       // (batch, h, w) f32: the windowed logarithms
    ltmi::DevBuf<hipfftComplex> spec;   // (batch, h, wc) c64
    ltmi::DevBuf<float> window;         // (h, w)
    ltmi::DevBuf<float> scale;          // (oh, ow): float32(keep / (h w))
    ltmi::FftHandle fwd;                // batched R2C of (h, w)
    char last_kernel[128] = {0};
};

namespace ltmi {

// out[f, p] = logf(max(tile[f, p], 0) + offset) * window[p], frames of the tile ld elements apart, those of `out`
// n_px.  A thread owns V consecutive pixels from p -- the 64 lanes of a wave read and write consecutive elements --,
// loads their window values once and walks every gridDim.y-th frame of the tile: the grid has a row per CEPS_FPT frames,
// 65535 at the most, and the loop covers the rest.  V = 4 (one vector load of the pixels, one 16-B store) where the
// rows of tile, window and out are aligned for it and n_px is a multiple of 4, V = 1 otherwise.
template <typename T, int V>
__global__ void __launch_bounds__(256)
k_ceps_load(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_px, float offset,
            const float *__restrict__ window, float *__restrict__ out) {
    const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (p >= n_px) return;                      // (V divides n_px: p + V <= n_px)
    if constexpr (V == 4) {
        typedef T __attribute__((ext_vector_type(4))) vec_t;
        const float4 wp = *(const float4 *)(window + p);
        for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
            const vec_t x = *(const vec_t *)(tile + f * ld + p);
            const float y0 = (float)x[0], y1 = (float)x[1], y2 = (float)x[2], y3 = (float)x[3];
            *(float4 *)(out + f * n_px + p) =
                make_float4(logf((y0 > 0.f ? y0 : 0.f) + offset) * wp.x, logf((y1 > 0.f ? y1 : 0.f) + offset) * wp.y,
                            logf((y2 > 0.f ? y2 : 0.f) + offset) * wp.z, logf((y3 > 0.f ? y3 : 0.f) + offset) * wp.w);
        }
    } else {
        const float wp = window[p];
        for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
            const float y = (float)tile[f * ld + p];
            out[f * n_px + p] = logf((y > 0.f ? y : 0.f) + offset) * wp;
        }
    }
}

// out[f, u, v] = |F[f, (u - oh/2) mod h, (v - ow/2) mod w]| * scale[u, v] from the half spectra S of real frames:
// column kx <= w/2 is stored, S[ky, kx]; the others have the magnitude of S[-ky mod h, w - kx].  A thread owns one
// output element (u, v) and walks the frames of its grid row; along v its loads run down a spectrum row (mirrored kx,
// v < ow/2) and then up one (stored kx).  Every float32 operation is rounded on its own (no contraction into an FMA,
// the correctly rounded square root): NumPy float32 gives the same bytes.
__global__ void __launch_bounds__(256)
k_ceps_store(const float2 *__restrict__ spec, int64_t ld_spec, int64_t n_frames, int h, int w, int oh, int ow,
             const float *__restrict__ scale, float *__restrict__ out, int64_t ld_out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)oh * ow) return;
    const int u = (int)(i / ow), v = (int)(i - (int64_t)u * ow);
    int ky = u - oh / 2;                        // in (-h, h): oh <= h
    ky += ky < 0 ? h : 0;
    int kx = v - ow / 2;
    kx += kx < 0 ? w : 0;
    const bool mirrored = kx > w / 2;
    const int ry = mirrored ? (ky == 0 ? 0 : h - ky) : ky;
    const int rx = mirrored ? w - kx : kx;
    const int64_t src = (int64_t)ry * (w / 2 + 1) + rx;
    const float s = scale[i];
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float2 c = spec[f * ld_spec + src];
        const float rr = c.x * c.x;
        const float ii = c.y * c.y;
        const float m = __builtin_sqrtf(rr + ii);     // (correctly rounded: hipcc's default for float32 sqrt and divide)
        out[f * ld_out + i] = m * s;
    }
}

// gridDim.y of both kernels: one row per CEPS_FPT frames, so that a thread's window / scale values serve several
// frames, and 65535 rows at the most; the kernels' frame loops walk the frames of a row
constexpr int64_t CEPS_MAX_GRID_Y = 65535;
constexpr int64_t CEPS_FPT = 4;

static dim3 ceps_grid(int64_t n_threads, int64_t n_frames) {
    return dim3((unsigned)((n_threads + 255) / 256),
                (unsigned)std::min((n_frames + CEPS_FPT - 1) / CEPS_FPT, CEPS_MAX_GRID_Y));
}

template <typename T>
static int run_ceps_load(const void *tile, int64_t ld, int64_t n, int64_t n_px, float offset, const float *window,
                         float *out, hipStream_t stream) {
    const bool vec = n_px % 4 == 0 && ld % 4 == 0 && (uintptr_t)tile % (4 * sizeof(T)) == 0 &&
                     (uintptr_t)window % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (vec)
        hipLaunchKernelGGL((k_ceps_load<T, 4>), ceps_grid(n_px / 4, n), dim3(256), 0, stream, (const T *)tile, ld, n,
                           n_px, offset, window, out);
    else
        hipLaunchKernelGGL((k_ceps_load<T, 1>), ceps_grid(n_px, n), dim3(256), 0, stream, (const T *)tile, ld, n, n_px,
                           offset, window, out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int ceps_load_launch(const void *tile, int tile_dtype, int64_t ld, int64_t n, int64_t n_px, float offset,
                            const float *window, float *out, hipStream_t stream) {
    return visit_real_dtype(
        tile_dtype,
        [&](auto t) { return run_ceps_load<decltype(t)>(tile, ld, n, n_px, offset, window, out, stream); },
        (int)LTMI_E_DTYPE);
}

static int ceps_store_launch(const hipfftComplex *spec, int64_t ld_spec, int64_t n, int h, int w, int oh, int ow,
                             const float *scale, float *out, int64_t ld_out, hipStream_t stream) {
    hipLaunchKernelGGL(k_ceps_store, ceps_grid((int64_t)oh * ow, n), dim3(256), 0, stream, (const float2 *)spec,
                       ld_spec, n, h, w, oh, ow, scale, out, ld_out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

// what the entry points ask of the shapes
static int ceps_check_shapes(const char *who, int h, int w, int oh, int ow) {
    if (h <= 0 || w <= 0 || oh <= 0 || ow <= 0)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: frame %d x %d and output %d x %d must be positive", who, h, w, oh, ow);
    if (oh > h || ow > w)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: output %d x %d exceeds the %d x %d frame", who, oh, ow, h, w);
    return LTMI_OK;
}

// ... and of the offset: positive and finite (a NaN fails the first comparison)
static int ceps_check_offset(const char *who, float offset) {
    if (!(offset > 0.f) || std::isinf(offset))
        LTMI_FAIL(LTMI_E_INVALID, "%s: offset %g must be positive and finite", who, (double)offset);
    return LTMI_OK;
}

}  // namespace ltmi

using namespace ltmi;

// the hipFFT plan, the workspaces, the window and keep / (h w)
static int ceps_setup(ltmi_ceps_plan *p, const float *window_host, double dc_radius) {
    const int64_t n_px = (int64_t)p->h * p->w;
    const int n_spec = p->h * p->wc;
    const int n_out = p->oh * p->ow;
    std::vector<float> scale((size_t)n_out);
    for (int u = 0; u < p->oh; ++u)
        for (int v = 0; v < p->ow; ++v) {
            const bool keep = !(std::hypot((double)(u - p->oh / 2), (double)(v - p->ow / 2)) < dc_radius);
            scale[(size_t)u * p->ow + v] = (float)((keep ? 1.0 : 0.0) / (double)n_px);
        }
    hipError_t e = p->real_buf.alloc_zero((size_t)p->batch * n_px);
    if (e == hipSuccess) e = p->spec.alloc((size_t)p->batch * n_spec);
    if (e == hipSuccess) e = p->window.upload(window_host, (size_t)n_px);
    if (e == hipSuccess) e = p->scale.upload(scale.data(), (size_t)n_out);
    if (e != hipSuccess) LTMI_FAIL((int)e, "ltmi_ceps_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
    int n[2] = {p->h, p->w};
    return p->fwd.plan_many(2, n, p->h * p->w, n_spec, HIPFFT_R2C, p->batch);
}

extern "C" int ltmi_ceps_plan_create(int device, int sig_h, int sig_w, int out_h, int out_w, int max_batch, float offset,
                                     const float *window_host, double dc_radius, ltmi_ceps_plan **out) {
    if (!out || !window_host) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_plan_create: null pointer");
    if (max_batch <= 0) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_plan_create: batch %d must be positive", max_batch);
    int rc = ceps_check_offset("ltmi_ceps_plan_create", offset);
    if (rc != LTMI_OK) return rc;
    if (!(dc_radius >= 0.0))
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_plan_create: dc_radius %g must not be negative", dc_radius);
    rc = ceps_check_shapes("ltmi_ceps_plan_create", sig_h, sig_w, out_h, out_w);
    if (rc != LTMI_OK) return rc;
    if ((int64_t)max_batch * sig_h * sig_w > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_plan_create: a batch of %d frames of %d x %d exceeds 2^31 - 1 pixels",
                  max_batch, sig_h, sig_w);
    return plan_create(device, out, [&](ltmi_ceps_plan *p) {
        p->h = sig_h;
        p->w = sig_w;
        p->wc = sig_w / 2 + 1;
        p->oh = out_h;
        p->ow = out_w;
        p->batch = max_batch;
        p->offset = offset;
        return ceps_setup(p, window_host, dc_radius);
    });
}

extern "C" int ltmi_ceps_plan_destroy(ltmi_ceps_plan *p) { return plan_destroy(p); }

extern "C" const char *ltmi_ceps_plan_last_kernel(const ltmi_ceps_plan *p) {
    return p ? p->last_kernel : "";
}

extern "C" int ltmi_ceps_transform(ltmi_ceps_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                                   int64_t ld_tile, float *out, int64_t ld_out, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_transform: null plan");
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_transform: negative frame count");
    if (!corr_takes(tile_dtype))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_ceps_transform: unsupported tile dtype %s", dtype_name(tile_dtype));
    const int64_t n_px = (int64_t)p->h * p->w;
    const int64_t n_out = (int64_t)p->oh * p->ow;
    if (ld_tile < n_px) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_transform: ld_tile < frame size");
    if (ld_out < n_out) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_transform: ld_out < output size");
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_transform: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_bind = p->fwd.bind(stream);
    if (rc_bind != LTMI_OK) return rc_bind;
    snprintf(p->last_kernel, sizeof(p->last_kernel), "k_ceps_load<%s> + hipfft_r2c + k_ceps_store batch=%d",
             dtype_name(tile_dtype), p->batch);
    return for_each_batch(n_frames, p->batch, [&](int64_t f0, int64_t n) {
        int rc = ceps_load_launch(frame_at(tile, tile_dtype, ld_tile, f0), tile_dtype, ld_tile, n, n_px, p->offset,
                                  p->window, p->real_buf, stream);
        if (rc == LTMI_OK) rc = zero_tail(p->real_buf, n, p->batch, n_px, stream);
        if (rc == LTMI_OK) rc = p->fwd.r2c(p->real_buf, p->spec);
        if (rc != LTMI_OK) return rc;
        return ceps_store_launch(p->spec, (int64_t)p->h * p->wc, n, p->h, p->w, p->oh, p->ow, p->scale,
                                 out + f0 * ld_out, ld_out, stream);
    });
}

extern "C" int ltmi_ceps_load(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                              int64_t n_px, float offset, const float *window_dev, float *out, void *stream_) {
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_load: negative frame count");
    if (n_px <= 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_load: frame size %lld must be positive", (long long)n_px);
    if (ld_tile < n_px) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_load: ld_tile < frame size");
    if (!corr_takes(tile_dtype))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_ceps_load: unsupported tile dtype %s", dtype_name(tile_dtype));
    const int rc = ceps_check_offset("ltmi_ceps_load", offset);
    if (rc != LTMI_OK) return rc;
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !window_dev || !out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_load: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return ceps_load_launch(tile, tile_dtype, ld_tile, n_frames, n_px, offset, window_dev, out, (hipStream_t)stream_);
}

extern "C" int ltmi_ceps_store(int device, const void *spec, int64_t n_frames, int h, int w, int64_t ld_spec, int out_h,
                               int out_w, const float *scale_dev, float *out, int64_t ld_out, void *stream_) {
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_store: negative frame count");
    const int rc = ceps_check_shapes("ltmi_ceps_store", h, w, out_h, out_w);
    if (rc != LTMI_OK) return rc;
    if (ld_spec < (int64_t)h * (w / 2 + 1)) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_store: ld_spec < half-spectrum size");
    if (ld_out < (int64_t)out_h * out_w) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ceps_store: ld_out < output size");
    if (n_frames == 0) return LTMI_OK;
    if (!spec || !scale_dev || !out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ceps_store: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return ceps_store_launch((const hipfftComplex *)spec, ld_spec, n_frames, h, w, out_h, out_w, scale_dev, out, ld_out,
                             (hipStream_t)stream_);
}
