// ltmi_holo.hip -- off-axis hologram reconstruction by the Fourier method.
//
// For every frame of a tile: F = fft2(y) / (h w); one sideband of F, centred at (sy, sx) of the unshifted layout, is
// cut out in (oh, ow) signed frequencies, moved to the origin and multiplied by a real aperture; the unnormalised inverse
// DFT of that is the reconstructed wave, optionally divided by a reference wave.  Per batch of frames: k_corr_load
// (native pixels -> f32, ltmi_corr.hip), hipFFT R2C, k_holo_crop (the gather from the half spectrum, with wrap-around
// and Hermitian mirroring), hipFFT C2C backward in place, k_holo_store.  No atomics: a second call gives the same bytes.
#include "ltmi_fftshare.h"
#include <algorithm>

struct ltmi_holo_plan {
    int device = 0;
    int h = 0, w = 0, wc = 0;           // frame shape, complex columns w/2+1
    int oh = 0, ow = 0;                 // output shape
    int sy = 0, sx = 0;                 // the sideband in the unshifted fft2 layout
    int batch = 0;                      // frames per hipFFT execution
    ltmi::DevBuf<float> real_buf;       // (batch, h, w) f32
    ltmi::DevBuf<hipfftComplex> spec;   // (batch, h, wc) c64
    ltmi::DevBuf<hipfftComplex> work;   // (batch, oh, ow) c64: the cropped sideband, then the wave
    ltmi::DevBuf<float> aperture;       // (oh, ow): float32(aperture / (h w))
    ltmi::DevBuf<hipfftComplex> ref_inv;   // (oh, ow): 1 / reference_wave, or none
    ltmi::FftHandle fwd, inv;           // batched R2C of (h, w), batched C2C of (oh, ow)
    char last_kernel[128] = {0};
};

namespace ltmi {

// index i of an axis of n in the unshifted layout -> its signed frequency (numpy.fft.fftfreq order, even and odd n)
__host__ __device__ static inline int holo_signed(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }

// G[f, u, v] = F[f, (sy + s(u, oh)) mod h, (sx + s(v, ow)) mod w] * aperture[u, v] from the half spectra S of real
// frames: column kx <= w/2 is stored, S[ky, kx]; the others follow from F[ky, kx] = conj(F[-ky mod h, w - kx]).  A
// thread owns one output element (u, v) and walks the frames of its grid row; the 64 elements of a wave are consecutive
// in (u, v), so along v its loads run up a spectrum row (stored kx) or down one (mirrored kx), in at most three runs
// per output row: the run ends where kx wraps past w - 1 and where it crosses column w/2.
__global__ void __launch_bounds__(256)
k_holo_crop(const float2 *__restrict__ spec, int64_t ld_spec, int64_t n_frames, int h, int w, int oh, int ow, int sy,
            int sx, const float *__restrict__ aperture, float2 *__restrict__ g, int64_t ld_g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)oh * ow) return;
    const int u = (int)(i / ow), v = (int)(i - (int64_t)u * ow);
    int ky = sy + holo_signed(u, oh);           // in (-h, 2h): |s(u, oh)| < oh <= h
    ky += ky < 0 ? h : 0;
    ky -= ky >= h ? h : 0;
    int kx = sx + holo_signed(v, ow);
    kx += kx < 0 ? w : 0;
    kx -= kx >= w ? w : 0;
    const bool mirrored = kx > w / 2;
    const int ry = mirrored ? (ky == 0 ? 0 : h - ky) : ky;
    const int rx = mirrored ? w - kx : kx;
    const int64_t src = (int64_t)ry * (w / 2 + 1) + rx;
    const float a = aperture[i];
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float2 s = spec[f * ld_spec + src];
        g[f * ld_g + i] = make_float2(s.x * a, (mirrored ? -s.y : s.y) * a);
    }
}

// out[f, p] = work[f, p] (* ref_inv[p]) for the frames [0, n_frames); rows of `out` are ld_out elements apart
template <bool REF>
__global__ void __launch_bounds__(256)
k_holo_store(const float2 *__restrict__ work, int64_t n_out, int64_t n_frames, const float2 *__restrict__ ref_inv,
             float2 *__restrict__ out, int64_t ld_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    float2 r = make_float2(1.f, 0.f);
    if (REF) r = ref_inv[i];
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const float2 c = work[f * n_out + i];
        out[f * ld_out + i] = REF ? make_float2(c.x * r.x - c.y * r.y, c.x * r.y + c.y * r.x) : c;
    }
}

static dim3 holo_grid(int64_t n_out, int64_t n_frames) {
    return dim3((unsigned)((n_out + 255) / 256), (unsigned)std::min<int64_t>(n_frames, 65535));
}

static int holo_crop_launch(const hipfftComplex *spec, int64_t ld_spec, int64_t n, int h, int w, int oh, int ow, int sy,
                            int sx, const float *aperture, hipfftComplex *g, int64_t ld_g, hipStream_t stream) {
    hipLaunchKernelGGL(k_holo_crop, holo_grid((int64_t)oh * ow, n), dim3(256), 0, stream, (const float2 *)spec, ld_spec,
                       n, h, w, oh, ow, sy, sx, aperture, (float2 *)g, ld_g);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

// what both entry points ask of the shapes
static int holo_check_shapes(const char *who, int h, int w, int oh, int ow, int sy, int sx) {
    if (h <= 0 || w <= 0 || oh <= 0 || ow <= 0)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: frame %d x %d and output %d x %d must be positive", who, h, w, oh, ow);
    if (oh > h || ow > w)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: output %d x %d exceeds the %d x %d frame", who, oh, ow, h, w);
    if (sy < 0 || sy >= h || sx < 0 || sx >= w)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: sideband (%d, %d) lies outside the %d x %d frame", who, sy, sx, h, w);
    return LTMI_OK;
}

}  // namespace ltmi

using namespace ltmi;

// the two hipFFT plans, the workspaces, the scaled aperture and the inverse reference
static int holo_setup(ltmi_holo_plan *p, const float *aperture_host, const float *ref_inv_host) {
    const int64_t n_px = (int64_t)p->h * p->w;
    const int n_spec = p->h * p->wc;
    const int n_out = p->oh * p->ow;
    hipError_t e = p->real_buf.alloc_zero((size_t)p->batch * n_px);
    if (e == hipSuccess) e = p->spec.alloc((size_t)p->batch * n_spec);
    if (e == hipSuccess) e = p->work.alloc_zero((size_t)p->batch * n_out);
    std::vector<float> scaled((size_t)n_out);
    for (int i = 0; i < n_out; ++i) scaled[i] = (float)((double)aperture_host[i] / (double)n_px);
    if (e == hipSuccess) e = p->aperture.upload(scaled.data(), (size_t)n_out);
    if (e == hipSuccess && ref_inv_host) e = p->ref_inv.upload((const hipfftComplex *)ref_inv_host, (size_t)n_out);
    if (e != hipSuccess) LTMI_FAIL((int)e, "ltmi_holo_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
    int n[2] = {p->h, p->w};
    int m[2] = {p->oh, p->ow};                  // (hipFFT takes axes of one element, a 1 x 1 output included)
    const int rc = p->fwd.plan_many(2, n, p->h * p->w, n_spec, HIPFFT_R2C, p->batch);
    return rc == LTMI_OK ? p->inv.plan_many(2, m, n_out, n_out, HIPFFT_C2C, p->batch) : rc;
}

extern "C" int ltmi_holo_plan_create(int device, int sig_h, int sig_w, int out_h, int out_w, int max_batch, int sb_y,
                                     int sb_x, const float *aperture_host, const float *ref_inv_host,
                                     ltmi_holo_plan **out) {
    if (!out || !aperture_host) LTMI_FAIL(LTMI_E_INVALID, "ltmi_holo_plan_create: null pointer");
    if (max_batch <= 0) LTMI_FAIL(LTMI_E_INVALID, "ltmi_holo_plan_create: batch %d must be positive", max_batch);
    const int rc_shape = holo_check_shapes("ltmi_holo_plan_create", sig_h, sig_w, out_h, out_w, sb_y, sb_x);
    if (rc_shape != LTMI_OK) return rc_shape;
    if ((int64_t)max_batch * sig_h * sig_w > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_plan_create: a batch of %d frames of %d x %d exceeds 2^31 - 1 pixels",
                  max_batch, sig_h, sig_w);
    return plan_create(device, out, [&](ltmi_holo_plan *p) {
        p->h = sig_h;
        p->w = sig_w;
        p->wc = sig_w / 2 + 1;
        p->oh = out_h;
        p->ow = out_w;
        p->sy = sb_y;
        p->sx = sb_x;
        p->batch = max_batch;
        return holo_setup(p, aperture_host, ref_inv_host);
    });
}

extern "C" int ltmi_holo_plan_destroy(ltmi_holo_plan *p) { return plan_destroy(p); }

extern "C" const char *ltmi_holo_plan_last_kernel(const ltmi_holo_plan *p) {
    return p ? p->last_kernel : "";
}

extern "C" int ltmi_holo_reconstruct(ltmi_holo_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                                     int64_t ld_tile, void *out, int64_t ld_out, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_holo_reconstruct: null plan");
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_reconstruct: negative frame count");
    if (!corr_takes(tile_dtype))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_holo_reconstruct: unsupported tile dtype %s", dtype_name(tile_dtype));
    const int64_t n_px = (int64_t)p->h * p->w;
    const int64_t n_out = (int64_t)p->oh * p->ow;
    if (ld_tile < n_px) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_reconstruct: ld_tile < frame size");
    if (ld_out < n_out) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_reconstruct: ld_out < output size");
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_holo_reconstruct: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    int rc_bind = p->fwd.bind(stream);
    if (rc_bind == LTMI_OK) rc_bind = p->inv.bind(stream);
    if (rc_bind != LTMI_OK) return rc_bind;
    snprintf(p->last_kernel, sizeof(p->last_kernel),
             "k_corr_load<%s> + hipfft_r2c + k_holo_crop + hipfft_c2c + k_holo_store batch=%d", dtype_name(tile_dtype),
             p->batch);
    return for_each_batch(n_frames, p->batch, [&](int64_t f0, int64_t n) {
        int rc = load_and_forward(p->fwd, frame_at(tile, tile_dtype, ld_tile, f0), tile_dtype, ld_tile, n, p->batch, n_px,
                                  p->real_buf, p->spec, stream);
        if (rc == LTMI_OK)
            rc = holo_crop_launch(p->spec, (int64_t)p->h * p->wc, n, p->h, p->w, p->oh, p->ow, p->sy, p->sx,
                                  p->aperture, p->work, n_out, stream);
        if (rc == LTMI_OK) rc = p->inv.c2c(p->work, p->work, HIPFFT_BACKWARD);
        if (rc != LTMI_OK) return rc;
        float2 *dst = (float2 *)out + f0 * ld_out;
        if (p->ref_inv)
            hipLaunchKernelGGL(k_holo_store<true>, holo_grid(n_out, n), dim3(256), 0, stream,
                               (const float2 *)p->work.get(), n_out, n, (const float2 *)p->ref_inv.get(), dst, ld_out);
        else
            hipLaunchKernelGGL(k_holo_store<false>, holo_grid(n_out, n), dim3(256), 0, stream,
                               (const float2 *)p->work.get(), n_out, n, (const float2 *)nullptr, dst, ld_out);
        LTMI_HIP(hipGetLastError());
        return LTMI_OK;
    });
}

extern "C" int ltmi_holo_crop(int device, const void *spec, int64_t n_frames, int h, int w, int64_t ld_spec, int out_h,
                              int out_w, int sb_y, int sb_x, const float *aperture_dev, void *g_out, int64_t ld_g,
                              void *stream_) {
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_crop: negative frame count");
    const int rc = holo_check_shapes("ltmi_holo_crop", h, w, out_h, out_w, sb_y, sb_x);
    if (rc != LTMI_OK) return rc;
    if (ld_spec < (int64_t)h * (w / 2 + 1)) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_crop: ld_spec < half-spectrum size");
    if (ld_g < (int64_t)out_h * out_w) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_holo_crop: ld_g < output size");
    if (n_frames == 0) return LTMI_OK;
    if (!spec || !aperture_dev || !g_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_holo_crop: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return holo_crop_launch((const hipfftComplex *)spec, ld_spec, n_frames, h, w, out_h, out_w, sb_y, sb_x, aperture_dev,
                            (hipfftComplex *)g_out, ld_g, (hipStream_t)stream_);
}
