// ltmi_corr.hip -- template matching at given peaks.
//
// For every frame of a tile: the circular cross-correlation with ONE template through a batched real-to-complex
// hipFFT, a multiply by the template's stored spectrum and a batched complex-to-real hipFFT; then, in a window around
// every expected peak, the maximum, its position, a centre-of-mass refinement and the elevation of the maximum over
// the window.  Per batch of frames: k_corr_load (native pixels -> f32), hipFFT R2C, k_corr_mul, hipFFT C2R back into
// the frame workspace, k_corr_peaks (one wave per (frame, peak)).  The correlation never leaves the plan's workspace.
// ltmi_correlate_find (section 4.6d) runs the same transforms and then, in place of k_corr_peaks, the search of
// ltmi_peakfind.hip for the strongest local maxima of every map, rated by k_corr_found on the window code of k_corr_peaks.
#include "ltmi_fftshare.h"
#include <algorithm>

struct ltmi_corr_plan {
    int device = 0;
    int h = 0, w = 0, wc = 0;          // frame shape, complex columns w/2+1
    int batch = 0;                     // frames per hipFFT execution
    ltmi::DevBuf<float> real_buf;      // (batch, h, w) f32: the frames, then their correlations
    ltmi::DevBuf<hipfftComplex> spec;  // (batch, h, wc) c64
    ltmi::DevBuf<hipfftComplex> tspec; // (h, wc): conj(rfft2(ifftshift(t))) / (h w)
    ltmi::DevBuf<uint64_t> cand;       // candidate keys of ltmi_correlate_find (ltmi_peakfind.hip), grown on demand
    ltmi::FftHandle fwd, inv;          // batched R2C and C2R
    char last_kernel[128] = {0};
};

namespace ltmi {

// frames (native dtype, ld elements apart) -> contiguous f32.  A thread converts 8 consecutive pixels (one 16-B load
// for 2-byte pixels, two 16-B stores) where base and rows are 16-B aligned, single pixels otherwise.
template <typename T>
__global__ void __launch_bounds__(256)
k_corr_load(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_px, float *__restrict__ out,
            int vec_ok) {
    const int64_t n8 = vec_ok ? n_px / 8 : 0;
    // (the grid's y extent is capped at CORR_MAX_GRID_Y: a block walks every gridDim.y-th frame)
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const T *src = tile + f * ld;
        float *dst = out + f * n_px;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
            typedef T __attribute__((ext_vector_type(8))) vec_t;
            const vec_t x = __builtin_nontemporal_load((const vec_t *)(src + i * 8));
            *(float4 *)(dst + i * 8) = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
            *(float4 *)(dst + i * 8 + 4) = make_float4((float)x[4], (float)x[5], (float)x[6], (float)x[7]);
        }
        for (int64_t p = n8 * 8 + (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_px; p += (int64_t)gridDim.x * 256)
            dst[p] = (float)src[p];
    }
}

// tspec[i] = conj(spec[i]) * scale: the template's spectrum from the plan's own forward transform
__global__ void __launch_bounds__(256)
k_corr_template(const hipfftComplex *__restrict__ spec, int n_spec, float scale, hipfftComplex *__restrict__ tspec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_spec) return;
    const hipfftComplex c = spec[i];
    tspec[i] = make_float2(c.x * scale, -c.y * scale);
}

// spec[f, i] *= tspec[i] for the frames [0, n_frames).  A thread owns V consecutive elements of the half spectrum (V = 2:
// 16-B accesses, for an even element count) and walks `fpb` frames with the template's values in registers.
template <int V>
__global__ void __launch_bounds__(256)
k_corr_mul(hipfftComplex *__restrict__ spec, const hipfftComplex *__restrict__ tspec, int n_spec, int64_t n_frames,
           int fpb) {
    const int i = (blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n_spec) return;
    typedef float __attribute__((ext_vector_type(2 * V))) vec_t;
    const vec_t t = *(const vec_t *)(tspec + i);
    // (the grid's y extent is capped at CORR_MAX_GRID_Y: a block walks every gridDim.y-th group of fpb frames)
    for (int64_t f0 = (int64_t)blockIdx.y * fpb; f0 < n_frames; f0 += (int64_t)gridDim.y * fpb) {
        const int64_t f1 = min(n_frames, f0 + fpb);
        for (int64_t f = f0; f < f1; ++f) {
            vec_t *p = (vec_t *)(spec + f * n_spec + i);
            const vec_t s = *p;
            vec_t o;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                o[2 * j] = s[2 * j] * t[2 * j] - s[2 * j + 1] * t[2 * j + 1];
                o[2 * j + 1] = s[2 * j] * t[2 * j + 1] + s[2 * j + 1] * t[2 * j];
            }
            *p = o;
        }
    }
}

// The statistics of one window, by one wave: the lanes stride the window of radius r around (py, px) (row-major, clipped
// to the frame) and keep the maximum, the first index that holds it, and the float64 sums of (v - v0) and (v - v0)^2
// about the window's first value v0; a fixed-order shuffle tree combines the lanes.  Lane 0 then takes the centre of
// mass of the (2q+1)^2 neighbourhood of the maximum and stores the four results at slot `o`.  A non-finite value in the
// window (a frame with a non-finite pixel: the transforms carry it to every value of its correlation) gives
// peak_value = NaN.  Shared by k_corr_peaks and k_corr_found: the same instructions, so the same bits.
__device__ __forceinline__ void corr_window(const float *c, int h, int w, int py, int px, int r, int q, int lane,
                                            int64_t o, int32_t *centers, float *refineds, float *peak_values,
                                            float *peak_elevations) {
    // (the host has checked the peak; the clamps keep a bad one inside the frame all the same)
    const int y0 = min(max(py - r, 0), h - 1), y1 = max(min(py + r, h - 1), y0);
    const int x0 = min(max(px - r, 0), w - 1), x1 = max(min(px + r, w - 1), x0);
    const int ww = x1 - x0 + 1;
    const int cnt = ww * (y1 - y0 + 1);
    const float v0 = c[(int64_t)y0 * w + x0];
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    double s1 = 0.0, s2 = 0.0;
    int bad = 0;
    for (int i = lane; i < cnt; i += 64) {
        const int yy = i / ww;
        const float v = c[(int64_t)(y0 + yy) * w + x0 + (i - yy * ww)];
        bad |= !(fabsf(v) <= 3.402823466e+38f);
        if (v > best) {
            best = v;
            best_i = i;
        }
        const double d = (double)v - (double)v0;
        s1 += d;
        s2 += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(best_i, off, 64);
        if (ob > best || (ob == best && oi < best_i)) {
            best = ob;
            best_i = oi;
        }
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    bad = __any(bad);
    if (lane != 0) return;
    if (bad || best_i >= cnt) {
        const float nan = __builtin_nanf("");
        centers[2 * o] = y0;
        centers[2 * o + 1] = x0;
        refineds[2 * o] = (float)y0;
        refineds[2 * o + 1] = (float)x0;
        peak_values[o] = nan;
        peak_elevations[o] = nan;
        return;
    }
    const int cy = y0 + best_i / ww, cx = x0 + best_i % ww;
    const int ny0 = max(cy - q, 0), ny1 = min(cy + q, h - 1);
    const int nx0 = max(cx - q, 0), nx1 = min(cx + q, w - 1);
    float mn = best;
    for (int yy = ny0; yy <= ny1; ++yy)
        for (int xx = nx0; xx <= nx1; ++xx) mn = fminf(mn, c[(int64_t)yy * w + xx]);
    double sw = 0.0, sy = 0.0, sx = 0.0;
    for (int yy = ny0; yy <= ny1; ++yy)
        for (int xx = nx0; xx <= nx1; ++xx) {
            const double wgt = (double)c[(int64_t)yy * w + xx] - (double)mn;
            sw += wgt;
            sy += wgt * (double)yy;
            sx += wgt * (double)xx;
        }
    const bool flat = !(sw > 0.0);
    const double inv_n = 1.0 / (double)cnt;
    const double mean_d = s1 * inv_n;                       // mean(W) - v0
    const double var = fmax(s2 * inv_n - mean_d * mean_d, 0.0);
    const double sd = sqrt(var);
    centers[2 * o] = cy;
    centers[2 * o + 1] = cx;
    refineds[2 * o] = flat ? (float)cy : (float)(sy / sw);
    refineds[2 * o + 1] = flat ? (float)cx : (float)(sx / sw);
    peak_values[o] = best;
    peak_elevations[o] = sd > 0.0 ? (float)((((double)best - (double)v0) - mean_d) / sd) : 0.f;
}

// One wave per (frame, peak); peak k of frame f is peaks[f * peaks_stride + 2 k ..] (stride 0: one list for all frames).
__global__ void __launch_bounds__(256)
k_corr_peaks(const float *__restrict__ corr, int h, int w, int64_t n_frames, const int32_t *__restrict__ peaks,
             int64_t peaks_stride, int n_peaks, int r, int q, int32_t *__restrict__ centers,
             float *__restrict__ refineds, float *__restrict__ peak_values, float *__restrict__ peak_elevations) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_frames * n_peaks) return;                    // (the whole wave)
    const int64_t f = g / n_peaks;
    const int k = (int)(g - f * n_peaks);
    const int32_t *pk = peaks + f * peaks_stride + 2 * k;
    corr_window(corr + f * (int64_t)h * w, h, w, pk[0], pk[1], r, q, lane, f * n_peaks + k, centers, refineds,
                peak_values, peak_elevations);
}

// The same for the peaks a search found (section 4.6d): slot k < n_found[f] of frame f holds its centre in `centers`
// and gets the statistics of the window of radius r around it -- by step 1 of the search its first maximum is the
// centre itself, so the slot's centre is rewritten with the same value --; the other slots become (-1, -1) and NaN.
__global__ void __launch_bounds__(256)
k_corr_found(const float *__restrict__ maps, int64_t ld_map, int h, int w, int64_t n_frames,
             const int32_t *__restrict__ n_found, int n_peaks, int r, int q, int32_t *centers, float *refineds,
             float *peak_values, float *peak_elevations) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_frames * n_peaks) return;                    // (the whole wave)
    const int64_t f = g / n_peaks;
    const int k = (int)(g - f * n_peaks);
    const int64_t o = f * n_peaks + k;
    if (k >= n_found[f]) {
        if (lane == 0) {
            const float nan = __builtin_nanf("");
            centers[2 * o] = -1;
            centers[2 * o + 1] = -1;
            refineds[2 * o] = nan;
            refineds[2 * o + 1] = nan;
            peak_values[o] = nan;
            peak_elevations[o] = nan;
        }
        return;
    }
    const int py = centers[2 * o], px = centers[2 * o + 1];
    corr_window(maps + f * ld_map, h, w, py, px, r, q, lane, o, centers, refineds, peak_values, peak_elevations);
}

// gridDim.y of k_corr_load and k_corr_mul: the frames of a batch (max_batch of the plan, bounded only by 2^31 - 1
// pixels) beyond it are walked by the kernels' frame loops, as in ltmi_fft.hip
constexpr int64_t CORR_MAX_GRID_Y = 65535;

template <typename T>
static int run_corr_load(const void *tile, int64_t ld, int64_t n, int64_t n_px, float *out, hipStream_t stream) {
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_px / 8 + 255) / 256, 32));
    const int vec_ok = (sizeof(T) <= 4) && ((uintptr_t)tile % 16 == 0) && ((ld * (int64_t)sizeof(T)) % 16 == 0) &&
                       (n_px % 8 == 0);
    hipLaunchKernelGGL((k_corr_load<T>), dim3(gx, (unsigned)std::min(n, CORR_MAX_GRID_Y)), dim3(256), 0, stream,
                       (const T *)tile, ld, n, n_px, out, vec_ok);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

int corr_load(const void *src, int tile_dtype, int64_t ld, int64_t n, int64_t n_px, float *out, hipStream_t stream) {
    if (!corr_takes(tile_dtype)) LTMI_FAIL(LTMI_E_DTYPE, "k_corr_load: unsupported tile dtype %s", dtype_name(tile_dtype));
    return visit_real_dtype(tile_dtype, [&](auto t) { return run_corr_load<decltype(t)>(src, ld, n, n_px, out, stream); },
                            (int)LTMI_E_DTYPE);
}

static void corr_mul(ltmi_corr_plan *p, int64_t n, hipStream_t stream) {
    const int n_spec = p->h * p->wc;
    const int fpb = 8;
    const unsigned gy = (unsigned)std::min((n + fpb - 1) / fpb, CORR_MAX_GRID_Y);
    if (n_spec % 2 == 0)
        hipLaunchKernelGGL((k_corr_mul<2>), dim3((unsigned)((n_spec / 2 + 255) / 256), gy), dim3(256), 0, stream,
                           (hipfftComplex *)p->spec, (const hipfftComplex *)p->tspec, n_spec, n, fpb);
    else
        hipLaunchKernelGGL((k_corr_mul<1>), dim3((unsigned)((n_spec + 255) / 256), gy), dim3(256), 0, stream,
                           (hipfftComplex *)p->spec, (const hipfftComplex *)p->tspec, n_spec, n, fpb);
}

}  // namespace ltmi

using namespace ltmi;

// the two hipFFT plans, the workspace and the template's spectrum
static int corr_setup(ltmi_corr_plan *p, const float *template_host) {
    const int64_t n_px = (int64_t)p->h * p->w;
    const int n_spec = p->h * p->wc;
    hipError_t e = p->real_buf.alloc_zero((size_t)p->batch * n_px);
    if (e == hipSuccess) e = p->spec.alloc((size_t)p->batch * n_spec);
    if (e == hipSuccess) e = p->tspec.alloc((size_t)n_spec);
    if (e != hipSuccess) LTMI_FAIL((int)e, "ltmi_corr_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
    int n[2] = {p->h, p->w};
    int rc = p->fwd.plan_many(2, n, p->h * p->w, n_spec, HIPFFT_R2C, p->batch);
    if (rc == LTMI_OK) rc = p->inv.plan_many(2, n, n_spec, p->h * p->w, HIPFFT_C2R, p->batch);
    if (rc != LTMI_OK) return rc;
    // ifftshift(t)[y, x] = t[(y + h/2) % h, (x + w/2) % w] as frame 0 of a zero batch, through the forward plan
    std::vector<float> shifted((size_t)n_px);
    for (int y = 0; y < p->h; ++y)
        for (int x = 0; x < p->w; ++x)
            shifted[(size_t)y * p->w + x] =
                template_host[(size_t)((y + p->h / 2) % p->h) * p->w + (x + p->w / 2) % p->w];
    LTMI_HIP(hipMemcpy(p->real_buf, shifted.data(), (size_t)n_px * sizeof(float), hipMemcpyHostToDevice));
    rc = p->fwd.r2c(p->real_buf, p->spec);
    if (rc != LTMI_OK) return rc;
    hipLaunchKernelGGL(k_corr_template, dim3((unsigned)((n_spec + 255) / 256)), dim3(256), 0, nullptr,
                       (const hipfftComplex *)p->spec, n_spec, (float)(1.0 / (double)n_px), (hipfftComplex *)p->tspec);
    LTMI_HIP(hipGetLastError());
    LTMI_HIP(hipStreamSynchronize(nullptr));
    return LTMI_OK;
}

extern "C" int ltmi_corr_plan_create(int device, int sig_h, int sig_w, int max_batch, const float *template_host,
                                     ltmi_corr_plan **out) {
    if (!out || !template_host || sig_h <= 0 || sig_w <= 0 || max_batch <= 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_corr_plan_create: bad arguments (%d x %d, batch %d)", sig_h, sig_w, max_batch);
    if ((int64_t)max_batch * sig_h * sig_w > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_corr_plan_create: a batch of %d frames of %d x %d exceeds 2^31 - 1 pixels",
                  max_batch, sig_h, sig_w);
    return plan_create(device, out, [&](ltmi_corr_plan *p) {
        p->h = sig_h;
        p->w = sig_w;
        p->wc = sig_w / 2 + 1;
        p->batch = max_batch;
        return corr_setup(p, template_host);
    });
}

extern "C" int ltmi_corr_plan_destroy(ltmi_corr_plan *p) { return plan_destroy(p); }

extern "C" const char *ltmi_corr_plan_last_kernel(const ltmi_corr_plan *p) {
    return p ? p->last_kernel : "";
}

// frames [f0, f0 + n) of the tile, n <= batch -> their correlation maps in real_buf, on `stream`: k_corr_load, R2C,
// k_corr_mul, C2R
static int corr_transform(ltmi_corr_plan *p, const void *tile, int tile_dtype, int64_t ld_tile, int64_t f0, int64_t n,
                          hipStream_t stream) {
    int rc = p->fwd.bind(stream);
    if (rc == LTMI_OK) rc = p->inv.bind(stream);
    if (rc == LTMI_OK)
        rc = load_and_forward(p->fwd, frame_at(tile, tile_dtype, ld_tile, f0), tile_dtype, ld_tile, n, p->batch,
                              (int64_t)p->h * p->w, p->real_buf, p->spec, stream);
    if (rc != LTMI_OK) return rc;
    corr_mul(p, n, stream);
    LTMI_HIP(hipGetLastError());
    return p->inv.c2r(p->spec, p->real_buf);
}

extern "C" int ltmi_correlate_peaks(ltmi_corr_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                                    int64_t ld_tile, const int32_t *peaks, int n_peaks, int crop_radius,
                                    int refine_radius, int32_t *centers, float *refineds, float *peak_values,
                                    float *peak_elevations, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_correlate_peaks: null plan");
    if (n_frames < 0 || n_peaks < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_correlate_peaks: negative frame or peak count");
    if (crop_radius < 1 || refine_radius < 1)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_correlate_peaks: crop_radius %d and refine_radius %d must be at least 1",
                  crop_radius, refine_radius);
    if (!corr_takes(tile_dtype))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_correlate_peaks: unsupported tile dtype %s", dtype_name(tile_dtype));
    const int64_t n_px = (int64_t)p->h * p->w;
    if (ld_tile < n_px) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_correlate_peaks: ld_tile < frame size");
    if (n_frames == 0 || n_peaks == 0) return LTMI_OK;
    if (!tile || !peaks || !centers || !refineds || !peak_values || !peak_elevations)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_correlate_peaks: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    {
        std::vector<int32_t> host((size_t)2 * n_peaks);
        LTMI_HIP(hipMemcpyAsync(host.data(), peaks, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        LTMI_HIP(hipStreamSynchronize(stream));
        for (int k = 0; k < n_peaks; ++k)
            if (host[2 * k] < 0 || host[2 * k] >= p->h || host[2 * k + 1] < 0 || host[2 * k + 1] >= p->w)
                LTMI_FAIL(LTMI_E_SHAPE, "ltmi_correlate_peaks: peak %d at (%d, %d) lies outside the %d x %d frame", k,
                          host[2 * k], host[2 * k + 1], p->h, p->w);
    }
    // (windows and neighbourhoods are clipped to the frame: a radius beyond its longer edge changes nothing)
    const int r = std::min(crop_radius, std::max(p->h, p->w));
    const int q = std::min(refine_radius, std::max(p->h, p->w));
    snprintf(p->last_kernel, sizeof(p->last_kernel),
             "k_corr_load<%s> + hipfft_r2c + k_corr_mul + hipfft_c2r + k_corr_peaks batch=%d", dtype_name(tile_dtype),
             p->batch);
    return for_each_batch(n_frames, p->batch, [&](int64_t f0, int64_t n) {
        const int rc = corr_transform(p, tile, tile_dtype, ld_tile, f0, n, stream);
        if (rc != LTMI_OK) return rc;
        const int64_t waves = n * n_peaks;
        hipLaunchKernelGGL(k_corr_peaks, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream,
                           (const float *)p->real_buf, p->h, p->w, n, peaks, (int64_t)0, n_peaks, r, q,
                           centers + 2 * f0 * n_peaks, refineds + 2 * f0 * n_peaks, peak_values + f0 * n_peaks,
                           peak_elevations + f0 * n_peaks);
        LTMI_HIP(hipGetLastError());
        return LTMI_OK;
    });
}

// the statistics of the peaks a search found, for ltmi_peakfind.hip
int ltmi::corr_found_stats(const float *maps, int64_t n_frames, int h, int w, int64_t ld_map, const PeakFind &pf,
                           const int32_t *n_found, int32_t *centers, float *refineds, float *peak_values,
                           float *peak_elevations, hipStream_t stream) {
    const int64_t waves = n_frames * pf.n_peaks;
    hipLaunchKernelGGL(k_corr_found, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, maps, ld_map, h, w,
                       n_frames, n_found, pf.n_peaks, pf.d, pf.q, centers, refineds, peak_values, peak_elevations);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

extern "C" int ltmi_correlate_find(ltmi_corr_plan *p, const void *tile, int tile_dtype, int64_t n_frames,
                                   int64_t ld_tile, int num_peaks, int min_distance, int border, float threshold_abs,
                                   float threshold_rel, int refine_radius, int32_t *n_found, int32_t *centers,
                                   float *refineds, float *peak_values, float *peak_elevations, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_correlate_find: null plan");
    if (n_frames < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_correlate_find: negative frame count");
    PeakFind pf;
    int rc = peakfind_params("ltmi_correlate_find", p->h, p->w, num_peaks, min_distance, border, threshold_abs,
                             threshold_rel, refine_radius, &pf);
    if (rc != LTMI_OK) return rc;
    if (!corr_takes(tile_dtype))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_correlate_find: unsupported tile dtype %s", dtype_name(tile_dtype));
    const int64_t n_px = (int64_t)p->h * p->w;
    if (ld_tile < n_px) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_correlate_find: ld_tile < frame size");
    if (n_frames == 0) return LTMI_OK;
    if (!tile || !n_found || !centers || !refineds || !peak_values || !peak_elevations)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_correlate_find: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    snprintf(p->last_kernel, sizeof(p->last_kernel),
             "k_corr_load<%s> + hipfft_r2c + k_corr_mul + hipfft_c2r + %s batch=%d", dtype_name(tile_dtype),
             peakfind_kernels(), p->batch);
    const int64_t N = pf.n_peaks;
    return for_each_batch(n_frames, p->batch, [&](int64_t f0, int64_t n) {
        const int rc = corr_transform(p, tile, tile_dtype, ld_tile, f0, n, stream);
        if (rc != LTMI_OK) return rc;
        return peakfind_search(p->real_buf, n, p->h, p->w, n_px, pf, p->cand, n_found + f0, centers + 2 * f0 * N,
                               refineds + 2 * f0 * N, peak_values + f0 * N, peak_elevations + f0 * N, stream);
    });
}
