// ltmi_wdd.hip -- Wigner-distribution deconvolution of a focused-probe 4D-STEM scan, the object's DC row (DESIGN.md
// section 4.6i).
//
// For every spatial frequency Q of the scan the probe's Wigner function on a (By, Bx) window of the detector is
// deconvolved with a Wiener filter.  With F[K, Q] = sum_rho W[rho] exp(+2 pi i K rho / B), a function of the geometry
// alone, the deconvolved value is S[Q] = sum_K G[K, Q] F[K, Q] / (By Bx): the spectra G are never transformed over the
// detector.  ltmi_wdd_filter builds F, a batch of Qs at a time: k_wdd_gamma (the float64 disk predicates of
// ltmi_ssb.hip as complex64 0 / 1), one batched backward C2C hipFFT of (By, Bx) (= chi), k_wdd_wiener (pointwise), the
// same hipFFT again.  The plan keeps F for all Qs, produces G with the front end of the single-sideband plan
// (ltmi_ssbshare.h) and sums with k_wdd_dot, which reduces exactly as k_ssb_trotter does: thread-strided, a fixed
// shuffle tree, the waves in order through LDS, the batches in order through a per-Q accumulator.  k_wdd_finish
// mirrors, conjugates and normalises.  No atomics: a second call gives the same bytes.
#include "ltmi_ssbshare.h"
#include <algorithm>
#include <cmath>

// the disk predicates agree with a NumPy float64 evaluation of the same expressions bit for bit
#pragma clang fp contract(off)

namespace ltmi {

// the detector window [y0, y0 + by) x [x0, x0 + bx), row-major
struct WddWindow {
    int y0, x0, by, bx;
};

__host__ __device__ static inline bool wdd_in_a(const SsbGeom &g, const WddWindow &w, int k) {
    const int v = k / w.bx;
    return ssb_in_disk((double)(w.y0 + v), (double)(w.x0 + (k - v * w.bx)), g.cy, g.cx, g.semiconv_pix * g.semiconv_pix);
}

// gamma[j, k] = 1 where window pixel k lies in the disk around (cy, cx) and in the one around (cy, cx) - d(q0 + j),
// else 0, for j < n.  A thread owns one window pixel and walks the Qs of its grid row.
__global__ void __launch_bounds__(256)
k_wdd_gamma(float2 *__restrict__ gamma, int64_t q0, int64_t n, SsbGeom g, WddWindow w) {
    const int n_k = w.by * w.bx;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_k) return;
    const int v = k / w.bx;
    const double y = (double)(w.y0 + v), x = (double)(w.x0 + (k - v * w.bx));
    const double r2 = g.semiconv_pix * g.semiconv_pix;
    const bool in_a = ssb_in_disk(y, x, g.cy, g.cx, r2);
    for (int64_t j = blockIdx.y; j < n; j += gridDim.y) {
        const int64_t q = q0 + j;
        const int iy = (int)(q / g.nx), ix = (int)(q - (int64_t)iy * g.nx);
        double d_y, d_x;
        ssb_shift(g, iy, ix, &d_y, &d_x);
        const bool in_m = ssb_in_disk(y, x, g.cy - d_y, g.cx - d_x, r2);
        gamma[j * n_k + k] = make_float2(in_a && in_m ? 1.f : 0.f, 0.f);
    }
}

// chi -> W = conj(chi) / (|chi|^2 + epsilon P^2), in place; the quotient is float64, cast once
__global__ void __launch_bounds__(256)
k_wdd_wiener(float2 *__restrict__ chi, int64_t total, double eps_p2) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float2 c = chi[i];
        const double re = (double)c.x, im = (double)c.y;
        const double den = re * re + im * im + eps_p2;
        chi[i] = make_float2((float)(re / den), (float)(-im / den));
    }
}

// One workgroup per Q = (iy, ix), walking the Qs with a grid stride: acc[Q] (+)= sum over j < n_k of G[j, Q] F[Q, j].
// spec[(ry nxc + rx) ld_spec + j] is G[j, ry, rx] for rx <= nx / 2; a Q with ix > nx / 2 reads the conjugate at
// ((ny - iy) mod ny, nx - ix).  filt[Q ld_filt + j] is F.  Thread t takes the columns t, t + 256, ... in that order, a
// wave adds its lanes by a fixed shuffle tree, thread 0 adds the four waves in order: the float64 sums repeat bit for
// bit.  first: the accumulator starts at zero.
__global__ void __launch_bounds__(256)
k_wdd_dot(const float2 *__restrict__ spec, int64_t ld_spec, const float2 *__restrict__ filt, int64_t ld_filt, int n_k,
          int ny, int nx, double2 *__restrict__ acc, int first) {
    __shared__ double s_sum[4][2];
    const int nxc = nx / 2 + 1;
    const int64_t n_q = (int64_t)ny * nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = blockIdx.x; q < n_q; q += gridDim.x) {
        const int iy = (int)(q / nx), ix = (int)(q - (int64_t)iy * nx);
        const bool mirrored = ix > nx / 2;
        const int ry = mirrored ? (iy == 0 ? 0 : ny - iy) : iy;
        const int rx = mirrored ? nx - ix : ix;
        const float2 *row = spec + ((int64_t)ry * nxc + rx) * ld_spec;
        const float2 *f = filt + q * ld_filt;
        double sr = 0., si = 0.;
        for (int k = threadIdx.x; k < n_k; k += 256) {
            const float2 v = row[k], c = f[k];
            const double gr = (double)v.x, gi = mirrored ? -(double)v.y : (double)v.y;
            const double fr = (double)c.x, fi = (double)c.y;
            sr += gr * fr - gi * fi;
            si += gr * fi + gi * fr;
        }
        for (int off = 32; off > 0; off >>= 1) {
            sr += __shfl_down(sr, off, 64);
            si += __shfl_down(si, off, 64);
        }
        if (lane == 0) {
            s_sum[wave][0] = sr;
            s_sum[wave][1] = si;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double2 a = make_double2(0., 0.);
            if (!first) a = acc[q];
            for (int w = 0; w < 4; ++w) {
                a.x += s_sum[w][0];
                a.y += s_sum[w][1];
            }
            acc[q] = a;
        }
        __syncthreads();
    }
}

// fourier[Q] = conj(S[-Q mod (ny, nx)]) / |S[0, 0]| with S = acc / n_window, float64, cast once
__global__ void __launch_bounds__(256)
k_wdd_finish(const double2 *__restrict__ acc, int ny, int nx, double n_window, float2 *__restrict__ fourier) {
    const int64_t n_q = (int64_t)ny * nx;
    const double2 dc = acc[0];
    const double norm = hypot(dc.x / n_window, dc.y / n_window);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n_q; q += (int64_t)gridDim.x * 256) {
        const int iy = (int)(q / nx), ix = (int)(q - (int64_t)iy * nx);
        const double2 s = acc[(int64_t)(iy == 0 ? 0 : ny - iy) * nx + (ix == 0 ? 0 : nx - ix)];
        fourier[q] = make_float2((float)(s.x / n_window / norm), (float)(-(s.y / n_window) / norm));
    }
}

// gridDim.y of k_wdd_gamma: the Qs beyond it are walked by the kernel's loop
constexpr int64_t WDD_MAX_GRID_Y = 65535;
// workgroups of k_wdd_dot, k_wdd_wiener and k_wdd_finish: what lies beyond them is walked with a grid stride
constexpr int64_t WDD_MAX_GRID_X = 1 << 20;
// the Qs of one hipFFT execution of the filter builder, where the caller does not say: 64 MiB of chi
constexpr int64_t WDD_FILTER_BYTES = 64 << 20;

// what every entry point asks of the window; the scan and the geometry go through ssb_check
static int wdd_check(const char *who, int ny, int nx, const int *window, const double *geom, double epsilon,
                     SsbGeom *g, WddWindow *w) {
    if (window[2] < 1 || window[3] < 1)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: window %d x %d must be positive", who, window[2], window[3]);
    if ((int64_t)window[2] * window[3] > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: window %d x %d exceeds 2^31 - 1 pixels", who, window[2], window[3]);
    if (!(std::isfinite(epsilon) && epsilon > 0.))
        LTMI_FAIL(LTMI_E_SHAPE, "%s: epsilon %g must be positive and finite", who, epsilon);
    *w = WddWindow{window[0], window[1], window[2], window[3]};
    return ssb_check(who, ny, nx, window[2] * window[3], 1, geom, 1, g);
}

// P: the window pixels inside the disk, by the predicate the device evaluates
static int wdd_disk_pixels(const SsbGeom &g, const WddWindow &w) {
    int n = 0;
    for (int k = 0; k < w.by * w.bx; ++k) n += wdd_in_a(g, w, k) ? 1 : 0;
    return n;
}

// The filter builder: one batched backward C2C hipFFT of (by, bx) and `batch` windows of workspace.
struct WddFilter {
    int batch = 0;
    double eps_p2 = 0.;
    DevBuf<hipfftComplex> work;         // (batch, by bx) c64: gamma, chi, W in turn
    FftHandle c2c;

    int setup(const char *who, const SsbGeom &g, const WddWindow &w, double epsilon, int batch_) {
        const int p = wdd_disk_pixels(g, w);
        if (p < 1) LTMI_FAIL(LTMI_E_SHAPE, "%s: no pixel of the window lies within semiconv_pix %g of (%g, %g)", who,
                             g.semiconv_pix, g.cy, g.cx);
        eps_p2 = epsilon * (double)p * (double)p;
        batch = batch_;
        const int n_k = w.by * w.bx;
        const hipError_t e = work.alloc_zero((size_t)batch * n_k);
        if (e != hipSuccess) LTMI_FAIL((int)e, "%s: workspace allocation failed: %s", who, hipGetErrorString(e));
        int n[2] = {w.by, w.bx};                // a window of one row or one column is a batch of 1D transforms
        if (w.by == 1) return c2c.plan_many(1, n + 1, n_k, n_k, HIPFFT_C2C, batch);
        if (w.bx == 1) return c2c.plan_many(1, n, n_k, n_k, HIPFFT_C2C, batch);
        return c2c.plan_many(2, n, n_k, n_k, HIPFFT_C2C, batch);
    }

    // F of the Qs [q0, q0 + n_q) -> out[(q - q0) n_k + k]
    int run(const SsbGeom &g, const WddWindow &w, int64_t q0, int64_t n_q, hipfftComplex *out, hipStream_t stream) {
        const int rc_bind = c2c.bind(stream);
        if (rc_bind != LTMI_OK) return rc_bind;
        const int64_t n_k = (int64_t)w.by * w.bx;
        return for_each_batch(n_q, batch, [&](int64_t j0, int64_t n) {
            // the plan always transforms `batch` windows: behind a partial last batch lie those of an earlier one
            hipLaunchKernelGGL(k_wdd_gamma, dim3((unsigned)((n_k + 255) / 256), (unsigned)std::min(n, WDD_MAX_GRID_Y)),
                               dim3(256), 0, stream, (float2 *)work.get(), q0 + j0, n, g, w);
            LTMI_HIP(hipGetLastError());
            int rc = c2c.c2c(work, work, HIPFFT_BACKWARD);
            if (rc != LTMI_OK) return rc;
            const int64_t total = n * n_k;
            hipLaunchKernelGGL(k_wdd_wiener, dim3((unsigned)std::min((total + 255) / 256, WDD_MAX_GRID_X)), dim3(256),
                               0, stream, (float2 *)work.get(), total, eps_p2);
            LTMI_HIP(hipGetLastError());
            hipfftComplex *dst = out + j0 * n_k;
            if (n == batch) return c2c.c2c(work, dst, HIPFFT_BACKWARD);
            // a partial batch would write past its Qs: transform in place and copy what belongs to them
            rc = c2c.c2c(work, work, HIPFFT_BACKWARD);
            if (rc != LTMI_OK) return rc;
            LTMI_HIP(hipMemcpyAsync(dst, work.get(), (size_t)total * sizeof(hipfftComplex), hipMemcpyDeviceToDevice,
                                    stream));
            return (int)LTMI_OK;
        });
    }
};

static int wdd_dot_launch(const hipfftComplex *spec, int64_t ld_spec, const hipfftComplex *filt, int64_t ld_filt,
                          int n_k, int ny, int nx, double2 *acc, bool first, hipStream_t stream) {
    const int64_t n_q = (int64_t)ny * nx;
    hipLaunchKernelGGL(k_wdd_dot, dim3((unsigned)std::min(n_q, WDD_MAX_GRID_X)), dim3(256), 0, stream,
                       (const float2 *)spec, ld_spec, (const float2 *)filt, ld_filt, n_k, ny, nx, acc, first ? 1 : 0);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int wdd_finish_launch(const double2 *acc, int ny, int nx, int n_window, hipfftComplex *fourier,
                             hipStream_t stream) {
    const int64_t n_q = (int64_t)ny * nx;
    hipLaunchKernelGGL(k_wdd_finish, dim3((unsigned)std::min((n_q + 255) / 256, WDD_MAX_GRID_X)), dim3(256), 0, stream,
                       acc, ny, nx, (double)n_window, (float2 *)fourier);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

}  // namespace ltmi

using namespace ltmi;

struct ltmi_wdd_plan {
    int device = 0;
    int n_window = 0;                   // By Bx
    int batch = 0;                      // window pixels per hipFFT execution over the scan
    SsbGeom g = {};
    DevBuf<hipfftComplex> filt;         // (ny nx, By Bx) c64: F, built at creation
    DevBuf<double2> acc;                // (ny nx): the sums of the batches so far
    SsbFront front;                     // bf columns -> spectra (ny nxc, batch), and its workspace
    char last_kernel[128] = {0};
};

extern "C" int ltmi_wdd_filter(int device, int nav_y, int nav_x, const int *window, const double *geom, double epsilon,
                               int64_t q0, int64_t n_q, int q_batch, void *filter_out, void *stream_) {
    if (!window || !geom) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_filter: null pointer");
    if (q_batch <= 0) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_filter: batch %d must be positive", q_batch);
    SsbGeom g;
    WddWindow w;
    const int rc = wdd_check("ltmi_wdd_filter", nav_y, nav_x, window, geom, epsilon, &g, &w);
    if (rc != LTMI_OK) return rc;
    if (q0 < 0 || n_q < 0 || q0 + n_q > (int64_t)nav_y * nav_x)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_filter: the Qs [%lld, %lld) lie outside the %d x %d scan", (long long)q0,
                  (long long)(q0 + n_q), nav_y, nav_x);
    const int batch = (int)std::min<int64_t>(q_batch, std::max<int64_t>(n_q, 1));
    if ((int64_t)batch * w.by * w.bx > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_filter: a batch of %d windows of %d x %d exceeds 2^31 - 1 values", batch, w.by,
                  w.bx);
    if (n_q == 0) return LTMI_OK;
    if (!filter_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_filter: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    WddFilter f;
    int rc_run = f.setup("ltmi_wdd_filter", g, w, epsilon, batch);
    if (rc_run == LTMI_OK) rc_run = f.run(g, w, q0, n_q, (hipfftComplex *)filter_out, stream);
    // the workspace and the hipFFT plan go with this call: not before the work that uses them is done
    const hipError_t e = hipStreamSynchronize(stream);
    if (rc_run != LTMI_OK) return rc_run;
    LTMI_HIP(e);
    return LTMI_OK;
}

extern "C" int ltmi_wdd_dot(int device, const void *spec, int64_t ld_spec, int nav_y, int nav_x, const void *filter,
                            int64_t ld_filter, int k0, int n_k, double *acc, int first, void *stream_) {
    if (nav_y <= 0 || nav_x <= 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_dot: scan %d x %d must be positive", nav_y, nav_x);
    if ((int64_t)nav_y * nav_x > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_dot: scan %d x %d exceeds 2^31 - 1 positions", nav_y, nav_x);
    if (k0 < 0 || n_k <= 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_dot: pixel range [%d, %d + %d) is empty or negative", k0, k0, n_k);
    if (ld_spec < n_k) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_dot: ld_spec < the %d pixels of the range", n_k);
    if (ld_filter < (int64_t)k0 + n_k) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_dot: ld_filter < the end of the pixel range");
    if (!spec || !filter || !acc) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_dot: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return wdd_dot_launch((const hipfftComplex *)spec, ld_spec, (const hipfftComplex *)filter + k0, ld_filter, n_k, nav_y,
                          nav_x, (double2 *)acc, first != 0, (hipStream_t)stream_);
}

extern "C" int ltmi_wdd_finish(int device, const double *acc, int nav_y, int nav_x, int n_window, void *fourier_out,
                               void *stream_) {
    if (nav_y <= 0 || nav_x <= 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_finish: scan %d x %d must be positive", nav_y, nav_x);
    if ((int64_t)nav_y * nav_x > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_finish: scan %d x %d exceeds 2^31 - 1 positions", nav_y, nav_x);
    if (n_window < 1) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_finish: a window of %d pixels", n_window);
    if (!acc || !fourier_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_finish: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return wdd_finish_launch((const double2 *)acc, nav_y, nav_x, n_window, (hipfftComplex *)fourier_out,
                             (hipStream_t)stream_);
}

extern "C" int ltmi_wdd_plan_create(int device, int nav_y, int nav_x, const int *window, int max_batch,
                                    const double *geom, double epsilon, ltmi_wdd_plan **out) {
    if (!out || !window || !geom) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_plan_create: null pointer");
    if (max_batch <= 0) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_plan_create: batch %d must be positive", max_batch);
    SsbGeom g;
    WddWindow w;
    const int rc_shape = wdd_check("ltmi_wdd_plan_create", nav_y, nav_x, window, geom, epsilon, &g, &w);
    if (rc_shape != LTMI_OK) return rc_shape;
    ssb_column_as_row(&g);
    const int n_window = w.by * w.bx;
    const int64_t n_q = (int64_t)nav_y * nav_x;
    const int batch = std::min(max_batch, n_window);
    if ((int64_t)batch * n_q > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_plan_create: a batch of %d scans of %d x %d exceeds 2^31 - 1 values", batch,
                  nav_y, nav_x);
    return plan_create(device, out, [&](ltmi_wdd_plan *p) {
        p->n_window = n_window;
        p->batch = batch;
        p->g = g;
        // F for every Q stays in the plan
        const unsigned long long need = (unsigned long long)n_q * n_window * sizeof(hipfftComplex);
        size_t free_b = 0, total_b = 0;
        LTMI_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b || p->filt.alloc((size_t)n_q * n_window) != hipSuccess) {
            (void)hipGetLastError();
            LTMI_FAIL(LTMI_E_NOMEM, "ltmi_wdd_plan_create: the filter of %lld Qs x %d window pixels needs %llu bytes of "
                      "device memory, %zu are free", (long long)n_q, n_window, need, free_b);
        }
        const hipError_t e = p->acc.alloc_zero((size_t)n_q);
        if (e != hipSuccess) LTMI_FAIL((int)e, "ltmi_wdd_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
        {
            WddFilter f;                        // its workspace goes when F stands
            const int q_batch = (int)std::max<int64_t>(1, std::min<int64_t>(n_q, WDD_FILTER_BYTES / ((int64_t)n_window * 8)));
            int rc = f.setup("ltmi_wdd_plan_create", g, w, epsilon, q_batch);
            if (rc == LTMI_OK) rc = f.run(g, w, 0, n_q, p->filt, nullptr);
            const hipError_t done = hipStreamSynchronize(nullptr);
            if (rc != LTMI_OK) return rc;
            LTMI_HIP(done);
        }
        return p->front.setup("ltmi_wdd_plan_create", p->g, p->batch);
    });
}

extern "C" int ltmi_wdd_plan_destroy(ltmi_wdd_plan *p) { return plan_destroy(p); }

extern "C" const char *ltmi_wdd_plan_last_kernel(const ltmi_wdd_plan *p) {
    return p ? p->last_kernel : "";
}

extern "C" int ltmi_wdd_reconstruct(ltmi_wdd_plan *p, const float *bf, int64_t ld_bf, void *fourier_out,
                                    void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_reconstruct: null plan");
    if (ld_bf < p->n_window) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_wdd_reconstruct: ld_bf < the plan's %d pixels", p->n_window);
    if (!bf || !fourier_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_wdd_reconstruct: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_bind = p->front.fwd.bind(stream);
    if (rc_bind != LTMI_OK) return rc_bind;
    snprintf(p->last_kernel, sizeof(p->last_kernel),
             "k_transpose<4> + hipfft_r2c + k_transpose<8> + k_wdd_dot + k_wdd_finish batch=%d", p->batch);
    // the batches are window pixels here
    const int rc = for_each_batch(p->n_window, p->batch, [&](int64_t k0, int64_t n) {
        const int rc_front = p->front.run(p->device, p->g, bf, ld_bf, k0, n, stream_);
        if (rc_front != LTMI_OK) return rc_front;
        return wdd_dot_launch(p->front.spec_t, p->batch, p->filt + k0, p->n_window, (int)n, p->g.ny, p->g.nx, p->acc,
                              k0 == 0, stream);
    });
    if (rc != LTMI_OK) return rc;
    return wdd_finish_launch(p->acc, p->g.ny, p->g.nx, p->n_window, (hipfftComplex *)fourier_out, stream);
}
