// ltmi_parallax.hip -- tilt-corrected bright-field imaging ("parallax") of a defocused-probe 4D-STEM scan (DESIGN.md
// section 4.6j).
//
// Every bright-field pixel K records a scan image I_K; under defocus the images are copies of one another, shifted by
// sh[K].  The plan keeps the half spectra G[K] = rfft2(I_K) of all P pixels (ltmi_transpose2d and one batched R2C
// hipFFT per batch, the first half of the single-sideband front end), pixel-major.  One iteration measures the shifts
// against the aligned mean: k_plx_ramps (the two separable Fourier ramps of every pixel, Ny + Nxc sincos instead of
// Ny Nxc), k_plx_sum (S = mean over K of G[K] ey[K] ex[K], a stream over the store), k_plx_herm (the columns ix = 0 and
// Nx / 2 of S projected onto their Hermitian part, which is all a real inverse transform takes from them), and per
// batch k_plx_mul (G[K] conj(R)), one batched C2R hipFFT (the circular cross-correlation maps) and k_plx_peaks (the
// first maximum inside the window and a three-point parabola per axis, float64).  No atomics: a second call gives the
// same bytes.
#include "ltmi_ssbshare.h"
#include <algorithm>
#include <climits>
#include <cmath>

// k_plx_mul and k_plx_peaks are compared with NumPy byte for byte: every product and sum is rounded on its own
#pragma clang fp contract(off)

namespace ltmi {

// ey[k, iy] = exp(2 pi i (s(iy, ny) sh[k, 0] / ny)) for iy < ny, ex[k, ix] = exp(2 pi i (s(ix, nx) sh[k, 1] / nx)) for
// ix <= nx / 2: one thread per value, the angle evaluated as written, one sincos each
__global__ void __launch_bounds__(256)
k_plx_ramps(const double *__restrict__ sh, int64_t n, int ny, int nx, double2 *__restrict__ ey,
            double2 *__restrict__ ex) {
    const int nxc = nx / 2 + 1;
    const int per = ny + nxc;
    const int64_t total = n * per;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t k = i / per;
        const int j = (int)(i - k * per);
        const bool along_y = j < ny;
        const int idx = along_y ? j : j - ny;
        const int len = along_y ? ny : nx;
        const double shift = sh[2 * k + (along_y ? 0 : 1)];
        const double angle = 6.283185307179586 * ((double)ssb_signed(idx, len) * shift / (double)len);
        double sn, cs;
        sincos(angle, &sn, &cs);
        if (along_y) ey[k * ny + idx] = make_double2(cs, sn);
        else ex[k * nxc + idx] = make_double2(cs, sn);
    }
}

// the lanes of a wave run along Q (64 neighbouring Qs of a pixel's spectrum are 512 contiguous bytes), the four waves
// of a workgroup each take a quarter of the pixels, ascending
constexpr int PLX_SUM_Q = 64;

// S[Q] = (1 / n) sum over k < n of G[k, Q] (ey[k, iy] ex[k, ix]), Q = iy nxc + ix, float64, cast once.  Wave w sums
// the pixels [w c, (w + 1) c), c = ceil(n / 4), in ascending order; lane l of wave 0 adds the four partial sums of its
// Q in the order of the waves.
__global__ void __launch_bounds__(256)
k_plx_sum(const float2 *__restrict__ spec, int n, int ny, int nx, const double2 *__restrict__ ey,
          const double2 *__restrict__ ex, float2 *__restrict__ out) {
    __shared__ double s_part[4][PLX_SUM_Q][2];
    const int nxc = nx / 2 + 1;
    const int64_t n_q = (int64_t)ny * nxc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = (n + 3) / 4;
    const int k_lo = wave * chunk < n ? wave * chunk : n, k_hi = k_lo + chunk < n ? k_lo + chunk : n;
    for (int64_t q0 = (int64_t)blockIdx.x * PLX_SUM_Q; q0 < n_q; q0 += (int64_t)gridDim.x * PLX_SUM_Q) {
        const int64_t q = q0 + lane;
        double sr = 0., si = 0.;
        if (q < n_q) {
            const int iy = (int)(q / nxc), ix = (int)(q - (int64_t)iy * nxc);
            for (int k = k_lo; k < k_hi; ++k) {
                const float2 g = spec[(int64_t)k * n_q + q];
                const double2 a = ey[(int64_t)k * ny + iy], b = ex[(int64_t)k * nxc + ix];
                const double rr = a.x * b.x - a.y * b.y, ri = a.x * b.y + a.y * b.x;
                const double gr = (double)g.x, gi = (double)g.y;
                sr += gr * rr - gi * ri;
                si += gr * ri + gi * rr;
            }
        }
        s_part[wave][lane][0] = sr;
        s_part[wave][lane][1] = si;
        __syncthreads();
        if (wave == 0 && q < n_q) {
            double tr = s_part[0][lane][0], ti = s_part[0][lane][1];
            for (int w = 1; w < 4; ++w) {
                tr += s_part[w][lane][0];
                ti += s_part[w][lane][1];
            }
            out[q] = make_float2((float)(tr / (double)n), (float)(ti / (double)n));
        }
        __syncthreads();
    }
}

// The columns ix = 0 and, for an even nx, nx / 2 of a half spectrum pair with themselves: a real inverse transform takes
// (S[iy] + conj(S[-iy])) / 2 from them and nothing else.  In place, one thread per pair (iy, (ny - iy) mod ny); with
// zero_dc, S[0, 0] = 0 afterwards.
__global__ void __launch_bounds__(256)
k_plx_herm(float2 *__restrict__ s, int ny, int nx, int zero_dc) {
    const int nxc = nx / 2 + 1;
    const int n_col = nx % 2 == 0 ? 2 : 1;
    const int half = ny / 2 + 1;                // iy in [0, ny / 2] meets every pair
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= half * n_col) return;
    const int iy = i / n_col, ix = (i - iy * n_col) == 0 ? 0 : nx / 2;
    const int jy = iy == 0 ? 0 : ny - iy;
    const float2 a = s[(int64_t)iy * nxc + ix], b = s[(int64_t)jy * nxc + ix];
    float2 u = make_float2((a.x + b.x) / 2.f, (a.y - b.y) / 2.f);
    if (zero_dc && iy == 0 && ix == 0) u = make_float2(0.f, 0.f);
    s[(int64_t)iy * nxc + ix] = u;
    if (jy != iy) s[(int64_t)jy * nxc + ix] = make_float2(u.x, -u.y);
}

// X[k, Q] = G[k, Q] conj(R[Q]) in float32, X[k, 0] = 0
__global__ void __launch_bounds__(256)
k_plx_mul(const float2 *__restrict__ spec, int64_t n, int64_t n_q, const float2 *__restrict__ ref,
          float2 *__restrict__ out) {
    const int64_t total = n * n_q;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t q = i % n_q;
        const float2 g = spec[i], r = ref[q];
        float2 x = make_float2(g.x * r.x + g.y * r.y, g.y * r.x - g.x * r.y);
        if (q == 0) x = make_float2(0.f, 0.f);
        out[i] = x;
    }
}

__device__ static inline int plx_wrap(int t, int n) {
    const int r = t % n;
    return r < 0 ? r + n : r;
}

// the vertex of the parabola through (-1, cm), (0, c0), (1, cp), clipped to half a pixel; 0 where it has no maximum
__device__ static inline double plx_sub(double cm, double c0, double cp) {
    const double d = cm - 2. * c0 + cp;
    if (!(d < 0.)) return 0.;
    const double v = (cm - cp) / (2. * d);
    return v < -0.5 ? -0.5 : (v > 0.5 ? 0.5 : v);
}

// One wave per map (ny, nx): candidate c = (ty + m) (2 m + 1) + (tx + m) for -m <= ty, tx <= m is the value at
// (ty mod ny, tx mod nx).  Lane l looks at the candidates l, l + 64, ... and keeps the first of its largest; the
// shuffle tree keeps the larger value and, of two equal ones, the smaller c: the first maximum in row-major order.
// Lane 0 fits the two parabolas in float64 from the stored values.  A map of NaNs gives candidate 0.
__global__ void __launch_bounds__(256)
k_plx_peaks(const float *__restrict__ maps, int64_t n, int ny, int nx, int m, double *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int side = 2 * m + 1, n_cand = side * side;
    const int64_t n_px = (int64_t)ny * nx;
    for (int64_t f = (int64_t)blockIdx.x * 4 + wave; f < n; f += (int64_t)gridDim.x * 4) {
        const float *map = maps + f * n_px;
        float best = -INFINITY;
        int best_c = lane < n_cand ? lane : INT_MAX;
        for (int c = lane; c < n_cand; c += 64) {
            const int ty = c / side - m, tx = c - (c / side) * side - m;
            const float v = map[(int64_t)plx_wrap(ty, ny) * nx + plx_wrap(tx, nx)];
            if (v > best) {
                best = v;
                best_c = c;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_down(best, off, 64);
            const int oc = __shfl_down(best_c, off, 64);
            if (ov > best || (ov == best && oc < best_c)) {
                best = ov;
                best_c = oc;
            }
        }
        if (lane == 0) {
            const int ty = best_c / side - m, tx = best_c - (best_c / side) * side - m;
            const int y0 = plx_wrap(ty, ny), ym = plx_wrap(ty - 1, ny), yp = plx_wrap(ty + 1, ny);
            const int x0 = plx_wrap(tx, nx), xm = plx_wrap(tx - 1, nx), xp = plx_wrap(tx + 1, nx);
            const double c0 = (double)map[(int64_t)y0 * nx + x0];
            out[2 * f] = (double)ty + plx_sub((double)map[(int64_t)ym * nx + x0], c0, (double)map[(int64_t)yp * nx + x0]);
            out[2 * f + 1] = (double)tx + plx_sub((double)map[(int64_t)y0 * nx + xm], c0, (double)map[(int64_t)y0 * nx + xp]);
        }
    }
}

// workgroups of the kernels above: what lies beyond them is walked with a grid stride
constexpr int64_t PLX_MAX_GRID_X = 1 << 20;

static unsigned plx_grid(int64_t items, int64_t per_group) {
    return (unsigned)std::max<int64_t>(1, std::min((items + per_group - 1) / per_group, PLX_MAX_GRID_X));
}

// what every entry point asks of the scan
static int plx_check_scan(const char *who, int ny, int nx) {
    if (ny <= 0 || nx <= 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: scan %d x %d must be positive", who, ny, nx);
    if ((int64_t)ny * nx > INT32_MAX) LTMI_FAIL(LTMI_E_SHAPE, "%s: scan %d x %d exceeds 2^31 - 1 positions", who, ny, nx);
    return LTMI_OK;
}

// ... and of the window of shifts: every t in [-m, m] is its own index mod the axis
static int plx_check_window(const char *who, int ny, int nx, int m) {
    if (m < 1) LTMI_FAIL(LTMI_E_SHAPE, "%s: max_shift %d must be at least 1", who, m);
    if (m > (INT32_MAX - 1) / 2 || ny < 2 * m + 1 || nx < 2 * m + 1)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: both axes of the %d x %d scan must hold the 2 * %d + 1 shifts of max_shift", who, ny,
                  nx, m);
    return LTMI_OK;
}

static int plx_ramps_launch(const double *sh, int64_t n, int ny, int nx, double2 *ey, double2 *ex, hipStream_t stream) {
    hipLaunchKernelGGL(k_plx_ramps, dim3(plx_grid(n * (ny + nx / 2 + 1), 256)), dim3(256), 0, stream, sh, n, ny, nx, ey,
                       ex);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int plx_sum_launch(const hipfftComplex *spec, int n, int ny, int nx, const double2 *ey, const double2 *ex,
                          hipfftComplex *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_plx_sum, dim3(plx_grid((int64_t)ny * (nx / 2 + 1), PLX_SUM_Q)), dim3(256), 0, stream,
                       (const float2 *)spec, n, ny, nx, ey, ex, (float2 *)out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int plx_herm_launch(hipfftComplex *s, int ny, int nx, bool zero_dc, hipStream_t stream) {
    hipLaunchKernelGGL(k_plx_herm, dim3(plx_grid((int64_t)(ny / 2 + 1) * 2, 256)), dim3(256), 0, stream, (float2 *)s, ny,
                       nx, zero_dc ? 1 : 0);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int plx_mul_launch(const hipfftComplex *spec, int64_t n, int64_t n_q, const hipfftComplex *ref, hipfftComplex *out,
                          hipStream_t stream) {
    hipLaunchKernelGGL(k_plx_mul, dim3(plx_grid(n * n_q, 256)), dim3(256), 0, stream, (const float2 *)spec, n, n_q,
                       (const float2 *)ref, (float2 *)out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int plx_peaks_launch(const float *maps, int64_t n, int ny, int nx, int m, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(k_plx_peaks, dim3(plx_grid(n, 4)), dim3(256), 0, stream, maps, n, ny, nx, m, out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

}  // namespace ltmi

using namespace ltmi;

struct ltmi_plx_plan {
    int device = 0;
    int ny = 0, nx = 0;
    int n_idx = 0;                      // P
    int batch = 0;                      // bright-field pixels per hipFFT execution
    int max_shift = 0;
    bool loaded = false;
    DevBuf<hipfftComplex> store;        // (P, ny nxc) c64: the half spectrum of every pixel's scan image
    DevBuf<float> real_buf;             // (batch, ny, nx) f32: scan images on the way in, correlation maps on the way out
    DevBuf<hipfftComplex> xspec;        // (batch, ny nxc) c64: G conj(R) of a batch (and a partial batch's spectra)
    DevBuf<double2> ey, ex;             // (P, ny), (P, nxc) c128: the ramps
    DevBuf<hipfftComplex> mean;         // (ny nxc) c64: S, then R
    FftHandle fwd, inv;                 // batched R2C and C2R over the scan axes
    char last_kernel[160] = {0};
};

extern "C" int ltmi_plx_ramps(int device, const double *sh, int64_t n, int nav_y, int nav_x, void *ey_out, void *ex_out,
                              void *stream_) {
    const int rc = plx_check_scan("ltmi_plx_ramps", nav_y, nav_x);
    if (rc != LTMI_OK) return rc;
    if (n < 0 || n > INT32_MAX) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_ramps: %lld pixels", (long long)n);
    if (n == 0) return LTMI_OK;
    if (!sh || !ey_out || !ex_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_ramps: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return plx_ramps_launch(sh, n, nav_y, nav_x, (double2 *)ey_out, (double2 *)ex_out, (hipStream_t)stream_);
}

extern "C" int ltmi_plx_sum(int device, const void *spec, int n, int nav_y, int nav_x, const void *ey, const void *ex,
                            void *s_out, void *stream_) {
    const int rc = plx_check_scan("ltmi_plx_sum", nav_y, nav_x);
    if (rc != LTMI_OK) return rc;
    if (n < 1) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_sum: %d bright-field pixels: at least one is needed", n);
    if (!spec || !ey || !ex || !s_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_sum: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return plx_sum_launch((const hipfftComplex *)spec, n, nav_y, nav_x, (const double2 *)ey, (const double2 *)ex,
                          (hipfftComplex *)s_out, (hipStream_t)stream_);
}

extern "C" int ltmi_plx_mul(int device, const void *spec, int64_t n, int nav_y, int nav_x, const void *ref, void *x_out,
                            void *stream_) {
    const int rc = plx_check_scan("ltmi_plx_mul", nav_y, nav_x);
    if (rc != LTMI_OK) return rc;
    if (n < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_mul: %lld spectra", (long long)n);
    if (n == 0) return LTMI_OK;
    if (!spec || !ref || !x_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_mul: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return plx_mul_launch((const hipfftComplex *)spec, n, (int64_t)nav_y * (nav_x / 2 + 1), (const hipfftComplex *)ref,
                          (hipfftComplex *)x_out, (hipStream_t)stream_);
}

extern "C" int ltmi_plx_peaks(int device, const float *maps, int64_t n, int nav_y, int nav_x, int max_shift,
                              double *shifts_out, void *stream_) {
    int rc = plx_check_scan("ltmi_plx_peaks", nav_y, nav_x);
    if (rc == LTMI_OK) rc = plx_check_window("ltmi_plx_peaks", nav_y, nav_x, max_shift);
    if (rc != LTMI_OK) return rc;
    if (max_shift > 16383) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_peaks: max_shift %d exceeds 16383", max_shift);
    if (n < 0) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_peaks: %lld maps", (long long)n);
    if (n == 0) return LTMI_OK;
    if (!maps || !shifts_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_peaks: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return plx_peaks_launch(maps, n, nav_y, nav_x, max_shift, shifts_out, (hipStream_t)stream_);
}

extern "C" int ltmi_plx_plan_create(int device, int nav_y, int nav_x, int n_idx, int max_batch, int max_shift,
                                    int64_t store_limit_bytes, ltmi_plx_plan **out) {
    if (!out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_create: null pointer");
    if (max_batch <= 0) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_create: batch %d must be positive", max_batch);
    int rc_shape = plx_check_scan("ltmi_plx_plan_create", nav_y, nav_x);
    if (rc_shape == LTMI_OK) rc_shape = plx_check_window("ltmi_plx_plan_create", nav_y, nav_x, max_shift);
    if (rc_shape != LTMI_OK) return rc_shape;
    if (max_shift > 16383) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_plan_create: max_shift %d exceeds 16383", max_shift);
    if (n_idx <= 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_plan_create: %d bright-field pixels: at least one is needed", n_idx);
    const int batch = std::min(max_batch, n_idx);
    if ((int64_t)batch * nav_y * nav_x > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_plan_create: a batch of %d scans of %d x %d exceeds 2^31 - 1 values", batch,
                  nav_y, nav_x);
    const int64_t n_nav = (int64_t)nav_y * nav_x;
    const int64_t n_spec = (int64_t)nav_y * (nav_x / 2 + 1);
    return plan_create(device, out, [&](ltmi_plx_plan *p) {
        p->ny = nav_y;
        p->nx = nav_x;
        p->n_idx = n_idx;
        p->batch = batch;
        p->max_shift = max_shift;
        // the spectra of all pixels stay in the plan
        const unsigned long long need = (unsigned long long)n_idx * n_spec * sizeof(hipfftComplex);
        if (store_limit_bytes < 0 || need > (unsigned long long)store_limit_bytes)
            LTMI_FAIL(LTMI_E_NOMEM, "ltmi_plx_plan_create: the spectra of %d bright-field pixels x %lld Qs need %llu bytes "
                      "of device memory, the limit is %lld", n_idx, (long long)n_spec, need, (long long)store_limit_bytes);
        size_t free_b = 0, total_b = 0;
        LTMI_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b || p->store.alloc((size_t)n_idx * n_spec) != hipSuccess) {
            (void)hipGetLastError();
            LTMI_FAIL(LTMI_E_NOMEM, "ltmi_plx_plan_create: the spectra of %d bright-field pixels x %lld Qs need %llu bytes "
                      "of device memory, %zu are free", n_idx, (long long)n_spec, need, free_b);
        }
        hipError_t e = p->real_buf.alloc_zero((size_t)batch * n_nav);
        if (e == hipSuccess) e = p->xspec.alloc_zero((size_t)batch * n_spec);
        if (e == hipSuccess) e = p->ey.alloc_zero((size_t)n_idx * nav_y);
        if (e == hipSuccess) e = p->ex.alloc_zero((size_t)n_idx * (nav_x / 2 + 1));
        if (e == hipSuccess) e = p->mean.alloc_zero((size_t)n_spec);
        if (e != hipSuccess)
            LTMI_FAIL((int)e, "ltmi_plx_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
        int n[2] = {nav_y, nav_x};
        const int rc = p->fwd.plan_many(2, n, (int)n_nav, (int)n_spec, HIPFFT_R2C, batch);
        return rc == LTMI_OK ? p->inv.plan_many(2, n, (int)n_spec, (int)n_nav, HIPFFT_C2R, batch) : rc;
    });
}

extern "C" int ltmi_plx_plan_destroy(ltmi_plx_plan *p) { return plan_destroy(p); }

extern "C" const char *ltmi_plx_plan_last_kernel(const ltmi_plx_plan *p) {
    return p ? p->last_kernel : "";
}

extern "C" int ltmi_plx_plan_load(ltmi_plx_plan *p, const float *bf, int64_t ld_bf, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_load: null plan");
    if (ld_bf < p->n_idx) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_plx_plan_load: ld_bf < the plan's %d pixels", p->n_idx);
    if (!bf) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_load: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_bind = p->fwd.bind(stream);
    if (rc_bind != LTMI_OK) return rc_bind;
    snprintf(p->last_kernel, sizeof(p->last_kernel), "k_transpose<4> + hipfft_r2c batch=%d", p->batch);
    const int64_t n_nav = (int64_t)p->ny * p->nx;
    const int64_t n_spec = (int64_t)p->ny * (p->nx / 2 + 1);
    p->loaded = false;
    // the batches are bright-field pixels: column k of bf = the scan image of pixel k
    const int rc = for_each_batch(p->n_idx, p->batch, [&](int64_t k0, int64_t n) {
        int rc_b = ltmi_transpose2d(p->device, bf + k0, ld_bf, n_nav, n, 4, p->real_buf, n_nav, stream_);
        if (rc_b != LTMI_OK) return rc_b;
        hipfftComplex *dst = p->store + k0 * n_spec;
        if (n == p->batch) return p->fwd.r2c(p->real_buf, dst);
        // the plan always transforms `batch` images: a partial batch would write past the store
        rc_b = p->fwd.r2c(p->real_buf, p->xspec);
        if (rc_b != LTMI_OK) return rc_b;
        LTMI_HIP(hipMemcpyAsync(dst, p->xspec.get(), (size_t)(n * n_spec) * sizeof(hipfftComplex),
                                hipMemcpyDeviceToDevice, stream));
        return (int)LTMI_OK;
    });
    p->loaded = rc == LTMI_OK;
    return rc;
}

// S(sh) of the stored spectra -> p->mean, its self-paired columns Hermitian
static int plx_mean(ltmi_plx_plan *p, const double *sh, bool zero_dc, hipStream_t stream) {
    int rc = plx_ramps_launch(sh, p->n_idx, p->ny, p->nx, p->ey, p->ex, stream);
    if (rc == LTMI_OK) rc = plx_sum_launch(p->store, p->n_idx, p->ny, p->nx, p->ey, p->ex, p->mean, stream);
    if (rc == LTMI_OK) rc = plx_herm_launch(p->mean, p->ny, p->nx, zero_dc, stream);
    return rc;
}

extern "C" int ltmi_plx_plan_iterate(ltmi_plx_plan *p, double *shifts, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_iterate: null plan");
    if (!shifts) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_iterate: null pointer");
    if (!p->loaded) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_iterate: no spectra yet: ltmi_plx_plan_load comes first");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_bind = p->inv.bind(stream);
    if (rc_bind != LTMI_OK) return rc_bind;
    snprintf(p->last_kernel, sizeof(p->last_kernel),
             "k_plx_ramps + k_plx_sum + k_plx_herm + k_plx_mul + hipfft_c2r + k_plx_peaks batch=%d", p->batch);
    const int rc_mean = plx_mean(p, shifts, true, stream);
    if (rc_mean != LTMI_OK) return rc_mean;
    const int64_t n_spec = (int64_t)p->ny * (p->nx / 2 + 1);
    // the ramps are made: from here on `shifts` is the result.  The C2R transform always takes `batch` spectra: behind
    // a partial batch lie those of an earlier one, whose maps are never searched.
    return for_each_batch(p->n_idx, p->batch, [&](int64_t k0, int64_t n) {
        int rc = plx_mul_launch(p->store + k0 * n_spec, n, n_spec, p->mean, p->xspec, stream);
        if (rc == LTMI_OK) rc = p->inv.c2r(p->xspec, p->real_buf);
        if (rc == LTMI_OK) rc = plx_peaks_launch(p->real_buf, n, p->ny, p->nx, p->max_shift, shifts + 2 * k0, stream);
        return rc;
    });
}

extern "C" int ltmi_plx_plan_sum(ltmi_plx_plan *p, const double *shifts, void *half_out, void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_sum: null plan");
    if (!shifts || !half_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_sum: null pointer");
    if (!p->loaded) LTMI_FAIL(LTMI_E_INVALID, "ltmi_plx_plan_sum: no spectra yet: ltmi_plx_plan_load comes first");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    snprintf(p->last_kernel, sizeof(p->last_kernel), "k_plx_ramps + k_plx_sum + k_plx_herm");
    const int rc = plx_mean(p, shifts, false, stream);
    if (rc != LTMI_OK) return rc;
    LTMI_HIP(hipMemcpyAsync(half_out, p->mean.get(), (size_t)p->ny * (p->nx / 2 + 1) * sizeof(hipfftComplex),
                            hipMemcpyDeviceToDevice, stream));
    return LTMI_OK;
}
