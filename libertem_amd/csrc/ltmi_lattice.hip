// ltmi_lattice.hip -- per-frame lattice fit to matched peaks.
//
// Per frame, for P peaks with positions r_k (float32 (y, x)), weights w_k (float32, or 1), integer lattice indices
// (i_k, j_k), a start lattice zero0, a0, b0 (float64 (y, x) pairs) and a tolerance tau >= 0 in pixels; all arithmetic
// is float64, the results are cast once at the end:
//   1. p_k = zero0 + i_k a0 + j_k b0
//   2. selector[k] = r_k finite in both components, w_k finite, w_k > 0, |r_k - p_k|_2 <= tau (and peak_values[k]
//      finite where peak_values is given)
//   3. a fit EXISTS iff the index pairs of the selected peaks are not collinear, decided on the integers: k0 = the
//      first selected k, k1 = the first selected k with another index pair; some selected k has
//      (i_k - i_k0)(j_k1 - j_k0) - (j_k - j_k0)(i_k1 - i_k0) != 0 in int64
//   4. if it exists, (zero, a, b) minimises sum_sel w_k |zero + i_k a + j_k b - r_k|^2 (the 3 x 3 normal system with
//      two right-hand sides) and error = sqrt(sum_sel w_k |res_k|^2 / sum_sel w_k)
//   5. otherwise zero, a, b and error are NaN; selector is as in step 2.
//
// k_lattice_fit: one wave per frame, four waves per workgroup.  The lanes stride the peaks in four short passes
// (selector bytes and k0; k1 and the twelve sums of the normal system; the collinearity test; the residuals), each
// closed by a fixed-order butterfly of shuffles that leaves the same bits in every lane; every lane then solves the
// system by LDL^T and lane 0 stores.  The sums are taken about the index pair of k0 (exact in integers), so a lattice
// far from index 0 loses nothing to its offset.  No atomics, no LDS: the results of a call repeat bit for bit.  The
// indices never address memory.
#include "ltmi_common.h"

namespace {

struct lattice_start { double zy, zx, ay, ax, by, bx; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }

__global__ void __launch_bounds__(256)
k_lattice_fit(const float *__restrict__ refineds, const float *__restrict__ weights,
              const float *__restrict__ peak_values, int64_t n_frames, int n_peaks,
              const int32_t *__restrict__ indices, lattice_start s0, double tol, float *__restrict__ zero,
              float *__restrict__ a, float *__restrict__ b, uint8_t *__restrict__ selector, float *__restrict__ error) {
    const int lane = threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_frames) return;                              // (the whole wave)
    const float *r = refineds + f * n_peaks * 2;
    const float *wt = weights ? weights + f * n_peaks : nullptr;
    const float *pv = peak_values ? peak_values + f * n_peaks : nullptr;
    uint8_t *sel = selector + f * n_peaks;
    const int none = 0x7fffffff;

    // step 2 for peak k of this frame; the weight of a selected peak
    auto selected = [&](int k, double &w) -> bool {
        const float ry = r[2 * k], rx = r[2 * k + 1];
        const float wf = wt ? wt[k] : 1.f;
        const double i = (double)indices[2 * k], j = (double)indices[2 * k + 1];
        const double dy = (double)ry - (s0.zy + i * s0.ay + j * s0.by);
        const double dx = (double)rx - (s0.zx + i * s0.ax + j * s0.bx);
        w = (double)wf;
        bool ok = finite_f(ry) && finite_f(rx) && finite_f(wf) && wf > 0.f;
        if (pv) ok = ok && finite_f(pv[k]);
        return ok && sqrt(dy * dy + dx * dx) <= tol;
    };

    double w;
    int k0 = none;
    for (int k = lane; k < n_peaks; k += 64) {
        const bool ok = selected(k, w);
        sel[k] = ok ? 1 : 0;
        if (ok) k0 = min(k0, k);
    }
    k0 = wave_min(k0);
    int64_t i0 = 0, j0 = 0;
    if (k0 != none) {
        i0 = indices[2 * k0];
        j0 = indices[2 * k0 + 1];
    }
    // the normal system about (i0, j0): M = sum w (1, di, dj)^T (1, di, dj), right-hand sides sum w (1, di, dj) r
    int k1 = none;
    double m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0, y0 = 0, y1 = 0, y2 = 0, x0 = 0, x1 = 0, x2 = 0;
    if (k0 != none) {
        for (int k = lane; k < n_peaks; k += 64) {
            if (!selected(k, w)) continue;
            const int64_t di = (int64_t)indices[2 * k] - i0, dj = (int64_t)indices[2 * k + 1] - j0;
            if (di != 0 || dj != 0) k1 = min(k1, k);
            const double ci = (double)di, cj = (double)dj, ry = (double)r[2 * k], rx = (double)r[2 * k + 1];
            m00 += w;
            m01 += w * ci;
            m02 += w * cj;
            m11 += w * ci * ci;
            m12 += w * ci * cj;
            m22 += w * cj * cj;
            y0 += w * ry;
            y1 += w * ci * ry;
            y2 += w * cj * ry;
            x0 += w * rx;
            x1 += w * ci * rx;
            x2 += w * cj * rx;
        }
    }
    k1 = wave_min(k1);
    int spans = 0;
    if (k1 != none) {
        const int64_t i1 = (int64_t)indices[2 * k1] - i0, j1 = (int64_t)indices[2 * k1 + 1] - j0;
        for (int k = lane; k < n_peaks; k += 64) {
            if (!selected(k, w)) continue;
            const int64_t di = (int64_t)indices[2 * k] - i0, dj = (int64_t)indices[2 * k + 1] - j0;
            spans |= (di * j1 - dj * i1) != 0;
        }
    }
    spans = __any(spans);
    if (!spans) {                                           // (wave-uniform)
        if (lane == 0) {
            const float nan = __builtin_nanf("");
            zero[2 * f] = zero[2 * f + 1] = a[2 * f] = a[2 * f + 1] = b[2 * f] = b[2 * f + 1] = error[f] = nan;
        }
        return;
    }
    m00 = wave_sum(m00); m01 = wave_sum(m01); m02 = wave_sum(m02);
    m11 = wave_sum(m11); m12 = wave_sum(m12); m22 = wave_sum(m22);
    y0 = wave_sum(y0); y1 = wave_sum(y1); y2 = wave_sum(y2);
    x0 = wave_sum(x0); x1 = wave_sum(x1); x2 = wave_sum(x2);
    // M = L D L^T (positive definite: the selected weights are positive and their index pairs span the plane)
    const double l10 = m01 / m00, l20 = m02 / m00;
    const double d1 = m11 - l10 * m01;
    const double t21 = m12 - l20 * m01;
    const double l21 = t21 / d1;
    const double d2 = m22 - l20 * m02 - l21 * t21;
    // forward, diagonal, backward: (c, a, b) with c the lattice's value at (i0, j0)
    const double fy1 = y1 - l10 * y0, fy2 = y2 - l20 * y0 - l21 * fy1;
    const double fx1 = x1 - l10 * x0, fx2 = x2 - l20 * x0 - l21 * fx1;
    const double by = fy2 / d2, bx = fx2 / d2;
    const double ay = fy1 / d1 - l21 * by, ax = fx1 / d1 - l21 * bx;
    const double cy = y0 / m00 - l10 * ay - l20 * by, cx = x0 / m00 - l10 * ax - l20 * bx;
    double ss = 0;
    for (int k = lane; k < n_peaks; k += 64) {
        if (!selected(k, w)) continue;
        const double ci = (double)((int64_t)indices[2 * k] - i0), cj = (double)((int64_t)indices[2 * k + 1] - j0);
        const double ey = cy + ci * ay + cj * by - (double)r[2 * k];
        const double ex = cx + ci * ax + cj * bx - (double)r[2 * k + 1];
        ss += w * (ey * ey + ex * ex);
    }
    ss = wave_sum(ss);
    if (lane != 0) return;
    zero[2 * f] = (float)(cy - (double)i0 * ay - (double)j0 * by);
    zero[2 * f + 1] = (float)(cx - (double)i0 * ax - (double)j0 * bx);
    a[2 * f] = (float)ay;
    a[2 * f + 1] = (float)ax;
    b[2 * f] = (float)by;
    b[2 * f + 1] = (float)bx;
    error[f] = (float)sqrt(ss / m00);
}

// the kernel of the last launch issued by this thread ("" before the first): ltmi_lattice_last_kernel
thread_local const char *t_last_kernel = "";

}  // namespace

extern "C" const char *ltmi_lattice_last_kernel(void) { return t_last_kernel; }

extern "C" int ltmi_lattice_fit(int device, const float *refineds, const float *weights, const float *peak_values,
                                int64_t n_frames, int n_peaks, const int32_t *indices, const double *start,
                                double tolerance, float *zero, float *a, float *b, uint8_t *selector, float *error,
                                void *stream_) {
    if (n_frames < 0 || n_peaks < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_lattice_fit: negative frame or peak count");
    if (!(tolerance >= 0.0)) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_lattice_fit: tolerance %g must be at least 0", tolerance);
    if (n_frames / 4 >= INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_lattice_fit: %lld frames exceed one launch", (long long)n_frames);
    if (!start) LTMI_FAIL(LTMI_E_INVALID, "ltmi_lattice_fit: null pointer");
    for (int k = 0; k < 6; ++k)
        if (!(fabs(start[k]) <= 1.7976931348623157e308))
            LTMI_FAIL(LTMI_E_SHAPE, "ltmi_lattice_fit: start lattice value %d is not finite", k);
    if (n_frames == 0 || n_peaks == 0) return LTMI_OK;
    if (!refineds || !indices || !zero || !a || !b || !selector || !error)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_lattice_fit: null pointer");
    LTMI_HIP(hipSetDevice(device));
    const lattice_start s0 = {start[0], start[1], start[2], start[3], start[4], start[5]};
    hipLaunchKernelGGL(k_lattice_fit, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, (hipStream_t)stream_,
                       refineds, weights, peak_values, n_frames, n_peaks, indices, s0, tolerance, zero, a, b, selector,
                       error);
    LTMI_HIP(hipGetLastError());
    t_last_kernel = "k_lattice_fit";
    return LTMI_OK;
}
