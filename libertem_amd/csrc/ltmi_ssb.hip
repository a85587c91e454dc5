// ltmi_ssb.hip -- single-sideband ptychography of a focused-probe 4D-STEM scan.
//
// k_ssb_gather<dtype>: the bright-field pixels of every frame of a tile, native dtype -> float32 (n, P).
// k_ssb_trotter: for every spatial frequency Q of the scan, the sums of the spectra G[K, Q] over the two "trotter"
// regions of the bright-field disk, which are evaluated analytically in float64 -- no mask stack exists anywhere.
// The plan produces G for `batch` bright-field pixels at a time: ltmi_transpose2d (bf (N, P) -> (batch, N)), one
// batched 2D real-to-complex hipFFT over the scan axes, ltmi_transpose2d ((batch, Ny Nxc) -> (Ny Nxc, batch)), so that
// the workgroup of one Q reads its pixels contiguously; the partial sums of a batch wait in a per-Q accumulator.
// No atomics: a second call gives the same bytes.
#include "ltmi_ssbshare.h"
#include <algorithm>
#include <cmath>

// the three disk predicates agree with a NumPy float64 evaluation of the same expressions bit for bit: every product
// and sum below is rounded on its own
#pragma clang fp contract(off)

namespace ltmi {

// what a Q has summed so far: the complex sums over pos and neg in float64, and the two pixel counts
struct SsbAcc {
    double pr, pi, nr, ni;
    int np, nn;
};

// out[f, k] = (float)tile[f, idx[k]]; an index outside [0, n_px) gives 0 and reads nothing.  A thread owns one list
// entry and walks the frames of its grid row: along k the loads of a wave run up the detector rows that cross the
// disk, in runs of one chord each, and its stores are one contiguous segment.
template <typename T>
__global__ void __launch_bounds__(256)
k_ssb_gather(const T *__restrict__ tile, int64_t ld, int64_t n_frames, int64_t n_px, const int32_t *__restrict__ idx,
             int n_idx, float *__restrict__ out, int64_t ld_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_idx) return;
    const int64_t i = idx[k];
    const bool inside = i >= 0 && i < n_px;
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y)
        out[f * ld_out + k] = inside ? (float)tile[f * ld + i] : 0.f;
}

// One workgroup per Q = (iy, ix), walking the Qs with a grid stride.  Thread t takes the pixels t, t + 256, ... of
// the n_k listed ones in that order, a wave adds its lanes by a fixed shuffle tree, thread 0 adds the four waves in
// order: the float64 sums of a call repeat bit for bit.  spec[(ry nxc + rx) ld_spec + k] is G[k, ry, rx] for
// rx <= nx / 2; a Q with ix > nx / 2 reads the conjugate at ((ny - iy) mod ny, nx - ix).  Only pixels inside a
// trotter are loaded.  first: the accumulator starts at zero; last: the cutoff rule is applied and fourier[Q]
// written; between the two the sums wait in acc[Q].
__global__ void __launch_bounds__(256)
k_ssb_trotter(const float2 *__restrict__ spec, int64_t ld_spec, const int32_t *__restrict__ idx, int n_k, SsbGeom g,
              SsbAcc *__restrict__ acc, int first, int last, float2 *__restrict__ fourier) {
    __shared__ double s_sum[4][4];
    __shared__ int s_cnt[4][2];
    const int nxc = g.nx / 2 + 1;
    const int64_t n_q = (int64_t)g.ny * g.nx;
    const double r2 = g.semiconv_pix * g.semiconv_pix;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = blockIdx.x; q < n_q; q += gridDim.x) {
        const int iy = (int)(q / g.nx), ix = (int)(q - (int64_t)iy * g.nx);
        const bool mirrored = ix > g.nx / 2;
        const int ry = mirrored ? (iy == 0 ? 0 : g.ny - iy) : iy;
        const int rx = mirrored ? g.nx - ix : ix;
        const float2 *row = spec + ((int64_t)ry * nxc + rx) * ld_spec;
        double d_y, d_x;
        ssb_shift(g, iy, ix, &d_y, &d_x);
        const double py = g.cy + d_y, px = g.cx + d_x;
        const double my = g.cy - d_y, mx = g.cx - d_x;
        double pr = 0., pi = 0., nr = 0., ni = 0.;
        int np = 0, nn = 0;
        for (int k = threadIdx.x; k < n_k; k += 256) {
            const int i = idx[k];
            const int yi = i / g.sig_w;
            const double y = (double)yi, x = (double)(i - yi * g.sig_w);
            const bool in_p = ssb_in_disk(y, x, py, px, r2);
            const bool in_m = ssb_in_disk(y, x, my, mx, r2);
            const bool pos = q == 0 || (in_p && !in_m);
            const bool neg = q != 0 && in_m && !in_p;
            if (pos || neg) {
                const float2 v = row[k];
                const double re = (double)v.x, im = mirrored ? -(double)v.y : (double)v.y;
                if (pos) {
                    pr += re;
                    pi += im;
                    ++np;
                } else {
                    nr += re;
                    ni += im;
                    ++nn;
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            pr += __shfl_down(pr, off, 64);
            pi += __shfl_down(pi, off, 64);
            nr += __shfl_down(nr, off, 64);
            ni += __shfl_down(ni, off, 64);
            np += __shfl_down(np, off, 64);
            nn += __shfl_down(nn, off, 64);
        }
        if (lane == 0) {
            s_sum[wave][0] = pr;
            s_sum[wave][1] = pi;
            s_sum[wave][2] = nr;
            s_sum[wave][3] = ni;
            s_cnt[wave][0] = np;
            s_cnt[wave][1] = nn;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            SsbAcc a = {0., 0., 0., 0., 0, 0};
            if (!first) a = acc[q];
            for (int w = 0; w < 4; ++w) {
                a.pr += s_sum[w][0];
                a.pi += s_sum[w][1];
                a.nr += s_sum[w][2];
                a.ni += s_sum[w][3];
                a.np += s_cnt[w][0];
                a.nn += s_cnt[w][1];
            }
            if (!last) {
                acc[q] = a;
            } else if (q == 0) {
                fourier[0] = make_float2((float)(a.pr / (double)a.np), (float)(a.pi / (double)a.np));
            } else if (a.np >= g.cutoff && a.nn >= g.cutoff) {
                fourier[q] = make_float2((float)((a.pr / (double)a.np - a.nr / (double)a.nn) / 2.),
                                         (float)((a.pi / (double)a.np - a.ni / (double)a.nn) / 2.));
            } else {
                fourier[q] = make_float2(0.f, 0.f);
            }
        }
        __syncthreads();
    }
}

// gridDim.y of k_ssb_gather: the frames beyond it are walked by the kernel's frame loop
constexpr int64_t SSB_MAX_GRID_Y = 65535;
// workgroups of k_ssb_trotter: the Qs beyond them are walked with a grid stride
constexpr int64_t SSB_MAX_GRID_X = 1 << 20;

template <typename T>
static int run_ssb_gather(const void *tile, int64_t ld, int64_t n, int64_t n_px, const int32_t *idx, int n_idx,
                          float *out, int64_t ld_out, hipStream_t stream) {
    hipLaunchKernelGGL((k_ssb_gather<T>), dim3((unsigned)((n_idx + 255) / 256), (unsigned)std::min(n, SSB_MAX_GRID_Y)),
                       dim3(256), 0, stream, (const T *)tile, ld, n, n_px, idx, n_idx, out, ld_out);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

static int ssb_trotter_launch(const hipfftComplex *spec, int64_t ld_spec, const int32_t *idx, int n_k,
                              const SsbGeom &g, SsbAcc *acc, bool first, bool last, hipfftComplex *fourier,
                              hipStream_t stream) {
    const int64_t n_q = (int64_t)g.ny * g.nx;
    hipLaunchKernelGGL(k_ssb_trotter, dim3((unsigned)std::min(n_q, SSB_MAX_GRID_X)), dim3(256), 0, stream,
                       (const float2 *)spec, ld_spec, idx, n_k, g, acc, first ? 1 : 0, last ? 1 : 0, (float2 *)fourier);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

// what the plans and the single-step entry points ask of the shapes and of the geometry; fills `g`
int ssb_check(const char *who, int ny, int nx, int n_idx, int sig_w, const double *geom, int cutoff, SsbGeom *g) {
    if (ny <= 0 || nx <= 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: scan %d x %d must be positive", who, ny, nx);
    if ((int64_t)ny * nx < 2)
        LTMI_FAIL(LTMI_E_SHAPE, "%s: a scan of one position has no spatial frequency to reconstruct", who);
    if ((int64_t)ny * nx > INT32_MAX) LTMI_FAIL(LTMI_E_SHAPE, "%s: scan %d x %d exceeds 2^31 - 1 positions", who, ny, nx);
    if (n_idx <= 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: %d bright-field pixels: at least one is needed", who, n_idx);
    if (sig_w <= 0) LTMI_FAIL(LTMI_E_SHAPE, "%s: frame width %d must be positive", who, sig_w);
    if (cutoff < 1) LTMI_FAIL(LTMI_E_SHAPE, "%s: cutoff %d must be at least 1", who, cutoff);
    for (int i = 0; i < LTMI_SSB_GEOM; ++i)
        if (!std::isfinite(geom[i])) LTMI_FAIL(LTMI_E_SHAPE, "%s: geometry value %d is not finite", who, i);
    if (!(geom[0] > 0.) || !(geom[1] > 0.) || !(geom[2] > 0.) || !(geom[3] > 0.) || !(geom[4] > 0.))
        LTMI_FAIL(LTMI_E_SHAPE, "%s: lamb, dy, dx, semiconv and semiconv_pix must be positive", who);
    *g = SsbGeom{geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8], geom[9], geom[10],
                 ny, nx, sig_w, cutoff};
    return LTMI_OK;
}

int SsbFront::setup(const char *who, const SsbGeom &g, int batch_) {
    const int64_t n_nav = (int64_t)g.ny * g.nx;
    const int n_spec = g.ny * (g.nx / 2 + 1);
    batch = batch_;
    hipError_t e = real_buf.alloc_zero((size_t)batch * n_nav);
    if (e == hipSuccess) e = spec.alloc_zero((size_t)batch * n_spec);
    if (e == hipSuccess) e = spec_t.alloc_zero((size_t)batch * n_spec);
    if (e != hipSuccess) LTMI_FAIL((int)e, "%s: workspace allocation failed: %s", who, hipGetErrorString(e));
    int n[2] = {g.ny, g.nx};                    // a line scan is a batch of 1D transforms
    return g.ny == 1 ? fwd.plan_many(1, n + 1, (int)n_nav, n_spec, HIPFFT_R2C, batch)
                     : fwd.plan_many(2, n, (int)n_nav, n_spec, HIPFFT_R2C, batch);
}

int SsbFront::run(int device, const SsbGeom &g, const float *bf, int64_t ld_bf, int64_t k0, int64_t n, void *stream) {
    const int64_t n_nav = (int64_t)g.ny * g.nx;
    const int64_t n_spec = (int64_t)g.ny * (g.nx / 2 + 1);
    // column k of bf = the scan image of pixel k
    int rc = ltmi_transpose2d(device, bf + k0, ld_bf, n_nav, n, 4, real_buf, n_nav, stream);
    if (rc == LTMI_OK) rc = fwd.r2c(real_buf, spec);
    if (rc == LTMI_OK) rc = ltmi_transpose2d(device, spec, n_spec, n, n_spec, 8, spec_t, batch, stream);
    return rc;
}

}  // namespace ltmi

using namespace ltmi;

struct ltmi_ssb_plan {
    int device = 0;
    int n_idx = 0;                      // P
    int batch = 0;                      // bright-field pixels per hipFFT execution
    SsbGeom g = {};
    DevBuf<int32_t> idx;                // (P): the bright-field list
    SsbFront front;                     // bf columns -> spectra (ny nxc, batch), and its workspace
    DevBuf<SsbAcc> acc;                 // (ny nx): the sums of the batches so far (plans of more than one batch)
    char last_kernel[128] = {0};
};

static int ssb_setup(ltmi_ssb_plan *p, const int32_t *idx_host) {
    hipError_t e = p->idx.upload(idx_host, (size_t)p->n_idx);
    if (e == hipSuccess && p->batch < p->n_idx) e = p->acc.alloc_zero((size_t)p->g.ny * p->g.nx);
    if (e != hipSuccess) LTMI_FAIL((int)e, "ltmi_ssb_plan_create: workspace allocation failed: %s", hipGetErrorString(e));
    return p->front.setup("ltmi_ssb_plan_create", p->g, p->batch);
}

extern "C" int ltmi_ssb_gather(int device, const void *tile, int tile_dtype, int64_t n_frames, int64_t ld_tile,
                               int64_t n_px, const int32_t *idx_dev, int n_idx, float *out, int64_t ld_out,
                               void *stream_) {
    if (n_frames < 0 || n_px <= 0 || n_idx < 0)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ssb_gather: negative frame count or list length, or an empty frame");
    if (!corr_takes(tile_dtype))
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_ssb_gather: unsupported tile dtype %s", dtype_name(tile_dtype));
    if (ld_tile < n_px) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ssb_gather: ld_tile < frame size");
    if (ld_out < n_idx) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ssb_gather: ld_out < list length");
    if (n_frames == 0 || n_idx == 0) return LTMI_OK;
    if (!tile || !idx_dev || !out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_gather: null pointer");
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    return visit_real_dtype(tile_dtype, [&](auto t) {
        return run_ssb_gather<decltype(t)>(tile, ld_tile, n_frames, n_px, idx_dev, n_idx, out, ld_out, stream);
    }, (int)LTMI_E_DTYPE);                      // (corr_takes above: never)
}

extern "C" int ltmi_ssb_plan_create(int device, int nav_y, int nav_x, int sig_w, const int32_t *idx_host, int n_idx,
                                    int max_batch, const double *geom, int cutoff, ltmi_ssb_plan **out) {
    if (!out || !idx_host || !geom) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_plan_create: null pointer");
    if (max_batch <= 0) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_plan_create: batch %d must be positive", max_batch);
    SsbGeom g;
    const int rc_shape = ssb_check("ltmi_ssb_plan_create", nav_y, nav_x, n_idx, sig_w, geom, cutoff, &g);
    if (rc_shape != LTMI_OK) return rc_shape;
    ssb_column_as_row(&g);
    const int batch = std::min(max_batch, n_idx);
    if ((int64_t)batch * nav_y * nav_x > INT32_MAX)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ssb_plan_create: a batch of %d scans of %d x %d exceeds 2^31 - 1 values", batch,
                  nav_y, nav_x);
    return plan_create(device, out, [&](ltmi_ssb_plan *p) {
        p->n_idx = n_idx;
        p->batch = batch;
        p->g = g;
        return ssb_setup(p, idx_host);
    });
}

extern "C" int ltmi_ssb_plan_destroy(ltmi_ssb_plan *p) { return plan_destroy(p); }

extern "C" const char *ltmi_ssb_plan_last_kernel(const ltmi_ssb_plan *p) {
    return p ? p->last_kernel : "";
}

extern "C" int ltmi_ssb_reconstruct(ltmi_ssb_plan *p, const float *bf, int64_t ld_bf, void *fourier_out,
                                    void *stream_) {
    if (!p) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_reconstruct: null plan");
    if (ld_bf < p->n_idx) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ssb_reconstruct: ld_bf < the plan's %d pixels", p->n_idx);
    if (!bf || !fourier_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_reconstruct: null pointer");
    LTMI_HIP(hipSetDevice(p->device));
    hipStream_t stream = (hipStream_t)stream_;
    const int rc_bind = p->front.fwd.bind(stream);
    if (rc_bind != LTMI_OK) return rc_bind;
    snprintf(p->last_kernel, sizeof(p->last_kernel), "k_transpose<4> + hipfft_r2c + k_transpose<8> + k_ssb_trotter batch=%d",
             p->batch);
    // the batches are bright-field pixels here
    return for_each_batch(p->n_idx, p->batch, [&](int64_t k0, int64_t n) {
        const int rc = p->front.run(p->device, p->g, bf, ld_bf, k0, n, stream_);
        if (rc != LTMI_OK) return rc;
        return ssb_trotter_launch(p->front.spec_t, p->batch, p->idx + k0, (int)n, p->g, p->acc, k0 == 0,
                                  k0 + n == p->n_idx, (hipfftComplex *)fourier_out, stream);
    });
}

extern "C" int ltmi_ssb_trotter(int device, const void *spec, int64_t ld_spec, int nav_y, int nav_x,
                                const int32_t *idx_dev, int n_idx, int sig_w, const double *geom, int cutoff,
                                void *fourier_out, void *stream_) {
    if (!geom) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_trotter: null pointer");
    SsbGeom g;
    const int rc = ssb_check("ltmi_ssb_trotter", nav_y, nav_x, n_idx, sig_w, geom, cutoff, &g);
    if (rc != LTMI_OK) return rc;
    if (ld_spec < n_idx) LTMI_FAIL(LTMI_E_SHAPE, "ltmi_ssb_trotter: ld_spec < list length");
    if (!spec || !idx_dev || !fourier_out) LTMI_FAIL(LTMI_E_INVALID, "ltmi_ssb_trotter: null pointer");
    LTMI_HIP(hipSetDevice(device));
    return ssb_trotter_launch((const hipfftComplex *)spec, ld_spec, idx_dev, n_idx, g, nullptr, true, true,
                              (hipfftComplex *)fourier_out, (hipStream_t)stream_);
}
