// What the two ptychography routes share (ltmi_ssb.hip, ltmi_wdd.hip): the geometry, the float64 disk predicates and
// the batch front end that turns columns of bf into spectra over the scan axes, a Q's pixels contiguous.
#pragma once
#include "ltmi_fftshare.h"
#include <algorithm>

// the disk predicates agree with a NumPy float64 evaluation of the same expressions bit for bit: every product and
// sum below is rounded on its own (the pragma holds for the rest of the file that includes this one)
#pragma clang fp contract(off)

namespace ltmi {

// the geometry of include/ltmi.h's `geom` array, plus the shapes the kernels need
struct SsbGeom {
    double lamb, dy, dx, semiconv, semiconv_pix, cy, cx, t00, t01, t10, t11;
    int ny, nx, sig_w, cutoff;
};

__host__ __device__ static inline int ssb_signed(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }

// d = T q lamb semiconv_pix / semiconv for Q = (iy, ix), q = (s(iy) / (Ny dy), s(ix) / (Nx dx)): the shift of the
// diffracted disks in detector pixels, evaluated left to right
__host__ __device__ static inline void ssb_shift(const SsbGeom &g, int iy, int ix, double *d_y, double *d_x) {
    const double qy = (double)ssb_signed(iy, g.ny) / ((double)g.ny * g.dy);
    const double qx = (double)ssb_signed(ix, g.nx) / ((double)g.nx * g.dx);
    const double ty = g.t00 * qy + g.t01 * qx;
    const double tx = g.t10 * qy + g.t11 * qx;
    *d_y = ty * g.lamb * g.semiconv_pix / g.semiconv;
    *d_x = tx * g.lamb * g.semiconv_pix / g.semiconv;
}

__host__ __device__ static inline bool ssb_in_disk(double y, double x, double cy, double cx, double r2) {
    return (y - cy) * (y - cy) + (x - cx) * (x - cx) < r2;
}

// what the plans and the single-step entry points ask of the shapes and of the geometry; fills `g` (ltmi_ssb.hip)
int ssb_check(const char *who, int ny, int nx, int n_idx, int sig_w, const double *geom, int cutoff, SsbGeom *g);

// a scan of one column is a scan of one row with the roles of the axes exchanged: the same scan images, the same Qs
// in the same order, and T q = (t00 qy + 0, t10 qy + 0) either way, bit for bit
static inline void ssb_column_as_row(SsbGeom *g) {
    if (g->nx != 1) return;
    g->nx = g->ny;
    g->ny = 1;
    std::swap(g->dy, g->dx);
    std::swap(g->t00, g->t01);
    std::swap(g->t10, g->t11);
}

// The front end of a batch: ltmi_transpose2d (bf (N, P) -> (batch, N)), one batched real-to-complex hipFFT over the
// scan axes, ltmi_transpose2d ((batch, Ny Nxc) -> (Ny Nxc, batch)).  Defined in ltmi_ssb.hip.
struct SsbFront {
    int batch = 0;                      // pixels per hipFFT execution
    DevBuf<float> real_buf;             // (batch, ny, nx) f32: one scan image per pixel
    DevBuf<hipfftComplex> spec;         // (batch, ny, nxc) c64
    DevBuf<hipfftComplex> spec_t;       // (ny nxc, batch) c64: the same, a Q's pixels contiguous
    FftHandle fwd;                      // batched R2C over the scan axes

    // the workspace and the hipFFT plan for `batch` pixels of a (g.ny, g.nx) scan; `who` names the caller in errors
    int setup(const char *who, const SsbGeom &g, int batch);
    // columns [k0, k0 + n) of bf, n <= batch -> spec_t[(ry nxc + rx) batch + j] = G[k0 + j, ry, rx] on the stream the
    // handle is bound to.  The plan always transforms `batch` images: a partial last batch leaves the images of an
    // earlier one in the tail, whose spectra are never read.
    int run(int device, const SsbGeom &g, const float *bf, int64_t ld_bf, int64_t k0, int64_t n, void *stream);
};

}  // namespace ltmi
