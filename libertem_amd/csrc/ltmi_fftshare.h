// What the hipFFT routes share (ltmi_fft.hip, ltmi_corr.hip, ltmi_holo.hip, ltmi_ssb.hip, ltmi_wdd.hip, ltmi_ceps.hip).
#pragma once
#include "ltmi_common.h"
#include <hipfft/hipfft.h>
#include <new>

namespace ltmi {

const char *fft_err(hipfftResult r);   // ltmi_fft.hip

// One batched hipFFT plan and its owner: destroyed by the destructor, move-only, the counterpart of DevBuf.  Every
// call returns an LTMI_* code with the error text set.  The device of the plan must be current when the handle goes
// (the ltmi_*_plan_destroy functions see to it).
class FftHandle {
    hipfftHandle h_ = 0;
    bool made_ = false, bound_ = false;
    hipStream_t stream_ = nullptr;

public:
    FftHandle() = default;
    FftHandle(const FftHandle &) = delete;
    FftHandle &operator=(const FftHandle &) = delete;
    FftHandle(FftHandle &&o) noexcept : h_(o.h_), made_(o.made_), bound_(o.bound_), stream_(o.stream_) { o.made_ = false; }
    FftHandle &operator=(FftHandle &&o) noexcept {
        std::swap(h_, o.h_);
        std::swap(made_, o.made_);
        std::swap(bound_, o.bound_);
        std::swap(stream_, o.stream_);
        return *this;
    }
    ~FftHandle() {
        if (made_) (void)hipfftDestroy(h_);
    }
    bool made() const { return made_; }
    explicit operator bool() const { return made_; }
    // `batch` contiguous transforms of n[0] (x n[1]), input and output idist / odist elements apart
    int plan_many(int rank, int *n, int idist, int odist, hipfftType type, int batch) {
        if (made_) LTMI_FAIL(LTMI_E_INVALID, "hipfftPlanMany: the handle holds a plan already");
        const hipfftResult r = hipfftPlanMany(&h_, rank, n, nullptr, 1, idist, nullptr, 1, odist, type, batch);
        if (r != HIPFFT_SUCCESS)
            LTMI_FAIL(LTMI_E_INVALID, "hipfftPlanMany(%s %d x %d, batch %d) failed: %s",
                      type == HIPFFT_R2C ? "R2C" : type == HIPFFT_C2R ? "C2R" : "C2C", rank == 1 ? 1 : n[0], n[rank - 1],
                      batch, fft_err(r));
        made_ = true;
        return LTMI_OK;
    }
    // the transforms run on `stream` from here on
    int bind(hipStream_t stream) {
        if (bound_ && stream_ == stream) return LTMI_OK;
        const hipfftResult r = hipfftSetStream(h_, stream);
        if (r != HIPFFT_SUCCESS) LTMI_FAIL(LTMI_E_INVALID, "hipfftSetStream failed: %s", fft_err(r));
        stream_ = stream;
        bound_ = true;
        return LTMI_OK;
    }
    int r2c(float *in, hipfftComplex *out) {
        const hipfftResult r = hipfftExecR2C(h_, in, out);
        if (r != HIPFFT_SUCCESS) LTMI_FAIL(LTMI_E_INVALID, "hipfftExecR2C failed: %s", fft_err(r));
        return LTMI_OK;
    }
    int c2r(hipfftComplex *in, float *out) {
        const hipfftResult r = hipfftExecC2R(h_, in, out);
        if (r != HIPFFT_SUCCESS) LTMI_FAIL(LTMI_E_INVALID, "hipfftExecC2R failed: %s", fft_err(r));
        return LTMI_OK;
    }
    int c2c(hipfftComplex *in, hipfftComplex *out, int direction) {
        const hipfftResult r = hipfftExecC2C(h_, in, out, direction);
        if (r != HIPFFT_SUCCESS) LTMI_FAIL(LTMI_E_INVALID, "hipfftExecC2C failed: %s", fft_err(r));
        return LTMI_OK;
    }
};

// The skeleton of the ltmi_*_plan_create functions: a plan P on `device`, filled and set up by setup(p) -> LTMI_*;
// a plan whose set-up fails is deleted (its members free what they hold) and its code returned.
template <typename P, typename Setup>
static int plan_create(int device, P **out, Setup setup) {
    LTMI_HIP(hipSetDevice(device));
    P *p = new (std::nothrow) P();
    if (!p) LTMI_FAIL(LTMI_E_NOMEM, "out of host memory");
    p->device = device;
    const int rc = setup(p);
    if (rc != LTMI_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return LTMI_OK;
}

// ... and of the ltmi_*_plan_destroy functions: the members go with the plan's device current
template <typename P>
static int plan_destroy(P *p) {
    if (!p) return LTMI_OK;
    (void)hipSetDevice(p->device);
    delete p;
    return LTMI_OK;
}

// body(f0, n) -> LTMI_* for the batches [f0, f0 + n) of `total` frames, n <= batch, in order; stops at the first error
template <typename Body>
static int for_each_batch(int64_t total, int64_t batch, Body body) {
    for (int64_t f0 = 0; f0 < total; f0 += batch) {
        const int rc = body(f0, std::min(batch, total - f0));
        if (rc != LTMI_OK) return rc;
    }
    return LTMI_OK;
}

// frame f0 of a tile whose frames are ld elements of tile_dtype apart
static inline const void *frame_at(const void *tile, int tile_dtype, int64_t ld, int64_t f0) {
    return (const char *)tile + (size_t)f0 * ld * (size_t)dtype_size(tile_dtype);
}

// The plans always transform `batch` frames: after a partial batch of n the unused tail of real_buf holds zeros, not
// what an earlier batch left there (its transforms are never read).
static inline int zero_tail(float *real_buf, int64_t n, int64_t batch, int64_t n_px, hipStream_t stream) {
    if (n < batch) LTMI_HIP(hipMemsetAsync(real_buf + n * n_px, 0, (size_t)(batch - n) * n_px * sizeof(float), stream));
    return LTMI_OK;
}

// f(T()) for the element type T of the tile dtypes k_corr_load and k_ssb_gather convert -- bool, 1- / 2- / 4-byte
// integers, float32, float64 --, `otherwise` for every other dtype
template <typename F, typename R>
static R visit_real_dtype(int tile_dtype, F f, R otherwise) {
    switch (tile_dtype) {
        case LTMI_BOOL:
        case LTMI_U8: return f(uint8_t());
        case LTMI_I8: return f(int8_t());
        case LTMI_U16: return f(uint16_t());
        case LTMI_I16: return f(int16_t());
        case LTMI_U32: return f(uint32_t());
        case LTMI_I32: return f(int32_t());
        case LTMI_F32: return f(float());
        case LTMI_F64: return f(double());
        default: return otherwise;
    }
}
static inline bool corr_takes(int tile_dtype) {
    return visit_real_dtype(tile_dtype, [](auto) { return true; }, false);
}
// n frames of n_px pixels (native dtype, ld elements apart) -> contiguous float32 at `out`, by k_corr_load<dtype> (ltmi_corr.hip)
int corr_load(const void *src, int tile_dtype, int64_t ld, int64_t n, int64_t n_px, float *out, hipStream_t stream);

// The first steps of a batch of correlation and holography: n <= batch frames at `src` -> real_buf (k_corr_load), the
// tail cleared, the batched forward transform into `spec`
static inline int load_and_forward(FftHandle &fwd, const void *src, int tile_dtype, int64_t ld, int64_t n, int64_t batch,
                                   int64_t n_px, float *real_buf, hipfftComplex *spec, hipStream_t stream) {
    int rc = corr_load(src, tile_dtype, ld, n, n_px, real_buf, stream);
    if (rc == LTMI_OK) rc = zero_tail(real_buf, n, batch, n_px, stream);
    return rc == LTMI_OK ? fwd.r2c(real_buf, spec) : rc;
}

}  // namespace ltmi
