// What the hipFFT routes share (ltmi_fft.hip, ltmi_corr.hip, ltmi_holo.hip).
#pragma once
#include "ltmi_common.h"
#include <hipfft/hipfft.h>

namespace ltmi {

const char *fft_err(hipfftResult r);   // ltmi_fft.hip

// the tile dtypes k_corr_load converts: bool, 1- / 2- / 4-byte integers, float32, float64 (ltmi_corr.hip)
bool corr_takes(int tile_dtype);
// n frames of n_px pixels (native dtype, ld elements apart) -> contiguous float32 at `out`, by k_corr_load<dtype>
int corr_load(const void *src, int tile_dtype, int64_t ld, int64_t n, int64_t n_px, float *out, hipStream_t stream);

}  // namespace ltmi
