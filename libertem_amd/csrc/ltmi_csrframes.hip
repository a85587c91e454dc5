// Sparse frames (CSR over the flattened signal axis: the triple of a raw_csr dataset) on gfx950.
//
//   ltmi_csr_check        one pass over every row: index range, row order, indptr
//   ltmi_csr_densify      frames of the triple -> a dense tile (zero fill + scatter)
//   ltmi_apply_masks_csr  out[f, m] (+)= sum_k data[k] * W[indices[k], m] over the stored entries of frame f
//   ltmi_csr_sum_sig      out[f] (+)= sum_k data[k] over the stored entries of frame f
//   ltmi_csr_sum_frames   out[p] (+)= sum over the frames of their entry at pixel p
//
// The rows are canonical (strictly ascending indices, checked once by ltmi_csr_check): every pixel of a
// frame is stored at most once, so the scatter uses plain stores and the product needs no atomics.
#include "ltmi_common.h"

namespace ltmi {

constexpr int CSR_MAX_MASKS = 64;      // the pixel-major image pads M to 4 .. 64 columns (a power of two)

// ---- check ------------------------------------------------------------------------------------------
// flags[0] |= 1: data that cannot be read (index outside [0, n_px), indptr decreasing or outside [0, nnz],
//                not starting at 0 or not ending at nnz);  |= 2: a row that is unsorted or holds a pixel twice
__global__ void k_csr_check(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n_rows,
                            int64_t n_px, int64_t nnz, int *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int bad = 0;
    if (wave == 0 && lane == 0 && (indptr[0] != 0 || indptr[n_rows] != nnz)) bad |= 1;
    for (int64_t r = wave; r < n_rows; r += n_waves) {
        const int64_t a = indptr[r], b = indptr[r + 1];
        if (a < 0 || b > nnz || a > b) {            // (nothing of this row is read)
            bad |= 1;
            continue;
        }
        for (int64_t k = a + lane; k < b; k += 64) {
            const int32_t i = indices[k];
            if (i < 0 || (int64_t)i >= n_px) bad |= 1;
            if (k > a && indices[k - 1] >= i) bad |= 2;
        }
    }
    if (bad) atomicOr(flags, bad);
}

// ---- densify ----------------------------------------------------------------------------------------
// one workgroup per frame: zero the n_px pixels of its row of the tile (16-byte stores over the aligned
// middle), barrier, scatter the stored entries
template <typename T>
__global__ void k_csr_densify(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                              const T *__restrict__ data, const int32_t *__restrict__ rows, int64_t row0,
                              int64_t n_frames, int64_t n_px, T *__restrict__ out, int64_t ld) {
    for (int64_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
        T *dst = out + f * ld;
        const uintptr_t p0 = (uintptr_t)dst, p1 = p0 + (uintptr_t)n_px * sizeof(T);
        uintptr_t a0 = (p0 + 15) & ~(uintptr_t)15, a1 = p1 & ~(uintptr_t)15;
        if (a0 > a1) a0 = a1 = p0;                                  // (shorter than one aligned unit)
        const int64_t head = (int64_t)((a0 - p0) / sizeof(T)), body = (int64_t)((a1 - a0) / 16);
        const int64_t tail0 = (int64_t)((a1 - p0) / sizeof(T));
        for (int64_t i = threadIdx.x; i < head; i += blockDim.x) dst[i] = T(0);
        uint4 *mid = (uint4 *)a0;
        for (int64_t i = threadIdx.x; i < body; i += blockDim.x) mid[i] = make_uint4(0, 0, 0, 0);
        for (int64_t i = tail0 + threadIdx.x; i < n_px; i += blockDim.x) dst[i] = T(0);
        __syncthreads();
        const int64_t r = rows ? (int64_t)rows[f] : row0 + f;
        const int64_t a = indptr[r], b = indptr[r + 1];
        for (int64_t k = a + threadIdx.x; k < b; k += blockDim.x) {
            const int32_t i = indices[k];
            if ((uint32_t)i < (uint64_t)n_px) dst[i] = data[k];
        }
        __syncthreads();
    }
}

// ---- pixel-major image of a dense stack ---------------------------------------------------------------
template <typename A>
__global__ void k_csr_build_px(const A *__restrict__ gmasks, A *__restrict__ img, int64_t n_masks, int64_t n_px,
                               int m_pad) {
    const int64_t total = n_px * m_pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i / m_pad, m = i % m_pad;
        img[i] = m < n_masks ? gmasks[m * n_px + p] : A(0);
    }
}

// ---- the product --------------------------------------------------------------------------------------
// One wave per frame.  A lane owns V = 16 / sizeof(A) neighbouring masks (one 16-byte load of the image row
// of an event) of mask group g = lane % G, G = m_pad / V, and walks the events s, s + S, s + 2 S, ... of the
// frame, s = lane / G, S = 64 / G: a wave-wide load fetches the whole m_pad-column rows of S events.  The S
// partial sums of a mask are added across the lanes in a fixed order (xor shuffles), slot 0 stores.
template <typename T, typename A>
__global__ void __launch_bounds__(256)
k_apply_csr(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const T *__restrict__ data,
            const int32_t *__restrict__ rows, int64_t row0, int64_t n_frames, int64_t n_px,
            const A *__restrict__ img, int m_pad, int n_masks, A *__restrict__ out, int64_t ld_out,
            int accumulate) {
    constexpr int V = 16 / (int)sizeof(A);
    const int lane = threadIdx.x & 63;
    const int G = m_pad / V, S = 64 / G;
    const int g = lane % G, s = lane / G;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t f = wave; f < n_frames; f += n_waves) {
        const int64_t r = rows ? (int64_t)rows[f] : row0 + f;
        const int64_t a = indptr[r], b = indptr[r + 1];
        A acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = A(0);
        for (int64_t k = a + s; k < b; k += S) {
            const int32_t i = indices[k];
            if ((uint32_t)i >= (uint64_t)n_px) continue;
            const A x = (A)data[k];
            const A *w = img + (int64_t)i * m_pad + g * V;
            A wv[V];
            __builtin_memcpy(wv, __builtin_assume_aligned(w, 16), 16);      // one 16-byte load
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += x * wv[j];
        }
        for (int off = G; off < 64; off <<= 1) {
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
        }
        if (s == 0) {
            A *o = out + f * ld_out + g * V;
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (g * V + j < n_masks) o[j] = accumulate ? o[j] + acc[j] : acc[j];
        }
    }
}

static int pad_masks(int64_t n_masks, int v) {
    int m = v;
    while (m < n_masks) m <<= 1;
    return m;
}

template <typename A>
static int ensure_px_image(ltmi_masks *m, hipStream_t stream) {
    if (m->img_px) return LTMI_OK;
    constexpr int V = 16 / (int)sizeof(A);
    m->m_pad_px = pad_masks(m->n_masks, V);
    const size_t n = (size_t)m->n_px * m->m_pad_px;
    LTMI_HIP(m->img_px.alloc(n * sizeof(A)));
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 65535);
    hipLaunchKernelGGL((k_csr_build_px<A>), dim3(blocks), dim3(256), 0, stream, (const A *)m->gmasks.get(),
                       (A *)m->img_px.get(), m->n_masks, m->n_px, m->m_pad_px);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

template <typename T, typename A>
static int launch_apply_csr(ltmi_masks *m, const int64_t *indptr, const int32_t *indices, const void *data,
                            const int32_t *rows, int64_t row0, int64_t n_frames, void *out, int64_t ld_out,
                            int accumulate, hipStream_t stream, const char *tname, const char *aname) {
    const int rc = ensure_px_image<A>(m, stream);
    if (rc != LTMI_OK) return rc;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_frames + 3) / 4, 1 << 20);
    hipLaunchKernelGGL((k_apply_csr<T, A>), dim3(blocks), dim3(256), 0, stream, indptr, indices, (const T *)data,
                       rows, row0, n_frames, m->n_px, (const A *)m->img_px.get(), m->m_pad_px, (int)m->n_masks,
                       (A *)out, ld_out, accumulate);
    LTMI_HIP(hipGetLastError());
    snprintf(m->last_kernel, sizeof(m->last_kernel), "k_apply_csr<%s,%s> m_pad=%d%s grid=(%u)", tname, aname,
             m->m_pad_px, rows ? " rows" : "", blocks);
    return LTMI_OK;
}

// ---- sums on the stored entries -------------------------------------------------------------------------
// the kernel of the last sum launched by this thread ("" before the first): ltmi_csr_last_kernel
thread_local char t_last_kernel[64] = {0};

template <typename T> struct SumAcc { typedef int64_t type; };      // integers: exact
template <> struct SumAcc<float> { typedef double type; };          // float32: rounded once, at the end

// One wave per frame, lanes striding the row; the 64 partial sums are added in a fixed order (xor shuffles),
// lane 0 stores.  An index outside [0, n_px) is skipped.
template <typename T, typename O>
__global__ void __launch_bounds__(256)
k_csr_sum_sig(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const T *__restrict__ data,
              const int32_t *__restrict__ rows, int64_t row0, int64_t n_frames, int64_t n_px, O *__restrict__ out,
              int accumulate) {
    typedef typename SumAcc<T>::type A;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t f = wave; f < n_frames; f += n_waves) {
        const int64_t r = rows ? (int64_t)rows[f] : row0 + f;
        const int64_t a = indptr[r], b = indptr[r + 1];
        A acc = A(0);
        for (int64_t k = a + lane; k < b; k += 64)
            if ((uint32_t)indices[k] < (uint64_t)n_px) acc += (A)data[k];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) out[f] = accumulate ? out[f] + (O)acc : (O)acc;
    }
}

// Workgroup (bx, by) owns the CSR_SUM_PX pixels from bx * CSR_SUM_PX -- int64 sums in LDS -- and the frames of
// split by.  A wave takes 64 frames at a time: lane l finds the sub-range of frame l that falls into the
// block (binary search in the ascending row), then the wave's four groups of 16 lanes walk one sub-range
// each and add into LDS (integer adds: any order gives the same bits).  The block's sums go to
// part[by][pixel] with plain stores; k_csr_sum_frames_store adds the splits.
constexpr int CSR_SUM_PX = 4096;          // 32 KiB of LDS: four workgroups per CU
constexpr int CSR_SUM_MIN_FRAMES = 64;    // frames a split holds at least: one trip of one wave
constexpr int CSR_SUM_MAX_SPLITS = 64;
constexpr int CSR_SUM_WGS = 1024;         // workgroups wanted at most: four per CU

__device__ __forceinline__ int64_t csr_lower_bound(const int32_t *__restrict__ indices, int64_t a, int64_t b,
                                                   int64_t p) {
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if ((int64_t)indices[m] < p) a = m + 1; else b = m;
    }
    return a;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_csr_sum_frames(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const T *__restrict__ data,
                 const int32_t *__restrict__ rows, int64_t row0, int64_t n_frames, int64_t n_px,
                 int64_t frames_per_split, int64_t *__restrict__ part) {
    __shared__ unsigned long long acc[CSR_SUM_PX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n_wv = blockDim.x >> 6;
    const int grp = lane >> 4, sub = lane & 15;
    const int64_t p0 = (int64_t)blockIdx.x * CSR_SUM_PX, p1 = min(p0 + (int64_t)CSR_SUM_PX, n_px);
    const int64_t f0 = (int64_t)blockIdx.y * frames_per_split, f1 = min(f0 + frames_per_split, n_frames);
    for (int i = threadIdx.x; i < CSR_SUM_PX; i += blockDim.x) acc[i] = 0ull;
    __syncthreads();
    for (int64_t base = f0 + (int64_t)wv * 64; base < f1; base += (int64_t)n_wv * 64) {
        int64_t lo = 0, hi = 0;
        if (base + lane < f1) {
            const int64_t f = base + lane;
            const int64_t r = rows ? (int64_t)rows[f] : row0 + f;
            const int64_t a = indptr[r], b = indptr[r + 1];
            // (the first and the last block take the row's own ends: an index below 0 or from n_px on is left to
            // the range test below)
            lo = p0 == 0 ? a : csr_lower_bound(indices, a, b, p0);
            hi = p1 == n_px ? b : csr_lower_bound(indices, lo, b, p1);
        }
        const int nf = (int)min((int64_t)64, f1 - base);
        for (int j0 = 0; j0 < nf; j0 += 4) {
            const int j = min(j0 + grp, 63);
            // (both shuffles with every lane active: lane j may belong to a group that has no frame in this trip)
            const int64_t l = __shfl(lo, j, 64), hj = __shfl(hi, j, 64);
            const int64_t h = j0 + grp < nf ? hj : l;
            for (int64_t k = l + sub; k < h; k += 16) {
                const int64_t i = (int64_t)indices[k] - p0;
                if ((uint64_t)i < (uint64_t)(p1 - p0)) atomicAdd(&acc[i], (unsigned long long)(int64_t)data[k]);
            }
        }
    }
    __syncthreads();
    int64_t *dst = part + (int64_t)blockIdx.y * n_px + p0;
    for (int64_t i = threadIdx.x; i < p1 - p0; i += blockDim.x) dst[i] = (int64_t)acc[i];
}

template <typename O>
__global__ void k_csr_sum_frames_store(const int64_t *__restrict__ part, int n_splits, int64_t n_px,
                                       O *__restrict__ out, int accumulate) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_px;
         p += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = 0;
        for (int k = 0; k < n_splits; ++k) s += part[(int64_t)k * n_px + p];
        out[p] = accumulate ? out[p] + (O)s : (O)s;
    }
}

static int64_t csr_sum_blocks(int64_t n_px) { return (n_px + CSR_SUM_PX - 1) / CSR_SUM_PX; }

static int csr_sum_max_splits(int64_t n_px) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(CSR_SUM_MAX_SPLITS, CSR_SUM_WGS / csr_sum_blocks(n_px)));
}

static void csr_sum_name(const char *kernel, const char *tname, int out_dtype, bool rows) {
    snprintf(t_last_kernel, sizeof(t_last_kernel), "%s<%s,%s>%s", kernel, tname,
             out_dtype == LTMI_F64 ? "f64" : "f32", rows ? " rows" : "");
}

template <typename T>
static int launch_csr_sum_sig(const int64_t *indptr, const int32_t *indices, const void *data, const int32_t *rows,
                              int64_t row0, int64_t n_frames, int64_t n_px, void *out, int out_dtype, int accumulate,
                              hipStream_t stream, const char *tname) {
    const unsigned blocks = (unsigned)std::min<int64_t>((n_frames + 3) / 4, 1 << 20);
    if (out_dtype == LTMI_F64)
        hipLaunchKernelGGL((k_csr_sum_sig<T, double>), dim3(blocks), dim3(256), 0, stream, indptr, indices,
                           (const T *)data, rows, row0, n_frames, n_px, (double *)out, accumulate);
    else
        hipLaunchKernelGGL((k_csr_sum_sig<T, float>), dim3(blocks), dim3(256), 0, stream, indptr, indices,
                           (const T *)data, rows, row0, n_frames, n_px, (float *)out, accumulate);
    LTMI_HIP(hipGetLastError());
    csr_sum_name("k_csr_sum_sig", tname, out_dtype, rows != nullptr);
    return LTMI_OK;
}

template <typename T>
static int launch_csr_sum_frames(const int64_t *indptr, const int32_t *indices, const void *data,
                                 const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px, void *out,
                                 int out_dtype, int accumulate, int64_t *part, hipStream_t stream,
                                 const char *tname) {
    const int64_t n_blocks = csr_sum_blocks(n_px);
    int64_t splits = std::min<int64_t>(csr_sum_max_splits(n_px),
                                       (n_frames + CSR_SUM_MIN_FRAMES - 1) / CSR_SUM_MIN_FRAMES);
    const int64_t per_split = (n_frames + splits - 1) / splits;
    splits = (n_frames + per_split - 1) / per_split;              // (no split without frames)
    hipLaunchKernelGGL((k_csr_sum_frames<T>), dim3((unsigned)n_blocks, (unsigned)splits), dim3(256), 0, stream,
                       indptr, indices, (const T *)data, rows, row0, n_frames, n_px, per_split, part);
    LTMI_HIP(hipGetLastError());
    const unsigned blocks = (unsigned)std::min<int64_t>((n_px + 255) / 256, 65535);
    if (out_dtype == LTMI_F64)
        hipLaunchKernelGGL((k_csr_sum_frames_store<double>), dim3(blocks), dim3(256), 0, stream, part, (int)splits,
                           n_px, (double *)out, accumulate);
    else
        hipLaunchKernelGGL((k_csr_sum_frames_store<float>), dim3(blocks), dim3(256), 0, stream, part, (int)splits,
                           n_px, (float *)out, accumulate);
    LTMI_HIP(hipGetLastError());
    csr_sum_name("k_csr_sum_frames", tname, out_dtype, rows != nullptr);
    return LTMI_OK;
}

}  // namespace ltmi

extern "C" int ltmi_csr_check(int device, const int64_t *indptr, const int32_t *indices, int64_t n_rows,
                              int64_t n_px, int64_t nnz, int *flags, void *stream_) {
    if (!indptr || !flags || n_rows < 0 || n_px <= 0 || nnz < 0 || (nnz > 0 && !indices))
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_csr_check: bad arguments (n_rows=%lld n_px=%lld nnz=%lld)",
                  (long long)n_rows, (long long)n_px, (long long)nnz);
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    LTMI_HIP(hipMemsetAsync(flags, 0, sizeof(int), stream));
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_rows + 3) / 4, 1 << 16));
    hipLaunchKernelGGL(ltmi::k_csr_check, dim3(blocks), dim3(256), 0, stream, indptr, indices, n_rows, n_px, nnz,
                       flags);
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

extern "C" int ltmi_csr_densify(int device, const int64_t *indptr, const int32_t *indices, const void *data,
                                int data_dtype, const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px,
                                void *out, int64_t ld_out, void *stream_) {
    if (!indptr || !out || n_frames < 0 || n_px <= 0 || ld_out < n_px || row0 < 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_csr_densify: bad arguments (n_frames=%lld n_px=%lld ld_out=%lld)",
                  (long long)n_frames, (long long)n_px, (long long)ld_out);
    if (n_frames == 0) return LTMI_OK;
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)std::min<int64_t>(n_frames, 1 << 20)), block(256);
#define LTMI_DENSIFY(T)                                                                                     \
    hipLaunchKernelGGL((ltmi::k_csr_densify<T>), grid, block, 0, stream, indptr, indices, (const T *)data, \
                       rows, row0, n_frames, n_px, (T *)out, ld_out)
    // (the bytes are moved, not interpreted: one kernel per item size)
    switch (ltmi::dtype_size(data_dtype)) {
        case 1: LTMI_DENSIFY(uint8_t); break;
        case 2: LTMI_DENSIFY(uint16_t); break;
        case 4: LTMI_DENSIFY(uint32_t); break;
        case 8: LTMI_DENSIFY(uint64_t); break;
        default:
            LTMI_FAIL(LTMI_E_DTYPE, "ltmi_csr_densify: data dtype %s is not supported", ltmi::dtype_name(data_dtype));
    }
#undef LTMI_DENSIFY
    LTMI_HIP(hipGetLastError());
    return LTMI_OK;
}

extern "C" int ltmi_apply_masks_csr(ltmi_masks *m, const int64_t *indptr, const int32_t *indices, const void *data,
                                    int data_dtype, const int32_t *rows, int64_t row0, int64_t n_frames, void *out,
                                    int64_t ld_out, int accumulate, void *stream_, int *handled) {
    if (!m || !indptr || !out || !handled || n_frames < 0 || row0 < 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_apply_masks_csr: bad arguments");
    *handled = 0;
    // real floating stacks that are held dense and multiplied dense, of at most CSR_MAX_MASKS masks
    if ((m->kind != 0 && m->kind != 1) || !m->gmasks || m->sparse_origin != nullptr ||
        (m->result_dtype != LTMI_F32 && m->result_dtype != LTMI_F64) || m->n_masks > ltmi::CSR_MAX_MASKS)
        return LTMI_OK;
    if (ld_out < m->n_masks)
        LTMI_FAIL(LTMI_E_SHAPE, "ltmi_apply_masks_csr: ld_out %lld < %lld masks", (long long)ld_out,
                  (long long)m->n_masks);
    const bool f64 = m->result_dtype == LTMI_F64;
    switch (data_dtype) {
        case LTMI_U8: case LTMI_U16: case LTMI_I16: case LTMI_U32: case LTMI_I32: case LTMI_F32: break;
        default: return LTMI_OK;
    }
    *handled = 1;
    if (n_frames == 0) return LTMI_OK;
    LTMI_HIP(hipSetDevice(m->device));
    hipStream_t stream = (hipStream_t)stream_;
#define LTMI_APPLY_CSR(T, NAME)                                                                               \
    return f64 ? ltmi::launch_apply_csr<T, double>(m, indptr, indices, data, rows, row0, n_frames, out, ld_out, \
                                                   accumulate, stream, NAME, "f64")                           \
               : ltmi::launch_apply_csr<T, float>(m, indptr, indices, data, rows, row0, n_frames, out, ld_out,  \
                                                  accumulate, stream, NAME, "f32")
    switch (data_dtype) {
        case LTMI_U8: LTMI_APPLY_CSR(uint8_t, "u8");
        case LTMI_U16: LTMI_APPLY_CSR(uint16_t, "u16");
        case LTMI_I16: LTMI_APPLY_CSR(int16_t, "i16");
        case LTMI_U32: LTMI_APPLY_CSR(uint32_t, "u32");
        case LTMI_I32: LTMI_APPLY_CSR(int32_t, "i32");
        default: LTMI_APPLY_CSR(float, "f32");
    }
#undef LTMI_APPLY_CSR
}

extern "C" int ltmi_csr_max_masks(void) { return ltmi::CSR_MAX_MASKS; }

extern "C" int ltmi_csr_sum_sig(int device, const int64_t *indptr, const int32_t *indices, const void *data,
                                int data_dtype, const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px,
                                void *out, int out_dtype, int accumulate, void *stream_) {
    if (!indptr || !out || n_frames < 0 || n_px <= 0 || row0 < 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_csr_sum_sig: bad arguments (n_frames=%lld n_px=%lld)", (long long)n_frames,
                  (long long)n_px);
    if (out_dtype != LTMI_F32 && out_dtype != LTMI_F64)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_csr_sum_sig: output dtype %s is not supported", ltmi::dtype_name(out_dtype));
    switch (data_dtype) {
        case LTMI_U8: case LTMI_U16: case LTMI_I16: case LTMI_U32: case LTMI_I32: case LTMI_F32: break;
        default:
            LTMI_FAIL(LTMI_E_DTYPE, "ltmi_csr_sum_sig: data dtype %s is not supported", ltmi::dtype_name(data_dtype));
    }
    if (n_frames == 0) return LTMI_OK;
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
#define LTMI_CSR_SUM_SIG(T, NAME)                                                                                  \
    return ltmi::launch_csr_sum_sig<T>(indptr, indices, data, rows, row0, n_frames, n_px, out, out_dtype, accumulate, \
                                       stream, NAME)
    switch (data_dtype) {
        case LTMI_U8: LTMI_CSR_SUM_SIG(uint8_t, "u8");
        case LTMI_U16: LTMI_CSR_SUM_SIG(uint16_t, "u16");
        case LTMI_I16: LTMI_CSR_SUM_SIG(int16_t, "i16");
        case LTMI_U32: LTMI_CSR_SUM_SIG(uint32_t, "u32");
        case LTMI_I32: LTMI_CSR_SUM_SIG(int32_t, "i32");
        default: LTMI_CSR_SUM_SIG(float, "f32");
    }
#undef LTMI_CSR_SUM_SIG
}

extern "C" int64_t ltmi_csr_sum_frames_workspace(int64_t n_px) {
    if (n_px <= 0) return 0;
    return (int64_t)ltmi::csr_sum_max_splits(n_px) * n_px * (int64_t)sizeof(int64_t);
}

extern "C" int ltmi_csr_sum_frames(int device, const int64_t *indptr, const int32_t *indices, const void *data,
                                   int data_dtype, const int32_t *rows, int64_t row0, int64_t n_frames, int64_t n_px,
                                   void *out, int out_dtype, int accumulate, void *workspace, void *stream_) {
    if (!indptr || !out || !workspace || n_frames < 0 || n_px <= 0 || row0 < 0)
        LTMI_FAIL(LTMI_E_INVALID, "ltmi_csr_sum_frames: bad arguments (n_frames=%lld n_px=%lld)",
                  (long long)n_frames, (long long)n_px);
    if (out_dtype != LTMI_F32 && out_dtype != LTMI_F64)
        LTMI_FAIL(LTMI_E_DTYPE, "ltmi_csr_sum_frames: output dtype %s is not supported",
                  ltmi::dtype_name(out_dtype));
    switch (data_dtype) {
        case LTMI_U8: case LTMI_U16: case LTMI_I16: case LTMI_U32: case LTMI_I32: break;
        default:
            LTMI_FAIL(LTMI_E_DTYPE, "ltmi_csr_sum_frames: data dtype %s is not supported (integer data only)",
                      ltmi::dtype_name(data_dtype));
    }
    if (n_frames == 0) return LTMI_OK;
    LTMI_HIP(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
#define LTMI_CSR_SUM_FRAMES(T, NAME)                                                                          \
    return ltmi::launch_csr_sum_frames<T>(indptr, indices, data, rows, row0, n_frames, n_px, out, out_dtype, \
                                          accumulate, (int64_t *)workspace, stream, NAME)
    switch (data_dtype) {
        case LTMI_U8: LTMI_CSR_SUM_FRAMES(uint8_t, "u8");
        case LTMI_U16: LTMI_CSR_SUM_FRAMES(uint16_t, "u16");
        case LTMI_I16: LTMI_CSR_SUM_FRAMES(int16_t, "i16");
        case LTMI_U32: LTMI_CSR_SUM_FRAMES(uint32_t, "u32");
        default: LTMI_CSR_SUM_FRAMES(int32_t, "i32");
    }
#undef LTMI_CSR_SUM_FRAMES
}

extern "C" const char *ltmi_csr_last_kernel(void) { return ltmi::t_last_kernel; }
