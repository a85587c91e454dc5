// What the kernels that walk the frames of a tile share (ltmi_reduce.hip, ltmi_moments.hip,
// ltmi_framestats.hip): the stored dtype -> part type dispatch, the frame slab count, the
// element-aligned vector type and the sig-slice argument check.
#pragma once
#include "ltmi_common.h"

namespace ltmi {

// ---- stored dtype -> (part type T, parts per pixel L) -------------------------------------------
// sets of tile dtypes, one bit per LTMI_* code; an entry point accepts a union of these groups
constexpr unsigned dtype_bit(int dt) { return 1u << dt; }
constexpr unsigned DT_BOOL = dtype_bit(LTMI_BOOL);          // read as uint8
constexpr unsigned DT_INT8_32 = dtype_bit(LTMI_U8) | dtype_bit(LTMI_I8) | dtype_bit(LTMI_U16) |
                                dtype_bit(LTMI_I16) | dtype_bit(LTMI_U32) | dtype_bit(LTMI_I32);
constexpr unsigned DT_INT64 = dtype_bit(LTMI_U64) | dtype_bit(LTMI_I64);
constexpr unsigned DT_FLOAT = dtype_bit(LTMI_F32) | dtype_bit(LTMI_F64);
constexpr unsigned DT_CPLX = dtype_bit(LTMI_C64) | dtype_bit(LTMI_C128);    // two parts per pixel

static inline bool dtype_in(int dt, unsigned set) {
    return dt >= 0 && dt <= LTMI_C128 && ((set >> dt) & 1u);
}

template <typename T, int L = 1> struct Part {
    typedef T type;
    static constexpr int parts = L;
};
#define LTMI_PART_T(part) typename decltype(part)::type
#define LTMI_PART_L(part) decltype(part)::parts

// `return fn(Part<T, L>())` for the part type and parts per pixel of `tile_dtype`, e.g.
//     return dispatch_tile<SET>(tile_dtype, [&](auto part) { return run<LTMI_PART_T(part)>(...); });
// `fn` is instantiated for the dtypes of SET only (no kernels for the others); the caller tests
// dtype_in(tile_dtype, SET) first and fails with its own message, so the last line is not reached.
template <unsigned SET, typename F> int dispatch_tile(int tile_dtype, F &&fn) {
#define LTMI_TILE_CASE(DT, T, L)                                                                 \
    case DT:                                                                                     \
        if constexpr ((SET >> DT) & 1u) return fn(Part<T, L>());                                 \
        break;
    switch (tile_dtype) {
        LTMI_TILE_CASE(LTMI_BOOL, uint8_t, 1)
        LTMI_TILE_CASE(LTMI_U8, uint8_t, 1)
        LTMI_TILE_CASE(LTMI_I8, int8_t, 1)
        LTMI_TILE_CASE(LTMI_U16, uint16_t, 1)
        LTMI_TILE_CASE(LTMI_I16, int16_t, 1)
        LTMI_TILE_CASE(LTMI_U32, uint32_t, 1)
        LTMI_TILE_CASE(LTMI_I32, int32_t, 1)
        LTMI_TILE_CASE(LTMI_U64, uint64_t, 1)
        LTMI_TILE_CASE(LTMI_I64, int64_t, 1)
        LTMI_TILE_CASE(LTMI_F32, float, 1)
        LTMI_TILE_CASE(LTMI_F64, double, 1)
        LTMI_TILE_CASE(LTMI_C64, float, 2)
        LTMI_TILE_CASE(LTMI_C128, double, 2)
    }
#undef LTMI_TILE_CASE
    return LTMI_E_DTYPE;
}

// ---- frame slabs --------------------------------------------------------------------------------
// how many slabs to cut the frames of a tile into (<= 256, >= 8 frames each).  Independent of the
// tile dtype so that a workspace query and the launch always agree.
static inline int frames_split(int64_t n_frames, int64_t n_px) {
    const int64_t px_blocks = (n_px + 2047) / 2048;
    int64_t want = (2048 + px_blocks - 1) / px_blocks;      // aim at >= 2048 workgroups
    want = std::max<int64_t>(1, std::min<int64_t>(want, n_frames / 8));
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, 256));
}

// ---- vector loads -------------------------------------------------------------------------------
// VEC elements of T aligned like ONE element: rows of odd length start at any element boundary; the
// target has unaligned access enabled, so a 16-byte load stays one global_load_dwordx4
template <typename T, int VEC> struct TileVec {
    typedef T vec_a __attribute__((ext_vector_type(VEC)));
    typedef vec_a type __attribute__((aligned(sizeof(T))));
};
template <typename T, int VEC> using tile_vec_t = typename TileVec<T, VEC>::type;

// ---- sig slices ---------------------------------------------------------------------------------
// a tile's sig slice is rows of `cols` pixels that lie at stride `ld_out` in the full-frame buffer: pixel p
// of the slice is element (p / cols) * ld_out + p % cols.  (The two merge kernels spell that out: as a
// function of its own the compiler reassociates it, and ltmi_moments_frames measured 5 - 7 % slower.)
static inline int check_sig_slice(const char *entry, int64_t n_px, int64_t cols, int64_t ld_out) {
    if (n_px > 0 && (cols <= 0 || n_px % cols != 0 || ld_out < cols))
        LTMI_FAIL(LTMI_E_SHAPE, "%s: cols %lld / ld_out %lld do not fit %lld pixels", entry,
                  (long long)cols, (long long)ld_out, (long long)n_px);
    return LTMI_OK;
}

}  // namespace ltmi
