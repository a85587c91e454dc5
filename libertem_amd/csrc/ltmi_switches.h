// Every LTMI_* environment variable the native library reads, declared once: the only getenv of csrc/ is in this file.
// Host-only (nothing from HIP).  The table of INTEGRATION.md ("Environment switches", native library) repeats this
// list name for name and class for class; tests/test_switch_table_cpu.py compares the two.
//
//   X(name, read, class, meaning)
//     read   once   at the first query of the process, the value then stays whatever the environment does
//            every  at every query: the place in the code decides what that means (per launch, per call, when a handle
//                   or plan is created) and the meaning says so
//     class  behaviour    a supported choice of route or policy; results stay right
//            measurement  exists for benchmarks and profiles; results stay right but for what the meaning names
//            garbage      timing-only ablation: results are WRONG by design
// How a site parses the text (set at all, first character, atoi, atof) is the site's business and part of the meaning.
#pragma once
#include <stdlib.h>
#include <string.h>

#define LTMI_SWITCHES(X)                                                                                               \
    X(LTMI_ABORT_BACKTRACE, once, behaviour, "1: native call stack on SIGABRT (read when the library is loaded)")      \
    X(LTMI_ALIGNED_DMA_ONLY, once, behaviour, "set: vector / LDS-DMA kernels only for tiles with 16-byte aligned rows") \
    X(LTMI_BAND_DEBUG, every, behaviour, "set: stderr says why a CSR stack got no banded image")                       \
    X(LTMI_BELL_ABLATE, every, garbage, "per launch; 1: blocked-ELL kernels without frame DMA, 2: without records")    \
    X(LTMI_BELL_F16, every, behaviour, "per blocked image built; 0: no float16 image, float32 instruction for integer pixels") \
    X(LTMI_BELL_MAX_RATIO, every, behaviour, "per CSR handle created; padding factor up to which the blocked image is built (atof, default 8)") \
    X(LTMI_BELL_NATURAL_CHUNKS, every, measurement, "per blocked image built; set: chunks in natural order, no planning") \
    X(LTMI_BELL_TILES, once, measurement, "frame tiles per wave of the blocked-ELL kernels (atoi), not the modelled choice") \
    X(LTMI_COPY_SPREAD, once, behaviour, "0: threads of ltmi_host_copy not bound to one L3 domain each")               \
    X(LTMI_CRYST_ABLATE, once, garbage, "1..5: k_cryst_fused with stages left out (uint16 frames, 16 waves)")          \
    X(LTMI_CRYST_CORR_PASS, every, measurement, "per call; set: corrected frames through the conversion pass, not inside the row stage") \
    X(LTMI_CRYST_PASS_MIB, once, measurement, "MiB of frames per pass of the two-pass crystallinity kernels (atol)")   \
    X(LTMI_CRYST_WAVES, once, measurement, "8: k_cryst_fused with 8 waves per workgroup, not 16")                      \
    X(LTMI_DENSE_F16, every, behaviour, "per dense handle created; 0: no float16 images, float32 instruction for integer pixels") \
    X(LTMI_DENSE_F32_INSTR, every, behaviour, "per launch; 1: float32 matrix instruction also where exact float16 products apply") \
    X(LTMI_DENSE_FOLD, every, behaviour, "per ltmi_masks_set_sig_shape; 0: never fold a stack about a row mirror, 2: also single-group stacks") \
    X(LTMI_FFT_FUSED, every, behaviour, "per Fourier plan created; 0: 256 x 256 frames through hipFFT, not k_cryst_fused") \
    X(LTMI_FOLD_TURN, once, measurement, "0 / 1: parts of a pixel split of k_dense_fold contiguous / in turn")         \
    X(LTMI_FOLD_WAVES, every, measurement, "per launch; 8: k_dense_fold8 (two waves per SIMD), any other number: never") \
    X(LTMI_KSPLIT_FUSED, once, measurement, "set: the last workgroup reduces the partials of a pixel split in the kernel") \
    X(LTMI_KSPLIT_STRIDED, once, measurement, "0: contiguous parts of a pixel split, v > 0: runs of 2^(v-1) slots in turn") \
    X(LTMI_MIB_WORDS, every, behaviour, "per ltmi_mib_decode call; set: the per-word kernel k_mib_decode for every shape") \
    X(LTMI_NONFINITE_GUARD, once, measurement, "0: no detect-and-redo on sparse / banded stacks: frames with non-finite pixels get the fast kernels' own NaN patterns, finite frames are unchanged") \
    X(LTMI_RCCL_LIB, every, behaviour, "per load attempt; librccl to open when the process has none mapped")           \
    X(LTMI_SCATTER_ABLATE, every, garbage, "per launch; 1..7: k_scatter<uint16> with stages left out")                 \
    X(LTMI_SCATTER_NATURAL, once, measurement, "set: chunks of the scatter image in natural order, no mixing")         \
    X(LTMI_SCATTER_SEG, once, measurement, "bytes of adjacent row segments that a chunk of the scatter image keeps together (atoi)") \
    X(LTMI_SELL_ABLATE, every, garbage, "per launch; 1: k_sell_apply loader only, 2: gathers only")                    \
    X(LTMI_SPARSE_BAND, every, behaviour, "per CSR handle / set_sig_shape; 0: no banded image, 1: whatever the cost estimate") \
    X(LTMI_SPARSE_BELL, every, behaviour, "per CSR handle created; 0 / 1: never / always build the blocked-ELL image") \
    X(LTMI_SPARSE_LABELS, every, behaviour, "per CSR handle created; 1: label image and k_labels for partition stacks") \
    X(LTMI_SPARSE_SCATTER, every, behaviour, "per CSR handle created; 0 / 1: never / every pixel type on k_scatter")   \
    X(LTMI_SPLIT, once, behaviour, "1: float32 frames against 2 - 4 column groups on k_dense_split (bf16 x 3)")        \
    X(LTMI_SPLIT_TILES, once, measurement, "2 / 4: frame tiles per wave of k_dense_split, not the choice by frame count")

namespace ltmi {

enum class ReadWhen { once, every };
enum class SwitchClass { behaviour, measurement, garbage };
struct SwitchInfo {
    const char *name;
    ReadWhen read;
    SwitchClass cls;
    const char *meaning;
};

#define LTMI_SWITCH_ID(name, read, cls, meaning) name,
enum Switch { LTMI_SWITCHES(LTMI_SWITCH_ID) N_SWITCHES };
#undef LTMI_SWITCH_ID
#define LTMI_SWITCH_ROW(name, read, cls, meaning) {#name, ReadWhen::read, SwitchClass::cls, meaning},
constexpr SwitchInfo SWITCH_TABLE[] = {LTMI_SWITCHES(LTMI_SWITCH_ROW)};
#undef LTMI_SWITCH_ROW

// the text of a switch, nullptr if unset; a `once` switch keeps (a copy of) what its first query of the process saw
template <Switch S>
inline const char *switch_text() {
    if constexpr (SWITCH_TABLE[S].read == ReadWhen::once) {
        static const char *const first = [] {
            const char *e = getenv(SWITCH_TABLE[S].name);
            return e ? strdup(e) : (const char *)nullptr;
        }();
        return first;
    } else {
        return getenv(SWITCH_TABLE[S].name);
    }
}
template <Switch S>
inline bool switch_set() { return switch_text<S>() != nullptr; }
// atoi of the text, `unset` without one
template <Switch S>
inline int switch_int(int unset) {
    const char *e = switch_text<S>();
    return e ? atoi(e) : unset;
}
// the first character of the text is `c`
template <Switch S>
inline bool switch_is(char c) {
    const char *e = switch_text<S>();
    return e && e[0] == c;
}

}  // namespace ltmi
