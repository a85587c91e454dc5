// The tuning record of a mask handle: what ltmi_masks_set_tuning stored, and the questions the launchers ask of it.
// Host-only (nothing from HIP): tests/native/tuning_table.cpp checks every predicate against the table of
// include/ltmi.h without a GPU.
#pragma once
#include "../../include/ltmi.h"

namespace ltmi {

struct Tuning {
    int mt = 0, waves = 0;      // shape of the direct-load kernel k_dense_mfma (0: dispatched)
    int ksplit = 0;             // parts of the pixel split (0: chosen per launch)
    int variant = 0;            // enum ltmi_variant

    // the two forms of ltmi_masks_set_tuning: (0, variant code, ksplit) or (mt, waves, ksplit); LTMI_E_INVALID and
    // nothing stored for anything else
    int set(int mt_, int waves_, int ksplit_) {
        const bool dense_code = waves_ >= LTMI_VARIANT_DENSE_DEFAULT && waves_ <= LTMI_VARIANT_DENSE_UNFOLDED;
        const bool sparse_code = waves_ >= LTMI_VARIANT_SPARSE_DEFAULT && waves_ <= LTMI_VARIANT_SPARSE_NO_SCATTER;
        if (mt_ == 0 && (dense_code || sparse_code)) {
            *this = Tuning{0, 0, ksplit_, waves_};
            return LTMI_OK;
        }
        if (!(mt_ == 0 || mt_ == 1 || mt_ == 2) || !(waves_ == 0 || waves_ == 4 || waves_ == 8) || ksplit_ < 0)
            return LTMI_E_INVALID;
        *this = Tuning{mt_, waves_, ksplit_, LTMI_VARIANT_NONE};
        return LTMI_OK;
    }

    // no kernel shape forced: the LDS-DMA kernels, column blocks and row lists are open
    bool dispatched_shape() const { return mt == 0 && waves == 0; }

    // ---- dense stacks
    // timing-only ablation of k_dense_lds / k_dense_fold: 2 = no frame DMA, 1 = no matrix instruction (garbage results)
    int ablation() const {
        return variant == LTMI_VARIANT_DENSE_NO_DMA ? 2 : (variant == LTMI_VARIANT_DENSE_NO_MFMA ? 1 : 0);
    }
    // padded column groups instead of VALU columns; a wide stack as one image, not column blocks; no row-list launch
    bool padded_groups() const { return variant == LTMI_VARIANT_DENSE_PADDED_GROUPS; }
    // one 16-frame tile per wave (uint16 tiles, one column group, no row list)
    bool one_tile() const { return variant == LTMI_VARIANT_DENSE_ONE_TILE; }
    // k_dense_split: asked for by the handle / still allowed (LTMI_SPLIT=1 asks too; every other code rules it out)
    bool split_forced() const { return variant == LTMI_VARIANT_DENSE_SPLIT_BF16; }
    bool split_eligible() const { return variant == LTMI_VARIANT_NONE || variant == LTMI_VARIANT_DENSE_SPLIT_BF16; }
    // the float32 matrix instruction also where the exact float16 products apply (LTMI_DENSE_F32_INSTR=1 asks too)
    bool f32_instruction() const { return variant == LTMI_VARIANT_DENSE_F32_INSTR; }
    // not the kernels of the row-mirror image (k_dense_fold, k_dense_fold16)
    bool unfolded() const { return variant == LTMI_VARIANT_DENSE_UNFOLDED; }

    // ---- sparse stacks: the routes a code closes (k_sell_apply is what remains)
    bool no_band() const { return variant == LTMI_VARIANT_SPARSE_SELL || variant == LTMI_VARIANT_SPARSE_NO_SCATTER; }
    bool no_scatter() const { return variant == LTMI_VARIANT_SPARSE_SELL || variant == LTMI_VARIANT_SPARSE_NO_SCATTER; }
    bool no_bell() const { return variant == LTMI_VARIANT_SPARSE_SELL; }
    bool no_labels() const { return variant == LTMI_VARIANT_SPARSE_SELL || variant == LTMI_VARIANT_SPARSE_NO_SCATTER; }
};

}  // namespace ltmi
