// Host-only check of csrc/ltmi_tuning.h and csrc/ltmi_switches.h (tests/test_switch_table_cpu.py builds this with
// -fsanitize=address,undefined and runs it).  The tables below are written out by hand from the prototype comment of
// ltmi_masks_set_tuning: they do not use the header's own predicates or constants to say what is right.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/ltmi.h"
#include "../../libertem_amd/csrc/ltmi_switches.h"
#include "../../libertem_amd/csrc/ltmi_tuning.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__); \
            fputc('\n', stderr);          \
        }                                 \
    } while (0)

struct Row {
    int variant, ablation;
    bool padded, one_tile, split_forced, split_eligible, f32_instr, unfolded, no_band, no_scatter, no_bell, no_labels;
};
static const Row ROWS[] = {
    //  code abl  padded one    forced elig.  f32    unfold band   scat   bell   labels
    {0,  0, false, false, false, true,  false, false, false, false, false, false},
    {30, 0, false, false, false, false, false, false, false, false, false, false},
    {31, 2, false, false, false, false, false, false, false, false, false, false},
    {32, 1, false, false, false, false, false, false, false, false, false, false},
    {33, 0, true,  false, false, false, false, false, false, false, false, false},
    {34, 0, false, true,  false, false, false, false, false, false, false, false},
    {35, 0, false, false, false, false, false, false, false, false, false, false},
    {36, 0, false, false, true,  true,  false, false, false, false, false, false},
    {37, 0, false, false, false, false, true,  false, false, false, false, false},
    {38, 0, false, false, false, false, false, true,  false, false, false, false},
    {40, 0, false, false, false, false, false, false, false, false, false, false},
    {41, 0, false, false, false, false, false, false, true,  true,  true,  true},
    {42, 0, false, false, false, false, false, false, true,  true,  false, true},
};

static const Row *row_of(int variant) {
    for (const Row &r : ROWS)
        if (r.variant == variant) return &r;
    return nullptr;
}

static void check_predicates(const ltmi::Tuning &t, int mt, int waves, int ksplit) {
    const Row *r = row_of(t.variant);
    CHECK(r != nullptr, "variant %d after set(%d, %d, %d)", t.variant, mt, waves, ksplit);
    if (!r) return;
#define SAME(pred, field) CHECK(t.pred() == r->field, "variant %d: " #pred, t.variant)
    SAME(ablation, ablation);
    SAME(padded_groups, padded);
    SAME(one_tile, one_tile);
    SAME(split_forced, split_forced);
    SAME(split_eligible, split_eligible);
    SAME(f32_instruction, f32_instr);
    SAME(unfolded, unfolded);
    SAME(no_band, no_band);
    SAME(no_scatter, no_scatter);
    SAME(no_bell, no_bell);
    SAME(no_labels, no_labels);
#undef SAME
    CHECK(t.dispatched_shape() == (mt == 0 && (waves == 0 || waves >= 30)), "set(%d, %d, %d)", mt, waves, ksplit);
}

static void check_tuning() {
    CHECK(LTMI_VARIANT_NONE == 0 && LTMI_VARIANT_DENSE_DEFAULT == 30 && LTMI_VARIANT_DENSE_NO_DMA == 31 &&
          LTMI_VARIANT_DENSE_NO_MFMA == 32 && LTMI_VARIANT_DENSE_PADDED_GROUPS == 33 &&
          LTMI_VARIANT_DENSE_ONE_TILE == 34 && LTMI_VARIANT_DENSE_TWO_TILES == 35 &&
          LTMI_VARIANT_DENSE_SPLIT_BF16 == 36 && LTMI_VARIANT_DENSE_F32_INSTR == 37 &&
          LTMI_VARIANT_DENSE_UNFOLDED == 38 && LTMI_VARIANT_SPARSE_DEFAULT == 40 && LTMI_VARIANT_SPARSE_SELL == 41 &&
          LTMI_VARIANT_SPARSE_NO_SCATTER == 42, "enum ltmi_variant was renumbered");
    const int ksplits[] = {-1, 0, 1, 7};
    int accepted = 0;
    for (int mt = -1; mt <= 3; ++mt)
        for (int waves = -1; waves <= 50; ++waves)
            for (int ksplit : ksplits) {
                const bool code = mt == 0 && ((waves >= 30 && waves <= 38) || (waves >= 40 && waves <= 42));
                const bool shape = mt >= 0 && mt <= 2 && (waves == 0 || waves == 4 || waves == 8) && ksplit >= 0;
                ltmi::Tuning t;
                CHECK(t.set(0, 36, 5) == LTMI_OK, "set(0, 36, 5)");           // something to keep or to replace
                const int rc = t.set(mt, waves, ksplit);
                CHECK(rc == ((code || shape) ? LTMI_OK : LTMI_E_INVALID), "set(%d, %d, %d) -> %d", mt, waves, ksplit, rc);
                if (rc != LTMI_OK) {                                        // a rejected triple stores nothing
                    CHECK(t.mt == 0 && t.waves == 0 && t.ksplit == 5 && t.variant == 36, "set(%d, %d, %d) stored",
                          mt, waves, ksplit);
                    continue;
                }
                ++accepted;
                CHECK(t.ksplit == ksplit, "set(%d, %d, %d): ksplit %d", mt, waves, ksplit, t.ksplit);
                if (code)
                    CHECK(t.mt == 0 && t.waves == 0 && t.variant == waves, "set(%d, %d, %d): (%d, %d, %d)", mt, waves,
                          ksplit, t.mt, t.waves, t.variant);
                else
                    CHECK(t.mt == mt && t.waves == waves && t.variant == 0, "set(%d, %d, %d): (%d, %d, %d)", mt, waves,
                          ksplit, t.mt, t.waves, t.variant);
                check_predicates(t, mt, waves, ksplit);
            }
    // 12 codes with any of the 4 splits (a code does not look at ksplit) + 3 x 3 shapes with the 3 splits >= 0
    CHECK(accepted == 12 * 4 + 9 * 3, "%d triples accepted", accepted);
    const ltmi::Tuning fresh;
    CHECK(fresh.mt == 0 && fresh.waves == 0 && fresh.ksplit == 0 && fresh.variant == 0, "a fresh record is (0, 0, 0, 0)");
}

// an `every` switch follows the environment, a `once` switch keeps what its first query saw
template <ltmi::Switch S>
static void check_switch() {
    const ltmi::SwitchInfo &info = ltmi::SWITCH_TABLE[S];
    const bool once = info.read == ltmi::ReadWhen::once;
    CHECK(strncmp(info.name, "LTMI_", 5) == 0 && info.meaning[0], "row %d", (int)S);
    setenv(info.name, "17", 1);
    const char *a = ltmi::switch_text<S>();
    CHECK(a && strcmp(a, "17") == 0, "%s: first query", info.name);
    CHECK(ltmi::switch_set<S>() && ltmi::switch_int<S>(-1) == 17 && ltmi::switch_is<S>('1') && !ltmi::switch_is<S>('0'),
          "%s: parsers", info.name);
    setenv(info.name, "0", 1);
    const char *b = ltmi::switch_text<S>();
    CHECK(b && strcmp(b, once ? "17" : "0") == 0, "%s after a change: %s", info.name, b ? b : "(null)");
    unsetenv(info.name);
    const char *c = ltmi::switch_text<S>();
    if (once)
        CHECK(c && strcmp(c, "17") == 0 && ltmi::switch_int<S>(-1) == 17, "%s after unsetenv", info.name);
    else
        CHECK(c == nullptr && !ltmi::switch_set<S>() && ltmi::switch_int<S>(-1) == -1 && !ltmi::switch_is<S>('1'),
              "%s after unsetenv", info.name);
}

// a `once` switch that is unset at its first query stays unset
static void check_once_unset() {
    unsetenv("LTMI_SPLIT_TILES");
    CHECK(ltmi::SWITCH_TABLE[ltmi::LTMI_SPLIT_TILES].read == ltmi::ReadWhen::once, "LTMI_SPLIT_TILES is read once");
    CHECK(ltmi::switch_text<ltmi::LTMI_SPLIT_TILES>() == nullptr, "unset at the first query");
    setenv("LTMI_SPLIT_TILES", "4", 1);
    CHECK(ltmi::switch_text<ltmi::LTMI_SPLIT_TILES>() == nullptr && ltmi::switch_int<ltmi::LTMI_SPLIT_TILES>(0) == 0,
          "set after the first query");
    unsetenv("LTMI_SPLIT_TILES");
}

int main() {
    check_tuning();
    check_once_unset();                     // (before check_switch gives the switch a first value)
    int n_once = 0, n_every = 0;
#define LTMI_CHECK_SWITCH(name, read, cls, meaning)                        \
    if (ltmi::name != ltmi::LTMI_SPLIT_TILES) check_switch<ltmi::name>();  \
    (ltmi::ReadWhen::read == ltmi::ReadWhen::once ? n_once : n_every) += 1;
    LTMI_SWITCHES(LTMI_CHECK_SWITCH)
#undef LTMI_CHECK_SWITCH
    CHECK(n_once + n_every == (int)ltmi::N_SWITCHES && n_once > 0 && n_every > 0, "%d once + %d every", n_once, n_every);
    // what the library relies on: read per launch / per call
    CHECK(ltmi::SWITCH_TABLE[ltmi::LTMI_DENSE_F32_INSTR].read == ltmi::ReadWhen::every, "LTMI_DENSE_F32_INSTR");
    CHECK(ltmi::SWITCH_TABLE[ltmi::LTMI_MIB_WORDS].read == ltmi::ReadWhen::every, "LTMI_MIB_WORDS");
    CHECK(ltmi::SWITCH_TABLE[ltmi::LTMI_FFT_FUSED].read == ltmi::ReadWhen::every, "LTMI_FFT_FUSED");
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("tuning_table: ok (%d switches: %d once, %d every)\n", (int)ltmi::N_SWITCHES, n_once, n_every);
    return 0;
}
