// tuning.hip -- the knob table: morec_tuning_set, the one read of the MOREC_* environment, the deterministic-mode switch and the
// CU count.  No kernel lives here.  No reference counterpart (the reference has no kernels to select: SURVEY.md section 2).
#include <stdlib.h>
#include <string.h>
#include "common.hpp"

namespace {
enum Handling {
    RAW,         // the integer as given
    FLAG,        // value != 0
    TMR,         // 0 | 1 | 224 | 192, anything else = 1
    RESERVE,     // 0..128
    TAIL_BIAS,   // 0..16
    MFMA,        // 0 | 16 | 32; morec_tuning_set refuses anything else, the environment falls back to 0
    AT_LEAST_1,
    TILE,        // 0 | 128 | 129 | 256 | 1024 | 2128; morec_tuning_set refuses anything else, the environment passes its integer on as given
    EPI,         // morec_tuning_set: 0 | 1 | 2, anything else refused; environment: 'w...' = 1, anything else = 0
    // environment-only spellings
    NOT_CHAR_0,  // 0 if the variable starts with '0', else 1
    IS_CHAR_1,   // 1 if the variable starts with '1', else 0
};
struct Row {
    const char* key;      // morec_tuning_set key, or null: environment only
    const char* env;      // environment variable that supplies the default, or null: morec_tuning_set only
    int Tuning::*field;
    int def;
    Handling how;
};
// One row per knob.  include/morec_hip.h documents them in this order.
const Row ROWS[] = {
    {"gemm8p", "MOREC_GEMM8P", &Tuning::gemm8p, 0, RAW},
    {"gemm2w", "MOREC_GEMM2W", &Tuning::gemm2w, 0, RAW},
    {"gemm_small", "MOREC_GEMM_SMALL", &Tuning::gemm_small, 0, RAW},
    {"gemm_skinny", "MOREC_GEMM_SKINNY", &Tuning::gemm_skinny, 0, RAW},
    {"ce8p", "MOREC_CE8P", &Tuning::ce8p, 0, RAW},
    {"featproj", "MOREC_FEATPROJ", &Tuning::featproj, 0, RAW},
    {"featfuse", "MOREC_FEATFUSE", &Tuning::featfuse, 0, RAW},
    {"gemm8p_tmr", "MOREC_GEMM8P_TMR", &Tuning::gemm8p_tmr, 1, TMR},
    {"gemm8p_ngroup", "MOREC_GEMM8P_NGROUP", &Tuning::gemm8p_ngroup, -1, RAW},
    {"gemm8p_reserve_cus", "MOREC_GEMM8P_RESERVE_CUS", &Tuning::gemm8p_reserve_cus, 0, RESERVE},
    {"gemm8p_tail_split", "MOREC_GEMM8P_TAIL_SPLIT", &Tuning::gemm8p_tail_split, 0, FLAG},
    {"gemm8p_tail_bias", nullptr, &Tuning::gemm8p_tail_bias, 2, TAIL_BIAS},
    {"gemm8p_mfma", "MOREC_GEMM8P_MFMA", &Tuning::gemm8p_mfma, 0, MFMA},
    {"gemm8p_debug", "MOREC_GEMM8P_DEBUG", &Tuning::gemm8p_debug, 0, RAW},
    {"gemm8p_stamps_lo", nullptr, &Tuning::gemm8p_stamps_lo, 0, RAW},
    {"gemm8p_stamps_hi", nullptr, &Tuning::gemm8p_stamps_hi, 0, RAW},
    {"deterministic", "MOREC_DETERMINISTIC", &Tuning::deterministic, 0, FLAG},
    {"fold_defer", "MOREC_FOLD_DEFER", &Tuning::fold_defer, 1, FLAG},
    {"attn_stream", "MOREC_ATTN_STREAM", &Tuning::attn_stream, 0, RAW},
    {"gemm_tile", "MOREC_GEMM_TILE", &Tuning::gemm_tile, 0, TILE},
    {"gemm_epi", "MOREC_GEMM_EPI", &Tuning::gemm_epi, 2, EPI},
    {nullptr, "MOREC_GEMM2W_STAGGER", &Tuning::gemm2w_stagger, 0, RAW},
    {nullptr, "MOREC_TN8P_SKIP", &Tuning::tn8p_skip, 1, FLAG},
    {nullptr, "MOREC_ATTN_MFMA64", &Tuning::attn_mfma64, 1, NOT_CHAR_0},
    {nullptr, "MOREC_ATTN_F32_MFMA", &Tuning::attn_f32_mfma, 1, NOT_CHAR_0},
    {nullptr, "MOREC_SWIN_WPW_MIN", &Tuning::swin_wpw_min, 8, AT_LEAST_1},
    {nullptr, "MOREC_SWIN_BWD_WIDE", &Tuning::swin_bwd_wide, 1, RAW},
    {nullptr, "MOREC_QUIET", &Tuning::quiet, 0, IS_CHAR_1},
};

int handled(Handling how, int v) {
    switch (how) {
        case FLAG: return v != 0;
        case TMR: return (v == 0 || v == 1 || v == 224 || v == 192) ? v : 1;
        case RESERVE: return v < 0 ? 0 : v > 128 ? 128 : v;
        case TAIL_BIAS: return v < 0 ? 0 : v > 16 ? 16 : v;
        case MFMA: return (v == 16 || v == 32) ? v : 0;
        case AT_LEAST_1: return v < 1 ? 1 : v;
        default: return v;
    }
}

// morec_tuning_set: the kinds that refuse a value instead of mapping it (everything else goes through handled())
bool accepted(Handling how, int v) {
    switch (how) {
        case MFMA: return v == 0 || v == 16 || v == 32;
        case TILE: return v == 0 || v == 128 || v == 129 || v == 256 || v == 1024 || v == 2128;
        case EPI: return v >= 0 && v <= 2;
        default: return true;
    }
}

Tuning& table() {
    static Tuning t = [] {      // function-local static: the environment is read once, by whichever thread comes first
        Tuning x{};
        for (const Row& r : ROWS) {
            const char* e = r.env ? getenv(r.env) : nullptr;
            x.*r.field = !e                    ? r.def
                         : r.how == NOT_CHAR_0 ? e[0] != '0'
                         : r.how == IS_CHAR_1  ? e[0] == '1'
                         : r.how == EPI        ? e[0] == 'w'
                                               : handled(r.how, atoi(e));
        }
        return x;
    }();
    return t;
}
}  // namespace

const Tuning& tuning() { return table(); }

extern "C" int morec_tuning_set(const char* key, int value) {
    if (!key) return MOREC_E_ARG;
    for (const Row& r : ROWS)
        if (r.key && !strcmp(key, r.key)) {
            if (!accepted(r.how, value)) return MOREC_E_UNSUPPORTED;
            table().*r.field = handled(r.how, value);
            return MOREC_OK;
        }
    return MOREC_E_UNSUPPORTED;
}

// ---- deterministic mode (common.hpp) ----------------------------------------------------------------------------------------------
bool morec_deterministic() { return tuning().deterministic != 0; }
void morec_set_deterministic(int on) { table().deterministic = on ? 1 : 0; }

int device_cu_count() {
    static const int n = [] {
        int dev = 0, c = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
        return c;
    }();
    return n;
}

int gemm8p_cu_count() {
    const int n_dev = device_cu_count() & ~7;
    const int n = (n_dev < 8 ? 8 : n_dev) - (tuning().gemm8p_reserve_cus & ~7);
    return n < 8 ? 8 : n;
}
