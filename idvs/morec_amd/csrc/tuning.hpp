// tuning.hpp -- every process-wide knob of the library in one struct (plain C++: no HIP include, usable from host-only code).
// tuning.hip holds the ONE table of {key, environment variable, default, value handling} rows behind it.  The environment is
// read once, thread-safely, the first time the table is touched (by a launch or by morec_tuning_set) and supplies the defaults;
// a morec_tuning_set call wins over it from then on, whichever came first.  include/morec_hip.h lists keys and values.
#pragma once

struct Tuning {
    // kernel selection: 0 = automatic, 1 = never, 2 = wherever eligible (gemm_skinny 2: gemm_skinny only, no gemm_skinny_wide / recompute)
    int gemm8p, gemm2w, gemm_small, gemm_skinny, ce8p;
    int featfuse;              // the fused gather + projection + ID fusion of the id-two-stage tower (featfuse.hip): same values as featproj
    int featproj;              // the fused gather + first projection of the two-stage tower (featproj.hip): 0 automatic | 1 never | 2 wherever the rules allow
    // gemm8p launch parameters
    int gemm8p_tmr;            // tile height: 0 = always 256, 1 = automatic, 224 / 192 = forced where an instantiation exists
    int gemm8p_ngroup;         // tile order: -1 = automatic column groups, 0 = row-major, n = groups of n N-tiles
    int gemm8p_reserve_cus;    // 0..128 CUs left out of the persistent grid
    int gemm8p_tail_split, gemm8p_tail_bias;
    int gemm8p_mfma;           // MFMA shape of the main loop: 0 = automatic (gemm_plan), 16 = 16x16x32, 32 = 32x32x16
    int gemm8p_debug;          // ablation bits
    int gemm8p_stamps_lo, gemm8p_stamps_hi;      // device address of the cycle-stamp buffer, in halves
    int deterministic;
    int fold_defer;            // deterministic mode: morec_fold_defer_begin opens a scope (0: it does not, every fold launches in place)
    int attn_stream;           // the streaming attention kernels (attention_stream.hip): 0 = for T > 256 only, 1 = never (T > 256 is unsupported), 2 = for every T > 64
    // the two-buffer GEMMs (gemm_plan rule 6): tuning and test overrides
    int gemm_tile;             // "gemm_tile" / MOREC_GEMM_TILE: 0 = automatic, 128 / 129 / 256 / 1024 / 2128 = one two-buffer tile shape everywhere
    int gemm_epi;              // "gemm_epi" / MOREC_GEMM_EPI: 2 = automatic, 1 = per-wave epilogue (w...), 0 = block epilogue (anything else)
    // environment only
    int gemm2w_stagger;        // MOREC_GEMM2W_STAGGER: first-round stagger experiment of gemm2w, 0 = off
    int tn8p_skip;             // MOREC_TN8P_SKIP=0: never the block-skipping gemm_tn8p variant
    int attn_mfma64;           // MOREC_ATTN_MFMA64=0: the VALU kernels for 32 < T <= 64
    int attn_f32_mfma;         // MOREC_ATTN_F32_MFMA=0: the VALU kernels for fp32 attention
    int swin_wpw_min;          // MOREC_SWIN_WPW_MIN: fewest windows per workgroup of the window-attention backward (>= 1)
    int swin_bwd_wide;         // MOREC_SWIN_BWD_WIDE=0: the narrow window-attention backward
    int quiet;                 // MOREC_QUIET=1: no once-per-process notes on stderr

    unsigned long long gemm8p_stamps() const {
        return ((unsigned long long)(unsigned)gemm8p_stamps_hi << 32) | (unsigned)gemm8p_stamps_lo;
    }
};

const Tuning& tuning();

// CUs of the current device (asked once per process; 256 if the query fails), and what gemm8p's persistent grid uses of them right now:
// the count rounded down to the 8 XCDs (workgroup b and its later tiles b + k * grid stay on XCD b % 8) minus the reserved CUs, >= 8.
int device_cu_count();
int gemm8p_cu_count();
