// gemm_plan.hpp -- which kernel runs an NT GEMM, and with which host-chosen parameters: ONE function, plain C++17 (no HIP include, no
// device call, no allocation), so that a selection can be asked and tested without a GPU (morec_gemm_plan, tests/test_gemm_plan_cpu.py).
// morec_gemm_nt_colsum validates, fills GemmArgs, calls gemm_plan() and switches over the family; the kernel files only launch.
// The rules are tried in this order and the first that holds wins: skinny, skinny_wide, two_w, eight_p, small, generic.
#pragma once
#include <initializer_list>
#include "morec_hip.h"
#include "tuning.hpp"

enum GemmFamily {           // the ids of include/morec_hip.h (morec_gemm_plan_info.family)
    GEMM_UNSUPPORTED = MOREC_GEMM_UNSUPPORTED,      // GemmPlan::error says why
    GEMM_SKINNY = MOREC_GEMM_SKINNY,                // gemm_skinny.hip: streaming kernel, narrow outputs over very many rows
    GEMM_SKINNY_WIDE = MOREC_GEMM_SKINNY_WIDE,      // gemm_skinny_wide.hip: the same for GELU(product + bias), 288 < N <= 768
    GEMM_TWO_W = MOREC_GEMM_TWO_W,                  // gemm2w.hip: 256 x 128 tiles, two workgroups per CU
    GEMM_EIGHT_P = MOREC_GEMM_EIGHT_P,              // gemm8p.hip: 256 (224, 192) x 256 tiles, eight-phase main loop, persistent grid
    GEMM_SMALL = MOREC_GEMM_SMALL,                  // gemm_small.hip: 64 x 64 tiles on a four-stage ring
    GEMM_GENERIC = MOREC_GEMM_GENERIC,              // gemm_nt_generic.hpp: the two-buffer kernels (bf16 / fp32: gemm.hip, fp16: gemm_f16.hip)
};
// tile shapes of the two-buffer kernels (gemm_core.hpp GemmTileCfg)
enum GemmGenericTile {
    GEMM_TILE_128_W8,       // 128 x 128, 8 waves of 64 x 32
    GEMM_TILE_256_W16,      // 256 x 256, 16 waves of 64 x 64
    GEMM_TILE_128_W4,       // 128 x 128, 4 waves            (MOREC_GEMM_TILE=128)
    GEMM_TILE_256_W8,       // 256 x 256, 8 waves of 128 x 64 (MOREC_GEMM_TILE=256)
    GEMM_TILE_256x128,      // 256 x 128, 8 waves, two workgroups per CU (MOREC_GEMM_TILE=2128)
};

namespace gplan {
// the tile constants the rules need; the kernel files static_assert their own against these
constexpr int P8_TM = 256, P8_TN = 256, P8_KE = 64;      // gemm8p
constexpr int W2_TM = 256, W2_TN = 128, W2_KE = 64;      // gemm2w
constexpr int SK_TR = 32;                                // gemm_skinny / gemm_skinny_wide: rows per streamed tile
constexpr int SMALL_T = 64;                              // gemm_small
inline bool is16(int dtype) { return dtype == MOREC_BF16 || dtype == MOREC_F16; }
}  // namespace gplan

// The operand facts the rules use (everything else is in the descriptor).
struct GemmOperands {
    bool bias, aux_out, dact_in, colsum;
    bool vec_store;         // output rows (and aux_out) are 16-byte addressable: the LDS-staged epilogues
    bool bias_aligned16;
};

struct GemmPlan {
    int family;             // GemmFamily
    int error;              // GEMM_UNSUPPORTED: the MOREC_E_* code morec_gemm_nt returns
    int in_dtype, out_dtype;
    int mode;               // epilogue: 0 plain (+ bias), 1 GELU, 2 ReLU, 3 x GELU'(dact_in), 4 x ReLU'(dact_in), 5 x dact_in
    int colsum;             // column sums of C fused into the epilogue
    int tile_rows, tile_cols;
    int ngroup;             // eight_p, two_w: N-tiles per column group of the tile order (0: row-major)
    int tail_split;         // eight_p: the tail round is split along K (needs its workspace)
    int n_cu;               // eight_p: workgroups of the persistent grid (the n_cu the plan was made for)
    int mfma;               // eight_p: MFMA shape of the main loop, 16 (16x16x32) or 32 (32x32x16).  Internal: not in morec_gemm_plan_info
    int nbh, ksteps;        // skinny: 16-column blocks per wave half, 32-element k-steps
    int generic_tile;       // generic: GemmGenericTile
    int split_k;            // generic
    int wave_epilogue;      // generic, small: per-wave LDS slices instead of workgroup barriers in the epilogue
};

// act / dact of a descriptor -> epilogue mode (the ACT template argument of every tile kernel)
inline int gemm_epilogue_mode(int act, int dact) {
    return dact == MOREC_ACT_GELU ? 3 : dact == MOREC_ACT_RELU ? 4 : dact == MOREC_DACT_MUL ? 5
           : act == MOREC_ACT_GELU ? 1 : act == MOREC_ACT_RELU ? 2 : 0;
}

// ---- gemm8p tile height.  A launch is ceil(tiles / CUs) ROUNDS of tiles; with 256-row tiles the encoder's N = 768 products at ~55 k token rows
// are 645 tiles = 2.52 rounds, i.e. THREE rounds of tile time for 2.52 rounds of work (16 % of the launch is idle CUs), N = 3072 is 10.08
// rounds -> eleven.  The number of rounds is an integer either way, but the tile's height need not be 256: with 224-row tiles (wave row 1
// owns three 32-row blocks instead of four; its fourth block's MFMAs are branched around, everything else -- barriers, DMA, LDS image --
// is the 256-row schedule) the same N = 768 product is 738 tiles = 2.88 rounds of 7/8-size tiles: three rounds x 0.875.  pick_tmr takes
// the height in {256, 224, 192} with the smallest rounds x (K-tiles x height / 256 + fixed per-tile cost in K-tile units), 256 on ties.
// The result is the same numbers bit for bit (a tile boundary does not enter any sum).  MOREC_GEMM8P_TMR=0 / tuning key "gemm8p_tmr" 0: off.
inline int pick_tmr(int tmr_mode, int M, int tiles_n, int nk, int n_cu) {
    using namespace gplan;
    if (tmr_mode == 0) return P8_TM;
    if (tmr_mode == 224 || tmr_mode == 192) return tmr_mode;
    const double fixed = 4.0;      // prologue + first barrier + epilogue of a tile, in K-tile times (profiles/r03_gemm8p_stamps.txt: ~8.4 k of 2.25 k cycles)
    int best = P8_TM;
    double best_cost = 0.0;
    for (int t : {256, 224, 192}) {
        const long tiles = (long)((M + t - 1) / t) * tiles_n;
        if (tiles <= n_cu && t != P8_TM) continue;                                        // a single round: nothing to balance
        const double cost = (double)((tiles + n_cu - 1) / n_cu) * ((double)nk * t / 256.0 + fixed);
        if (t == P8_TM || cost < best_cost * 0.985) { if (t == P8_TM || cost < best_cost) { best = t; best_cost = cost; } }
    }
    return best;
}

// n_cu: the CUs gemm8p's persistent grid may use (gemm8p_cu_count(): the device's, rounded to the 8 XCDs, minus the reserved ones).
inline GemmPlan gemm_plan(const morec_gemm_desc& d, const GemmOperands& o, const Tuning& t, int n_cu) {
    using namespace gplan;
    GemmPlan p{};
    p.in_dtype = d.in_dtype;
    p.out_dtype = d.out_dtype;
    p.mode = gemm_epilogue_mode(d.act, d.dact);
    p.colsum = o.colsum;
    p.split_k = d.split_k < 1 ? 1 : d.split_k;
    // epilogue form of the two-buffer kernels: per-wave LDS slices without workgroup barriers pay off where the epilogue is heavy (GELU + the
    // second output) or the tile row is short (N <= 1024); measured per shape with scripts/gemm_bench.py.  MOREC_GEMM_EPI=w|b forces one.
    p.wave_epilogue = t.gemm_epi == 2 ? ((o.aux_out || d.N <= 1024) ? 1 : 0) : t.gemm_epi;
    const bool same16 = is16(d.in_dtype) && d.out_dtype == d.in_dtype;
    // what every tile kernel but the two-buffer ones needs: plain stores of LDS-staged 16-bit-operand tiles
    const bool staged16 = is16(d.in_dtype) && d.accumulate == 0 && o.vec_store && d.split_k <= 1;
    const bool streaming = !o.aux_out && !o.dact_in && !o.colsum && d.dact == MOREC_ACT_NONE && d.accumulate == 0 && d.split_k <= 1 &&
                           d.alpha == 1.0f && !(o.bias && (d.N % 4 || !o.bias_aligned16)) && d.lda % 8 == 0 && d.ldb % 8 == 0 && d.ldc % 8 == 0 &&
                           d.N % 8 == 0 && d.K % 8 == 0 && d.M >= 8192 && (long)SK_TR * d.lda * 2 < 0x7fffffffL;

    // 1. skinny -- narrow outputs over very many rows (Swin stage 1 / 2): plain products and products with a bias (no activation /
    //    accumulation / second output), 64 <= N <= 128 with K <= 384, or N <= 288 with K <= 96 (the stage-1 q|k|v projection: 9 column
    //    blocks x 3 k-steps of B = 108 registers)
    if (t.gemm_skinny != 1 && same16 && streaming && d.act == MOREC_ACT_NONE && d.N <= 288 && d.N >= 64 && d.K <= 384 && !(d.N > 128 && d.K > 96)) {
        p.family = GEMM_SKINNY;
        p.nbh = d.N <= 96 ? 3 : (d.N <= 128 ? 4 : 9);
        p.ksteps = (d.K + 31) / 32;
        p.tile_rows = SK_TR;
        p.tile_cols = 32 * p.nbh;
        return p;
    }
    // 2. skinny_wide -- 288 < N <= 768, 32 <= K <= 192, only GELU(product + bias) without a second output (stage-1 / stage-2 fc1): a plain /
    //    bias-only product of these widths is faster on the tile kernel (measured: Swin-B stage-1 q|k|v 306 vs 334 us); what the streaming
    //    form buys is the epilogue-heavy, write-heavy launch
    if (t.gemm_skinny != 1 && t.gemm_skinny != 2 && same16 && streaming && d.act == MOREC_ACT_GELU && d.N > 288 && d.N <= 768 && d.K <= 192 &&
        d.K >= 32 && (long)SK_TR * d.ldc * 2 < 0x7fffffffL) {
        p.family = GEMM_SKINNY_WIDE;
        p.tile_rows = SK_TR;
        p.tile_cols = d.N;      // a streamed tile is 32 whole rows
        return p;
    }
    // 3. two_w -- epilogue-heavy 16-bit products: 256 x 128 tiles, two workgroups per CU.  Epilogues: plain / bias, GELU (+ second output),
    //    x dact_in (+ column sums)
    if (t.gemm2w != 1 && same16 && staged16 && d.K % W2_KE == 0 && d.K >= W2_KE && d.N % 8 == 0 && d.M >= 1 &&
        (d.dact == MOREC_ACT_NONE || d.dact == MOREC_DACT_MUL) && !(d.dact == MOREC_DACT_MUL && o.bias) && d.act != MOREC_ACT_RELU &&
        !(o.aux_out && d.act != MOREC_ACT_GELU) && !(o.colsum && (d.dact != MOREC_DACT_MUL || d.M < 128))) {
        const int tiles_m = (d.M + W2_TM - 1) / W2_TM, tiles_n = (d.N + W2_TN - 1) / W2_TN;
        // Automatic: where this kernel measured FASTER than gemm8p on random operands (profiles/r06_gemm2w_shapes.txt).  Both kernels hold the part's
        // power limit on random fp16 data (same binary on zero operands: gemm2w 1.43 PFLOP/s, gemm8p 1.18 at N = 3072, K = 768, against 0.93 / 0.96
        // on N(0, 0.5) operands: profiles/r06_gemm_power_probe.txt), so what is left to win is work, not schedule:
        //  (a) plain products whose N fills 256-wide tiles badly (N = 384: three 128-wide tiles instead of two 256-wide ones, a quarter of whose
        //      MFMAs, LDS and DMA traffic are padding): Swin-T stage 3, 1.11 - 1.30 x;
        //  (b) x act' + column sums over fewer rows (Swin-T stage 4, Swin-B stage 3): 1.04 - 1.07 x.
        // (`narrow` also holds for N = 128, 192, 320, 576, which nobody measured: ADVICE.md.  Recorded by tests/test_gemm_plan_cpu.py.)
        const long waste = (long)((d.N + 255) / 256) * 256 - d.N;
        const bool narrow = p.mode == 0 && !o.colsum && waste * 4 >= d.N && d.M >= 8192 && d.K <= 2048;
        const bool dmul = p.mode == 5 && d.M >= 16384 && ((d.M <= 40000 && d.K <= 768) || (d.M <= 70000 && d.K <= 512));
        if ((long)tiles_m * tiles_n >= 64 && (t.gemm2w == 2 || narrow || dmul)) {
            p.family = GEMM_TWO_W;
            p.tile_rows = W2_TM;
            p.tile_cols = W2_TN;
            p.ngroup = tiles_n <= 8 ? 0 : 8;
            return p;
        }
    }
    // 4. eight_p -- 16-bit, large: the 256 x 256 eight-phase kernel.  16-byte K slots; at least two K-tiles (the last may be partial); the
    //    column-sum workspace is sized per 64 rows; no bias register set in the derivative epilogues; fp32 outputs only plain
    if (t.gemm8p != 1 && staged16 && d.K % 8 == 0 && d.K > P8_KE && d.N >= 64 && d.M >= 1 && !(o.colsum && d.M < 128) &&
        !(d.dact != MOREC_ACT_NONE && o.bias) &&
        (d.out_dtype == d.in_dtype ? !(o.colsum && p.mode < 3) : (d.out_dtype == MOREC_F32 && p.mode == 0 && !o.colsum))) {
        const int tiles_n = (d.N + P8_TN - 1) / P8_TN;
        const long tiles = (long)((d.M + P8_TM - 1) / P8_TM) * tiles_n;
        // automatic: enough tiles to fill the 256 CUs, and at most a quarter of the tile columns past N (N = 192, 384, 576 of the Swin
        // stages: faster here than in the two-buffer kernel; N = 96 is not -- profiles/r02_swin_gemm_shapes_modes.txt)
        // (long-K problems already from 160 tiles: the scoring backward's dE = dl^T P, 168 tiles of 40 K-tiles each)
        if (t.gemm8p == 2 || !(tiles < (d.K >= 2048 ? 160 : 192) || tiles_n * P8_TN * 100L > d.N * 134L)) {
            p.family = GEMM_EIGHT_P;
            p.n_cu = n_cu;
            p.tile_rows = P8_TM;
            // tile height (see pick_tmr): the 224- / 192-row instantiations exist for the three kernels of the encoder step -- plain,
            // FFN-up + GELU (+ act'), x act' + column sums -- with 16-bit outputs
            if (d.out_dtype == d.in_dtype && ((p.mode == 0 && !o.colsum) || (p.mode == 1 && !o.colsum) || (p.mode == 5 && o.colsum)))
                p.tile_rows = pick_tmr(t.gemm8p_tmr, d.M, tiles_n, (d.K + P8_KE - 1) / P8_KE, n_cu);
            p.tile_cols = P8_TN;
            // MFMA shape of the main loop.  Automatic = 16x16x32 everywhere: at the six products of the encoder step (M = 54 919; K = 768, 2304, 3072;
            // plain, GELU + act', x act' + column sums) it measured 1.033 - 1.070 x the 32x32x16 launch on fp16 and on bf16, at a run-to-run spread
            // of at most 0.9 % of a cell (profiles/mfma_shape_launches.txt) -- same tiles, LDS and HBM traffic; the chip holds a higher clock under its power limit
            // on the 16-row shape.  No dtype, mode or K measured the other way, so the rule has no condition.  "gemm8p_mfma" = 32: the former loop.
            p.mfma = t.gemm8p_mfma ? t.gemm8p_mfma : 16;
            // column groups of the tile order: automatic = groups of about 6 N-tiles (a 32-CU XCD then works on a ~5 x 6 block)
            const int ng = (tiles_n + 5) / 6;
            p.ngroup = t.gemm8p_ngroup < 0 ? (tiles_n + ng - 1) / ng : t.gemm8p_ngroup;
            // Tail split: OPT-IN (tuning key "gemm8p_tail_split" / MOREC_GEMM8P_TAIL_SPLIT=1).  It is as accurate as the unsplit sum (same
            // error against an exact product) but rounds 0.02 % of the outputs the other way, and a 12-layer bf16 encoder at random init
            // turns that into +-1e-2 on the step-0 loss (tests/test_bench_mode_parity_gpu.py); the default keeps the summation order of
            // the two-buffer kernels (bit-identical outputs) for 0.35 % of the step time.
            const long nwg = (long)((d.M + p.tile_rows - 1) / p.tile_rows) * tiles_n;
            p.tail_split = p.tile_rows == P8_TM && t.gemm8p_tail_split && nwg > n_cu && nwg % n_cu && 2 * (nwg % n_cu) <= n_cu &&
                           d.K >= 24 * P8_KE && !(t.gemm8p_debug & 128);
            return p;
        }
    }
    // 5. small -- latency-class 16-bit products (the SASRec layers): 64 x 64 tiles on a four-stage ring
    if (t.gemm_small != 1 && same16 && staged16 && d.K >= 64 && d.M >= 1) {
        // automatic: where it measured faster than the 128 x 128 kernel in isolation (scripts/small_gemm_check.py, profiles/r06_small_gemm.txt):
        // narrow outputs with a long contraction -- fewer than 128 tiles of 128 x 128 and K >= 1024 (f2 / dx1 at K = 2048: 19.7 -> 14.0 us,
        // dx0 at K = 1536: 15.6 -> 11.3, the one-GPU scoring backward's dE at K = 2560: 30 -> 21).  With N >= 1536 the wider tile's
        // half LDS-fill traffic per flop wins (qkv 9.0 vs 11.0 us, f1 + ReLU 14.7 vs 17.6); at K = 512 the two are level.
        const long t128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
        if (t.gemm_small == 2 || !(t128 > 128 || d.K < 1024 || d.N < 256 || o.aux_out || o.colsum)) {
            if (o.colsum && p.mode < 3) { p.error = MOREC_E_UNSUPPORTED; return p; }
            p.family = GEMM_SMALL;
            p.tile_rows = p.tile_cols = SMALL_T;
            p.wave_epilogue = 1;      // the 64-wide tile row: per-wave LDS slices, no workgroup barriers in the epilogue
            return p;
        }
    }
    // 6. generic -- the two-buffer kernels, every dtype pair and every epilogue, split-K, accumulation
    if (!((d.in_dtype == MOREC_F32 && d.out_dtype == MOREC_F32) || (is16(d.in_dtype) && (d.out_dtype == d.in_dtype || d.out_dtype == MOREC_F32)))) {
        p.error = MOREC_E_DTYPE;
        return p;
    }
    if (o.colsum && p.mode < 3) { p.error = MOREC_E_UNSUPPORTED; return p; }      // fused bias gradient: only behind the activation-derivative epilogues
    p.family = GEMM_GENERIC;
    // 256 x 256 tiles when the problem is large enough to fill the 256 CUs with them, 128 x 128 tiles otherwise
    const long big_tiles = (long)((d.M + 255) / 256) * ((d.N + 255) / 256) * p.split_k;
    if (t.gemm_tile == 128) p.generic_tile = GEMM_TILE_128_W4;      // MOREC_GEMM_TILE: tuning override
    else if (t.gemm_tile == 256) p.generic_tile = GEMM_TILE_256_W8;
    else if (t.gemm_tile == 129) p.generic_tile = GEMM_TILE_128_W8;
    else if (t.gemm_tile == 2128) p.generic_tile = GEMM_TILE_256x128;
    else if (t.gemm_tile == 1024) p.generic_tile = GEMM_TILE_256_W16;
    // narrow outputs (N <= 128: the Swin stage-1 projections) and very short K (<= 96) are streaming problems: a 256-wide
    // tile would be mostly padding / a 3-step main loop, and two independent 128 x 128 workgroups per CU overlap one's loads
    // with the other's stores (measured per shape in scripts/swin_gemm_shapes.py)
    else if (d.N <= 128 || d.K <= 96) p.generic_tile = GEMM_TILE_128_W8;
    // 256 x 256 as 16 waves of 64 x 64 (4 waves per SIMD, 118 VGPRs): 3 - 14 % faster than 8 waves of 128 x 64 on every encoder
    // shape (scripts/gemm_bench.py) -- the extra waves cover each other's LDS / barrier waits
    else if (big_tiles >= 192) p.generic_tile = GEMM_TILE_256_W16;
    else p.generic_tile = GEMM_TILE_128_W8;      // 128 x 128 as 8 waves of 64 x 32 (same reasoning)
    p.tile_rows = (p.generic_tile == GEMM_TILE_128_W8 || p.generic_tile == GEMM_TILE_128_W4) ? 128 : 256;
    p.tile_cols = p.generic_tile == GEMM_TILE_256x128 ? 128 : p.tile_rows;
    return p;
}
