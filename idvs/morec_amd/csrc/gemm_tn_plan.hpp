// gemm_tn_plan.hpp -- what a weight-gradient GEMM (morec_gemm_tn, gemm_tn.hip / gemm_tn8p.hip) launches: ONE function, plain C++17 (no HIP
// include, no device call, no allocation), so that a selection can be asked and tested without a GPU (morec_gemm_tn_plan,
// tests/test_gemm_tn_cpu.py).  gemm_tn_launch asks it and launches what it says; gemm_tn8p_launch takes the plan and only launches.
// The checks stand in the order callers see their codes.
#pragma once
#include "morec_hip.h"
#include "tuning.hpp"

enum TnKernel {             // the ids of include/morec_hip.h (morec_gemm_tn_plan_info.kernel)
    TN_UNSUPPORTED = MOREC_TN_UNSUPPORTED,          // TnPlan::error says why
    TN_TWO_BUFFER = MOREC_TN_TWO_BUFFER,            // gemm_tn.hip: gemm_tn_kernel
    TN_EIGHT_P = MOREC_TN_EIGHT_P,                  // gemm_tn8p.hip: gemm_tn8p_kernel<T, false>
    TN_EIGHT_P_SKIP = MOREC_TN_EIGHT_P_SKIP,        // gemm_tn8p.hip: gemm_tn8p_kernel<T, true> (no MFMAs on 32 x 32 blocks outside the matrix)
};
enum TnPath {               // how the result reaches C (morec_gemm_tn_plan_info.path)
    TN_PATH_NONE = MOREC_TN_PATH_NONE,
    TN_PATH_STORE = MOREC_TN_PATH_STORE,            // one token chunk, overwrite: plain 16-byte stores
    TN_PATH_RMW = MOREC_TN_PATH_RMW,                // one token chunk, accumulate: read-modify-write of the lane's own four elements
    TN_PATH_ATOMIC = MOREC_TN_PATH_ATOMIC,          // several chunks, no workspace: fp32 atomicAdd into a caller-zeroed / accumulated C
    TN_PATH_SLABS = MOREC_TN_PATH_SLABS,            // several chunks: one fp32 slab per chunk, folded by reduce_slabs_kernel
};

namespace tnplan {
// the tile constants the rules need; the kernel files static_assert their own against these
constexpr int TT = 64;       // tokens per stage (both kernels)
constexpr int TC = 256;      // output tile: TC (n) x TC (k)
inline bool is16(int dtype) { return dtype == MOREC_BF16 || dtype == MOREC_F16; }
}  // namespace tnplan

struct TnPlan {
    int kernel;             // TnKernel
    int error;              // TN_UNSUPPORTED: the MOREC_E_* code morec_gemm_tn returns
    int mchunk;             // tokens per chunk: ceil(M / split_m) rounded up to a stage
    int zs;                 // chunks launched: ceil(M / mchunk) <= split_m
    int tiles_n, tiles_k;
    int path;               // TnPath
    int fold;               // reduce_slabs_kernel follows (path == TN_PATH_SLABS)
};

// c_dtype: MOREC_F32, or the operands' 16-bit type for the scoring backward's rounded fold (slabs + overwrite only).
// ptrs_aligned: DY, X and C are 16-byte aligned; ws_aligned: the workspace is (both true where there are no operands to ask).
inline TnPlan gemm_tn_plan(int M, int N, int K, int ldy, int ldx, int ldc, int dtype, int c_dtype, int split_m, int accumulate,
                           bool has_workspace, bool ptrs_aligned, bool ws_aligned, const Tuning& t) {
    using namespace tnplan;
    TnPlan p{};
    auto refuse = [&](int code) { p.kernel = TN_UNSUPPORTED; p.error = code; return p; };
    if (M <= 0 || N <= 0 || K <= 0) return refuse(MOREC_E_ARG);
    if (!is16(dtype)) return refuse(MOREC_E_UNSUPPORTED);   // the exact-fp32 path uses transposed copies + morec_gemm_nt
    if (c_dtype != MOREC_F32 && c_dtype != dtype) return refuse(MOREC_E_DTYPE);
    if (N % 8 || K % 8 || ldy % 8 || ldx % 8 || ldc % 4 || !ptrs_aligned) return refuse(MOREC_E_ALIGN);
    if (split_m > 1 && !accumulate && !has_workspace) return refuse(MOREC_E_ARG);      // the atomic path needs a caller-zeroed C
    const int split = split_m < 1 ? 1 : split_m;
    int mchunk = (M + split - 1) / split;
    mchunk = ((mchunk + TT - 1) / TT) * TT;
    p.mchunk = mchunk;
    const int zs = (M + mchunk - 1) / mchunk;
    p.zs = zs;
    p.tiles_n = (N + TC - 1) / TC; p.tiles_k = (K + TC - 1) / TC;
    const bool slabs = zs > 1 && has_workspace;
    if (slabs && (K % 4 || !ws_aligned)) return refuse(MOREC_E_ALIGN);
    if (c_dtype != MOREC_F32 && (!slabs || accumulate)) return refuse(MOREC_E_UNSUPPORTED);
    if (zs > 1 && !slabs && !accumulate) return refuse(MOREC_E_ARG);
    p.path = slabs ? TN_PATH_SLABS : !accumulate ? TN_PATH_STORE : zs == 1 ? TN_PATH_RMW : TN_PATH_ATOMIC;
    p.fold = slabs ? 1 : 0;
    p.kernel = TN_TWO_BUFFER;
    // The eight-phase kernel writes plain stores only -- split-m partials into slabs, or one chunk that overwrites C -- and needs two whole
    // stages in flight: every chunk, the last one too, holds at least 2 TT tokens.  (Its 16-byte column slots and output rows -- N % 8, K % 8,
    // a pitch of K or ldc floats -- and mchunk % TT hold for everything that got here.)
    if (!(slabs || (zs == 1 && !accumulate))) return p;
    if (t.gemm8p == 1) return p;
    if (mchunk < 2 * TT) return p;
    if (zs > 1 && M - (zs - 1) * (long)mchunk < 2 * TT) return p;     // the last chunk needs two stages as well
    if (zs == 1 && M < 2 * TT) return p;
    // automatic: enough work per workgroup.  (No tile-fill rule: on every Swin-T / BERT weight-gradient shape measured --
    // down to 96 x 96 outputs, 86 % of the tile outside the matrix -- this kernel is at least as fast as the two-buffer one,
    // which is HBM-bound there as well: profiles/r02_swin_gemm_shapes_modes.txt.)
    if (t.gemm8p != 2 && mchunk < 8 * TT) return p;
    if ((long)M * ldy * 2 >= 0x7fffffffL || (long)M * ldx * 2 >= 0x7fffffffL) return p;   // 32-bit stage offsets
    // a 32-wide block row or column of some tile lies outside the matrix: the variant that skips those blocks' MFMAs
    // (MOREC_TN8P_SKIP=0: never, an A/B aid)
    const bool skip = t.tn8p_skip && ((N % TC != 0 && N % TC <= 224) || (K % TC != 0 && K % TC <= 224));
    p.kernel = skip ? TN_EIGHT_P_SKIP : TN_EIGHT_P;
    return p;
}
