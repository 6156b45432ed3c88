// featproj_core.hpp -- the main loop shared by featproj.hip and featfuse.hip: a 64 x 64 tile of  table[idx[r], :] . W^T  per workgroup on
// v_mfma_f32_16x16x32_{bf16,f16}, both operands one 16-byte global load per lane straight into the fragment (lane l: row l & 15, k from
// 8 (l >> 4)), nothing staged through LDS.  W is the FIRST operand and the gathered rows the second, so a lane's four accumulator registers
// are four consecutive output COLUMNS of one output row.  Four waves as 2 x 2, a wave owns 32 x 32 (2 x 2 accumulators).  A K step is 64
// elements (two MFMA k-steps: a lane's two loads of a row are one 128-byte line between the four lanes that share the row); the loads of
// step s + 1 are issued into a second register set before the MFMAs of step s.  Rows >= R and columns >= D are loaded from a clamped (valid)
// address; k >= Kw is zero-filled in registers; idx is clamped into [0, n_rows).  Both kernels run literally this accumulation: the same
// products in the same order, so their pre-activations carry the same bits.
#pragma once
#include "common.hpp"

namespace {
constexpr int FP_TR = 64, FP_TC = 64;      // rows x columns of a workgroup's tile
constexpr int FP_KU = 2;                   // MFMA k-steps (32 elements) per K step

struct FpFrags {
    bf16x8_t w[2][FP_KU], x[2][FP_KU];
};

struct FpRows {      // this lane's two W rows and two (looked-up) table rows
    const bf16* w[2];
    const bf16* x[2];
};
// the fragments of K step s: element offset k = 64 s + 32 u + 8 q of this lane's rows.  The address is always a valid one (k clamped to
// the last whole vector of the row); what lies past Kw is replaced by zeros AFTER the load, so no load is guarded.
__device__ __forceinline__ void fp_load(FpFrags& f, const FpRows& rows, int s, int q, int Kw) {
    const bf16x8_t zero = {};
#pragma unroll
    for (int u = 0; u < FP_KU; ++u) {
        const int k = s * (32 * FP_KU) + u * 32 + q * 8;
        const bool in = k < Kw;
        const int kc = in ? k : Kw - 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bf16x8_t wv = *reinterpret_cast<const bf16x8_t*>(rows.w[i] + kc);
            const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(rows.x[i] + kc);
            f.w[i][u] = in ? wv : zero;
            f.x[i][u] = in ? xv : zero;
        }
    }
}

template <typename T16>
__device__ __forceinline__ void fp_mma(f32x4_t (&acc)[2][2], const FpFrags& f) {
#pragma unroll
    for (int u = 0; u < FP_KU; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = h16<T16>::mma16(f.w[j][u], f.x[i][u], acc[i][j]);
}

// This wave's 32 rows from r0 and 32 columns from d0 of the tile numbered blockIdx.x (column tiles vary fastest: neighbouring workgroups
// share their table rows).
struct FpTile {
    int r0, d0, c16, q;
};
__device__ __forceinline__ FpTile fp_tile(int D) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ctiles = (D + FP_TC - 1) / FP_TC;
    FpTile t;
    t.c16 = lane & 15;
    t.q = lane >> 4;
    t.r0 = (blockIdx.x / ctiles) * FP_TR + (wave >> 1) * 32;
    t.d0 = (blockIdx.x % ctiles) * FP_TC + (wave & 1) * 32;
    return t;
}

// acc[i][j], register e = sum_k table[ids[i], k] W[d0 + 16 j + 4 q + e, k] for output row r0 + 16 i + c16;  ids[i]: that row's clamped id
// (operand rows of this lane: W rows d0 + 16 j + c16, table rows idx[r0 + 16 i + c16] -- the lane's operand rows ARE its output rows)
template <typename T16>
__device__ __forceinline__ void fp_accumulate(f32x4_t (&acc)[2][2], int (&ids)[2], const FpTile& t, const T16* __restrict__ table,
                                              const int32_t* __restrict__ idx, const T16* __restrict__ W, int R, int n_rows, int Kw, int D) {
    FpRows rows;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int d = min(t.d0 + 16 * i + t.c16, D - 1);
        const int r = min(t.r0 + 16 * i + t.c16, R - 1);
        ids[i] = min(max(idx[r], 0), n_rows - 1);
        rows.w[i] = reinterpret_cast<const bf16*>(W) + (size_t)d * Kw;
        rows.x[i] = reinterpret_cast<const bf16*>(table) + (size_t)ids[i] * Kw;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int KS = (Kw + 32 * FP_KU - 1) / (32 * FP_KU);
    FpFrags fa, fb;
    fp_load(fa, rows, 0, t.q, Kw);
    int s = 0;
    for (; s + 2 <= KS; s += 2) {      // two K steps per trip: both register sets have compile-time names
        fp_load(fb, rows, s + 1, t.q, Kw);
        fp_mma<T16>(acc, fa);
        fp_load(fa, rows, min(s + 2, KS - 1), t.q, Kw);      // the last trip re-reads a step it does not use
        fp_mma<T16>(acc, fb);
    }
    if (s < KS) fp_mma<T16>(acc, fa);
}
}  // namespace
