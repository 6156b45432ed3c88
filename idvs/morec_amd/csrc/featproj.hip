// featproj.hip -- the first layer of the two-stage item tower (bce_text/main-2stage(SASRec)/model/encoders.py MLP_Layers.fc + GELU over
// looked-up rows of a frozen feature table; the reference gathers on the host, data_utils/dataset.py BuildTrainDataset.__getitem__):
//   out[r, :] = GELU(table[idx[r], :] . W^T + b),  pre[r, :] = the pre-activation (optional),  r < R
// in ONE launch: the gather is folded into the projection.  table [n_rows, Kw] and W [D, Kw] are 16-bit, K-contiguous, so both MFMA operands
// of v_mfma_f32_16x16x32_{bf16,f16} are one 16-byte global load per lane straight into the fragment (lane l: row l & 15, k from 8 (l >> 4)):
// nothing is staged through LDS.  W is the FIRST operand and the gathered rows the second, so a lane's four accumulator registers are four
// consecutive output COLUMNS of one output row: bias is one float4, out / pre are 8-byte stores, no transpose.
// Workgroup: four waves as 2 x 2 over 64 rows x 64 columns, a wave owns 32 x 32 (2 x 2 accumulators).  A K step is 64 elements (two MFMA
// k-steps: a lane's two loads of a row are one 128-byte line between the four lanes that share the row); the loads of step s + 1 are issued
// into a second register set before the MFMAs of step s.  Rows >= R and columns >= D are loaded from a clamped (valid) address and never
// stored; k >= Kw is zero-filled in registers; idx is clamped into [0, n_rows).  One writer per element, no atomics: the same bits every run.
// The main loop lives in featproj_core.hpp, shared with featfuse.hip.
#include "featproj_core.hpp"

namespace {
template <typename T16>
__global__ __launch_bounds__(256) void featproj_fwd_kernel(const T16* __restrict__ table, const int32_t* __restrict__ idx,
                                                           const T16* __restrict__ W, const float* __restrict__ bias, T16* __restrict__ out,
                                                           T16* __restrict__ pre, int R, int n_rows, int Kw, int D) {
    const FpTile t = fp_tile(D);
    const int r0 = t.r0, d0 = t.d0, c16 = t.c16, q = t.q;
    f32x4_t acc[2][2];
    int ids[2];
    fp_accumulate<T16>(acc, ids, t, table, idx, W, R, n_rows, Kw, D);

    // accumulator (i, j), register e: output row r0 + 16 i + c16, column d0 + 16 j + 4 q + e (D % 8 == 0: the four columns are in or out together)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int d = d0 + 16 * j + 4 * q;
        if (d >= D) continue;
        const float4 b = bias ? *reinterpret_cast<const float4*>(bias + d) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r0 + 16 * i + c16;
            if (r >= R) continue;
            float v[4] = {acc[i][j][0] + b.x, acc[i][j][1] + b.y, acc[i][j][2] + b.z, acc[i][j][3] + b.w};
            const size_t o = (size_t)r * D + d;
            if (pre) io<T16>::store4(pre + o, v);
            gelu4(v);
            io<T16>::store4(out + o, v);
        }
    }
}
}  // namespace

// Automatic rule (tuning.featproj == 0), from profiles/two_stage_step.txt: one launch beats gather + GEMM while the product is small
// (R Kw D up to 1344 x 768 x 512: 15 us against 16 us; 21504 x 128 x 64: 9 us against 17 us), and loses once every wave re-reading its own
// operand rows through L2 outweighs the launch it saves (5376 x 768 x 512: 39 us against 21 us).  Nothing in between was measured: the
// threshold is the largest product at which the fused kernel was seen ahead.
extern "C" int morec_featproj_supported(int R, int Kw, int D, int dtype) {
    const int knob = tuning().featproj;
    if (knob == 1) return 0;
    if (!(R > 0 && Kw > 0 && D > 0 && is_h16(dtype) && Kw % 8 == 0 && D % 8 == 0)) return 0;
    return knob == 2 || (long long)R * Kw * D <= (1LL << 29);
}

extern "C" int morec_featproj_fwd(const void* table, const int32_t* idx, const void* W, const float* bias, void* out, void* pre, int R,
                                  int n_rows, int Kw, int D, int dtype, void* stream) {
    // the sizes and the type are judged first, then the pointers: a descriptor alone (null pointers) already gets the shape's answer
    if (R <= 0 || n_rows <= 0 || Kw <= 0 || D <= 0) return MOREC_E_ARG;
    if (!is_h16(dtype)) return MOREC_E_DTYPE;      // fp32: the composed path (morec_indexed_rows_copy + morec_gemm_nt)
    if (Kw % 8 || D % 8) return MOREC_E_ALIGN;
    if (!table || !idx || !W || !out) return MOREC_E_ARG;
    if (!aligned16(table) || !aligned16(W) || !aligned16(out) || (pre && !aligned16(pre)) || (bias && !aligned16(bias))) return MOREC_E_ALIGN;
    const long tiles = (((long)R + FP_TR - 1) / FP_TR) * ((D + FP_TC - 1) / FP_TC);
    if (tiles > 0x7fffffffL) return MOREC_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((unsigned)tiles);
    by_h16(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        hipLaunchKernelGGL((featproj_fwd_kernel<T>), grid, dim3(256), 0, s, (const T*)table, idx, (const T*)W, bias, (T*)out, (T*)pre, R,
                           n_rows, Kw, D);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
