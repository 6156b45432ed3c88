// featfuse.hip -- the item tower of the two-stage ID (+) modality packages (bce_text/id_plus_mo-2stage/model/model.py:48-50 with
// mo_dnn_layers = 0: fc(id_embedding(id), turn_dim(features[id])), turn_dim = Linear + GELU, fc = ADD | the head of CAT) in ONE launch:
//   y[r, :]  = GELU(table[idx[r], :] . W^T + b)                       (pre[r, :] = the pre-activation, optional)
//   ADD: out[r, 0:D]  = id_table[idx[r], :] + y[r, :]                 out [R, D]
//   CAT: out[r, 0:D]  = drop(id_table[idx[r], :]),  out[r, D:2D] = drop(y[r, :])      out [R, 2D], one dropout stream over the [R, 2D] matrix
// The main loop is featproj.hip's (featproj_core.hpp): the same products in the same order.  The epilogue stays in the accumulator layout
// (a lane holds four consecutive columns of one row): y is rounded to the 16-bit type FIRST, then added to the id row's four floats (ADD:
// one 16-byte load, one 8-byte store) or multiplied by inv_keep with __fmul_rn (CAT) and rounded again -- every bit of out and pre is what
// morec_featproj_fwd followed by morec_fuse_add_fwd / morec_fuse_cat_fwd writes for the same inputs, p and seed.  CAT: the workgroup of
// column tile c writes columns [64 c, 64 c + 64) of BOTH halves of its rows, so the id half needs no pass of its own; keep flags are
// drop_keep_vec<4> at element index r 2D + column (fuse_cat_fwd_kernel's stream).  idx is clamped into [0, n_rows) for both tables.  Rows
// >= R and columns >= D are never stored.  Only 8-byte stores follow the MFMA loop (common.hpp: the 16-byte-store hazard).  One writer per
// element, no atomics: the same bits every run.
#include "featproj_core.hpp"

namespace {
template <typename T16, bool CAT>
__global__ __launch_bounds__(256) void featfuse_fwd_kernel(const T16* __restrict__ table, const int32_t* __restrict__ idx,
                                                           const T16* __restrict__ W, const float* __restrict__ bias,
                                                           const float* __restrict__ id_table, T16* __restrict__ out, T16* __restrict__ pre,
                                                           int R, int n_rows, int Kw, int D, DropRng dr) {
    if (CAT) dr = drop_resolve(dr);
    const FpTile t = fp_tile(D);
    f32x4_t acc[2][2];
    int ids[2];
    fp_accumulate<T16>(acc, ids, t, table, idx, W, R, n_rows, Kw, D);

    // accumulator (i, j), register e: output row r0 + 16 i + c16, column d0 + 16 j + 4 q + e (D % 8 == 0: the four columns are in or out together)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int d = t.d0 + 16 * j + 4 * t.q;
        if (d >= D) continue;
        const float4 b = bias ? *reinterpret_cast<const float4*>(bias + d) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = t.r0 + 16 * i + t.c16;
            if (r >= R) continue;
            float v[4] = {acc[i][j][0] + b.x, acc[i][j][1] + b.y, acc[i][j][2] + b.z, acc[i][j][3] + b.w};
            if (pre) io<T16>::store4(pre + (size_t)r * D + d, v);
            gelu4(v);
            float e[4];      // the id row's four columns (ids[i]: row r's clamped id)
            io<float>::load4(id_table + (size_t)ids[i] * D + d, e);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = io<T16>::round(v[k]);      // what the composition writes and reads back between its launches
            if (!CAT) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] += e[k];
                io<T16>::store4(out + (size_t)r * D + d, v);
            } else {
                const size_t base = (size_t)r * 2 * D;
                if (dr.thresh) {
                    bool ke[4], kv[4];
                    drop_keep_vec<4>(dr, base + d, ke);
                    drop_keep_vec<4>(dr, base + D + d, kv);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        e[k] = ke[k] ? __fmul_rn(e[k], dr.inv_keep) : 0.f;
                        v[k] = kv[k] ? __fmul_rn(v[k], dr.inv_keep) : 0.f;
                    }
                }
                io<T16>::store4(out + base + d, e);
                io<T16>::store4(out + base + D + d, v);
            }
        }
    }
}
}  // namespace

// Automatic rule (tuning.featfuse == 0), from profiles/id_two_stage_step.txt (fp16, add / cat, against the composition FeatFuseFn runs
// otherwise): ahead at 1024 and 1344 x 768 x 512 (15 - 17 us against 17 - 19 us for featproj + fuse), at 1536 and 2048 x 768 x 512 (16 - 17 us
// against 24 - 26 us for gather + GEMM + fuse) and at 21504 x 128 x 64 (11 us against 18 us); behind at 5376 x 768 x 512 (40 - 42 us against
// 25 - 27 us: featproj's loss there, every wave re-reading its operand rows through L2, is inherited).  Nothing between 2048 and 5376 rows was
// measured: the threshold is the largest product at which the fused kernel was seen ahead, 2048 x 768 x 512 = 3 . 2^28.
extern "C" int morec_featfuse_supported(int R, int Kw, int D, int dtype) {
    const int knob = tuning().featfuse;
    if (knob == 1) return 0;
    if (!(R > 0 && Kw > 0 && D > 0 && is_h16(dtype) && Kw % 8 == 0 && D % 8 == 0)) return 0;
    return knob == 2 || (long long)R * Kw * D <= (3LL << 28);
}

extern "C" int morec_featfuse_fwd(const void* table, const int32_t* idx, const void* W, const float* bias, const float* id_table, void* out,
                                  void* pre, int R, int n_rows, int Kw, int D, int dtype, int kind, float p, uint64_t seed, void* stream) {
    // morec_featproj_fwd's order: the sizes and the type are judged first, then the pointers
    if (R <= 0 || n_rows <= 0 || Kw <= 0 || D <= 0) return MOREC_E_ARG;
    if (!is_h16(dtype)) return MOREC_E_DTYPE;      // fp32: the composed path
    if (Kw % 8 || D % 8) return MOREC_E_ALIGN;
    if (kind != MOREC_FUSE_ADD && kind != MOREC_FUSE_CAT) return MOREC_E_ARG;
    if (!(p >= 0.f && p < 1.f)) return MOREC_E_ARG;
    if (!table || !idx || !W || !id_table || !out) return MOREC_E_ARG;
    if (!aligned16(table) || !aligned16(W) || !aligned16(id_table) || !aligned16(out) || (pre && !aligned16(pre)) || (bias && !aligned16(bias)))
        return MOREC_E_ALIGN;
    const long tiles = (((long)R + FP_TR - 1) / FP_TR) * ((D + FP_TC - 1) / FP_TC);
    if (tiles > 0x7fffffffL) return MOREC_E_UNSUPPORTED;
    const bool cat = kind == MOREC_FUSE_CAT;
    const DropRng dr = make_drop(cat ? p : 0.f, seed);      // ADD has no dropout: p is checked and unused
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((unsigned)tiles);
    by_h16(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        if (cat)
            hipLaunchKernelGGL((featfuse_fwd_kernel<T, true>), grid, dim3(256), 0, s, (const T*)table, idx, (const T*)W, bias, id_table, (T*)out,
                               (T*)pre, R, n_rows, Kw, D, dr);
        else
            hipLaunchKernelGGL((featfuse_fwd_kernel<T, false>), grid, dim3(256), 0, s, (const T*)table, idx, (const T*)W, bias, id_table, (T*)out,
                               (T*)pre, R, n_rows, Kw, D, dr);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
