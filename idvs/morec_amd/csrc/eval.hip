// eval.hip -- HR@10 / nDCG@10 ranking without an argsort (T/data_utils/metrics.py:96-102,49-57; T/data_utils/special.py for the
// cold-start and new-item protocol).
// The reference scores every user against every item, sets history scores to -inf, drops column 0 and
// runs a full descending argsort per user in a Python loop to find the 1-based position of the target.
// Equivalent for tie-free scores: rank = 1 + #{items i >= 1, i not in history(u), i != target :
// score(u, i) > score(u, target)}.  The score tiles come out of the exact-fp32 MFMA main loop and are
// consumed in registers -- the [U, item_num+1] score matrix is never written.
// The new-item protocol (special.py: eval_model_special) ranks a target that is NOT a catalogue row: its vector is a row of a
// separate candidate table, it is never masked and no catalogue column is excluded.  One rank kernel serves both; the template
// parameter says where the target vector comes from.
#include "gemm_core.hpp"

namespace {
using G = GemmTile<float, 2>;
constexpr int HBATCH = 16;      // history ids each thread loads per round trip of the history walk

struct EvalArgs {
    const float* prec;
    const float* emb;
    const int32_t* hist;
    const int32_t* target;      // catalogue column excluded from the count (catalogue variant only)
    const float* tscore;
    int32_t* rank;
    int U, I, D, Hmax, tiles_m, tiles_n;
};

// tscore[u] = prec[u] . tab[idx[u]] and rank[u] = 1.  CAND = false: tab is the catalogue, idx the target, and tscore = -inf when
// the target is itself in the (masked) history; CAND = true: tab is the candidate table, never masked.  The row read is clamped
// into [0, n_rows).  One wave per user.
template <bool CAND>
__global__ __launch_bounds__(256) void eval_target_kernel(const float* __restrict__ prec, const float* __restrict__ tab, int n_rows,
                                                          const int32_t* __restrict__ hist, const int32_t* __restrict__ idx,
                                                          float* __restrict__ tscore, int32_t* __restrict__ rank, int U, int D,
                                                          int Hmax) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;
    const int t = idx[u];
    const size_t row = (size_t)min(max(t, 0), n_rows - 1);
    float acc = 0.f;
    for (int c = lane; c < D; c += 64) acc += prec[(size_t)u * D + c] * tab[row * D + c];
    acc = wave_sum(acc);
    bool inhist = false;
    if (!CAND) {
        for (int h = lane; h < Hmax; h += 64) inhist |= (hist[(size_t)u * Hmax + h] == t);
        inhist = __any(inhist);
    }
    if (lane == 0) {
        tscore[u] = inhist ? -INFINITY : acc;
        rank[u] = 1;
    }
}

// Bit c of mask row r <- item n0 + c is in the history of user m0 + r, for the `rows` users of the block.  Their histories are one
// contiguous run of rows * Hmax ids; each thread loads HBATCH of them per round trip (indices clamped into the run: every load is in
// bounds and none is guarded), then tests them.  Padding (-1) and ids outside [n0, n0 + 128) set nothing, repeats set the same bit.
// The cost is one pass over the block's histories per tile, whatever the scores.
__device__ __forceinline__ void mark_history(const int32_t* __restrict__ hist, int Hmax, int rows, int m0, int n0,
                                             uint32_t* s_mask) {
    const int32_t* base = hist + (size_t)m0 * Hmax;
    const int total = rows * Hmax;
    for (int f0 = 0; f0 < total; f0 += 256 * HBATCH) {
        int id[HBATCH];
#pragma unroll
        for (int j = 0; j < HBATCH; ++j) id[j] = base[min(f0 + j * 256 + (int)threadIdx.x, total - 1)];
#pragma unroll
        for (int j = 0; j < HBATCH; ++j) {
            const int f = f0 + j * 256 + (int)threadIdx.x;
            const unsigned c = (unsigned)id[j] - (unsigned)n0;
            if (f < total && c < 128u) atomicOr(s_mask + (f / Hmax) * 4 + (c >> 5), 1u << (c & 31));
        }
    }
}

// rank[u] += #{ i in [n0, n0 + 128) : 1 <= i < I, i not in history(u), (CAND or i != target[u]), score(u, i) > tscore[u] }
template <bool CAND>
__global__ __launch_bounds__(256) void eval_rank_kernel(EvalArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wg = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    const int m0 = (wg / p.tiles_n) * 128, n0 = (wg % p.tiles_n) * 128;
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    gemm_mainloop<float, 2>(p.prec, p.emb, p.U, p.I, p.D, p.D, m0, n0, 0, p.D, smem, acc);
    // the main loop ends on a barrier: its LDS ring now holds the 128 x 128-bit history mask ([row][4 words])
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(smem);
    s_mask[threadIdx.x] = 0u;
    s_mask[threadIdx.x + 256] = 0u;
    __syncthreads();
    mark_history(p.hist, p.Hmax, min(128, p.U - m0), m0, n0, s_mask);
    __syncthreads();
    float ts[4];
    int tgt[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {      // per-row operands, clamped rows: unguarded loads the compiler can issue together
        const int uc = min(acc_row(m0, mi), p.U - 1);
        ts[mi] = p.tscore[uc];
        tgt[mi] = CAND ? -1 : p.target[uc];
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int u = acc_row(m0, mi);
        int cnt = 0;
        if (u < p.U) {
            const uint32_t* mrow = s_mask + (u - m0) * 4;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int n = acc_col(n0, ni);
                const uint32_t word = mrow[(n - n0) >> 5];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int item = n + r;
                    const bool masked = (word >> ((n - n0 + r) & 31)) & 1u;
                    cnt += (item >= 1 && item < p.I && (CAND || item != tgt[mi]) && !masked && acc[mi][ni][r] > ts[mi]) ? 1 : 0;
                }
            }
        }
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        if (u < p.U && ((threadIdx.x & 63) >> 4) == 0 && cnt) atomicAdd(p.rank + u, cnt);
    }
}

template <bool CAND>
int eval_rank_launch(const float* prec, const float* item_emb, const int32_t* hist, int Hmax, const float* tab, int n_rows,
                     const int32_t* idx, int32_t* rank, float* tscore_ws, int U, int n_items_plus1, int D, hipStream_t s) {
    hipLaunchKernelGGL(eval_target_kernel<CAND>, dim3((U + 3) / 4), dim3(256), 0, s, prec, tab, n_rows, hist, idx, tscore_ws,
                       rank, U, D, Hmax);
    MOREC_CHECK_LAUNCH();
    EvalArgs a{prec, item_emb, hist, idx, tscore_ws, rank, U, n_items_plus1, D, Hmax, (U + 127) / 128,
               (n_items_plus1 + 127) / 128};
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&eval_rank_kernel<CAND>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              G::LDS_BYTES);
    hipLaunchKernelGGL(eval_rank_kernel<CAND>, dim3(a.tiles_m * a.tiles_n), dim3(256), G::LDS_BYTES, s, a);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
static_assert(128 * 128 / 8 <= G::LDS_BYTES, "the history mask lives in the main loop's LDS ring");
}  // namespace

extern "C" int morec_eval_rank(const float* prec, const float* item_emb, const int32_t* hist, int Hmax,
                               const int32_t* target, int32_t* rank, float* tscore_ws, int U, int n_items_plus1,
                               int D, void* stream) {
    if (!prec || !item_emb || !hist || !target || !rank || !tscore_ws || U <= 0 || n_items_plus1 <= 1 || D <= 0 ||
        Hmax <= 0)
        return MOREC_E_ARG;
    if (D % 4 || !aligned16(prec) || !aligned16(item_emb)) return MOREC_E_ALIGN;
    if (Hmax > INT_MAX / 128) return MOREC_E_UNSUPPORTED;      // a block's 128 histories are indexed in int
    return eval_rank_launch<false>(prec, item_emb, hist, Hmax, item_emb, n_items_plus1, target, rank, tscore_ws, U, n_items_plus1,
                                   D, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int morec_eval_rank_cand(const float* prec, const float* item_emb, const int32_t* hist, int Hmax, const float* cand_emb,
                                    int n_cand_rows, const int32_t* cand_idx, int32_t* rank, float* tscore_ws, int U,
                                    int n_items_plus1, int D, void* stream) {
    if (!prec || !item_emb || !hist || !cand_emb || !cand_idx || !rank || !tscore_ws || U <= 0 || n_items_plus1 <= 1 ||
        n_cand_rows <= 0 || D <= 0 || Hmax <= 0)
        return MOREC_E_ARG;
    if (D % 4 || !aligned16(prec) || !aligned16(item_emb)) return MOREC_E_ALIGN;
    if (Hmax > INT_MAX / 128) return MOREC_E_UNSUPPORTED;
    return eval_rank_launch<true>(prec, item_emb, hist, Hmax, cand_emb, n_cand_rows, cand_idx, rank, tscore_ws, U, n_items_plus1,
                                  D, reinterpret_cast<hipStream_t>(stream));
}
