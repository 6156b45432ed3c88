// eval_topk.hip -- top-K recommendation lists without a score matrix (T/data_utils/metrics.py:96-102: score every item, set the history
// to -inf, argsort -- here read the other way round: not "where does the target land" (eval.hip) but "which K items come first").
// Row u of the result holds the K best eligible items (1 <= i < n_items_plus1, i not in hist[u, :]) in a STRICT TOTAL order: score
// descending, item id ascending among equal scores.  Because the order is total, the K best of a union of column strips are the K best
// of the strips' own K best: the catalogue is cut into `strips` runs of 128-column tiles, pass 1 keeps one sorted list per (user, strip)
// and pass 2 merges them; the answer does not depend on the cut, the grid or the CU count.
//
// Pass 1 (eval_topk_strip_kernel): a 256-thread workgroup owns 128 users and one strip.  Per tile the exact-fp32 MFMA main loop of
// eval_rank_kernel fills the 4 x 4 accumulators, the history mask is built as there (mark_history), and the tile's scores go into the
// main loop's LDS ring (128 x 128 fp32 = G::LDS_BYTES exactly), ineligible cells as NaN: every comparison below is an ordered one, so a
// NaN -- an ineligible cell or a NaN score alike -- never enters a list, while an eligible item that scores -inf still can.  Each wave
// then walks its 32 rows, two scores per lane: a ballot of "precedes the row's K-th entry"; empty (the common case after the first
// tiles of a strip) and the row is done, otherwise the survivors are inserted one at a time (wave_insert).  The lists live in LDS
// behind the ring and the mask: 128 rows x K x 8 B.
// Pass 2 (eval_topk_merge_kernel): one wave per user streams its strips * K workspace entries through the same insert.
#include "gemm_core.hpp"
#include <limits.h>

namespace {
using G = GemmTile<float, 2>;
// history ids each thread loads per round trip: half of eval.hip's 16 -- the accumulators are live across the walk here too, and with
// 8 the kernel stays under 256 registers without scratch, i.e. two workgroups per CU whenever the lists leave the LDS for them
constexpr int HBATCH = 8;
constexpr int TOPK_MAX_K = 64;             // one list entry per lane; at K = 64 a workgroup holds 64 KiB ring + 2 KiB mask + 64 KiB lists
constexpr int MASK_BYTES = 128 * 4 * 4;    // 128 rows x 128 bits
constexpr int EMPTY_ID = INT_MAX;          // an empty list slot is (-inf, EMPTY_ID): it follows every eligible item, -inf-scored ones too
// Automatic strips: the grid (row blocks x strips) is brought to TARGET_WGS = twice the 256 CUs, so that a small user batch (512
// users = 4 row blocks) still fills the chip and leaves the dispatcher a second wave of workgroups to even out the strips.  A
// constant, not a device query: the size query below is host code that runs without a GPU, and the result does not depend on it.
constexpr int TARGET_WGS = 512;

struct TopkPair {
    float score;
    int32_t id;
};
static_assert(sizeof(TopkPair) == 8, "workspace entries are 8 bytes");

struct TopkArgs {
    const float* prec;
    const float* emb;
    const int32_t* hist;       // NULL: nobody masks anything
    TopkPair* ws;              // [U, strips, K], strips > 1 only
    int32_t* out_ids;          // [U, K], written by pass 1 when strips == 1
    float* out_scores;
    int U, I, D, Hmax, K, strips, tiles_m, tiles_n;
};

static inline int tiles_of(int n) { return (n + 127) / 128; }
static inline int resolve_strips(int U, int n_items_plus1, int strips) {
    const int tn = tiles_of(n_items_plus1), tm = tiles_of(U);
    if (strips <= 0) strips = (TARGET_WGS + tm - 1) / tm;
    return strips < tn ? strips : tn;
}

// (s, i) comes strictly before (t, j) in the list order.  False whenever s is a NaN.
__device__ __forceinline__ bool precedes(float s, int i, float t, int j) { return s > t || (s == t && i < j); }

// The wave's sorted list has entry j in lane j (lanes >= K hold don't-cares).  Inserts every candidate (cs, ci) -- one per lane, NaN =
// none -- that precedes the K-th entry, first live lane first: the result is the K first of list + candidates in the total order,
// whatever the insertion order.  Called in wave-uniform control flow only (every lane takes part in the cross-lane operations).
// (The same chain on v_readlane for the wave-uniform lane reads and a DPP row_shr:1 shift, no ds_bpermute left, measured SLOWER at the
// bench's eval shape: 1 174 against 873 us at 512 users, 4 169 against 3 777 us at 4 096 -- profiles/eval_topk.txt.  Not used.)
__device__ __forceinline__ void wave_insert(float& ls, int& li, float cs, int ci, int K, int lane) {
    for (;;) {
        const float ks = __shfl(ls, K - 1, 64);
        const int ki = __shfl(li, K - 1, 64);
        const unsigned long long live = __ballot(precedes(cs, ci, ks, ki));
        if (!live) break;
        const int src = __ffsll(live) - 1;
        const float s = __shfl(cs, src, 64);
        const int i = __shfl(ci, src, 64);
        // the list is sorted: the entries that precede (s, i) are lanes 0 .. pos-1, and pos <= K-1 because (s, i) precedes entry K-1
        const int pos = __popcll(__ballot(lane < K && precedes(ls, li, s, i)));
        const float us = __shfl_up(ls, 1, 64);
        const int ui = __shfl_up(li, 1, 64);
        if (lane == pos) {
            ls = s;
            li = i;
        } else if (lane > pos) {
            ls = us;
            li = ui;
        }
        if (lane == src) cs = NAN;
    }
}

// Bit c of mask row r <- item n0 + c is in the history of user m0 + r (eval.hip's scheme: clamped, unguarded batched loads).
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

// Score tile in the ring: row pitch 512 B, the 16-byte slot of (row, col) XORed with row & 7 so that the eight rows one ds_write_b128
// lane group touches land on different banks; a row's own 128 scores stay a permutation of its 32 slots.
__device__ __forceinline__ int tile_off(int row, int col) { return row * 128 + ((((col >> 2) ^ (row & 7)) << 2) | (col & 3)); }

__global__ __launch_bounds__(256, 2) void eval_topk_strip_kernel(TopkArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* s_tile = reinterpret_cast<float*>(smem);
    uint32_t* s_mask = reinterpret_cast<uint32_t*>(smem + G::LDS_BYTES);
    float* s_ls = reinterpret_cast<float*>(smem + G::LDS_BYTES + MASK_BYTES);
    int* s_li = reinterpret_cast<int*>(s_ls + 128 * p.K);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = p.K;
    const int wg = xcd_remap(blockIdx.x, p.tiles_m * p.strips);
    const int m0 = (wg / p.strips) * 128, strip = wg % p.strips;
    // balanced cut: strip j owns tiles [j * tiles_n / strips, (j + 1) * tiles_n / strips), never empty since strips <= tiles_n
    const int t_beg = (int)((long long)strip * p.tiles_n / p.strips), t_end = (int)((long long)(strip + 1) * p.tiles_n / p.strips);
    const int rows = min(128, p.U - m0);
    const bool masking = p.hist != nullptr && p.Hmax > 0;

    // a wave owns the lists of rows wave * 32 .. + 31 from here to the end: no other wave touches them
    for (int e = lane; e < 32 * K; e += 64) {
        s_ls[wave * 32 * K + e] = -INFINITY;
        s_li[wave * 32 * K + e] = EMPTY_ID;
    }
    s_mask[threadIdx.x] = 0u;
    s_mask[threadIdx.x + 256] = 0u;

    for (int t = t_beg; t < t_end; ++t) {
        const int n0 = t * 128;
        f32x4_t acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        // the ring is free: the previous tile's row walk ended on a barrier
        gemm_mainloop<float, 2>(p.prec, p.emb, p.U, p.I, p.D, p.D, m0, n0, 0, p.D, smem, acc);
        if (masking) {
            // the mask was cleared before the main loop (whose barriers order the clear before these atomics)
            mark_history(p.hist, p.Hmax, rows, m0, n0, s_mask);
            __syncthreads();
        }
        // the main loop ended on a barrier: its ring now takes the score tile
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = acc_row(0, mi);
            const uint32_t* mrow = s_mask + row * 4;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int col = acc_col(0, ni);
                const uint32_t word = mrow[col >> 5];
                float4 v;
                float* vp = reinterpret_cast<float*>(&v);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int item = n0 + col + r;
                    const bool masked = (word >> ((col + r) & 31)) & 1u;
                    vp[r] = (item >= 1 && item < p.I && !masked) ? acc[mi][ni][r] : NAN;
                }
                *reinterpret_cast<float4*>(s_tile + tile_off(row, col)) = v;
            }
        }
        __syncthreads();
        if (masking) {      // every wave has read its mask bits: clear them for the next tile
            s_mask[threadIdx.x] = 0u;
            s_mask[threadIdx.x + 256] = 0u;
        }
        for (int rr = 0; rr < 32; ++rr) {
            const int row = wave * 32 + rr;
            if (row >= rows) break;      // wave-uniform
            const float2 sc = *reinterpret_cast<const float2*>(s_tile + tile_off(row, 2 * lane));
            const int i0 = n0 + 2 * lane, i1 = i0 + 1;
            const float ks = s_ls[row * K + K - 1];
            const int ki = s_li[row * K + K - 1];
            if (__ballot(precedes(sc.x, i0, ks, ki) || precedes(sc.y, i1, ks, ki))) {
                const int e = row * K + min(lane, K - 1);
                float ls = s_ls[e];
                int li = s_li[e];
                wave_insert(ls, li, sc.x, i0, K, lane);
                wave_insert(ls, li, sc.y, i1, K, lane);
                if (lane < K) {
                    s_ls[e] = ls;
                    s_li[e] = li;
                }
            }
        }
        __syncthreads();      // the next main loop refills the ring
    }

    for (int rr = 0; rr < 32; ++rr) {
        const int row = wave * 32 + rr;
        if (row >= rows) break;
        if (lane < K) {
            const float ls = s_ls[row * K + lane];
            const int li = s_li[row * K + lane];
            const size_t u = (size_t)(m0 + row);
            if (p.strips == 1) {
                p.out_ids[u * K + lane] = li == EMPTY_ID ? -1 : li;
                p.out_scores[u * K + lane] = ls;
            } else {
                p.ws[(u * p.strips + strip) * K + lane] = TopkPair{ls, li};
            }
        }
    }
}

// One wave per user: the K first of its strips * K workspace entries.
__global__ __launch_bounds__(256) void eval_topk_merge_kernel(const TopkPair* __restrict__ ws, int32_t* __restrict__ out_ids,
                                                              float* __restrict__ out_scores, int U, int K, int strips) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;      // whole waves leave
    const int total = strips * K;
    const TopkPair* src = ws + (size_t)u * total;
    float ls = -INFINITY;
    int li = EMPTY_ID;
    for (int c0 = 0; c0 < total; c0 += 64) {
        const TopkPair c = src[min(c0 + lane, total - 1)];
        wave_insert(ls, li, c0 + lane < total ? c.score : NAN, c.id, K, lane);
    }
    if (lane < K) {
        out_ids[(size_t)u * K + lane] = li == EMPTY_ID ? -1 : li;
        out_scores[(size_t)u * K + lane] = ls;
    }
}

static_assert(G::LDS_BYTES == 128 * 128 * 4, "the score tile is exactly the main loop's ring");
static_assert(G::LDS_BYTES + MASK_BYTES + 128 * TOPK_MAX_K * 8 <= 160 * 1024, "ring + mask + lists fit one CU's LDS");
}  // namespace

extern "C" int morec_eval_topk_max_k(void) { return TOPK_MAX_K; }

extern "C" size_t morec_eval_topk_ws_bytes(int U, int n_items_plus1, int K, int strips) {
    if (U <= 0 || n_items_plus1 <= 1 || K < 1) return 0;
    const size_t tm = (size_t)tiles_of(U), tn = (size_t)tiles_of(n_items_plus1);
    size_t rows_x_strips;      // >= U * resolve_strips(...), and monotone in U
    if (strips > 0) {
        rows_x_strips = (size_t)U * ((size_t)strips < tn ? (size_t)strips : tn);
    } else {
        // automatic: tm * ceil(TARGET_WGS / tm) <= TARGET_WGS - 1 + tm row blocks x strips, at most tm * tn; the product U * strips
        // itself is not monotone in U (129 users get half the strips of 128), its bound is
        const size_t blocks = TARGET_WGS - 1 + tm < tm * tn ? TARGET_WGS - 1 + tm : tm * tn;
        rows_x_strips = blocks * 128;
    }
    return rows_x_strips * (size_t)K * sizeof(TopkPair);
}

extern "C" int morec_eval_topk(const float* prec, const float* item_emb, const int32_t* hist, int Hmax, int K, int strips,
                               int32_t* out_ids, float* out_scores, void* ws, size_t ws_bytes, int U, int n_items_plus1, int D,
                               void* stream) {
    if (!prec || !item_emb || !out_ids || !out_scores || !ws || U <= 0 || n_items_plus1 <= 1 || D <= 0 || Hmax < 0 || K < 1 ||
        strips < 0)
        return MOREC_E_ARG;
    if (K > TOPK_MAX_K) return MOREC_E_UNSUPPORTED;
    if (D % 4 || !aligned16(prec) || !aligned16(item_emb)) return MOREC_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return MOREC_E_ALIGN;
    if (Hmax > INT_MAX / 128) return MOREC_E_UNSUPPORTED;      // a block's 128 histories are indexed in int
    if (ws_bytes < morec_eval_topk_ws_bytes(U, n_items_plus1, K, strips)) return MOREC_E_ARG;
    const int S = resolve_strips(U, n_items_plus1, strips);
    const int tm = tiles_of(U);
    if ((long long)tm * S > INT_MAX || (long long)S * K > INT_MAX) return MOREC_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TopkArgs a{prec, item_emb, hist, static_cast<TopkPair*>(ws), out_ids, out_scores, U, n_items_plus1, D, Hmax, K, S, tm,
               tiles_of(n_items_plus1)};
    const int lds = G::LDS_BYTES + MASK_BYTES + 128 * K * (int)sizeof(TopkPair);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&eval_topk_strip_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES + MASK_BYTES + 128 * TOPK_MAX_K * 8);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(eval_topk_strip_kernel, dim3(tm * S), dim3(256), lds, s, a);
    MOREC_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(eval_topk_merge_kernel, dim3((U + 3) / 4), dim3(256), 0, s, static_cast<const TopkPair*>(ws), out_ids,
                           out_scores, U, K, S);
        MOREC_CHECK_LAUNCH();
    }
    return MOREC_OK;
}
