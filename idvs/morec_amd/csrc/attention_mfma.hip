// attention_mfma.hip -- 16-bit small-tile attention on the matrix cores (T <= 64, head width a multiple of 32): one kernel
// template over the edge TT of the score tile, TT = 32 (T <= 32) and TT = 64 (32 < T <= 64).
//
// Same contract as attention.hip (which stays the exact-fp32 path): one wavefront per (sequence, head), no
// forward state kept for the backward, counter-based dropout on the probabilities.  What changes is where
// the arithmetic runs:
//   * S = Q K^T and dP = dO V^T: v_mfma_f32_16x16x32_bf16 with both operands read d-contiguous (NT form)
//     from LDS tiles, issued "swapped" so a lane ends up with S[query = qb*16 + (lane&15)]
//     [key = kb*16 + 4*(lane>>4) + r] -- a whole softmax row lives in 4 lanes x TT / 4 registers, the row
//     max / sum are two lane exchanges (xor 16, 32);
//   * the second products (P V, dS K, dS^T Q, P^T dO) contract over keys or queries, i.e. over the ROW index
//     of the row-major LDS tiles: those fragments come from ds_read_b64_tr_b16 (hardware transpose read,
//     semantics measured in profiles/r01_probe_mfma_trb16.txt: lane c of a 16-lane group receives
//     element (c & 3) of the 8-byte words addressed by lanes 4j + (c >> 2), j = 0..3).  The k-slot <-> key
//     permutation this induces is the same one the packed P / dS register fragments use, so nothing is shuffled.
// LDS rows carry a 32-byte pad (pitch / 32 odd) which makes both the b128 and the transpose reads conflict-free.
//
// TT = 32 is the tile of everything on the benchmarked path (titles of 30 tokens, histories of 20 / 10).  TT = 64 serves the
// reference's abstracts / bodies of 50 tokens (T/parameters.py:43-44: num_words_abstract = num_words_body = 50) and behaviour
// sequences of up to 64 items: the score tile is 4 x 4 MFMA blocks, and every product that contracts over keys or queries takes
// TWO k-steps (slots 0..31 | 32..63 of the row-major LDS tiles, each read exactly as the 32-row tile is).  Until round 5 these
// shapes ran the exact-fp32 VALU kernels even in the 16-bit modes (attention.hip); those remain the fallback for head widths
// that are not a multiple of 32 and the path of the fp32 modes.  The two tiles differ in ONE place, how the score phase requests
// its operands (`if constexpr (TT == 32)` in both kernels).
// Reference arithmetic: T/model/modules.py:24-49 (SASRec), HF modeling_bert.py BertSelfAttention (eager).
#include <stdlib.h>
#include "common.hpp"
#include "attention_frag.hpp"


namespace {
template <int TT>                             // TT = rows / columns of the score tile
struct Geo {
    static constexpr int NB = TT / 16;        // 16-row MFMA blocks per side
    static constexpr int NS = TT / 32;        // 32-slot k-steps of a product that contracts over keys / queries
    static constexpr int NR = TT / 8;         // 16-byte vectors a lane stages per [TT x DCH] tile
    static constexpr int TILE = TT * PITCH;   // one [TT x DCH] 16-bit tile
    static constexpr int PP = TT * 2 + 32;    // bytes per row of the [TT x TT] 16-bit probability / dS tiles
};

struct AttnMArgs {
    const bf16* qkv;
    const float* key_keep;
    bf16* ctx;          // fwd: output; bwd: dctx input
    bf16* dqkv;
    float* csum;        // bwd, optional: [n_seq][3 H] fp32 column sums of this sequence's dqkv rows (before their bf16 rounding), folded by the caller
    int n_seq, T, n_heads, dh, causal;
    float scale, mask_value;
    DropRng drop;
    const int32_t* cu;  // packed-row offsets (unpadded layout) or nullptr
    int total_rows;     // rows of the packed buffers; the spare ones (>= cu[n_seq]) are zero-filled by the blocks behind the grid
};



// Rows [0, T) x columns [col0, col0 + ncols) of a row-major global matrix -> registers -> LDS tile (rows >= T repeat row T - 1), in two
// halves: ALL global loads of a kernel phase are issued before the first LDS write.  (Interleaved load / ds_write pairs are
// kept in program order -- the generic LDS pointer may alias the source as far as the compiler knows -- and every pair then
// costs a full memory round trip.)
template <int NR>
__device__ __forceinline__ void load_tile_regs(const bf16* __restrict__ src, size_t row0, int pitch, int col0, int ncols,
                                               int Tlen, uint4 (&v)[NR]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int r = i * 8 + (lane >> 3), s = lane & 7;
        v[i] = load16(src + (row0 + min(r, Tlen - 1)) * (size_t)pitch + col0 + (s * 8 < ncols ? s * 8 : 0));
    }
}
template <int NR>
__device__ __forceinline__ void write_tile_lds(char* __restrict__ tile, const uint4 (&v)[NR]) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NR; ++i) *reinterpret_cast<uint4*>(tile + (i * 8 + (lane >> 3)) * PITCH + (lane & 7) * 16) = v[i];
}

template <int NR>
__device__ __forceinline__ void stage_tile(const bf16* __restrict__ src, size_t row0, int pitch, int col0, int ncols,
                                           int Tlen, char* __restrict__ tile) {
    uint4 v[NR];
    load_tile_regs(src, row0, pitch, col0, ncols, Tlen, v);
    write_tile_lds(tile, v);
}

// out[qb][st] = frag_regs(x[qb][2 st], x[qb][2 st + 1]): the packed fragments of every query block and k-step.  hipcc's schedule is
// sensitive to where this is written: the TT = 32 fp16 forward -- the headline's kernel -- keeps its instruction order only with this
// helper over the whole array, the TT = 64 forward only with the loop written in the kernel (see there); the backward kernels take either.
template <typename T16, int NB>
__device__ __forceinline__ void pack_frags(const f32x4_t (&x)[NB][NB], bf16x8_t (&out)[NB][NB / 2]) {
#pragma unroll
    for (int qb = 0; qb < NB; ++qb)
#pragma unroll
        for (int kb = 0; kb < NB; kb += 2) out[qb][kb / 2] = frag_regs<T16>(x[qb][kb], x[qb][kb + 1]);
}

// the lane's 4 NB key-padding flags (keys kb*16 + 4g + r), zero past T
template <int NB>
__device__ __forceinline__ void load_keep(const AttnMArgs& a, const float* keep_row, float (&keep)[NB][4]) {
    const int g = threadIdx.x >> 4;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // branch-free (clamped index, then select): a guarded load becomes its own basic block with an immediate
            // s_waitcnt vmcnt(0) -- eight serialised memory round trips per wavefront
            const int j = kb * 16 + 4 * g + r;
            const float v = keep_row[min(j, a.T - 1)];
            keep[kb][r] = (j < a.T) ? v : 0.f;
        }
}

// masked, scaled softmax (+ optional dropout mask out) of the lane's scores s[qb][kb][r]
template <int NB>
__device__ __forceinline__ void softmax_regs(f32x4_t (&s)[NB][NB], const AttnMArgs& a, const float (&keep)[NB][4]) {
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
        const int i = qb * 16 + c;
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = kb * 16 + 4 * g + r;
                const bool kept = (keep[kb][r] != 0.f) && (!a.causal || j <= i);
                const float v = s[qb][kb][r] * a.scale + (kept ? 0.f : a.mask_value);
                s[qb][kb][r] = (j < a.T) ? v : -INFINITY;
                m = fmaxf(m, s[qb][kb][r]);
            }
        m = rows4_max(m);
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = (kb * 16 + 4 * g + r < a.T) ? expf(s[qb][kb][r] - m) : 0.f;
                s[qb][kb][r] = e;
                sum += e;
            }
        sum = rows4_sum(sum);
        const float inv = (i < a.T) ? 1.0f / sum : 0.f;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[qb][kb][r] *= inv;
    }
}

// keep-mask scale of the lane's cells: element index ((tile * TT + query) * TT + key) -- the stream of the VALU kernels with the same
// tile edge (attention.hip)
template <int NB>
__device__ __forceinline__ void drop_mask_regs(const DropRng& d, uint64_t tile, float (&m)[NB][NB][4]) {
    constexpr int TT = 16 * NB;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int qb = 0; qb < NB; ++qb)
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
            bool kp[4];
            drop_keep_vec<4>(d, (tile * TT + (uint64_t)(qb * 16 + c)) * TT + (uint64_t)(kb * 16 + 4 * g), kp);   // even start
#pragma unroll
            for (int r = 0; r < 4; ++r) m[qb][kb][r] = kp[r] ? d.inv_keep : 0.f;
        }
}

// ctx[query][d0 .. d0 + 16 ND) = P_d V for the NB query blocks, NS k-steps over the keys; every lane writes 8 ND contiguous bytes of
// its row.  (The first MFMA of an accumulation takes the zero operand: `o = zero` followed by a loop over the k-steps is 26
// instructions and 8 registers more in the 32-row backward.)
template <typename T16, int NB, int ND>
__device__ __forceinline__ void fwd_pv(const AttnMArgs& a, const char* sV, const bf16x8_t (&pf)[NB][NB / 2], size_t row0, int H, int col0) {
    constexpr int NS = NB / 2;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    bf16x8_t vf[NS][ND];
#pragma unroll
    for (int st = 0; st < NS; ++st)
#pragma unroll
        for (int db = 0; db < ND; ++db) vf[st][db] = frag_tr_spread(sV + st * 32 * PITCH, PITCH, 4 * db, 4 * ND);
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
        f32x4_t o[ND];
#pragma unroll
        for (int db = 0; db < ND; ++db) {
            o[db] = h16<T16>::mma16(vf[0][db], pf[qb][0], zero);
            if constexpr (NS == 2) o[db] = h16<T16>::mma16(vf[1][db], pf[qb][1], o[db]);
        }
        const int q = qb * 16 + c;
        if (q < a.T) store_row_d<T16, ND>(a.ctx, row0 + q, H, col0 + 4 * ND * g, o);
    }
}

// dQ = dS K, dK = dS^T Q, dV = P_d^T dO for one head-width chunk of 16 ND columns (same d-contiguous output layout)
template <typename T16, int NB, int ND>
__device__ __forceinline__ void bwd_products(const AttnMArgs& a, const char* sQ, const char* sK, const char* sO,
                                             const bf16x8_t (&dsf)[NB][NB / 2], const bf16x8_t (&dsT)[NB][NB / 2], const bf16x8_t (&pT)[NB][NB / 2],
                                             size_t row0, int pitch, int H, int col0, int seq) {
    constexpr int NS = NB / 2;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    f32x4_t cq[ND], ck[ND], cv[ND];
#pragma unroll
    for (int db = 0; db < ND; ++db) { cq[db] = zero; ck[db] = zero; cv[db] = zero; }
    bf16x8_t kt[NS][ND], qt[NS][ND], ot[NS][ND];
#pragma unroll
    for (int st = 0; st < NS; ++st)
#pragma unroll
        for (int db = 0; db < ND; ++db) {
            kt[st][db] = frag_tr_spread(sK + st * 32 * PITCH, PITCH, 4 * db, 4 * ND);   // K [key slots][d]
            qt[st][db] = frag_tr_spread(sQ + st * 32 * PITCH, PITCH, 4 * db, 4 * ND);   // Q [query slots][d]
            ot[st][db] = frag_tr_spread(sO + st * 32 * PITCH, PITCH, 4 * db, 4 * ND);   // dO [query slots][d]
        }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int r = b * 16 + c;
        f32x4_t dq[ND], dk[ND], dv[ND];
#pragma unroll
        for (int db = 0; db < ND; ++db) {
            dq[db] = h16<T16>::mma16(kt[0][db], dsf[b][0], zero);      // dQ[query r][d] = sum_key dS[r][key] K[key][d]
            if constexpr (NS == 2) dq[db] = h16<T16>::mma16(kt[1][db], dsf[b][1], dq[db]);
            dk[db] = h16<T16>::mma16(qt[0][db], dsT[b][0], zero);      // dK[key r][d] = sum_query dS[query][r] Q[query][d]
            if constexpr (NS == 2) dk[db] = h16<T16>::mma16(qt[1][db], dsT[b][1], dk[db]);
            dv[db] = h16<T16>::mma16(ot[0][db], pT[b][0], zero);       // dV[key r][d] = sum_query P_d[query][r] dO[query][d]
            if constexpr (NS == 2) dv[db] = h16<T16>::mma16(ot[1][db], pT[b][1], dv[db]);
        }
        if (r < a.T) {
            const int dcol = col0 + 4 * ND * g;
            store_row_d<T16, ND>(a.dqkv, row0 + r, pitch, dcol, dq);
            store_row_d<T16, ND>(a.dqkv, row0 + r, pitch, H + dcol, dk);
            store_row_d<T16, ND>(a.dqkv, row0 + r, pitch, 2 * H + dcol, dv);
            if (a.csum) {
#pragma unroll
                for (int db = 0; db < ND; ++db)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {      // fp32 sums of the rows BEFORE their bf16 rounding (three VALU ops per value cheaper)
                        cq[db][e] += dq[db][e];
                        ck[db][e] += dk[db][e];
                        cv[db][e] += dv[db][e];
                    }
            }
        }
    }
    if (a.csum) {   // bias gradient of the fused projection: this (sequence, head)'s column sums, rows = the 16 lanes of a DPP row
#pragma unroll
        for (int db = 0; db < ND; ++db)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cq[db][e] = row16_sum(cq[db][e]);
                ck[db][e] = row16_sum(ck[db][e]);
                cv[db][e] = row16_sum(cv[db][e]);
            }
        if (c == 0) {
            float* w = a.csum + (size_t)seq * 3 * H + col0 + 4 * ND * g;
#pragma unroll
            for (int db = 0; db < ND; ++db) {
                *reinterpret_cast<float4*>(w + 4 * db) = make_float4(cq[db][0], cq[db][1], cq[db][2], cq[db][3]);
                *reinterpret_cast<float4*>(w + H + 4 * db) = make_float4(ck[db][0], ck[db][1], ck[db][2], ck[db][3]);
                *reinterpret_cast<float4*>(w + 2 * H + 4 * db) = make_float4(cv[db][0], cv[db][1], cv[db][2], cv[db][3]);
            }
        }
    }
}

template <typename T16, int TT>
__global__ __launch_bounds__(64) void attn_fwd_mfma_kernel(AttnMArgs a) {
    constexpr int NB = Geo<TT>::NB, NS = Geo<TT>::NS, NR = Geo<TT>::NR;
    if ((int)blockIdx.x >= a.n_seq * a.n_heads) {      // spare rows of a bucket-padded packed layout: ctx = 0 there
        zero_dead_rows(a.ctx, a.cu, a.n_seq, a.total_rows, (size_t)a.n_heads * a.dh * 2, (int)blockIdx.x - a.n_seq * a.n_heads);
        return;
    }
    a.drop = drop_resolve(a.drop);
    __shared__ __attribute__((aligned(16))) char sV[Geo<TT>::TILE];
    const int seq = blockIdx.x / a.n_heads, head = blockIdx.x % a.n_heads;
    const int H = a.n_heads * a.dh, pitch = 3 * H;
    const size_t row0 = a.cu ? (size_t)a.cu[seq] : (size_t)seq * a.T;
    if (a.cu) a.T = a.cu[seq + 1] - a.cu[seq];   // unpadded layout: this sequence's own length
    if (a.T <= 0) return;                         // nothing to read or write (and the clamped loads need a valid last row)
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    f32x4_t s[NB][NB];
#pragma unroll
    for (int qb = 0; qb < NB; ++qb)
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) s[qb][kb] = zero;
    const int nch = (a.dh + DCH - 1) / DCH;
    float keep[NB][4];
    load_keep(a, a.key_keep + row0, keep);
    if constexpr (TT == 32) {      // (NB == 2 here; the two-element aggregates below are the source form whose compiled code is the measured one)
        if (nch == 1) {
            // ONE memory round trip per wavefront: the V tile, the Q / K fragments of both k-steps and the padding flags are all
            // requested before the first of them is used (a missing second k-step, dh = 32, re-reads the first and is not multiplied)
            uint4 pv[NR];
            load_tile_regs(a.qkv, row0, pitch, 2 * H + head * a.dh, a.dh, a.T, pv);
            bf16x8_t qf[2][NB], kf[2][NB];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bool ok = ks * 32 < a.dh;
                const int dcol = head * a.dh + (ok ? ks * 32 : 0);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    qf[ks][b] = frag_nt_global(a.qkv, row0, pitch, dcol, b, a.T);
                    kf[ks][b] = frag_nt_global(a.qkv, row0, pitch, H + dcol, b, a.T);
                }
            }
            __builtin_amdgcn_sched_barrier(0);      // keep the whole load group ahead of the first use (the scheduler otherwise sinks the V loads)
            write_tile_lds(sV, pv);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks * 32 < a.dh) {
#pragma unroll
                    for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                        for (int kb = 0; kb < NB; ++kb) s[qb][kb] = h16<T16>::mma16(kf[ks][kb], qf[ks][qb], s[qb][kb]);
                }
            }
        } else {
            for (int d = 0; d < a.dh; d += 32) {     // one MFMA k-step per 32 head columns, operands straight from global memory
                const bf16x8_t qf[2] = {frag_nt_global(a.qkv, row0, pitch, head * a.dh + d, 0, a.T), frag_nt_global(a.qkv, row0, pitch, head * a.dh + d, 1, a.T)};
                const bf16x8_t kf[2] = {frag_nt_global(a.qkv, row0, pitch, H + head * a.dh + d, 0, a.T), frag_nt_global(a.qkv, row0, pitch, H + head * a.dh + d, 1, a.T)};
#pragma unroll
                for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                    for (int kb = 0; kb < NB; ++kb) s[qb][kb] = h16<T16>::mma16(kf[kb], qf[qb], s[qb][kb]);
            }
        }
    } else {
        uint4 pv[NR];
        if (nch == 1) load_tile_regs(a.qkv, row0, pitch, 2 * H + head * a.dh, a.dh, a.T, pv);      // the V tile rides with the first fragments
        for (int d = 0; d < a.dh; d += 32) {     // one MFMA k-step per 32 head columns, operands straight from global memory
            bf16x8_t qf[NB], kf[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                qf[b] = frag_nt_global(a.qkv, row0, pitch, head * a.dh + d, b, a.T);
                kf[b] = frag_nt_global(a.qkv, row0, pitch, H + head * a.dh + d, b, a.T);
            }
#pragma unroll
            for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                for (int kb = 0; kb < NB; ++kb) s[qb][kb] = h16<T16>::mma16(kf[kb], qf[qb], s[qb][kb]);
        }
        if (nch == 1) write_tile_lds(sV, pv);
    }
    __syncthreads();
    softmax_regs(s, a, keep);
    if (a.drop.thresh) {
        float m[NB][NB][4];
        drop_mask_regs(a.drop, blockIdx.x, m);
#pragma unroll
        for (int qb = 0; qb < NB; ++qb)
#pragma unroll
            for (int kb = 0; kb < NB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[qb][kb][r] *= m[qb][kb][r];
    }
    bf16x8_t pf[NB][NS];
    if constexpr (TT == 32) {
        pack_frags<T16>(s, pf);
    } else {      // the same packing written out: through the helper the compiler reschedules the whole softmax / dropout region of this kernel
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
            pf[qb][0] = frag_regs<T16>(s[qb][0], s[qb][1]);
            pf[qb][1] = frag_regs<T16>(s[qb][2], s[qb][3]);
        }
    }
    for (int ch = 0; ch < nch; ++ch) {
        const int d0 = ch * DCH, nc = min(DCH, a.dh - d0);
        if (nch > 1) {
            stage_tile<NR>(a.qkv, row0, pitch, 2 * H + head * a.dh + d0, nc, a.T, sV);
            __syncthreads();
        }
        if (nc == 64) fwd_pv<T16, NB, 4>(a, sV, pf, row0, H, head * a.dh + d0);
        else fwd_pv<T16, NB, 2>(a, sV, pf, row0, H, head * a.dh + d0);
        if (nch > 1) __syncthreads();
    }
}

template <typename T16, int TT>
__global__ __launch_bounds__(64) void attn_bwd_mfma_kernel(AttnMArgs a) {
    constexpr int NB = Geo<TT>::NB, NS = Geo<TT>::NS, NR = Geo<TT>::NR, PP = Geo<TT>::PP;
    if ((int)blockIdx.x >= a.n_seq * a.n_heads) {      // spare rows: dqkv = 0 there
        zero_dead_rows(a.dqkv, a.cu, a.n_seq, a.total_rows, (size_t)3 * a.n_heads * a.dh * 2, (int)blockIdx.x - a.n_seq * a.n_heads);
        return;
    }
    a.drop = drop_resolve(a.drop);
    __shared__ __attribute__((aligned(16))) char sQ[Geo<TT>::TILE];
    __shared__ __attribute__((aligned(16))) char sK[Geo<TT>::TILE];
    __shared__ __attribute__((aligned(16))) char sO[Geo<TT>::TILE];
    __shared__ __attribute__((aligned(16))) char sP[TT * PP];    // dropped probabilities  [query][key] 16-bit
    __shared__ __attribute__((aligned(16))) char sS[TT * PP];    // dS                     [query][key] 16-bit
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int seq = blockIdx.x / a.n_heads, head = blockIdx.x % a.n_heads;
    const int H = a.n_heads * a.dh, pitch = 3 * H;
    const size_t row0 = a.cu ? (size_t)a.cu[seq] : (size_t)seq * a.T;
    if (a.cu) a.T = a.cu[seq + 1] - a.cu[seq];   // unpadded layout: this sequence's own length
    if (a.T <= 0) {                               // nothing to read or write (and the clamped loads need a valid last row)
        if (a.csum)
            for (int j = lane; j < 3 * a.dh; j += 64) a.csum[(size_t)seq * 3 * H + (j / a.dh) * H + head * a.dh + j % a.dh] = 0.f;
        return;
    }
    const bf16* dctx = a.ctx;
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    f32x4_t s[NB][NB], dp[NB][NB];
#pragma unroll
    for (int qb = 0; qb < NB; ++qb)
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) { s[qb][kb] = zero; dp[qb][kb] = zero; }
    const int nch = (a.dh + DCH - 1) / DCH;
    float keep[NB][4];
    load_keep(a, a.key_keep + row0, keep);
    if constexpr (TT == 32) {      // (NB == 2 here, as in the forward kernel)
        if (nch == 1) {
            // ONE memory round trip: the Q / K / dO tiles, the V fragments of both k-steps and the padding flags are requested together
            uint4 pq[NR], pk[NR], po[NR];
            load_tile_regs(a.qkv, row0, pitch, head * a.dh, a.dh, a.T, pq);
            load_tile_regs(a.qkv, row0, pitch, H + head * a.dh, a.dh, a.T, pk);
            load_tile_regs(dctx, row0, H, head * a.dh, a.dh, a.T, po);
            bf16x8_t vf[2][NB];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bool ok = ks * 32 < a.dh;
                const int vcol = 2 * H + head * a.dh + (ok ? ks * 32 : 0);
#pragma unroll
                for (int b = 0; b < NB; ++b) vf[ks][b] = frag_nt_global(a.qkv, row0, pitch, vcol, b, a.T);
            }
            __builtin_amdgcn_sched_barrier(0);
            write_tile_lds(sQ, pq);
            write_tile_lds(sK, pk);
            write_tile_lds(sO, po);
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks * 32 < a.dh) {
                    const bf16x8_t qf[2] = {frag_nt(sQ, 0, ks), frag_nt(sQ, 1, ks)};
                    const bf16x8_t kf[2] = {frag_nt(sK, 0, ks), frag_nt(sK, 1, ks)};
                    const bf16x8_t of[2] = {frag_nt(sO, 0, ks), frag_nt(sO, 1, ks)};
#pragma unroll
                    for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                        for (int kb = 0; kb < NB; ++kb) {
                            s[qb][kb] = h16<T16>::mma16(kf[kb], qf[qb], s[qb][kb]);
                            dp[qb][kb] = h16<T16>::mma16(vf[ks][kb], of[qb], dp[qb][kb]);
                        }
                }
            }
        }
        for (int ch = 0; nch > 1 && ch < nch; ++ch) {
            const int d0 = ch * DCH, nc = min(DCH, a.dh - d0);
            stage_tile<NR>(a.qkv, row0, pitch, head * a.dh + d0, nc, a.T, sQ);
            stage_tile<NR>(a.qkv, row0, pitch, H + head * a.dh + d0, nc, a.T, sK);
            stage_tile<NR>(dctx, row0, H, head * a.dh + d0, nc, a.T, sO);
            __syncthreads();
            for (int ks = 0; ks < nc / 32; ++ks) {
                bf16x8_t qf[2] = {frag_nt(sQ, 0, ks), frag_nt(sQ, 1, ks)};
                bf16x8_t kf[2] = {frag_nt(sK, 0, ks), frag_nt(sK, 1, ks)};
                const int vcol = 2 * H + head * a.dh + d0 + ks * 32;     // V is only consumed d-contiguous: no LDS tile
                bf16x8_t vf[2] = {frag_nt_global(a.qkv, row0, pitch, vcol, 0, a.T), frag_nt_global(a.qkv, row0, pitch, vcol, 1, a.T)};
                bf16x8_t of[2] = {frag_nt(sO, 0, ks), frag_nt(sO, 1, ks)};
#pragma unroll
                for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                    for (int kb = 0; kb < NB; ++kb) {
                        s[qb][kb] = h16<T16>::mma16(kf[kb], qf[qb], s[qb][kb]);
                        dp[qb][kb] = h16<T16>::mma16(vf[kb], of[qb], dp[qb][kb]);
                    }
            }
            if (nch > 1) __syncthreads();
        }
    } else {
        for (int ch = 0; ch < nch; ++ch) {
            const int d0 = ch * DCH, nc = min(DCH, a.dh - d0);
            if (ch > 0) __syncthreads();
            {   // all global loads of the chunk before the first LDS write
                uint4 pq[NR], pk[NR], po[NR];
                load_tile_regs(a.qkv, row0, pitch, head * a.dh + d0, nc, a.T, pq);
                load_tile_regs(a.qkv, row0, pitch, H + head * a.dh + d0, nc, a.T, pk);
                load_tile_regs(dctx, row0, H, head * a.dh + d0, nc, a.T, po);
                __builtin_amdgcn_sched_barrier(0);
                write_tile_lds(sQ, pq);
                write_tile_lds(sK, pk);
                write_tile_lds(sO, po);
            }
            __syncthreads();
            for (int ks = 0; ks < nc / 32; ++ks) {
                const int vcol = 2 * H + head * a.dh + d0 + ks * 32;     // V is only consumed d-contiguous: no LDS tile
                bf16x8_t qf[NB], kf[NB], of[NB], vf[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    vf[b] = frag_nt_global(a.qkv, row0, pitch, vcol, b, a.T);
                    qf[b] = frag_nt(sQ, b, ks);
                    kf[b] = frag_nt(sK, b, ks);
                    of[b] = frag_nt(sO, b, ks);
                }
#pragma unroll
                for (int qb = 0; qb < NB; ++qb)
#pragma unroll
                    for (int kb = 0; kb < NB; ++kb) {
                        s[qb][kb] = h16<T16>::mma16(kf[kb], qf[qb], s[qb][kb]);
                        dp[qb][kb] = h16<T16>::mma16(vf[kb], of[qb], dp[qb][kb]);
                    }
            }
        }
    }
    softmax_regs(s, a, keep);
    float msk[NB][NB][4];
    if (a.drop.thresh) drop_mask_regs(a.drop, blockIdx.x, msk);
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
        float delta = 0.f;
#pragma unroll
        for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (a.drop.thresh) dp[qb][kb][r] *= msk[qb][kb][r];     // dP = dP_dropped o mask / (1 - p)
                delta += s[qb][kb][r] * dp[qb][kb][r];
            }
        delta = rows4_sum(delta);
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dp[qb][kb][r] = s[qb][kb][r] * (dp[qb][kb][r] - delta) * a.scale;   // dS
                if (a.drop.thresh) s[qb][kb][r] *= msk[qb][kb][r];                  // dV takes the dropped probabilities
            }
            const int q = qb * 16 + c, k0 = kb * 16 + 4 * g;
            *reinterpret_cast<uint2*>(sP + q * PP + k0 * 2) = make_uint2(h16<T16>::pack2(s[qb][kb][0], s[qb][kb][1]), h16<T16>::pack2(s[qb][kb][2], s[qb][kb][3]));
            *reinterpret_cast<uint2*>(sS + q * PP + k0 * 2) = make_uint2(h16<T16>::pack2(dp[qb][kb][0], dp[qb][kb][1]), h16<T16>::pack2(dp[qb][kb][2], dp[qb][kb][3]));
        }
    }
    bf16x8_t dsf[NB][NS];
    pack_frags<T16>(dp, dsf);
    __syncthreads();
    // transposed [key block][query slots] fragments of dS and P: NS k-steps over the queries
    bf16x8_t dsT[NB][NS], pT[NB][NS];
#pragma unroll
    for (int kb = 0; kb < NB; ++kb)
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            dsT[kb][st] = frag_tr(sS + st * 32 * PP, PP, kb * 16);
            pT[kb][st] = frag_tr(sP + st * 32 * PP, PP, kb * 16);
        }
    for (int ch = 0; ch < nch; ++ch) {
        const int d0 = ch * DCH, nc = min(DCH, a.dh - d0);
        if (nch > 1) {      // (one chunk: the tiles of the score phase are still in place)
            __syncthreads();
            stage_tile<NR>(a.qkv, row0, pitch, head * a.dh + d0, nc, a.T, sQ);
            stage_tile<NR>(a.qkv, row0, pitch, H + head * a.dh + d0, nc, a.T, sK);
            stage_tile<NR>(dctx, row0, H, head * a.dh + d0, nc, a.T, sO);
            __syncthreads();
        }
        if (nc == 64) bwd_products<T16, NB, 4>(a, sQ, sK, sO, dsf, dsT, pT, row0, pitch, H, head * a.dh + d0, seq);
        else bwd_products<T16, NB, 2>(a, sQ, sK, sO, dsf, dsT, pT, row0, pitch, H, head * a.dh + d0, seq);
    }
}

}  // namespace

int attn_spare_blocks(const morec_attn_desc* d);      // attention.hip
// MOREC_OK or an error; MOREC_E_UNSUPPORTED = the shape is outside this path (the caller goes on to the next: attention.hip)
int morec_attn_mfma_launch(const morec_attn_desc* d, const void* qkv, const float* key_keep, void* ctx_or_dctx,
                           void* dqkv, bool backward, hipStream_t s, float* csum) {
    if (!is_h16(d->dtype) || d->dh % 32 != 0 || d->T > 64) return MOREC_E_UNSUPPORTED;
    const bool wide = d->T > 32;      // the 64 x 64 tile
    if (wide && !tuning().attn_mfma64) return MOREC_E_UNSUPPORTED;
    AttnMArgs a{reinterpret_cast<const bf16*>(qkv), key_keep, reinterpret_cast<bf16*>(ctx_or_dctx),
                reinterpret_cast<bf16*>(dqkv), csum, d->n_seq, d->T, d->n_heads, d->dh, d->causal, d->scale, d->mask_value,
                make_drop(d->p_drop, d->seed), d->cu_seqlens, d->total_rows};
    dim3 grid(d->n_seq * d->n_heads + attn_spare_blocks(d)), block(64);
    by_h16(d->dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        if (wide) {
            if (backward) hipLaunchKernelGGL((attn_bwd_mfma_kernel<T, 64>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((attn_fwd_mfma_kernel<T, 64>), grid, block, 0, s, a);
        } else {
            if (backward) hipLaunchKernelGGL((attn_bwd_mfma_kernel<T, 32>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((attn_fwd_mfma_kernel<T, 32>), grid, block, 0, s, a);
        }
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
