// attention_stream.hip -- attention for sequences of up to 1024 positions: the keys are walked in tiles and no kernel ever holds a full
// score row (the row-strip kernels of attention.hip keep a [32 x T] fp32 strip in LDS and end at T = 256).
//
// Same contract as attention.hip: packed qkv[M, 3H], key_keep by row, cu_seqlens / total_rows / spare rows, counter-based dropout with the
// element index ((seq * n_heads + head) * TPD + i) * TPD + j, TPD = 32 * ceil(T / 32) from the DESCRIPTOR's T; no forward state is kept, the
// backward recomputes.  One workgroup per (sequence, head) writes every output element of that pair exactly once: no atomics, no global
// scratch, nothing handed between workgroups, the same bits on every call.
//
// The additive mask is reproduced literally: score = (q.k) * scale + (kept ? 0 : mask_value) in fp32, keys >= L_s never enter.  A query row
// without a kept key is therefore a softmax over ALL L_s keys (with `causal`: keys j > i included), so no key tile is skipped.  The running
// maximum starts at -inf and is finite after the first key tile (key 0 is always a key); the accumulators are rescaled by
// exp(m_old - m_new) at every tile, never behind a threshold.
//
// Two families:
//   stream16  -- 16-bit storage, dh % 32 == 0, dh <= 256: 4 wavefronts per (sequence, head); all five products on
//                v_mfma_f32_16x16x32_{bf16,f16} with the fragments of attention_frag.hpp.  Forward / statistics / dQ pass: a wavefront owns
//                16 query rows per round of 64 and the [64 keys x dh] K and V tiles are shared through LDS; dK / dV pass: a wavefront owns
//                16 keys and the Q / dO tiles are shared.  m, 1 / l and delta of all rows sit in LDS between the backward passes.
//                P~ = exp(s - m) and dS are rounded to the storage type before the products that consume them.
//   streamgen -- everything else (fp32 storage, other head widths): one wavefront per (sequence, head), fp32 arithmetic on the 4 x 4
//                register blocks of attention_valu.hpp: the row-strip kernels' phases with the strip cut into 32-key tiles.  Correctness
//                first: the forward runs a statistics pass and then recomputes the score tiles once per 64-column chunk of the head width.
//
// Both families also exist with a per-head additive position bias (BIAS = true, morec_attn_bias_fwd / _bwd; see StreamArgs below); only
// those hand anything to another kernel: the row statistics, in the caller's workspace, for the bias-gradient pass at the end of the file.
#include <stdio.h>
#include <stdlib.h>
#include "common.hpp"
#include "attention_valu.hpp"
#include "attention_frag.hpp"

namespace {
constexpr int ST_MAX = 1024;                 // longest sequence (check_desc in attention.hip)
constexpr int SKT = 64;                      // stream16: rows of a shared LDS tile = queries of a round = keys of a key tile
constexpr int S16_FIXED = 4 * ST_MAX * 4;    // stream16 LDS ahead of the tiles: key flags, m, 1 / l, delta (fp32, ST_MAX each)

// The reference's score, literally: the product with `scale` is rounded to fp32 BEFORE the mask is added (no fused multiply-add).  With
// mask_value = -10000 the sum lands on a grid of 2^-10, and a fully masked row is a softmax over those rounded values: one rounding
// fewer moves single probabilities of such a row by a factor exp(2^-10).
__device__ __forceinline__ float masked_score(float s, float scale, float add) {
#pragma clang fp contract(off)
    const float t = s * scale;
    return t + add;
}

// The position-bias variants (morec_attn_bias_fwd / _bwd, the BEiT tower): BIAS = true instantiations of the same kernels.  The bias is
// fp32 [heads][T][Tp], Tp = 64 ceil(T / 64) (rows padded to the key-tile width, pad cells zero), the same for every sequence, and is added
// in fp32 AFTER the mask.  A lane reads the cells of its own scores straight from global memory (the table of a layer stays in cache):
// rows are clamped to the sequence, columns stay below Tp by the layout, and a cell past the sequence only ever meets a score that is
// already -inf.  BIAS = false is the code it was: StreamArgs<false> is AttnArgs, no pointer is read and the LDS plan is untouched.
template <bool BIAS>
struct StreamArgs : AttnArgs {};
template <>
struct StreamArgs<true> : AttnArgs {
    const float* bias;      // [heads][T][Tp]
    float* stats;           // backward: m, 1 / l, delta of every query row, [n_seq * heads][3][T], for the bias-gradient pass; or nullptr
    int Tp;
};
constexpr int BIAS_NCH = 8;      // the bias-gradient pass folds the sequences in this many chunks, in chunk order

// ---------------------------------------------------------------------------------------------------------------------------------------
// stream16
// ---------------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int s16_pitch(int dh) { return dh * 2 + 32; }      // bytes per tile row: pitch / 32 odd (dh % 32 == 0)
inline size_t s16_lds(int dh) { return (size_t)S16_FIXED + 2 * SKT * s16_pitch(dh); }

// rows [base, base + 64) x columns [col, col + dh) of a row-major global matrix -> LDS tile, by the 256 threads of the workgroup; rows past
// the sequence repeat its last row (clamped, never guarded: attention_frag.hpp).  All loads are issued before the first LDS write.
// NC = 32-column chunks the instantiation is built for (dh <= 32 NC): thread t moves the 16-byte vectors t, t + 256, ...
template <int NC>
__device__ __forceinline__ void s16_stage(const bf16* __restrict__ src, size_t row0, int pitch, int col, int dh, int base, int L,
                                          char* __restrict__ tile) {
    const int vpr = dh >> 3, pb = s16_pitch(dh);
    uint4 v[NC];
    int off[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int idx = threadIdx.x + i * 256;
        const int r = min(idx / vpr, SKT - 1), sv = idx % vpr;
        v[i] = load16(src + (row0 + min(base + r, L - 1)) * (size_t)pitch + col + sv * 8);
        off[i] = r * pb + sv * 16;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i)
        if (i * 32 < dh) *reinterpret_cast<uint4*>(tile + off[i]) = v[i];
}

// the lane's NT fragments (one per 32-column chunk) of row `row` (clamped to the sequence) straight from global memory
template <int NC>
__device__ __forceinline__ void s16_row_frags(const bf16* __restrict__ src, size_t row0, int pitch, int col, int dh, int row, int L, int g,
                                              bf16x8_t (&f)[NC]) {
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        const uint4 v = load16(src + (row0 + min(row, L - 1)) * (size_t)pitch + col + (ch * 32 < dh ? ch * 32 : 0) + g * 8);
        f[ch] = __builtin_bit_cast(bf16x8_t, v);
    }
}

// x[b] = sum_d tile[row b*16 + 4g + r][d] * f[lane's row][d] for the four 16-row blocks of a shared tile: the lane ends up with
// x[b][r] = <its own row c, tile row b*16 + 4g + r>
template <typename T16, int NC>
__device__ __forceinline__ void s16_dots(const char* tile, int pb, int nch, int lane, const bf16x8_t (&f)[NC], f32x4_t (&x)[4]) {
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 4; ++b) x[b] = zero;
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
        if (ch < nch) {
#pragma unroll
            for (int b = 0; b < 4; ++b) x[b] = h16<T16>::mma16(frag_nt_pitch(tile, pb, b, ch, lane), f[ch], x[b]);
        }
}

// acc[ch][db] += sum over the 64 rows of a shared tile of w[row] * tile[row][32 ch + 8 g + 4 db + e]: w0 / w1 are the register fragments of
// the two 32-row k-steps (frag_regs), the lane's own row is the output row
template <typename T16, int NC>
__device__ __forceinline__ void s16_accum(const char* tile, int pb, int nch, int lane, const bf16x8_t& w0, const bf16x8_t& w1,
                                          f32x4_t (&acc)[NC][2]) {
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
        if (ch < nch) {
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                acc[ch][db] = h16<T16>::mma16(frag_tr_spread_lane(tile, pb, ch * 32 + 4 * db, 8, lane), w0, acc[ch][db]);
                acc[ch][db] = h16<T16>::mma16(frag_tr_spread_lane(tile + 32 * pb, pb, ch * 32 + 4 * db, 8, lane), w1, acc[ch][db]);
            }
        }
}

template <typename T16, int NC>
__device__ __forceinline__ void s16_store(bf16* dst, size_t row, int pitch, int col, int nch, int g, const f32x4_t (&acc)[NC][2]) {
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
        if (ch < nch) store_row_d<T16, 2>(dst, row, pitch, col + ch * 32 + 8 * g, acc[ch]);
}

struct S16Seq {
    size_t row0;
    int L, TPD, head, nkt;
    uint64_t tile;      // (sequence, head) index of the dropout stream
};
// false: nothing to do for this block (spare-row block, or a sequence of length 0)
__device__ __forceinline__ bool s16_enter(AttnArgs& a, void* out, size_t out_rowbytes, S16Seq& q) {
    if ((int)blockIdx.x >= a.n_seq * a.n_heads) {
        zero_dead_rows(out, a.cu, a.n_seq, a.total_rows, out_rowbytes, (int)blockIdx.x - a.n_seq * a.n_heads);
        return false;
    }
    a.drop = drop_resolve(a.drop);
    const int seq = blockIdx.x / a.n_heads;
    q.head = blockIdx.x % a.n_heads;
    q.row0 = a.cu ? (size_t)a.cu[seq] : (size_t)seq * a.T;
    q.TPD = ((a.T + 31) / 32) * 32;
    q.L = a.cu ? a.cu[seq + 1] - a.cu[seq] : a.T;
    q.nkt = (q.L + SKT - 1) / SKT;
    q.tile = blockIdx.x;
    return q.L > 0;
}
// key flags of the sequence into LDS, zero past its length (clamped index, then select)
__device__ __forceinline__ void s16_keep(const AttnArgs& a, const S16Seq& q, float* sKeep) {
    for (int j = threadIdx.x; j < q.nkt * SKT; j += 256) {
        const float v = a.key_keep[q.row0 + min(j, q.L - 1)];
        sKeep[j] = j < q.L ? v : 0.f;
    }
}

// masked scaled scores of the lane's query row i against the keys j = jb + kb*16 + 4g + r of one key tile (-inf past the sequence)
__device__ __forceinline__ void s16_mask(f32x4_t (&s)[4], const AttnArgs& a, const float* sKeep, int i, int jb, int g, int L) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = jb + kb * 16 + 4 * g + r;
            const bool kept = (sKeep[j] != 0.f) && (!a.causal || j <= i);
            const float v = masked_score(s[kb][r], a.scale, kept ? 0.f : a.mask_value);
            s[kb][r] = (j < L) ? v : -INFINITY;
        }
}
// the bias cells of the same scores: row i (clamped by the caller) of one head's table, 16 bytes per 16-key block
__device__ __forceinline__ void s16_bias_load(const float* __restrict__ brow, int jb, int g, f32x4_t (&b)[4]) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) b[kb] = *reinterpret_cast<const f32x4_t*>(brow + jb + kb * 16 + 4 * g);
}
// the same for a transposed tile: the lane's row is key j, its cells are the queries i = ib + qb*16 + 4g + r (clamped to the sequence)
__device__ __forceinline__ void s16_bias_load_t(const float* __restrict__ bhead, int Tp, int j, int ib, int g, int L, f32x4_t (&b)[4]) {
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
        for (int r = 0; r < 4; ++r) b[qb][r] = bhead[(size_t)min(ib + qb * 16 + 4 * g + r, L - 1) * Tp + j];
}
__device__ __forceinline__ void s16_bias_add(f32x4_t (&s)[4], const f32x4_t (&b)[4]) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) s[kb] += b[kb];
}
// dropout factors (0 or 1 / (1 - p)) of the same cells
__device__ __forceinline__ void s16_drop(const AttnArgs& a, const S16Seq& q, int i, int jb, int g, float (&ks)[4][4]) {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        bool kp[4];
        drop_keep_vec<4>(a.drop, (q.tile * (uint64_t)q.TPD + (uint64_t)i) * (uint64_t)q.TPD + (uint64_t)(jb + kb * 16 + 4 * g), kp);   // even start
#pragma unroll
        for (int r = 0; r < 4; ++r) ks[kb][r] = kp[r] ? a.drop.inv_keep : 0.f;
    }
}

template <typename T16, int NC, bool BIAS>
__global__ __launch_bounds__(256) void attn_fwd_stream16_kernel(StreamArgs<BIAS> a) {
    S16Seq q;
    if (!s16_enter(a, a.ctx, (size_t)a.n_heads * a.dh * 2, q)) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sKeep = reinterpret_cast<float*>(smem);
    const int pb = s16_pitch(a.dh), nch = a.dh / 32;
    char* sK = smem + S16_FIXED;
    char* sV = sK + SKT * pb;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int H = a.n_heads * a.dh, pitch = 3 * H, L = q.L;
    const bf16* qkv = reinterpret_cast<const bf16*>(a.qkv);
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    s16_keep(a, q, sKeep);
    for (int rd = 0; rd < q.nkt; ++rd) {
        const int i = rd * SKT + wave * 16 + c;      // the lane's query row
        bf16x8_t qf[NC];
        s16_row_frags<NC>(qkv, q.row0, pitch, q.head * a.dh, a.dh, i, L, g, qf);
        f32x4_t o[NC][2];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) { o[ch][0] = zero; o[ch][1] = zero; }
        float m = -INFINITY, l = 0.f;
        for (int kt = 0; kt < q.nkt; ++kt) {
            __syncthreads();      // the tiles of the previous step are consumed (first step: the key flags are written)
            s16_stage<NC>(qkv, q.row0, pitch, H + q.head * a.dh, a.dh, kt * SKT, L, sK);
            s16_stage<NC>(qkv, q.row0, pitch, 2 * H + q.head * a.dh, a.dh, kt * SKT, L, sV);
            __syncthreads();
            f32x4_t s[4];
            [[maybe_unused]] f32x4_t bz[4];
            if constexpr (BIAS) s16_bias_load(a.bias + ((size_t)q.head * a.T + min(i, L - 1)) * a.Tp, kt * SKT, g, bz);
            s16_dots<T16, NC>(sK, pb, nch, lane, qf, s);
            s16_mask(s, a, sKeep, i, kt * SKT, g, L);
            if constexpr (BIAS) s16_bias_add(s, bz);
            float mt = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[kb][r]);
            const float mn = fmaxf(m, rows4_max(mt));      // finite: the first tile holds key 0
            const float alpha = expf(m - mn);
            float ps = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[kb][r] = expf(s[kb][r] - mn);
                    ps += s[kb][r];
                }
            l = l * alpha + rows4_sum(ps);
            m = mn;
            if (a.drop.thresh) {
                float ks[4][4];
                s16_drop(a, q, i, kt * SKT, g, ks);
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[kb][r] *= ks[kb][r];
            }
#pragma unroll
            for (int ch = 0; ch < NC; ++ch)
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[ch][db][e] *= alpha;
            s16_accum<T16, NC>(sV, pb, nch, lane, frag_regs<T16>(s[0], s[1]), frag_regs<T16>(s[2], s[3]), o);
        }
        if (i < L) {
            const float inv = 1.0f / l;
#pragma unroll
            for (int ch = 0; ch < NC; ++ch)
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[ch][db][e] *= inv;
            s16_store<T16, NC>(reinterpret_cast<bf16*>(a.ctx), q.row0 + i, H, q.head * a.dh, nch, g, o);
        }
    }
}

// Backward: (A) m, 1 / l, delta = rowsum(P o dP) of every query row into LDS, delta accumulated next to l with the same rescaling;
// (B) dQ per query round; (C) dK, dV per key round, the score tiles computed transposed (the lane's row is its key).
template <typename T16, int NC, bool BIAS>
__global__ __launch_bounds__(256) void attn_bwd_stream16_kernel(StreamArgs<BIAS> a) {
    S16Seq q;
    if (!s16_enter(a, a.dqkv, (size_t)3 * a.n_heads * a.dh * 2, q)) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sKeep = reinterpret_cast<float*>(smem);
    float* st_m = sKeep + ST_MAX;
    float* st_i = st_m + ST_MAX;
    float* st_d = st_i + ST_MAX;
    const int pb = s16_pitch(a.dh), nch = a.dh / 32;
    char* sA = smem + S16_FIXED;      // K (passes A, B) | Q (pass C)
    char* sB = sA + SKT * pb;         // V               | dO
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int H = a.n_heads * a.dh, pitch = 3 * H, L = q.L;
    const bf16* qkv = reinterpret_cast<const bf16*>(a.qkv);
    const bf16* dctx = reinterpret_cast<const bf16*>(a.ctx);
    bf16* dqkv = reinterpret_cast<bf16*>(a.dqkv);
    const int colQ = q.head * a.dh, colK = H + colQ, colV = 2 * H + colQ;
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
    s16_keep(a, q, sKeep);
    // ---- pass A
    for (int rd = 0; rd < q.nkt; ++rd) {
        const int i = rd * SKT + wave * 16 + c;
        bf16x8_t qf[NC], of[NC];
        s16_row_frags<NC>(qkv, q.row0, pitch, colQ, a.dh, i, L, g, qf);
        s16_row_frags<NC>(dctx, q.row0, H, colQ, a.dh, i, L, g, of);
        float m = -INFINITY, l = 0.f, dl = 0.f;
        for (int kt = 0; kt < q.nkt; ++kt) {
            __syncthreads();
            s16_stage<NC>(qkv, q.row0, pitch, colK, a.dh, kt * SKT, L, sA);
            s16_stage<NC>(qkv, q.row0, pitch, colV, a.dh, kt * SKT, L, sB);
            __syncthreads();
            f32x4_t s[4], dp[4];
            [[maybe_unused]] f32x4_t bz[4];
            if constexpr (BIAS) s16_bias_load(a.bias + ((size_t)q.head * a.T + min(i, L - 1)) * a.Tp, kt * SKT, g, bz);
            s16_dots<T16, NC>(sA, pb, nch, lane, qf, s);
            s16_dots<T16, NC>(sB, pb, nch, lane, of, dp);
            s16_mask(s, a, sKeep, i, kt * SKT, g, L);
            if constexpr (BIAS) s16_bias_add(s, bz);
            if (a.drop.thresh) {
                float ks[4][4];
                s16_drop(a, q, i, kt * SKT, g, ks);
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dp[kb][r] *= ks[kb][r];      // dP = dP_dropped o mask / (1 - p)
            }
            float mt = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[kb][r]);
            const float mn = fmaxf(m, rows4_max(mt));
            const float alpha = expf(m - mn);
            float ps = 0.f, ds = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = expf(s[kb][r] - mn);
                    ps += e;
                    ds += e * dp[kb][r];
                }
            l = l * alpha + rows4_sum(ps);
            dl = dl * alpha + rows4_sum(ds);
            m = mn;
        }
        const float inv = (i < L) ? 1.0f / l : 0.f;      // rows past the sequence contribute nothing to dK / dV
        if (g == 0) { st_m[i] = m; st_i[i] = inv; st_d[i] = dl * inv; }
    }
    if constexpr (BIAS) {
        if (a.stats) {      // the row statistics leave for the bias-gradient pass
            __syncthreads();
            float* st = a.stats + (size_t)blockIdx.x * 3 * a.T;
            for (int i = threadIdx.x; i < L; i += 256) { st[i] = st_m[i]; st[a.T + i] = st_i[i]; st[2 * a.T + i] = st_d[i]; }
        }
    }
    // ---- pass B: dQ
    for (int rd = 0; rd < q.nkt; ++rd) {
        const int i = rd * SKT + wave * 16 + c;
        bf16x8_t qf[NC], of[NC];
        s16_row_frags<NC>(qkv, q.row0, pitch, colQ, a.dh, i, L, g, qf);
        s16_row_frags<NC>(dctx, q.row0, H, colQ, a.dh, i, L, g, of);
        f32x4_t dq[NC][2];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) { dq[ch][0] = zero; dq[ch][1] = zero; }
        float m = 0.f, inv = 0.f, delta = 0.f;
        for (int kt = 0; kt < q.nkt; ++kt) {
            __syncthreads();      // (first step of the first round: the statistics of pass A are written)
            s16_stage<NC>(qkv, q.row0, pitch, colK, a.dh, kt * SKT, L, sA);
            s16_stage<NC>(qkv, q.row0, pitch, colV, a.dh, kt * SKT, L, sB);
            __syncthreads();
            if (kt == 0) { m = st_m[i]; inv = st_i[i]; delta = st_d[i]; }
            f32x4_t s[4], dp[4];
            [[maybe_unused]] f32x4_t bz[4];
            if constexpr (BIAS) s16_bias_load(a.bias + ((size_t)q.head * a.T + min(i, L - 1)) * a.Tp, kt * SKT, g, bz);
            s16_dots<T16, NC>(sA, pb, nch, lane, qf, s);
            s16_dots<T16, NC>(sB, pb, nch, lane, of, dp);
            s16_mask(s, a, sKeep, i, kt * SKT, g, L);
            if constexpr (BIAS) s16_bias_add(s, bz);
            float ks[4][4];
            if (a.drop.thresh) s16_drop(a, q, i, kt * SKT, g, ks);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[kb][r] - m) * inv;
                    const float d = a.drop.thresh ? dp[kb][r] * ks[kb][r] : dp[kb][r];
                    s[kb][r] = p * (d - delta) * a.scale;      // dS
                }
            s16_accum<T16, NC>(sA, pb, nch, lane, frag_regs<T16>(s[0], s[1]), frag_regs<T16>(s[2], s[3]), dq);
        }
        if (i < L) s16_store<T16, NC>(dqkv, q.row0 + i, pitch, colQ, nch, g, dq);
    }
    // ---- pass C: dK, dV
    for (int rd = 0; rd < q.nkt; ++rd) {
        const int j = rd * SKT + wave * 16 + c;      // the lane's key
        bf16x8_t kf[NC], vf[NC];
        s16_row_frags<NC>(qkv, q.row0, pitch, colK, a.dh, j, L, g, kf);
        s16_row_frags<NC>(qkv, q.row0, pitch, colV, a.dh, j, L, g, vf);
        f32x4_t dk[NC][2], dv[NC][2];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) { dk[ch][0] = zero; dk[ch][1] = zero; dv[ch][0] = zero; dv[ch][1] = zero; }
        const bool jkeep = sKeep[j] != 0.f;
        for (int qt = 0; qt < q.nkt; ++qt) {
            __syncthreads();
            s16_stage<NC>(qkv, q.row0, pitch, colQ, a.dh, qt * SKT, L, sA);
            s16_stage<NC>(dctx, q.row0, H, colQ, a.dh, qt * SKT, L, sB);
            __syncthreads();
            f32x4_t s[4], dp[4];      // [key = the lane's j][query = qt*64 + qb*16 + 4g + r]
            [[maybe_unused]] f32x4_t bz[4];
            if constexpr (BIAS) s16_bias_load_t(a.bias + (size_t)q.head * a.T * a.Tp, a.Tp, j, qt * SKT, g, L, bz);
            s16_dots<T16, NC>(sA, pb, nch, lane, kf, s);
            s16_dots<T16, NC>(sB, pb, nch, lane, vf, dp);
#pragma unroll
            for (int qb = 0; qb < 4; ++qb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = qt * SKT + qb * 16 + 4 * g + r;
                    const bool kept = jkeep && (!a.causal || j <= i);
                    float v = masked_score(s[qb][r], a.scale, kept ? 0.f : a.mask_value);
                    if constexpr (BIAS) v += bz[qb][r];
                    const float p = (j < L) ? expf(v - st_m[i]) * st_i[i] : 0.f;      // st_i = 0 for query rows past the sequence
                    float ksc = 1.f;
                    if (a.drop.thresh)
                        ksc = drop_keep(a.drop, (q.tile * (uint64_t)q.TPD + (uint64_t)i) * (uint64_t)q.TPD + (uint64_t)j) ? a.drop.inv_keep : 0.f;
                    s[qb][r] = p * (dp[qb][r] * ksc - st_d[i]) * a.scale;      // dS
                    dp[qb][r] = p * ksc;                                       // dV takes the DROPPED probabilities
                }
            s16_accum<T16, NC>(sA, pb, nch, lane, frag_regs<T16>(s[0], s[1]), frag_regs<T16>(s[2], s[3]), dk);
            s16_accum<T16, NC>(sB, pb, nch, lane, frag_regs<T16>(dp[0], dp[1]), frag_regs<T16>(dp[2], dp[3]), dv);
        }
        if (j < L) {
            s16_store<T16, NC>(dqkv, q.row0 + j, pitch, colK, nch, g, dk);
            s16_store<T16, NC>(dqkv, q.row0 + j, pitch, colV, nch, g, dv);
        }
    }
}

template <typename T16, int NC, bool BIAS>
void s16_launch(bool backward, const StreamArgs<BIAS>& a, dim3 grid, size_t lds, hipStream_t s) {
    // the tiles of a 256-wide head pass the 64 KB a kernel gets without asking
    static const hipError_t rc_f = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_stream16_kernel<T16, NC, BIAS>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)s16_lds(32 * NC));
    static const hipError_t rc_b = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_stream16_kernel<T16, NC, BIAS>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)s16_lds(32 * NC));
    (void)rc_f;
    (void)rc_b;
    if (backward) hipLaunchKernelGGL((attn_bwd_stream16_kernel<T16, NC, BIAS>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((attn_fwd_stream16_kernel<T16, NC, BIAS>), grid, dim3(256), lds, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// streamgen
// ---------------------------------------------------------------------------------------------------------------------------------------
// s[r][c] = sum_d X[qt*32 + i0 + r][d] * Y[kt*32 + j0 + c][d] over the whole head width, as ONE chain of fused multiply-adds in the order
// d = 0, 1, 2, ... (long_dot of attention_valu.hpp sums groups of four first).  That is the order of a plain fp32 matrix product over a
// short inner dimension, so a score comes out with the bits such a product gives it -- which matters where the score is rounded once more
// on a coarse grid: with mask_value = -10000 a masked score lands on multiples of 2^-10, and a last-bit difference of q.k moves it by a step.
template <typename T>
__device__ __forceinline__ void gen_dot(const T* __restrict__ xsrc, int xpitch, int xcol, const T* __restrict__ ysrc, int ypitch, int ycol,
                                        size_t row0, int dh, int Tlen, int qt, int kt, float* sX, float* sY, float (&s)[4][4]) {
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[r][c] = 0.f;
    for (int d0 = 0; d0 < dh; d0 += LDC) {
        stage_chunk<T, LDC, 4>(xsrc, row0 + (size_t)qt * 32, xpitch, xcol, d0, dh, min(32, Tlen - qt * 32), sX);
        stage_chunk<T, LDC, 4>(ysrc, row0 + (size_t)kt * 32, ypitch, ycol, d0, dh, min(32, Tlen - kt * 32), sY);
        __syncthreads();
#pragma unroll 4
        for (int d = 0; d < LDC; d += 4) {
            float4 x[4], y[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = *reinterpret_cast<const float4*>(sX + (i0 + r) * LP + d);
#pragma unroll
            for (int c = 0; c < 4; ++c) y[c] = *reinterpret_cast<const float4*>(sY + (j0 + c) * LP + d);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    s[r][c] = fmaf(x[r].w, y[c].w, fmaf(x[r].z, y[c].z, fmaf(x[r].y, y[c].y, fmaf(x[r].x, y[c].x, s[r][c]))));
        }
        __syncthreads();
    }
}

// masked scaled scores of the lane's 4 x 4 block of tile (qt, kt); keys past the sequence are -inf
__device__ __forceinline__ void gen_mask(float (&s)[4][4], const AttnArgs& a, int L, int qt, int kt, const float* __restrict__ keep_row) {
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
        {
            const int i = qt * 32 + i0 + r, j = kt * 32 + j0 + c;
            const bool kept = (j < L) && (keep_row[min(j, L - 1)] != 0.f) && (!a.causal || j <= i);
            s[r][c] = (j < L) ? masked_score(s[r][c], a.scale, kept ? 0.f : a.mask_value) : -INFINITY;
        }
}
// + the bias cells of the same block (rows clamped to the sequence; the columns of a 32-key tile stay below Tp)
__device__ __forceinline__ void gen_bias(float (&s)[4][4], const float* __restrict__ bhead, int Tp, int L, int qt, int kt) {
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float4 b = *reinterpret_cast<const float4*>(bhead + (size_t)min(qt * 32 + i0 + r, L - 1) * Tp + kt * 32 + j0);
        s[r][0] += b.x; s[r][1] += b.y; s[r][2] += b.z; s[r][3] += b.w;
    }
}
__device__ __forceinline__ float row8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    return fmaxf(v, __shfl_xor(v, 4, 64));
}
__device__ __forceinline__ float row8_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v + __shfl_xor(v, 4, 64);
}
// the block transposed into an LDS tile [key][query] of pitch LPP
__device__ __forceinline__ void gen_put_t(float* W, const float (&x)[4][4]) {
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float col[4] = {x[0][c], x[1][c], x[2][c], x[3][c]};
        put_row<4>(W + (j0 + c) * LPP + i0, col);
    }
}
__device__ __forceinline__ void gen_zero(float (&o)[4][LCW]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < LCW; ++c) o[r][c] = 0.f;
}

struct GenSeq {
    size_t row0;
    int L, TPD, head, NT;
};
__device__ __forceinline__ bool gen_enter(AttnArgs& a, void* out, size_t out_rowbytes, GenSeq& q) {
    if ((int)blockIdx.x >= a.n_seq * a.n_heads) {
        zero_dead_rows(out, a.cu, a.n_seq, a.total_rows, out_rowbytes, (int)blockIdx.x - a.n_seq * a.n_heads);
        return false;
    }
    a.drop = drop_resolve(a.drop);
    const int seq = blockIdx.x / a.n_heads;
    q.head = blockIdx.x % a.n_heads;
    q.row0 = a.cu ? (size_t)a.cu[seq] : (size_t)seq * a.T;
    q.TPD = ((a.T + 31) / 32) * 32;
    q.L = a.cu ? a.cu[seq + 1] - a.cu[seq] : a.T;
    q.NT = (q.L + 31) / 32;
    return q.L > 0;
}

constexpr size_t gen_fwd_lds() { return (size_t)(3 * 32 * LP + 32 * LPP) * sizeof(float); }
constexpr size_t gen_bwd_lds() { return (size_t)(4 * 32 * LP + 2 * 32 * LPP + 3 * ST_MAX) * sizeof(float); }

template <typename T, bool BIAS>
__global__ __launch_bounds__(64) void attn_fwd_streamgen_kernel(StreamArgs<BIAS> a) {
    GenSeq q;
    if (!gen_enter(a, a.ctx, (size_t)a.n_heads * a.dh * sizeof(T), q)) return;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    float* sA = smem_f;
    float* sB = sA + 32 * LP;
    float* sC = sB + 32 * LP;
    float* W = sC + 32 * LP;                           // P of one tile, [key][query]
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4, c0 = (lane & 7) * LCW;
    const int H = a.n_heads * a.dh, pitch = 3 * H, L = q.L, NT = q.NT;
    const T* qkv = reinterpret_cast<const T*>(a.qkv);
    T* ctx = reinterpret_cast<T*>(a.ctx);
    const float* keep_row = a.key_keep + q.row0;
    const int colQ = q.head * a.dh, colK = H + colQ, colV = 2 * H + colQ;
    for (int qt = 0; qt < NT; ++qt) {
        // statistics of the tile's rows: running maximum and sum, rescaled whenever the maximum rises
        float m[4], l[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
        for (int kt = 0; kt < NT; ++kt) {
            float s[4][4];
            gen_dot<T>(qkv, pitch, colQ, qkv, pitch, colK, q.row0, a.dh, L, qt, kt, sA, sB, s);
            gen_mask(s, a, L, qt, kt, keep_row);
            if constexpr (BIAS) gen_bias(s, a.bias + (size_t)q.head * a.T * a.Tp, a.Tp, L, qt, kt);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float mn = fmaxf(m[r], row8_max(fmaxf(fmaxf(s[r][0], s[r][1]), fmaxf(s[r][2], s[r][3]))));      // finite: tile 0 holds key 0
                float ps = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) ps += expf(s[r][c] - mn);
                l[r] = l[r] * expf(m[r] - mn) + row8_sum(ps);
                m[r] = mn;
            }
        }
        float inv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) inv[r] = (qt * 32 + i0 + r < L) ? 1.0f / l[r] : 0.f;
        for (int d0 = 0; d0 < a.dh; d0 += LDC) {
            float o[4][LCW];
            gen_zero(o);
            for (int kt = 0; kt < NT; ++kt) {
                float s[4][4];
                gen_dot<T>(qkv, pitch, colQ, qkv, pitch, colK, q.row0, a.dh, L, qt, kt, sA, sB, s);
                gen_mask(s, a, L, qt, kt, keep_row);
                if constexpr (BIAS) gen_bias(s, a.bias + (size_t)q.head * a.T * a.Tp, a.Tp, L, qt, kt);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int i = qt * 32 + i0 + r, j = kt * 32 + j0 + c;
                        float p = expf(s[r][c] - m[r]) * inv[r];
                        if (a.drop.thresh) p = drop_keep(a.drop, ((uint64_t)blockIdx.x * q.TPD + (uint64_t)i) * q.TPD + (uint64_t)j) ? p * a.drop.inv_keep : 0.f;
                        s[r][c] = p;
                    }
                gen_put_t(W, s);
                const int klen = min(32, L - kt * 32);
                stage_chunk<T, LDC, 4>(qkv, q.row0 + (size_t)kt * 32, pitch, colV, d0, a.dh, klen, sC);
                __syncthreads();
                long_pv_acc(W, sC, i0, c0, klen, o);
                __syncthreads();
            }
            store_rows<T, LCW, 4>(ctx, q.row0 + (size_t)qt * 32, H, colQ + d0 + c0, i0, min(32, L - qt * 32), d0 + c0, a.dh, o);
        }
    }
}

template <typename T, bool BIAS>
__global__ __launch_bounds__(64) void attn_bwd_streamgen_kernel(StreamArgs<BIAS> a) {
    GenSeq q;
    if (!gen_enter(a, a.dqkv, (size_t)3 * a.n_heads * a.dh * sizeof(T), q)) return;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    float* sA = smem_f;                                // gen_dot's two tiles
    float* sB = sA + 32 * LP;
    float* sC = sB + 32 * LP;                          // operands of the second products
    float* sD = sC + 32 * LP;
    float* W1 = sD + 32 * LP;                          // dS of one tile
    float* W2 = W1 + 32 * LPP;                         // P (dropped) of one tile
    float* st_m = W2 + 32 * LPP;                       // row statistics of every query: max, 1 / sum, delta
    float* st_i = st_m + ST_MAX;
    float* st_d = st_i + ST_MAX;
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4, c0 = (lane & 7) * LCW;
    const int H = a.n_heads * a.dh, pitch = 3 * H, L = q.L, NT = q.NT;
    const T* qkv = reinterpret_cast<const T*>(a.qkv);
    const T* dctx = reinterpret_cast<const T*>(a.ctx);
    T* dqkv = reinterpret_cast<T*>(a.dqkv);
    const float* keep_row = a.key_keep + q.row0;
    const int colQ = q.head * a.dh, colK = H + colQ, colV = 2 * H + colQ;
    const int TPD = q.TPD;
    auto keep_scale = [&](int i, int j) -> float {       // dropout factor of element (i, j): 0 or 1 / (1 - p)
        if (!a.drop.thresh) return 1.f;
        return drop_keep(a.drop, ((uint64_t)blockIdx.x * TPD + (uint64_t)i) * TPD + (uint64_t)j) ? a.drop.inv_keep : 0.f;
    };
    // ---- phase A: m, 1 / l and delta = rowsum(P o dP), delta accumulated next to l with the same rescaling
    for (int qt = 0; qt < NT; ++qt) {
        float m[4], l[4], dl[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; dl[r] = 0.f; }
        for (int kt = 0; kt < NT; ++kt) {
            float s[4][4], dp[4][4];
            gen_dot<T>(qkv, pitch, colQ, qkv, pitch, colK, q.row0, a.dh, L, qt, kt, sA, sB, s);
            gen_dot<T>(dctx, H, colQ, qkv, pitch, colV, q.row0, a.dh, L, qt, kt, sA, sB, dp);
            gen_mask(s, a, L, qt, kt, keep_row);
            if constexpr (BIAS) gen_bias(s, a.bias + (size_t)q.head * a.T * a.Tp, a.Tp, L, qt, kt);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float mn = fmaxf(m[r], row8_max(fmaxf(fmaxf(s[r][0], s[r][1]), fmaxf(s[r][2], s[r][3]))));
                float ps = 0.f, ds = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float e = expf(s[r][c] - mn);
                    ps += e;
                    ds += e * (dp[r][c] * keep_scale(qt * 32 + i0 + r, kt * 32 + j0 + c));
                }
                const float alpha = expf(m[r] - mn);
                l[r] = l[r] * alpha + row8_sum(ps);
                dl[r] = dl[r] * alpha + row8_sum(ds);
                m[r] = mn;
            }
        }
        if ((lane & 7) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = qt * 32 + i0 + r;
                const float inv = (i < L) ? 1.0f / l[r] : 0.f;
                st_m[i] = m[r]; st_i[i] = inv; st_d[i] = dl[r] * inv;
            }
        }
    }
    __syncthreads();
    if constexpr (BIAS) {
        if (a.stats) {      // the row statistics leave for the bias-gradient pass
            float* st = a.stats + (size_t)blockIdx.x * 3 * a.T;
            for (int i = lane; i < L; i += 64) { st[i] = st_m[i]; st[a.T + i] = st_i[i]; st[2 * a.T + i] = st_d[i]; }
        }
    }
    // P (dropped) and dS of the lane's 4 x 4 block of tile (qt, kt) from the stored statistics
    auto tile_p_ds = [&](int qt, int kt, float (&p)[4][4], float (&ds)[4][4]) {
        float s[4][4], dp[4][4];
        gen_dot<T>(qkv, pitch, colQ, qkv, pitch, colK, q.row0, a.dh, L, qt, kt, sA, sB, s);
        gen_dot<T>(dctx, H, colQ, qkv, pitch, colV, q.row0, a.dh, L, qt, kt, sA, sB, dp);
        gen_mask(s, a, L, qt, kt, keep_row);
        if constexpr (BIAS) gen_bias(s, a.bias + (size_t)q.head * a.T * a.Tp, a.Tp, L, qt, kt);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = qt * 32 + i0 + r;
            const float m = st_m[i], inv = st_i[i], delta = st_d[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float pr = expf(s[r][c] - m) * inv;      // 0 for keys past the sequence (-inf) and query rows past it (inv = 0)
                const float ks = keep_scale(i, kt * 32 + j0 + c);
                ds[r][c] = pr * (dp[r][c] * ks - delta) * a.scale;
                p[r][c] = pr * ks;
            }
        }
    };
    // ---- phase B: dQ per query tile and head-width chunk
    for (int qt = 0; qt < NT; ++qt)
        for (int d0 = 0; d0 < a.dh; d0 += LDC) {
            float o[4][LCW];
            gen_zero(o);
            for (int kt = 0; kt < NT; ++kt) {
                float p[4][4], ds[4][4];
                tile_p_ds(qt, kt, p, ds);
                gen_put_t(W1, ds);
                const int klen = min(32, L - kt * 32);
                stage_chunk<T, LDC, 4>(qkv, q.row0 + (size_t)kt * 32, pitch, colK, d0, a.dh, klen, sC);
                __syncthreads();
                long_pv_acc(W1, sC, i0, c0, klen, o);      // dQ[i0 ..][cols] += sum_key dS^T[key][i0 ..] K[key][cols]
                __syncthreads();
            }
            store_rows<T, LCW, 4>(dqkv, q.row0 + (size_t)qt * 32, pitch, colQ + d0 + c0, i0, min(32, L - qt * 32), d0 + c0, a.dh, o);
        }
    // ---- phase C: dK, dV per key tile and head-width chunk (the lane's row block i0 doubles as its key block)
    for (int kt = 0; kt < NT; ++kt)
        for (int d0 = 0; d0 < a.dh; d0 += LDC) {
            float ok[4][LCW], ov[4][LCW];
            gen_zero(ok);
            gen_zero(ov);
            for (int qt = 0; qt < NT; ++qt) {
                float p[4][4], ds[4][4];
                tile_p_ds(qt, kt, p, ds);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    put_row<4>(W1 + (i0 + r) * LPP + j0, ds[r]);
                    put_row<4>(W2 + (i0 + r) * LPP + j0, p[r]);
                }
                const int qlen = min(32, L - qt * 32);
                stage_chunk<T, LDC, 4>(qkv, q.row0 + (size_t)qt * 32, pitch, colQ, d0, a.dh, qlen, sC);
                stage_chunk<T, LDC, 4>(dctx, q.row0 + (size_t)qt * 32, H, colQ, d0, a.dh, qlen, sD);
                __syncthreads();
                long_pv_acc(W1, sC, i0, c0, qlen, ok);     // dK[key i0 ..][cols] += sum_q dS[q][key] Q[q][cols]
                long_pv_acc(W2, sD, i0, c0, qlen, ov);     // dV[key i0 ..][cols] += sum_q P[q][key] dO[q][cols]
                __syncthreads();
            }
            const int klen = min(32, L - kt * 32);
            store_rows<T, LCW, 4>(dqkv, q.row0 + (size_t)kt * 32, pitch, colK + d0 + c0, i0, klen, d0 + c0, a.dh, ok);
            store_rows<T, LCW, 4>(dqkv, q.row0 + (size_t)kt * 32, pitch, colV + d0 + c0, i0, klen, d0 + c0, a.dh, ov);
        }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// bias gradient: d_pos_bias[h][i][j] = sum over the sequences of dS[n, h, i, j], dS = P o (dP - delta) -- the gradient at the score, so
// `scale` is not applied.  The backward kernels above leave m, 1 / l and delta of every query row in `stats`; a workgroup here owns one
// (head, query block, key block) tile and one of BIAS_NCH chunks of the sequences, walks its sequences in index order, recomputes the S
// and dP tiles and keeps the dS sums in registers (fp32, never rounded to the storage type).  The chunk partials are then added in chunk
// order by attn_bias_fold_kernel: no atomics, one fixed order, the same bits on every call.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct BiasGradArgs : StreamArgs<true> {      // ctx = dctx; stats is read
    float* part;                              // [BIAS_NCH][heads][T][Tp]; cells with j >= T are neither written nor read
};

template <typename T16, int NC>
__global__ __launch_bounds__(256) void attn_bias_grad16_kernel(BiasGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int pb = s16_pitch(a.dh), nch = a.dh / 32;
    char* sK = smem;
    char* sV = sK + SKT * pb;
    float* sKeep = reinterpret_cast<float*>(sV + SKT * pb);      // the flags of the 64 keys of the tile
    const int nt = a.Tp / SKT;
    const int head = blockIdx.x / (nt * nt), rem = blockIdx.x % (nt * nt), qb = rem / nt, kb = rem % nt;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int H = a.n_heads * a.dh, pitch = 3 * H, L = a.T;
    const bf16* qkv = reinterpret_cast<const bf16*>(a.qkv);
    const bf16* dctx = reinterpret_cast<const bf16*>(a.ctx);
    const int colQ = head * a.dh, colK = H + colQ, colV = 2 * H + colQ;
    const int i = qb * SKT + wave * 16 + c, ic = min(i, L - 1);      // the lane's query row
    const int per = (a.n_seq + BIAS_NCH - 1) / BIAS_NCH, s0 = blockIdx.y * per, s1 = min(s0 + per, a.n_seq);
    f32x4_t bz[4], acc[4];
    s16_bias_load(a.bias + ((size_t)head * a.T + ic) * a.Tp, kb * SKT, g, bz);
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = zero;
    for (int seq = s0; seq < s1; ++seq) {
        const size_t row0 = (size_t)seq * a.T;
        bf16x8_t qf[NC], of[NC];
        s16_row_frags<NC>(qkv, row0, pitch, colQ, a.dh, i, L, g, qf);
        s16_row_frags<NC>(dctx, row0, H, colQ, a.dh, i, L, g, of);
        const float* st = a.stats + ((size_t)seq * a.n_heads + head) * 3 * a.T;
        const float m = st[ic], inv = st[a.T + ic], delta = st[2 * a.T + ic];
        __syncthreads();      // the tiles of the previous sequence are consumed
        s16_stage<NC>(qkv, row0, pitch, colK, a.dh, kb * SKT, L, sK);
        s16_stage<NC>(qkv, row0, pitch, colV, a.dh, kb * SKT, L, sV);
        if (threadIdx.x < SKT) {
            const int j = kb * SKT + threadIdx.x;
            const float v = a.key_keep[row0 + min(j, L - 1)];
            sKeep[threadIdx.x] = j < L ? v : 0.f;
        }
        __syncthreads();
        f32x4_t s[4], dp[4];
        s16_dots<T16, NC>(sK, pb, nch, lane, qf, s);
        s16_dots<T16, NC>(sV, pb, nch, lane, of, dp);
        s16_mask(s, a, sKeep - kb * SKT, i, kb * SKT, g, L);      // (s16_mask indexes the flags by the key's position in the sequence)
        s16_bias_add(s, bz);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[k][r] - m) * inv;      // 0 for keys past the sequence (-inf)
                acc[k][r] += p * (dp[k][r] - delta);
            }
    }
    if (i < L) {
        float* dst = a.part + (((size_t)blockIdx.y * a.n_heads + head) * a.T + i) * a.Tp + kb * SKT;
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4_t*>(dst + k * 16 + 4 * g) = acc[k];
    }
}

// the same on streamgen's 32 x 32 tiles: one wavefront per (head, query tile, key tile) and chunk
template <typename T>
__global__ __launch_bounds__(64) void attn_bias_gradgen_kernel(BiasGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    float* sA = smem_f;
    float* sB = sA + 32 * LP;
    const int nt = (a.T + 31) / 32;
    const int head = blockIdx.x / (nt * nt), rem = blockIdx.x % (nt * nt), qt = rem / nt, kt = rem % nt;
    const int lane = threadIdx.x, i0 = (lane >> 3) * 4, j0 = (lane & 7) * 4;
    const int H = a.n_heads * a.dh, pitch = 3 * H, L = a.T;
    const T* qkv = reinterpret_cast<const T*>(a.qkv);
    const T* dctx = reinterpret_cast<const T*>(a.ctx);
    const int colQ = head * a.dh, colK = H + colQ, colV = 2 * H + colQ;
    const int per = (a.n_seq + BIAS_NCH - 1) / BIAS_NCH, s0 = blockIdx.y * per, s1 = min(s0 + per, a.n_seq);
    const float* bhead = a.bias + (size_t)head * a.T * a.Tp;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int seq = s0; seq < s1; ++seq) {
        const size_t row0 = (size_t)seq * a.T;
        float s[4][4], dp[4][4];
        gen_dot<T>(qkv, pitch, colQ, qkv, pitch, colK, row0, a.dh, L, qt, kt, sA, sB, s);
        gen_dot<T>(dctx, H, colQ, qkv, pitch, colV, row0, a.dh, L, qt, kt, sA, sB, dp);
        gen_mask(s, a, L, qt, kt, a.key_keep + row0);
        gen_bias(s, bhead, a.Tp, L, qt, kt);
        const float* st = a.stats + ((size_t)seq * a.n_heads + head) * 3 * a.T;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ic = min(qt * 32 + i0 + r, L - 1);
            const float m = st[ic], inv = st[a.T + ic], delta = st[2 * a.T + ic];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] += expf(s[r][c] - m) * inv * (dp[r][c] - delta);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = qt * 32 + i0 + r;
        if (i < L)
            *reinterpret_cast<float4*>(a.part + (((size_t)blockIdx.y * a.n_heads + head) * a.T + i) * a.Tp + kt * 32 + j0) =
                make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
}

// out[e] = part[0][e] + part[1][e] + ... in chunk order; the pad cells of a row (j >= T) are written as zero
__global__ __launch_bounds__(256) void attn_bias_fold_kernel(const float* __restrict__ part, float* __restrict__ out, size_t n, int T, int Tp) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        float acc = 0.f;
        if ((int)(e % Tp) < T)
            for (int c = 0; c < BIAS_NCH; ++c) acc += part[(size_t)c * n + e];
        out[e] = acc;
    }
}

template <typename T16, int NC>
void bias_grad16_launch(const BiasGradArgs& a, dim3 grid, hipStream_t s) {
    const size_t lds = 2 * SKT * s16_pitch(a.dh) + SKT * sizeof(float);
    static const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bias_grad16_kernel<T16, NC>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)(2 * SKT * s16_pitch(32 * NC) + SKT * sizeof(float)));
    (void)rc;
    hipLaunchKernelGGL((attn_bias_grad16_kernel<T16, NC>), grid, dim3(256), lds, s, a);
}

inline bool stream16_shape(const morec_attn_desc* d) { return is_h16(d->dtype) && d->dh % 32 == 0 && d->dh <= 256; }

// stream16 for 16-bit storage with a head width that is a multiple of 32 and at most 256, streamgen for everything else
template <bool BIAS>
int stream_launch(const morec_attn_desc* d, const StreamArgs<BIAS>& a, dim3 grid, bool backward, hipStream_t s) {
    if (stream16_shape(d)) {
        const size_t lds = s16_lds(d->dh);
        by_h16(d->dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            if (d->dh <= 64) s16_launch<T, 2, BIAS>(backward, a, grid, lds, s);
            else if (d->dh <= 128) s16_launch<T, 4, BIAS>(backward, a, grid, lds, s);
            else s16_launch<T, 8, BIAS>(backward, a, grid, lds, s);
        });
    } else if (!by_dtype(d->dtype, [&](auto* t) {
                   using T = MOREC_TAG_T(t);
                   if (backward) hipLaunchKernelGGL((attn_bwd_streamgen_kernel<T, BIAS>), grid, dim3(64), gen_bwd_lds(), s, a);
                   else hipLaunchKernelGGL((attn_fwd_streamgen_kernel<T, BIAS>), grid, dim3(64), gen_fwd_lds(), s, a);
               }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// what the bias entry points take: the descriptor is judged before any pointer
int bias_check_desc(const morec_attn_desc* d) {
    if (!d) return MOREC_E_ARG;
    if (d->n_seq <= 0 || d->T <= 0 || d->n_heads <= 0 || d->dh <= 0) return MOREC_E_ARG;
    if (d->p_drop < 0.f || d->p_drop >= 1.f) return MOREC_E_ARG;
    if (d->causal != 0 || d->p_drop > 0.f || d->cu_seqlens != nullptr || d->T > ST_MAX) return MOREC_E_UNSUPPORTED;      // no caller uses them
    if (d->dh % 8) return MOREC_E_ALIGN;
    if (d->dtype != MOREC_F32 && !is_h16(d->dtype)) return MOREC_E_DTYPE;
    return MOREC_OK;
}
inline int bias_tp(int T) { return (T + SKT - 1) / SKT * SKT; }
inline size_t bias_stats_floats(const morec_attn_desc* d) { return ((size_t)d->n_seq * d->n_heads * 3 * d->T + 3) & ~(size_t)3; }
inline size_t bias_table_floats(const morec_attn_desc* d) { return (size_t)d->n_heads * d->T * bias_tp(d->T); }

StreamArgs<true> bias_args(const morec_attn_desc* d, const void* qkv, const float* key_keep, const float* pos_bias, void* ctx_or_dctx,
                           void* dqkv, float* stats) {
    StreamArgs<true> a;
    static_cast<AttnArgs&>(a) = AttnArgs{qkv, key_keep, ctx_or_dctx, dqkv, d->n_seq, d->T, d->n_heads, d->dh, 0, d->scale, d->mask_value,
                                         make_drop(0.f, 0), nullptr, 0};
    a.bias = pos_bias;
    a.stats = stats;
    a.Tp = bias_tp(d->T);
    return a;
}
}  // namespace

int attn_spare_blocks(const morec_attn_desc* d);      // attention.hip

// The streaming kernels of a checked call (attn_dispatch in attention.hip decides WHETHER they run).  MOREC_E_UNSUPPORTED: a sequence
// beyond the cap.
int morec_attn_stream_launch(const morec_attn_desc* d, const void* qkv, const float* key_keep, void* ctx_or_dctx, void* dqkv, bool backward,
                             hipStream_t s) {
    if (d->T > ST_MAX) return MOREC_E_UNSUPPORTED;
    StreamArgs<false> a;
    static_cast<AttnArgs&>(a) = AttnArgs{qkv, key_keep, ctx_or_dctx, dqkv, d->n_seq, d->T, d->n_heads, d->dh, d->causal, d->scale, d->mask_value,
                                         make_drop(d->p_drop, d->seed), d->cu_seqlens, d->total_rows};
    return stream_launch<false>(d, a, dim3(d->n_seq * d->n_heads + attn_spare_blocks(d)), backward, s);
}

// ---- attention with a per-head position bias (include/morec_hip.h: morec_attn_bias_fwd) ------------------------------------------------
extern "C" size_t morec_attn_bias_ws_bytes(const morec_attn_desc* d) {
    if (bias_check_desc(d) != MOREC_OK) return 0;
    return (bias_stats_floats(d) + (size_t)BIAS_NCH * bias_table_floats(d)) * sizeof(float);
}

extern "C" int morec_attn_bias_fwd(const morec_attn_desc* d, const void* qkv, const float* key_keep, const float* pos_bias, void* ctx,
                                   void* stream) {
    const int rc = bias_check_desc(d);
    if (rc) return rc;
    if (!qkv || !key_keep || !pos_bias || !ctx) return MOREC_E_ARG;
    if (!aligned16(qkv) || !aligned16(pos_bias) || !aligned16(ctx)) return MOREC_E_ALIGN;
    return stream_launch<true>(d, bias_args(d, qkv, key_keep, pos_bias, ctx, nullptr, nullptr), dim3(d->n_seq * d->n_heads), false,
                               reinterpret_cast<hipStream_t>(stream));
}

extern "C" int morec_attn_bias_bwd(const morec_attn_desc* d, const void* qkv, const float* key_keep, const float* pos_bias, const void* dctx,
                                   void* dqkv, float* dqkv_bias, float* d_pos_bias, float* ws, size_t ws_bytes, void* stream) {
    int rc = bias_check_desc(d);
    if (rc) return rc;
    if (!qkv || !key_keep || !pos_bias || !dctx || !dqkv) return MOREC_E_ARG;
    if (d_pos_bias && (!ws || ws_bytes < morec_attn_bias_ws_bytes(d))) return MOREC_E_ARG;
    if (!aligned16(qkv) || !aligned16(pos_bias) || !aligned16(dctx) || !aligned16(dqkv) || (d_pos_bias && (!aligned16(d_pos_bias) || !aligned16(ws))))
        return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = stream_launch<true>(d, bias_args(d, qkv, key_keep, pos_bias, const_cast<void*>(dctx), dqkv, d_pos_bias ? ws : nullptr),
                             dim3(d->n_seq * d->n_heads), true, s);
    if (rc) return rc;
    const int H3 = 3 * d->n_heads * d->dh;
    if (dqkv_bias) {
        rc = morec_colsum(dqkv, dqkv_bias, d->n_seq * d->T, H3, H3, d->dtype, stream);
        if (rc) return rc;
    }
    if (!d_pos_bias) return MOREC_OK;      // a frozen table: nothing more is launched
    BiasGradArgs g;
    static_cast<StreamArgs<true>&>(g) = bias_args(d, qkv, key_keep, pos_bias, const_cast<void*>(dctx), nullptr, ws);
    g.part = ws + bias_stats_floats(d);
    if (stream16_shape(d)) {
        const int nt = g.Tp / SKT;
        dim3 grid(d->n_heads * nt * nt, BIAS_NCH);
        by_h16(d->dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            if (d->dh <= 64) bias_grad16_launch<T, 2>(g, grid, s);
            else if (d->dh <= 128) bias_grad16_launch<T, 4>(g, grid, s);
            else bias_grad16_launch<T, 8>(g, grid, s);
        });
    } else {
        const int nt = (d->T + 31) / 32;
        dim3 grid(d->n_heads * nt * nt, BIAS_NCH);
        by_dtype(d->dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((attn_bias_gradgen_kernel<T>), grid, dim3(64), 2 * 32 * LP * sizeof(float), s, g);
        });
    }
    MOREC_CHECK_LAUNCH();
    const size_t n = bias_table_floats(d);
    hipLaunchKernelGGL(attn_bias_fold_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, s, g.part, d_pos_bias, n,
                       d->T, g.Tp);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
