// deberta.hip -- DeBERTa's disentangled self-attention (HF modeling_deberta.py DisentangledSelfAttention, c2p + p2c) for T <= 64:
//     S[i][j] = (q_i.k_j + q_i.PK_h[d(i,j)] + k_j.PQ_h[d(i,j)]) * scale,   d(i,j) = i - j + T  (1 .. 2T-1),
// a score whose query or key is masked is REPLACED by the fill value, then softmax, dropout on P, ctx = P V.
//
// One workgroup of four wavefronts per (sequence, head).  The two position products are formed once as full [T x 2T] tiles (Q PK^T and
// K PQ^T) and kept in LDS in fp32 next to the [T x T] content scores; the thread that owns score (i, j) reads cell [i][d] of the first
// and [j][d] of the second.  In the backward the same two LDS tiles then take the gradient tiles G1[i][d(i,j)] = G2[j][d(i,j)] = dS[i][j]
// (a one-to-one scatter), so the position terms of dQ / dK and the gradients of PK / PQ are plain matrix products again.
//
// Every product goes through one primitive, `Mul::run(M, N, K, a, b, emit)` with element accessors a(m, k), b(k, n):
//   * MulMfma<T16> (bf16 / fp16 storage, dh % 32 == 0, dh <= 128): v_mfma_f32_16x16x32_{bf16,f16}, a wavefront per 16 x 16 output block,
//     fragments gathered element by element through the accessors (A: row lane & 15, k = 8 (lane >> 4) + e; B: the same k, column
//     lane & 15; C: column lane & 15, row 4 (lane >> 4) + r), operands held in fp32 (P, dS, G1, G2) rounded to the storage type;
//   * MulGen (fp32 storage, other head widths): one thread per output element, fp32 FMAs in k order.
// Indices past an edge are clamped before the load and the value replaced by zero after it: no access leaves a tile or a tensor.
//
// Gradients of PK / PQ (fp32 [2T][H], written): the sequences are cut into 8 chunks of ceil(n_seq / 8); a workgroup per (chunk, head)
// walks its sequences in index order, recomputes dS, and adds that sequence's G1^T Q and G2^T K into its partial in `ws` -- every cell
// has ONE owner thread, which adds in sequence order in fp32 -- and a last kernel adds the partials in chunk order.  No atomics, every
// output written once, the same bits on every call.
#include <algorithm>
#include "common.hpp"

namespace {
constexpr int DA_NCH = 8;            // chunks of sequences of the PK / PQ gradients
constexpr int DA_THREADS = 256;
constexpr int DA_TMAX = 64;
constexpr int DA_TP = 64;            // edge of the dropout stream's tile: element ((seq * heads + head) * 64 + i) * 64 + j

struct DisentArgs {
    const void* qkv;
    const float* key_keep;
    const void* pk;       // [2T][H] storage type
    const void* pq;
    void* ctx;            // forward: output; backward: dctx
    void* dqkv;
    float* part;          // [DA_NCH][2][2T][H]
    int n_seq, T, n_heads, dh;
    float scale, fill;
    DropRng drop;
};

// LDS geometry (floats): two [TT][W + 1] position tiles, then [TT][TT + 1] tiles (scores / P; backward: dP / dS), then the T mask flags
struct Geo {
    int TT, W, pc, ps;
    __host__ __device__ explicit Geo(int T) : TT((T + 15) & ~15), W(2 * TT), pc(2 * TT + 1), ps(TT + 1) {}
    __host__ __device__ size_t floats(bool bwd) const { return (size_t)2 * TT * pc + (size_t)(bwd ? 2 : 1) * TT * ps + DA_TMAX; }
};

template <typename T>
__device__ __forceinline__ float ld(const void* p, size_t i) { return io<T>::load1(reinterpret_cast<const T*>(p) + i); }

struct MulGen {
    template <class A, class B, class E>
    __device__ __forceinline__ static void run(int M, int N, int K, A a, B b, E emit) {
        for (int e = threadIdx.x; e < M * N; e += DA_THREADS) {
            const int m = e / N, n = e % N;
            float acc = 0.f;
            for (int k = 0; k < K; ++k) acc = fmaf(a(m, k), b(k, n), acc);
            emit(m, n, acc);
        }
    }
};

template <typename T16>
struct MulMfma {
    template <class A, class B, class E>
    __device__ __forceinline__ static void run(int M, int N, int K, A a, B b, E emit) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
        const int nbn = (N + 15) / 16, nblk = ((M + 15) / 16) * nbn;
        for (int blk = wave; blk < nblk; blk += DA_THREADS / 64) {      // (wave-uniform: every lane of the wavefront issues the MFMAs)
            const int mb = blk / nbn, nb = blk % nbn;
            const int m = mb * 16 + c, n = nb * 16 + c, mc = min(m, M - 1), nc = min(n, N - 1);
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < K; k0 += 32) {
                float av[8], bv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = k0 + 8 * g + e, kc = min(k, K - 1);
                    const float x = a(mc, kc), y = b(kc, nc);
                    av[e] = (k < K && m < M) ? x : 0.f;
                    bv[e] = (k < K && n < N) ? y : 0.f;
                }
                const uint4 ua = make_uint4(h16<T16>::pack2(av[0], av[1]), h16<T16>::pack2(av[2], av[3]), h16<T16>::pack2(av[4], av[5]), h16<T16>::pack2(av[6], av[7]));
                const uint4 ub = make_uint4(h16<T16>::pack2(bv[0], bv[1]), h16<T16>::pack2(bv[2], bv[3]), h16<T16>::pack2(bv[4], bv[5]), h16<T16>::pack2(bv[6], bv[7]));
                acc = h16<T16>::mma16(__builtin_bit_cast(bf16x8_t, ua), __builtin_bit_cast(bf16x8_t, ub), acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mb * 16 + 4 * g + r, col = nb * 16 + c;
                if (row < M && col < N) emit(row, col, acc[r]);
            }
        }
    }
};

// what one (sequence, head) needs from the arguments
template <typename T>
struct Head {
    const DisentArgs& a;
    size_t row0;
    int H, pitch, hc;      // hc = first column of the head
    uint64_t tile;
    __device__ Head(const DisentArgs& a_, int seq, int head)
        : a(a_), row0((size_t)seq * a_.T), H(a_.n_heads * a_.dh), pitch(3 * a_.n_heads * a_.dh), hc(head * a_.dh),
          tile((uint64_t)seq * a_.n_heads + head) {}
    __device__ __forceinline__ float q(int i, int d) const { return ld<T>(a.qkv, (row0 + i) * pitch + hc + d); }
    __device__ __forceinline__ float k(int i, int d) const { return ld<T>(a.qkv, (row0 + i) * pitch + H + hc + d); }
    __device__ __forceinline__ float v(int i, int d) const { return ld<T>(a.qkv, (row0 + i) * pitch + 2 * H + hc + d); }
    __device__ __forceinline__ float o(int i, int d) const { return ld<T>(a.ctx, (row0 + i) * H + hc + d); }      // dctx
    __device__ __forceinline__ float pk(int r, int d) const { return ld<T>(a.pk, (size_t)r * H + hc + d); }
    __device__ __forceinline__ float pq(int r, int d) const { return ld<T>(a.pq, (size_t)r * H + hc + d); }
    // dropout scale of P[i][j]
    __device__ __forceinline__ float ms(int i, int j) const {
        if (!a.drop.thresh) return 1.f;
        return drop_keep(a.drop, (tile * DA_TP + (uint64_t)i) * DA_TP + (uint64_t)j) ? a.drop.inv_keep : 0.f;
    }
};

// sS <- softmax of the masked scores (the probabilities BEFORE dropout); sC / sP are scratch for the two position tiles; sKeep <- the flags
template <typename T, typename Mul>
__device__ void probs(const Head<T>& h, const Geo& g, float* sC, float* sP, float* sS, float* sKeep) {
    const DisentArgs& a = h.a;
    const int L = a.T, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < L) sKeep[threadIdx.x] = a.key_keep[h.row0 + threadIdx.x];
    Mul::run(L, 2 * L, a.dh, [&](int i, int d) { return h.q(i, d); }, [&](int d, int r) { return h.pk(r, d); },
             [&](int i, int r, float x) { sC[i * g.pc + r] = x; });
    Mul::run(L, 2 * L, a.dh, [&](int j, int d) { return h.k(j, d); }, [&](int d, int r) { return h.pq(r, d); },
             [&](int j, int r, float x) { sP[j * g.pc + r] = x; });
    Mul::run(L, L, a.dh, [&](int i, int d) { return h.q(i, d); }, [&](int d, int j) { return h.k(j, d); },
             [&](int i, int j, float x) { sS[i * g.ps + j] = x; });
    __syncthreads();
    for (int e = threadIdx.x; e < L * L; e += DA_THREADS) {
        const int i = e / L, j = e % L, r = i - j + L;
        const float s = (sS[i * g.ps + j] + sC[i * g.pc + r] + sP[j * g.pc + r]) * a.scale;
        sS[i * g.ps + j] = (sKeep[i] != 0.f && sKeep[j] != 0.f) ? s : a.fill;
    }
    __syncthreads();
    for (int i = wave; i < L; i += DA_THREADS / 64) {      // a wavefront per row, a lane per key (T <= 64)
        const bool in = lane < L;
        const float s = in ? sS[i * g.ps + lane] : -INFINITY;
        const float m = wave_max(s);
        const float ex = in ? expf(s - m) : 0.f;
        const float sum = wave_sum(ex);
        if (in) sS[i * g.ps + lane] = ex / sum;
    }
    __syncthreads();
}

// backward of one (sequence, head) up to the gradient tiles: sS <- dropped P, sD <- dS (gradient at the raw score sum, scale applied,
// zero where the score was replaced), sC <- G1[i][r], sP <- G2[j][r]
template <typename T, typename Mul>
__device__ void grads(const Head<T>& h, const Geo& g, float* sC, float* sP, float* sS, float* sD, float* sKeep) {
    const DisentArgs& a = h.a;
    const int L = a.T, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    probs<T, Mul>(h, g, sC, sP, sS, sKeep);
    Mul::run(L, L, a.dh, [&](int i, int d) { return h.o(i, d); }, [&](int d, int j) { return h.v(j, d); },
             [&](int i, int j, float x) { sD[i * g.ps + j] = x; });
    for (int e = threadIdx.x; e < g.TT * g.pc; e += DA_THREADS) { sC[e] = 0.f; sP[e] = 0.f; }
    __syncthreads();
    for (int i = wave; i < L; i += DA_THREADS / 64) {
        const bool in = lane < L;
        const int j = in ? lane : 0;
        const float p = in ? sS[i * g.ps + j] : 0.f;
        const float m = in ? h.ms(i, j) : 0.f;
        const float dp = in ? sD[i * g.ps + j] * m : 0.f;
        const float delta = wave_sum(p * dp);
        const bool kept = in && sKeep[i] != 0.f && sKeep[j] != 0.f;
        const float ds = kept ? p * (dp - delta) * a.scale : 0.f;
        if (in) {
            sD[i * g.ps + j] = ds;
            sS[i * g.ps + j] = p * m;
            const int r = i - j + L;
            sC[i * g.pc + r] = ds;
            sP[j * g.pc + r] = ds;
        }
    }
    __syncthreads();
}

template <typename T, typename Mul>
__global__ __launch_bounds__(DA_THREADS) void disent_fwd_kernel(DisentArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    a.drop = drop_resolve(a.drop);
    const Geo g(a.T);
    float* sC = smem_f;
    float* sP = sC + g.TT * g.pc;
    float* sS = sP + g.TT * g.pc;
    float* sKeep = sS + g.TT * g.ps;
    const Head<T> h(a, blockIdx.x / a.n_heads, blockIdx.x % a.n_heads);
    probs<T, Mul>(h, g, sC, sP, sS, sKeep);
    T* ctx = reinterpret_cast<T*>(a.ctx);
    Mul::run(a.T, a.dh, a.T, [&](int i, int j) { return sS[i * g.ps + j] * h.ms(i, j); }, [&](int j, int d) { return h.v(j, d); },
             [&](int i, int d, float x) { io<T>::store1(ctx + (h.row0 + i) * h.H + h.hc + d, x); });
}

template <typename T, typename Mul>
__global__ __launch_bounds__(DA_THREADS) void disent_bwd_kernel(DisentArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    a.drop = drop_resolve(a.drop);
    const Geo g(a.T);
    float* sC = smem_f;
    float* sP = sC + g.TT * g.pc;
    float* sS = sP + g.TT * g.pc;
    float* sD = sS + g.TT * g.ps;
    float* sKeep = sD + g.TT * g.ps;
    const Head<T> h(a, blockIdx.x / a.n_heads, blockIdx.x % a.n_heads);
    grads<T, Mul>(h, g, sC, sP, sS, sD, sKeep);
    const int L = a.T;
    T* dqkv = reinterpret_cast<T*>(a.dqkv);
    // dQ = dS K + G1 PK: one product over the 3 T contraction slots [keys | relative positions]
    Mul::run(L, a.dh, 3 * L, [&](int i, int k) { return k < L ? sD[i * g.ps + k] : sC[i * g.pc + (k - L)]; },
             [&](int k, int d) { return k < L ? h.k(k, d) : h.pk(k - L, d); },
             [&](int i, int d, float x) { io<T>::store1(dqkv + (h.row0 + i) * h.pitch + h.hc + d, x); });
    // dK = dS^T Q + G2 PQ
    Mul::run(L, a.dh, 3 * L, [&](int j, int k) { return k < L ? sD[k * g.ps + j] : sP[j * g.pc + (k - L)]; },
             [&](int k, int d) { return k < L ? h.q(k, d) : h.pq(k - L, d); },
             [&](int j, int d, float x) { io<T>::store1(dqkv + (h.row0 + j) * h.pitch + h.H + h.hc + d, x); });
    // dV = P_d^T dO
    Mul::run(L, a.dh, L, [&](int j, int i) { return sS[i * g.ps + j]; }, [&](int i, int d) { return h.o(i, d); },
             [&](int j, int d, float x) { io<T>::store1(dqkv + (h.row0 + j) * h.pitch + 2 * h.H + h.hc + d, x); });
}

// grid (DA_NCH, heads): part[chunk][0] = sum over the chunk's sequences of G1^T Q, part[chunk][1] = of G2^T K (head columns)
template <typename T, typename Mul>
__global__ __launch_bounds__(DA_THREADS) void disent_pos_grad_kernel(DisentArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    a.drop = drop_resolve(a.drop);
    const Geo g(a.T);
    float* sC = smem_f;
    float* sP = sC + g.TT * g.pc;
    float* sS = sP + g.TT * g.pc;
    float* sD = sS + g.TT * g.ps;
    float* sKeep = sD + g.TT * g.ps;
    const int chunk = blockIdx.x, head = blockIdx.y, L = a.T, H = a.n_heads * a.dh;
    const int per = (a.n_seq + DA_NCH - 1) / DA_NCH, s0 = chunk * per, s1 = min(s0 + per, a.n_seq);
    float* pPK = a.part + (size_t)(chunk * 2) * 2 * L * H;
    float* pPQ = pPK + (size_t)2 * L * H;
    for (int seq = s0; seq < s1; ++seq) {
        const Head<T> h(a, seq, head);
        const bool first = seq == s0;
        grads<T, Mul>(h, g, sC, sP, sS, sD, sKeep);
        // (an output cell has the same owner thread for every sequence: its read-modify-write is a sum in sequence order)
        Mul::run(2 * L, a.dh, L, [&](int r, int i) { return sC[i * g.pc + r]; }, [&](int i, int d) { return h.q(i, d); },
                 [&](int r, int d, float x) {
                     float* p = pPK + (size_t)r * H + h.hc + d;
                     *p = first ? x : *p + x;
                 });
        Mul::run(2 * L, a.dh, L, [&](int r, int j) { return sP[j * g.pc + r]; }, [&](int j, int d) { return h.k(j, d); },
                 [&](int r, int d, float x) {
                     float* p = pPQ + (size_t)r * H + h.hc + d;
                     *p = first ? x : *p + x;
                 });
        __syncthreads();      // the tiles are consumed before the next sequence overwrites them
    }
}

// dPK[e] / dPQ[e] = the partials of the chunks that hold a sequence, added in chunk order
__global__ __launch_bounds__(256) void disent_fold_kernel(const float* __restrict__ part, float* __restrict__ dpk, float* __restrict__ dpq,
                                                          size_t n, int nch) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < 2 * n; e += (size_t)gridDim.x * 256) {
        const size_t which = e / n, i = e % n;
        float acc = 0.f;
        for (int c = 0; c < nch; ++c) acc += part[((size_t)c * 2 + which) * n + i];
        (which ? dpq : dpk)[i] = acc;
    }
}

// x[m][:] = keep[m] != 0 ? x[m][:] : 0, in place (the embedding stage's `LN(word) * mask`: exact zeros on the masked rows)
template <typename T>
__global__ __launch_bounds__(256) void rows_keep_kernel(T* __restrict__ x, const float* __restrict__ keep, size_t M, int N) {
    const size_t n = M * (size_t)N;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256)
        if (keep[e / N] == 0.f) io<T>::store1(x + e, 0.f);
}

inline bool mfma16_shape(const morec_attn_desc* d) { return is_h16(d->dtype) && d->dh % 32 == 0 && d->dh <= 128; }

int check_desc(const morec_attn_desc* d) {
    if (!d) return MOREC_E_ARG;
    if (d->n_seq <= 0 || d->T <= 0 || d->n_heads <= 0 || d->dh <= 0) return MOREC_E_ARG;
    if (d->p_drop < 0.f || d->p_drop >= 1.f) return MOREC_E_ARG;
    if (d->causal != 0 || d->cu_seqlens != nullptr || d->T > DA_TMAX) return MOREC_E_UNSUPPORTED;
    if (d->dtype != MOREC_F32 && !is_h16(d->dtype)) return MOREC_E_DTYPE;
    return MOREC_OK;
}

template <typename T, typename Mul>
int launch(int mode, const DisentArgs& a, hipStream_t s) {
    // every kernel may ask for the largest tile (T = 64, backward): 99 KiB of the CU's 160
    static const int max_lds = (int)(Geo(DA_TMAX).floats(true) * sizeof(float));
    static const hipError_t rc0 = hipFuncSetAttribute(reinterpret_cast<const void*>(&disent_fwd_kernel<T, Mul>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    static const hipError_t rc1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&disent_bwd_kernel<T, Mul>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    static const hipError_t rc2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&disent_pos_grad_kernel<T, Mul>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (rc0 != hipSuccess || rc1 != hipSuccess || rc2 != hipSuccess) return (int)(rc0 != hipSuccess ? rc0 : rc1 != hipSuccess ? rc1 : rc2);
    const size_t lds = Geo(a.T).floats(mode != 0) * sizeof(float);
    if (mode == 0) hipLaunchKernelGGL((disent_fwd_kernel<T, Mul>), dim3(a.n_seq * a.n_heads), dim3(DA_THREADS), lds, s, a);
    else if (mode == 1) hipLaunchKernelGGL((disent_bwd_kernel<T, Mul>), dim3(a.n_seq * a.n_heads), dim3(DA_THREADS), lds, s, a);
    else hipLaunchKernelGGL((disent_pos_grad_kernel<T, Mul>), dim3(DA_NCH, a.n_heads), dim3(DA_THREADS), lds, s, a);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

int dispatch(const morec_attn_desc* d, int mode, const DisentArgs& a, hipStream_t s) {
    int rc = MOREC_E_DTYPE;
    if (mfma16_shape(d)) {
        by_h16(d->dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            rc = launch<T, MulMfma<T>>(mode, a, s);
        });
    } else {
        by_dtype(d->dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            rc = launch<T, MulGen>(mode, a, s);
        });
    }
    return rc;
}

DisentArgs make_args(const morec_attn_desc* d, const void* qkv, const float* key_keep, const void* pk, const void* pq, void* ctx_or_dctx,
                     void* dqkv, float* part) {
    return DisentArgs{qkv, key_keep, pk, pq, ctx_or_dctx, dqkv, part, d->n_seq, d->T, d->n_heads, d->dh, d->scale, d->mask_value,
                      make_drop(d->p_drop, d->seed)};
}
}  // namespace

extern "C" size_t morec_disent_attn_ws_bytes(const morec_attn_desc* d) {
    if (check_desc(d) != MOREC_OK) return 0;
    return (size_t)DA_NCH * 2 * 2 * d->T * d->n_heads * d->dh * sizeof(float);
}

extern "C" int morec_disent_attn_fwd(const morec_attn_desc* d, const void* qkv, const float* key_keep, const void* pk, const void* pq,
                                     void* ctx, void* stream) {
    const int rc = check_desc(d);
    if (rc) return rc;
    if (!qkv || !key_keep || !pk || !pq || !ctx) return MOREC_E_ARG;
    return dispatch(d, 0, make_args(d, qkv, key_keep, pk, pq, ctx, nullptr, nullptr), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int morec_disent_attn_bwd(const morec_attn_desc* d, const void* qkv, const float* key_keep, const void* pk, const void* pq,
                                     const void* dctx, void* dqkv, float* dqkv_bias, float* dpk, float* dpq, float* ws, size_t ws_bytes,
                                     void* stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!qkv || !key_keep || !pk || !pq || !dctx || !dqkv) return MOREC_E_ARG;
    if ((dpk == nullptr) != (dpq == nullptr)) return MOREC_E_ARG;      // both or neither
    if (dpk && (!ws || ws_bytes < morec_disent_attn_ws_bytes(d))) return MOREC_E_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = dispatch(d, 1, make_args(d, qkv, key_keep, pk, pq, const_cast<void*>(dctx), dqkv, nullptr), s);
    if (rc) return rc;
    const int H3 = 3 * d->n_heads * d->dh;
    if (dqkv_bias) {
        rc = morec_colsum(dqkv, dqkv_bias, d->n_seq * d->T, H3, H3, d->dtype, stream);
        if (rc) return rc;
    }
    if (!dpk) return MOREC_OK;      // frozen position projections: nothing more is launched
    rc = dispatch(d, 2, make_args(d, qkv, key_keep, pk, pq, const_cast<void*>(dctx), nullptr, ws), s);
    if (rc) return rc;
    const size_t n = (size_t)2 * d->T * d->n_heads * d->dh;
    const int per = (d->n_seq + DA_NCH - 1) / DA_NCH, used = (d->n_seq + per - 1) / per;
    hipLaunchKernelGGL(disent_fold_kernel, dim3((unsigned)std::min<size_t>((2 * n + 255) / 256, 8192)), dim3(256), 0, s, ws, dpk, dpq, n, used);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_rows_keep(void* x, const float* keep, long M, int N, int dtype, void* stream) {
    if (!x || !keep || M <= 0 || N <= 0) return MOREC_E_ARG;
    const size_t n = (size_t)M * N;
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((rows_keep_kernel<T>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0,
                               reinterpret_cast<hipStream_t>(stream), reinterpret_cast<T*>(x), keep, (size_t)M, N);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
