// opt.hip -- the stages of the OPT text tower that no other tower has (HF transformers/models/opt/modeling_opt.py, the reference's
// Text_Encoder_mean, T/model/encoders.py:31-50): position ids counted from the attention mask, an embedding stage that is a plain
// sum of two table rows (no LayerNorm, no token type, no dropout), and the masked mean over a title's tokens with its backward.
// The embedding backward is morec_roberta_embed_bwd (embed.hip) walking the perm / cnt that morec_mask_pos_ids writes.
// No atomics, no LDS hand-off between workgroups, every output element written exactly once: the same bits on every call, in
// either setting of the deterministic mode.
#include "common.hpp"

// Mask-relative position ids (OPTLearnedPositionalEmbedding: cumsum(mask) * mask - 1 + offset): the k-th kept token of a sequence
// (k from 0) has id offset + k, a masked one offset - 1.  One wave per sequence, laid out as roberta_pos_ids_kernel (embed.hip) is:
// T is walked 64 lanes at a time, each trip a ballot of mask != 0, the popcount of the lanes below and a running base -- once to
// count (the masked slots of `perm` start there), once to write.  Holes in the mask are legal.
__global__ __launch_bounds__(256) void mask_pos_ids_kernel(const int32_t* __restrict__ mask, int n_seq, int Tlen, int offset,
                                                           int32_t* __restrict__ pos_ids, int32_t* __restrict__ perm,
                                                           int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_seq) return;      // (wave-uniform)
    const int32_t* row = mask + (size_t)n * Tlen;
    const unsigned long long below = (1ull << lane) - 1ull;
    int total = 0;
    for (int t0 = 0; t0 < Tlen; t0 += 64) {
        const int t = t0 + lane;
        total += __popcll(__ballot(t < Tlen && row[t] != 0));
    }
    int base = 0;
    for (int t0 = 0; t0 < Tlen; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < Tlen;
        const bool kept = in && row[t] != 0;
        const unsigned long long m = __ballot(kept);
        const int k = base + __popcll(m & below);      // kept tokens in front of position t
        if (in) {
            pos_ids[(size_t)n * Tlen + t] = kept ? offset + k : offset - 1;
            perm[(size_t)n * Tlen + (kept ? k : total + (t - k))] = t;
        }
        base += __popcll(m);
    }
    if (lane == 0) cnt[n] = total;
}

extern "C" int morec_mask_pos_ids(const int32_t* mask, int n_seq, int T, int offset, int n_pos, int32_t* pos_ids_out,
                                  int32_t* perm_out, int32_t* cnt_out, void* stream) {
    if (!mask || !pos_ids_out || !perm_out || !cnt_out || n_seq <= 0 || T <= 0) return MOREC_E_ARG;
    // the ids written lie in offset - 1 .. offset + T - 1: every one must be a row of the n_pos-row table
    if (offset < 1 || (long long)offset + T - 1 >= (long long)n_pos) return MOREC_E_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mask_pos_ids_kernel, dim3((n_seq + 3) / 4), dim3(256), 0, s, mask, n_seq, T, offset, pos_ids_out, perm_out,
                       cnt_out);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// out[m] = round(word[ids[m]] + pos[pos_ids[m]]): fp32 tables, fp32 add, one rounding.  A thread owns one 16-byte vector of the
// output row (EV elements: two 16-byte loads from each table); a block covers 256 / nv rows (nv = H / EV <= 256).
template <typename T>
__global__ __launch_bounds__(256) void opt_embed_fwd_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos_ids,
                                                            const float* __restrict__ word, const float* __restrict__ pos,
                                                            T* __restrict__ out, int M, int H, int rows_per_block) {
    constexpr int EV = vio<T>::EV;
    const int nv = H / EV;
    const int r = (int)threadIdx.x / nv, cv = (int)threadIdx.x - r * nv;
    if (r >= rows_per_block) return;
    const int m = blockIdx.x * rows_per_block + r;
    if (m >= M) return;
    float a[EV], b[EV];
    load_f32v<EV>(word + (size_t)ids[m] * H + cv * EV, a);
    load_f32v<EV>(pos + (size_t)pos_ids[m] * H + cv * EV, b);
#pragma unroll
    for (int k = 0; k < EV; ++k) a[k] += b[k];
    vio<T>::store(out + (size_t)m * H + cv * EV, a);
}

extern "C" int morec_opt_embed_fwd(const int32_t* ids, const int32_t* pos_ids, const float* word, const float* pos, void* out,
                                   int M, int H, int dtype, void* stream) {
    if (!ids || !pos_ids || !word || !pos || !out || M <= 0 || H <= 0) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && dtype != MOREC_BF16 && dtype != MOREC_F16) return MOREC_E_DTYPE;
    const int ev = dtype == MOREC_F32 ? 4 : 8;
    if (H % ev || H / ev > 256) return MOREC_E_UNSUPPORTED;      // one 16-byte vector per thread, one row inside a block
    if (!aligned16(word) || !aligned16(pos) || !aligned16(out)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rpb = 256 / (H / ev);
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        hipLaunchKernelGGL((opt_embed_fwd_kernel<T>), dim3((M + rpb - 1) / rpb), dim3(256), 0, s, ids, pos_ids, word, pos, (T*)out, M, H,
                           rpb);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// Rows of title n: n*T .. n*T + T - 1 (padded layout, cu == nullptr) or cu[n] .. cu[n+1] - 1 (packed layout).
__device__ __forceinline__ void title_rows(const int32_t* __restrict__ cu, int n, int Tlen, int& r0, int& r1) {
    if (cu) {
        r0 = cu[n];
        r1 = cu[n + 1];
    } else {
        r0 = n * Tlen;
        r1 = r0 + Tlen;
    }
}

// out[n] = sum of the kept rows of title n / max(count, 1e-9) (Text_Encoder_mean: sum(h * mask) / clamp(sum(mask), 1e-9)).  A block
// owns 256 / nv titles and a thread one 16-byte column vector of one title: it walks the title's rows in order with a running fp32
// sum (two rows in flight), so the summation order is the row order whatever the launch looks like.  The count is the number of
// rows with keep != 0 -- never the packed length: a title without a real token keeps one packed row, which is pooled out.
template <typename T>
__global__ __launch_bounds__(256) void masked_mean_fwd_kernel(const T* __restrict__ x, const float* __restrict__ keep,
                                                              const int32_t* __restrict__ cu, T* __restrict__ out, int n_seq, int Tlen,
                                                              int H, int seq_per_block) {
    constexpr int EV = vio<T>::EV;
    const int nv = H / EV;
    const int q = (int)threadIdx.x / nv, cv = (int)threadIdx.x - q * nv;
    if (q >= seq_per_block) return;
    const int n = blockIdx.x * seq_per_block + q;
    if (n >= n_seq) return;
    int r0, r1;
    title_rows(cu, n, Tlen, r0, r1);
    float acc[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) acc[k] = 0.f;
    int count = 0;
    const T* base = x + (size_t)cv * EV;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    int r = r0;
    for (; r + 1 < r1; r += 2) {
        const bool k0 = keep[r] != 0.f, k1 = keep[r + 1] != 0.f;
        const uint4 v0 = k0 ? vio<T>::load_raw(base + (size_t)r * H) : zero4;
        const uint4 v1 = k1 ? vio<T>::load_raw(base + (size_t)(r + 1) * H) : zero4;
        float e[EV];
        if (k0) {
            vio<T>::unpack(v0, e);
#pragma unroll
            for (int k = 0; k < EV; ++k) acc[k] += e[k];
            ++count;
        }
        if (k1) {
            vio<T>::unpack(v1, e);
#pragma unroll
            for (int k = 0; k < EV; ++k) acc[k] += e[k];
            ++count;
        }
    }
    if (r < r1 && keep[r] != 0.f) {
        float e[EV];
        vio<T>::load(base + (size_t)r * H, e);
#pragma unroll
        for (int k = 0; k < EV; ++k) acc[k] += e[k];
        ++count;
    }
    const float den = fmaxf((float)count, 1e-9f);
#pragma unroll
    for (int k = 0; k < EV; ++k) acc[k] = acc[k] / den;
    vio<T>::store(out + (size_t)n * H + cv * EV, acc);
}

// dx[row] = keep[row] ? g[n] / count : 0 for every row of title n.  The block layout of the forward; a thread counts its title's kept
// rows, forms the quotient once and writes it (or zeros) to each row.
template <typename T>
__global__ __launch_bounds__(256) void masked_mean_bwd_kernel(const T* __restrict__ g, const float* __restrict__ keep,
                                                              const int32_t* __restrict__ cu, T* __restrict__ dx, int n_seq, int Tlen,
                                                              int H, int seq_per_block) {
    constexpr int EV = vio<T>::EV;
    const int nv = H / EV;
    const int q = (int)threadIdx.x / nv, cv = (int)threadIdx.x - q * nv;
    if (q >= seq_per_block) return;
    const int n = blockIdx.x * seq_per_block + q;
    if (n >= n_seq) return;
    int r0, r1;
    title_rows(cu, n, Tlen, r0, r1);
    int count = 0;
    for (int r = r0; r < r1; ++r) count += keep[r] != 0.f ? 1 : 0;
    float gv[EV], zero[EV];
    vio<T>::load(g + (size_t)n * H + cv * EV, gv);
    const float den = fmaxf((float)count, 1e-9f);
#pragma unroll
    for (int k = 0; k < EV; ++k) {
        gv[k] = gv[k] / den;
        zero[k] = 0.f;
    }
    T* base = dx + (size_t)cv * EV;
    for (int r = r0; r < r1; ++r) {
        if (keep[r] != 0.f) vio<T>::store(base + (size_t)r * H, gv);
        else vio<T>::store(base + (size_t)r * H, zero);
    }
}

static int masked_mean_check(const void* a, const float* keep, const void* b, int n_seq, int T, int H, int dtype) {
    if (!a || !keep || !b || n_seq <= 0 || T <= 0 || H <= 0) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && dtype != MOREC_BF16 && dtype != MOREC_F16) return MOREC_E_DTYPE;
    const int ev = dtype == MOREC_F32 ? 4 : 8;
    if (H % ev || H / ev > 256) return MOREC_E_UNSUPPORTED;
    if (!aligned16(a) || !aligned16(b)) return MOREC_E_ALIGN;
    return MOREC_OK;
}

extern "C" int morec_masked_mean_fwd(const void* x, const float* keep, const int32_t* cu, void* out, int n_seq, int T, int H,
                                     int dtype, void* stream) {
    const int rc = masked_mean_check(x, keep, out, n_seq, T, H, dtype);
    if (rc != MOREC_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int spb = 256 / (H / (dtype == MOREC_F32 ? 4 : 8));
    by_dtype(dtype, [&](auto* t) {
        using T_ = MOREC_TAG_T(t);
        hipLaunchKernelGGL((masked_mean_fwd_kernel<T_>), dim3((n_seq + spb - 1) / spb), dim3(256), 0, s, (const T_*)x, keep, cu, (T_*)out,
                           n_seq, T, H, spb);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_masked_mean_bwd(const void* g, const float* keep, const int32_t* cu, void* dx, int n_seq, int T, int H,
                                     int dtype, void* stream) {
    const int rc = masked_mean_check(g, keep, dx, n_seq, T, H, dtype);
    if (rc != MOREC_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int spb = 256 / (H / (dtype == MOREC_F32 ? 4 : 8));
    by_dtype(dtype, [&](auto* t) {
        using T_ = MOREC_TAG_T(t);
        hipLaunchKernelGGL((masked_mean_bwd_kernel<T_>), dim3((n_seq + spb - 1) / spb), dim3(256), 0, s, (const T_*)g, keep, cu, (T_*)dx,
                           n_seq, T, H, spb);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
