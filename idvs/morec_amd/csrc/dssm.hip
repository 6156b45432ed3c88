// dssm.hip -- scoring loss of the DSSM two-tower model (bce_text/main-end2end(DSSM)/model/model.py: bmm of every user's 1 + neg_num
// sampled item vectors with the user vector, BCEWithLogitsLoss over all scores).
//   U [B, D] user vectors, E [R, D] item vectors (R = B n1, n1 = 1 + neg_num; user b owns rows b n1 .. b n1 + n1 - 1), labels fp32 [R].
//   scores[r] = U[r / n1] . E[r];  terms[r] = softplus(s) - y s;  loss_sum = sum_r terms[r]
//   c_r = g (sigmoid(s_r) - y_r);  dE[r] = c_r U[r / n1];  dU[b] = sum_j c_{b,j} E[b, j]
// No atomics anywhere: every output element has one writer and every sum a fixed order, so the bits do not depend on the schedule
// (nor on MOREC_DETERMINISTIC).  HBM / launch bound: the forward reads U and E once, the backward reads them once and writes dU, dE once.
#include "common.hpp"

namespace {
// EV elements per lane and access: 8 = one 16-byte load of a 16-bit type (needs D % 8 == 0), 4 = 16 bytes of fp32 / 8 bytes of a 16-bit type
template <typename T, int EV>
__device__ __forceinline__ void ld(const T* p, float (&o)[EV]) {
    if constexpr (EV == 4) io<T>::load4(p, o);
    else vio<T>::load(p, o);
}
template <typename T, int EV>
__device__ __forceinline__ void st(T* p, const float (&o)[EV]) {
    if constexpr (EV == 4) io<T>::store4(p, o);
    else vio<T>::store(p, o);
}

__device__ __forceinline__ float label_of(const float* labels, int r, int j) { return labels ? labels[r] : (j == 0 ? 1.f : 0.f); }

// softplus(s) - y s without the cancellation of the literal form at large |s|: max(s, 0) - y s is ONE rounding (exactly 0 at y = 1, s > 0),
// and log1p(exp(-|s|)) is the overflow-safe tail of softplus_f (inbatch_ce.hip)
__device__ __forceinline__ float bce_term(float s, float y) { return fmaf(-y, s, fmaxf(s, 0.f)) + log1pf(expf(-fabsf(s))); }

// sigmoid(s) - y with e = exp(-|s|) <= 1: nothing overflows, and with a hard label there is no subtraction of near-equal numbers
// (y = 1, s >> 0 and y = 0, s << 0 give exactly 0 once e underflows)
__device__ __forceinline__ float bce_dscore(float s, float y) {
    const float e = expf(-fabsf(s));
    const float num = s >= 0.f ? (1.f - y) - y * e : (1.f - y) * e - y;
    return num / (1.f + e);
}

// One wave per item row; four rows per block.
template <typename T, int EV>
__global__ __launch_bounds__(256) void dssm_bce_fwd_kernel(const T* __restrict__ U, const T* __restrict__ E, const float* __restrict__ labels,
                                                           float* __restrict__ scores, float* __restrict__ terms, int R, int n1, int D) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int b = r / n1;
    const T* u = U + (size_t)b * D;
    const T* e = E + (size_t)r * D;
    float s = 0.f;
    for (int c = lane * EV; c < D; c += 64 * EV) {
        float x[EV], y[EV];
        ld<T, EV>(u + c, x); ld<T, EV>(e + c, y);
#pragma unroll
        for (int k = 0; k < EV; ++k) s = fmaf(x[k], y[k], s);
    }
    s = wave_sum(s);
    if (lane == 0) {
        scores[r] = s;
        terms[r] = bce_term(s, label_of(labels, r, r - b * n1));
    }
}

// loss_sum[0] = sum of terms[0 .. R): one block, thread t adds the elements t, t + 1024, ... in ascending order (four independent partial
// sums so that the loads overlap), then a fixed tree over the 1024 partial sums.  The single writer of loss_sum.
__global__ __launch_bounds__(1024) void dssm_bce_fold_kernel(const float* __restrict__ terms, float* __restrict__ loss_sum, int R) {
    __shared__ float sh[1024];
    const int t = threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (long long i = t; i < R; i += 4096) {
        a0 += terms[i];
        if (i + 1024 < R) a1 += terms[i + 1024];
        if (i + 2048 < R) a2 += terms[i + 2048];
        if (i + 3072 < R) a3 += terms[i + 3072];
    }
    sh[t] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    if (t == 0) loss_sum[0] = sh[0];
}

// One block per (user b, chunk of 64 EV columns, segment of the user's rows), W = blockDim.x / 64 waves: wave w takes the segment's rows
// j = j0 + w, j0 + w + W, ... -- it writes its dE rows and keeps c_j E[b, j] in registers, j ascending; the W partial sums meet in LDS and
// wave 0 adds them in wave order.  With one segment per user (gridDim.y == 1) that sum is dU and is written once, as T.  With several
// (few users, n1 in the hundreds: the launcher cuts a user's rows into segments until the grid covers the card) it goes, in fp32, to
// part[b][segment][D], and dssm_bce_dU_fold_kernel adds a user's segments in ascending order and writes dU once.
template <typename T, int EV>
__global__ __launch_bounds__(1024) void dssm_bce_bwd_kernel(const T* __restrict__ U, const T* __restrict__ E, const float* __restrict__ labels,
                                                            const float* __restrict__ scores, const float* __restrict__ gscale,
                                                            T* __restrict__ dU, T* __restrict__ dE, float* __restrict__ part_out, int n1, int D,
                                                            int nchunk, int rows_per) {
    extern __shared__ __attribute__((aligned(16))) float part[];      // [W][EV][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
    const int b = blockIdx.x / nchunk;
    const int c = (blockIdx.x - b * nchunk) * 64 * EV + lane * EV;
    const bool in = c < D;
    const float g = gscale[0];
    float u[EV], acc[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) { u[k] = 0.f; acc[k] = 0.f; }
    if (in) ld<T, EV>(U + (size_t)b * D + c, u);
    const int j0 = blockIdx.y * rows_per, j1 = min(n1, j0 + rows_per);
    for (int j = j0 + w; j < j1; j += W) {
        const int r = b * n1 + j;
        const float coef = g * bce_dscore(scores[r], label_of(labels, r, j));
        if (in) {
            float e[EV], o[EV];
            ld<T, EV>(E + (size_t)r * D + c, e);
#pragma unroll
            for (int k = 0; k < EV; ++k) { o[k] = coef * u[k]; acc[k] = fmaf(coef, e[k], acc[k]); }
            st<T, EV>(dE + (size_t)r * D + c, o);
        }
    }
    if (W > 1) {
#pragma unroll
        for (int k = 0; k < EV; ++k) part[(w * EV + k) * 64 + lane] = acc[k];
        __syncthreads();
        if (w != 0) return;
#pragma unroll
        for (int k = 0; k < EV; ++k) {
            float t = part[k * 64 + lane];
            for (int q = 1; q < W; ++q) t += part[(q * EV + k) * 64 + lane];
            acc[k] = t;
        }
    }
    if (!in) return;
    if (part_out) store_f32v<EV>(part_out + ((size_t)b * gridDim.y + blockIdx.y) * D + c, acc);
    else st<T, EV>(dU + (size_t)b * D + c, acc);
}

// dU[b] = part[b][0] + part[b][1] + ... (segments ascending), four columns per thread
template <typename T>
__global__ __launch_bounds__(256) void dssm_bce_dU_fold_kernel(const float* __restrict__ part, T* __restrict__ dU, int B, int D, int nseg) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;      // index of a group of four columns
    const int d4 = D >> 2;
    if (q >= (long long)B * d4) return;
    const int b = (int)(q / d4), c = (int)(q - (long long)b * d4) * 4;
    float acc[4], v[4];
    load_f32v<4>(part + (size_t)b * nseg * D + c, acc);
    for (int k = 1; k < nseg; ++k) {
        load_f32v<4>(part + ((size_t)b * nseg + k) * D + c, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += v[i];
    }
    io<T>::store4(dU + (size_t)b * D + c, acc);
}

// 16-byte accesses of a 16-bit type need rows that start on 16 bytes
static inline int dssm_ev(int dtype, int D) { return (is_h16(dtype) && D % 8 == 0) ? 8 : 4; }
static inline int dssm_check(int B, int n1, int D, int dtype) {
    if (B < 1 || n1 < 1 || D < 1 || (long long)B * n1 > 0x7fffffffLL) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (D % 4) return MOREC_E_ALIGN;
    return MOREC_OK;
}
}  // namespace

extern "C" int morec_dssm_bce_fwd(const void* U, const void* E, const float* labels, float* scores, float* terms, float* loss_sum, int B,
                                  int n1, int D, int dtype, void* stream) {
    if (!U || !E || !scores || !terms || !loss_sum) return MOREC_E_ARG;
    if (const int rc = dssm_check(B, n1, D, dtype)) return rc;
    if (!aligned16(U) || !aligned16(E)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int R = B * n1;
    const dim3 grid((R + 3) / 4);
    const bool wide = dssm_ev(dtype, D) == 8;
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        if constexpr (std::is_same<T, float>::value) {
            hipLaunchKernelGGL((dssm_bce_fwd_kernel<T, 4>), grid, dim3(256), 0, s, (const T*)U, (const T*)E, labels, scores, terms, R, n1, D);
        } else {
            if (wide) hipLaunchKernelGGL((dssm_bce_fwd_kernel<T, 8>), grid, dim3(256), 0, s, (const T*)U, (const T*)E, labels, scores, terms, R, n1, D);
            else hipLaunchKernelGGL((dssm_bce_fwd_kernel<T, 4>), grid, dim3(256), 0, s, (const T*)U, (const T*)E, labels, scores, terms, R, n1, D);
        }
    });
    MOREC_CHECK_LAUNCH();
    hipLaunchKernelGGL(dssm_bce_fold_kernel, dim3(1), dim3(1024), 0, s, (const float*)terms, loss_sum, R);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_dssm_bce_bwd(const void* U, const void* E, const float* labels, const float* scores, const float* gscale, void* dU,
                                  void* dE, int B, int n1, int D, int dtype, void* stream) {
    if (!U || !E || !scores || !gscale || !dU || !dE) return MOREC_E_ARG;
    if (const int rc = dssm_check(B, n1, D, dtype)) return rc;
    if (!aligned16(U) || !aligned16(E) || !aligned16(dU) || !aligned16(dE)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ev = dssm_ev(dtype, D);
    const int nchunk = (D + 64 * ev - 1) / (64 * ev);
    if ((long long)B * nchunk > 0x7fffffffLL) return MOREC_E_ARG;
    const int W = n1 == 1 ? 1 : n1 == 2 ? 2 : n1 <= 8 ? 4 : n1 <= 32 ? 8 : 16;      // waves per user: at most ~n1 / 2 rows each up to 32, then 16
    // few users with many rows each: cut a user's rows into segments (at least one row per wave) until about 256 workgroups exist
    int rows_per = n1, nseg = 1;
    const long long blocks = (long long)B * nchunk;
    const int max_seg = n1 / W;
    if (blocks < 256 && max_seg >= 2) {
        const long long want = (256 + blocks - 1) / blocks;
        const int seg = (int)(want < max_seg ? want : max_seg);
        rows_per = (n1 + seg - 1) / seg;
        nseg = (n1 + rows_per - 1) / rows_per;
    }
    float* part = nullptr;
    if (nseg > 1) {
        part = morec_det_scratch(s, (size_t)B * nseg * D);
        if (!part || !aligned16(part)) {      // no scratch (a stream under capture that has none yet): one segment per user is always possible
            part = nullptr;
            nseg = 1;
            rows_per = n1;
        }
    }
    const dim3 grid(B * nchunk, nseg), block(64 * W);
    const size_t lds = W > 1 ? (size_t)W * ev * 64 * sizeof(float) : 0;
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        if constexpr (std::is_same<T, float>::value) {
            hipLaunchKernelGGL((dssm_bce_bwd_kernel<T, 4>), grid, block, lds, s, (const T*)U, (const T*)E, labels, scores, gscale, (T*)dU, (T*)dE, part, n1, D, nchunk, rows_per);
        } else {
            if (ev == 8) hipLaunchKernelGGL((dssm_bce_bwd_kernel<T, 8>), grid, block, lds, s, (const T*)U, (const T*)E, labels, scores, gscale, (T*)dU, (T*)dE, part, n1, D, nchunk, rows_per);
            else hipLaunchKernelGGL((dssm_bce_bwd_kernel<T, 4>), grid, block, lds, s, (const T*)U, (const T*)E, labels, scores, gscale, (T*)dU, (T*)dE, part, n1, D, nchunk, rows_per);
        }
    });
    MOREC_CHECK_LAUNCH();
    if (nseg > 1) {
        const long long groups = (long long)B * (D / 4);
        by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((dssm_bce_dU_fold_kernel<T>), dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, (const float*)part, (T*)dU, B, D, nseg);
        });
    }
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
