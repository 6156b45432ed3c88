// fuse.hip -- ID (+) modality fusion of item vectors (bce_text/id_plus_mo-end2end/model/encoders.py:8-39, model.py:43-47):
//   ADD: out = id_embedding(id) + encoder(content)                        -> fuse_add_fwd (backward: the output gradient itself and
//        morec_scatter_add_rows into the id table);
//   CAT: Dropout(cat([id_embedding(id), encoder(content)], 1)) -> Linear -> GELU (x 1 or 3): the gather, the concatenation and the first
//        Dropout in one pass (fuse_cat_fwd), the GEMMs are morec_gemm_nt; the backward splits the GEMM's input gradient into the content
//        gradient and the id-table scatter in one pass (fuse_cat_bwd).  dropout_apply: the Dropouts between the layers of the 3-layer MLP.
// One wave per row, four rows per workgroup, one 16-byte vector per lane and trip (embed.hip).  Masks are regenerated from (p, seed, element
// index), never stored.  Products that enter a sum are taken with __fmul_rn: a contraction into an FMA would make the deterministic scatter
// differ from "round the term, then add" by the last bit.
#include "common.hpp"

template <typename T>
__global__ __launch_bounds__(256) void fuse_add_fwd_kernel(const float* __restrict__ table, const int32_t* __restrict__ idx,
                                                           const T* __restrict__ content, T* __restrict__ out, int R, int D) {
    constexpr int EV = vio<T>::EV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float* src = table + (size_t)idx[row] * D;      // the pad row is a row like any other (model.py:39 overwrites it, :43 reads it)
    const size_t base = (size_t)row * D;
    for (int c = lane * EV; c < D; c += 64 * EV) {
        float a[EV], b[EV];
        load_f32v<EV>(src + c, a);
        vio<T>::load(content + base + c, b);
#pragma unroll
        for (int k = 0; k < EV; ++k) a[k] += b[k];
        vio<T>::store(out + base + c, a);
    }
}

extern "C" int morec_fuse_add_fwd(const float* table, const int32_t* idx, const void* content, void* out, int R, int D, int dtype,
                                  void* stream) {
    if (!table || !idx || !content || !out || R <= 0 || D <= 0) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (D % (dtype == MOREC_F32 ? 4 : 8)) return MOREC_E_ALIGN;
    if (!aligned16(table) || !aligned16(content) || !aligned16(out)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((R + 3) / 4);
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        hipLaunchKernelGGL((fuse_add_fwd_kernel<T>), grid, dim3(256), 0, s, table, idx, (const T*)content, (T*)out, R, D);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// a[r, 0:D] = drop(table[idx[r]]), a[r, D:2D] = drop(content[r]): ONE dropout stream over the [R, 2D] matrix (element index = position in it).
// D % EV == 0, so a lane's vector lies on one side of column D.
template <typename T>
__global__ __launch_bounds__(256) void fuse_cat_fwd_kernel(const float* __restrict__ table, const int32_t* __restrict__ idx,
                                                           const T* __restrict__ content, T* __restrict__ a_out, int R, int D, DropRng dr) {
    dr = drop_resolve(dr);
    constexpr int EV = vio<T>::EV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float* src = table + (size_t)idx[row] * D;
    const size_t base = (size_t)row * 2 * D;
    for (int c = lane * EV; c < 2 * D; c += 64 * EV) {
        float v[EV];
        if (c < D) load_f32v<EV>(src + c, v);
        else vio<T>::load(content + (size_t)row * D + (c - D), v);
        if (dr.thresh) {
            bool kp[EV];
            drop_keep_vec<EV>(dr, base + c, kp);
#pragma unroll
            for (int k = 0; k < EV; ++k) v[k] = kp[k] ? __fmul_rn(v[k], dr.inv_keep) : 0.f;
        }
        vio<T>::store(a_out + base + c, v);
    }
}

extern "C" int morec_fuse_cat_fwd(const float* table, const int32_t* idx, const void* content, void* a_out, int R, int D, int dtype,
                                  float p, uint64_t seed, void* stream) {
    if (!table || !idx || !content || !a_out || R <= 0 || D <= 0) return MOREC_E_ARG;
    if (!(p >= 0.f && p < 1.f)) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (D % (dtype == MOREC_F32 ? 4 : 8)) return MOREC_E_ALIGN;
    if (!aligned16(table) || !aligned16(content) || !aligned16(a_out)) return MOREC_E_ALIGN;
    const DropRng dr = make_drop(p, seed);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((R + 3) / 4);
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        hipLaunchKernelGGL((fuse_cat_fwd_kernel<T>), grid, dim3(256), 0, s, table, idx, (const T*)content, (T*)a_out, R, D, dr);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// EV elements of dA[row, c ...] through the forward's mask: keep ? dA * inv_keep : 0 (fp32, unrounded)
template <typename T>
__device__ __forceinline__ void cat_bwd_terms(const T* __restrict__ dA, const DropRng& dr, int row, int c, int D, float (&v)[vio<T>::EV]) {
    constexpr int EV = vio<T>::EV;
    const size_t e = (size_t)row * 2 * D + c;
    vio<T>::load(dA + e, v);
    if (dr.thresh) {
        bool kp[EV];
        drop_keep_vec<EV>(dr, e, kp);
#pragma unroll
        for (int k = 0; k < EV; ++k) v[k] = kp[k] ? __fmul_rn(v[k], dr.inv_keep) : 0.f;
    }
}

// d_content[r] = mask . inv_keep . dA[r, D:2D] (T);  d_table[idx[r]] += mask . inv_keep . dA[r, 0:D] (fp32) unless idx[r] == pad_id.
// DET = false: fp32 atomics (scatter_add_rows_kernel).  DET = true: the wave of row r adds to the table only when no EARLIER row carries
// the same id; it then sums the rows r, r' > r, ... with that id in row order and writes the table row alone (scatter_add_rows_det_kernel).
template <typename T, bool DET>
__global__ __launch_bounds__(256) void fuse_cat_bwd_kernel(const T* __restrict__ dA, const int32_t* __restrict__ idx,
                                                           T* __restrict__ d_content, float* __restrict__ d_table, int R, int D,
                                                           int pad_id, DropRng dr) {
    dr = drop_resolve(dr);
    constexpr int EV = vio<T>::EV;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    for (int c = lane * EV; c < D; c += 64 * EV) {
        float v[EV];
        cat_bwd_terms<T>(dA, dr, row, D + c, D, v);
        vio<T>::store(d_content + (size_t)row * D + c, v);
    }
    const int id = idx[row];
    if (id == pad_id) return;
    float* dst = d_table + (size_t)id * D;
    if (!DET) {
        // four columns per lane whatever the type (scatter_add_rows_kernel's layout): one atomic instruction of the wave then covers 1 KiB of the
        // table row; with the eight columns of a 16-byte half vector it covered 2 KiB and ran 1.4 x slower than the unfused scatter
        // (profiles/fusion_kernels.txt)
        for (int c = lane * 4; c < D; c += 256) {
            const size_t e = (size_t)row * 2 * D + c;
            float v[4];
            io<T>::load4(dA + e, v);
            if (dr.thresh) {
                bool kp[4];
                drop_keep_vec<4>(dr, e, kp);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = kp[k] ? __fmul_rn(v[k], dr.inv_keep) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(dst + c + k, v[k]);
        }
        return;
    }
    bool dup = false;
    for (int r0 = 0; r0 < row && !dup; r0 += 64) {
        const int r = r0 + lane;
        dup = __ballot(r < row && idx[r] == id) != 0ull;
    }
    if (dup) return;
    for (int c0 = 0; c0 < D; c0 += 64 * EV) {      // wave-uniform trip count: every lane takes part in the ballots below
        const int c = c0 + lane * EV;
        const bool mine = c < D;
        float acc[EV];
#pragma unroll
        for (int k = 0; k < EV; ++k) acc[k] = 0.f;
        for (int r0 = row; r0 < R; r0 += 64) {      // 64 candidate rows at a time: ALL lanes test, the wave walks the hits in order
            const int r = r0 + lane;
            unsigned long long hit = __ballot(r < R && idx[r] == id);
            while (hit) {
                const int b = __builtin_ctzll(hit);
                hit &= hit - 1;
                if (mine) {
                    float v[EV];
                    cat_bwd_terms<T>(dA, dr, r0 + b, c, D, v);
#pragma unroll
                    for (int k = 0; k < EV; ++k) acc[k] += v[k];
                }
            }
        }
        if (mine) {
            float o[EV];
            load_f32v<EV>(dst + c, o);
#pragma unroll
            for (int k = 0; k < EV; ++k) o[k] += acc[k];
            store_f32v<EV>(dst + c, o);
        }
    }
}

extern "C" int morec_fuse_cat_bwd(const void* dA, const int32_t* idx, void* d_content, float* d_table, int R, int D, int pad_id,
                                  int dtype, float p, uint64_t seed, void* stream) {
    if (!dA || !idx || !d_content || !d_table || R <= 0 || D <= 0) return MOREC_E_ARG;
    if (!(p >= 0.f && p < 1.f)) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (D % (dtype == MOREC_F32 ? 4 : 8)) return MOREC_E_ALIGN;
    if (!aligned16(dA) || !aligned16(d_content) || !aligned16(d_table)) return MOREC_E_ALIGN;
    const DropRng dr = make_drop(p, seed);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((R + 3) / 4);
    const bool det = morec_deterministic();
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        if (det) hipLaunchKernelGGL((fuse_cat_bwd_kernel<T, true>), grid, dim3(256), 0, s, (const T*)dA, idx, (T*)d_content, d_table, R, D, pad_id, dr);
        else hipLaunchKernelGGL((fuse_cat_bwd_kernel<T, false>), grid, dim3(256), 0, s, (const T*)dA, idx, (T*)d_content, d_table, R, D, pad_id, dr);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// out[e] = keep(e) ? x[e] * inv_keep : 0 over n elements (out may be x): whole 16-byte vectors, then the n % EV elements behind them
template <typename T>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const T* x, T* out, size_t n, DropRng dr) {
    dr = drop_resolve(dr);
    constexpr int EV = vio<T>::EV;
    const size_t nv = n / EV;
    const size_t tid = blockIdx.x * (size_t)256 + threadIdx.x, nthr = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < nv; i += nthr) {
        float v[EV];
        bool kp[EV];
        vio<T>::load(x + i * EV, v);
        drop_keep_vec<EV>(dr, i * EV, kp);
#pragma unroll
        for (int k = 0; k < EV; ++k) v[k] = kp[k] ? __fmul_rn(v[k], dr.inv_keep) : 0.f;
        vio<T>::store(out + i * EV, v);
    }
    for (size_t e = nv * EV + tid; e < n; e += nthr)
        io<T>::store1(out + e, drop_keep(dr, e) ? __fmul_rn(io<T>::load1(x + e), dr.inv_keep) : 0.f);
}

extern "C" int morec_dropout_apply(const void* x, void* out, size_t n, float p, uint64_t seed, int dtype, void* stream) {
    if (!x || !out || n == 0) return MOREC_E_ARG;
    if (!(p >= 0.f && p < 1.f)) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (!aligned16(x) || !aligned16(out)) return MOREC_E_ALIGN;
    const DropRng dr = make_drop(p, seed);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t nv = n / (dtype == MOREC_F32 ? 4 : 8) + 1, blocks = (nv + 255) / 256;
    dim3 grid((unsigned)(blocks > 4096 ? 4096 : blocks));
    by_dtype(dtype, [&](auto* t) {
        using T = MOREC_TAG_T(t);
        hipLaunchKernelGGL((dropout_apply_kernel<T>), grid, dim3(256), 0, s, (const T*)x, (T*)out, n, dr);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
