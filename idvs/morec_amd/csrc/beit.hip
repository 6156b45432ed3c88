// beit.hip -- the small kernels of the BEiT item tower (HF modeling_beit.py): the relative-position table <-> the [heads][T][Tp] bias of
// morec_attn_bias_fwd, layer scale fused with the residual add, the mean-pool head over the patch tokens, [CLS] assembly.
// The attention itself is attention_stream.hip (BIAS = true); the [CLS] backward is morec_mae_assemble_bwd (the plain row copy + the
// ordered [CLS] sum, no position pass).
#include <algorithm>
#include "common.hpp"

namespace {
constexpr int KT = 64;      // key-tile width of morec_attn_bias_*: rows of the expanded bias are padded to it

__host__ __device__ inline int beit_tp(int T) { return (T + KT - 1) / KT * KT; }

// BeitRelativePositionBias.generate_relative_position_index: token 0 is [CLS], token 1 + y * g + x the patch (y, x)
__device__ __forceinline__ int beit_rel_index(int i, int j, int g) {
    const int R = 2 * g - 1, nrd = R * R + 3;
    if (i == 0) return j == 0 ? nrd - 1 : nrd - 3;      // cls -> cls | cls -> token
    if (j == 0) return nrd - 2;                         // token -> cls
    const int yi = (i - 1) / g, xi = (i - 1) % g, yj = (j - 1) / g, xj = (j - 1) % g;
    return (yi - yj + g - 1) * R + (xi - xj + g - 1);
}

__global__ void beit_bias_expand_kernel(const float* __restrict__ table, float* __restrict__ bias, int g, int heads) {
    const int T = g * g + 1, Tp = beit_tp(T);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= heads * T * Tp) return;
    const int h = e / (T * Tp), r = e - h * T * Tp;
    const int i = r / Tp, j = r - i * Tp;
    bias[e] = j < T ? table[beit_rel_index(i, j, g) * heads + h] : 0.f;
}

// dtable[rel][h] += the cells behind the entry: ONE thread per table entry gathers them in a fixed order (swin_bias_reduce_kernel's plan)
__global__ void beit_bias_reduce_kernel(const float* __restrict__ dbias, float* __restrict__ dtable, int g, int heads) {
    const int T = g * g + 1, Tp = beit_tp(T), R = 2 * g - 1, nrd = R * R + 3;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nrd * heads) return;
    const int rel = e / heads, h = e - rel * heads;
    const float* d = dbias + (size_t)h * T * Tp;
    float acc = 0.f;
    if (rel == nrd - 1) {
        acc = d[0];
    } else if (rel == nrd - 3) {
        for (int j = 1; j < T; ++j) acc += d[j];
    } else if (rel == nrd - 2) {
        for (int i = 1; i < T; ++i) acc += d[(size_t)i * Tp];
    } else {
        const int dy = rel / R - (g - 1), dx = rel % R - (g - 1);      // yi - yj, xi - xj of every pair behind this entry
        for (int yi = 0; yi < g; ++yi) {
            const int yj = yi - dy;
            if (yj < 0 || yj >= g) continue;
            for (int xi = 0; xi < g; ++xi) {
                const int xj = xi - dx;
                if (xj < 0 || xj >= g) continue;
                acc += d[(size_t)(1 + yi * g + xi) * Tp + (1 + yj * g + xj)];
            }
        }
    }
    dtable[e] += acc;
}

// ---- layer scale + residual: h = res + rowscale[row / rps] * (lam * (a + bias)), HF's order (lambda * output, then DropPath, then the
// residual), every step in fp32 without contraction and one rounding to the storage type
template <typename T>
__global__ __launch_bounds__(256) void layerscale_res_fwd_kernel(const T* __restrict__ a, const float* __restrict__ bias,
                                                                 const float* __restrict__ lam, const T* __restrict__ res,
                                                                 const float* __restrict__ rowscale, int rps, T* __restrict__ out, size_t M,
                                                                 int N) {
#pragma clang fp contract(off)
    constexpr int EV = vio<T>::EV;
    const int vpr = N / EV;
    const size_t total = M * vpr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        float v[EV], r[EV], b[EV], l[EV];
        vio<T>::load(a + row * N + c, v);
        vio<T>::load(res + row * N + c, r);
        load_f32v<EV>(bias + c, b);
        load_f32v<EV>(lam + c, l);
        const float sc = rowscale ? rowscale[row / rps] : 1.f;
#pragma unroll
        for (int k = 0; k < EV; ++k) {
            float u = l[k] * (v[k] + b[k]);
            if (rowscale) u = u * sc;
            v[k] = r[k] + u;
        }
        vio<T>::store(out + row * N + c, v);
    }
}

constexpr int LS_CL = 8;          // column lanes of a block (16 bytes each)
constexpr int LS_RL = 32;         // row lanes
constexpr int LS_SLAB = 1024;     // rows of a block

// da = dh * rowscale * lam (storage type) and, per slab of LS_SLAB rows, the column sums of dh * rowscale * (a + bias) and of dh * rowscale:
// a row lane adds its rows in ascending order, then a fixed binary tree over the 32 row lanes.  part[slab][2][N].
template <typename T>
__global__ __launch_bounds__(256) void layerscale_res_bwd_kernel(const T* __restrict__ dh, const T* __restrict__ a, const float* __restrict__ bias,
                                                                 const float* __restrict__ lam, const float* __restrict__ rowscale, int rps,
                                                                 T* __restrict__ da, float* __restrict__ part, size_t M, int N) {
    constexpr int EV = vio<T>::EV;
    __shared__ float red[2][LS_RL][LS_CL * EV];
    const int cl = threadIdx.x % LS_CL, rl = threadIdx.x / LS_CL;
    const int c = (blockIdx.x * LS_CL + cl) * EV;
    const bool live = c < N;
    const size_t r0 = (size_t)blockIdx.y * LS_SLAB, r1 = std::min<size_t>(r0 + LS_SLAB, M);
    float s_l[EV], s_b[EV], l[EV], b[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) { s_l[k] = 0.f; s_b[k] = 0.f; l[k] = 0.f; b[k] = 0.f; }
    if (live) {
        load_f32v<EV>(lam + c, l);
        if (part) load_f32v<EV>(bias + c, b);
        for (size_t row = r0 + rl; row < r1; row += LS_RL) {
            float g[EV], o[EV];
            vio<T>::load(dh + row * N + c, g);
            const float sc = rowscale ? rowscale[row / rps] : 1.f;
#pragma unroll
            for (int k = 0; k < EV; ++k) {
                g[k] *= sc;
                o[k] = g[k] * l[k];
            }
            vio<T>::store(da + row * N + c, o);
            if (part) {
                float v[EV];
                vio<T>::load(a + row * N + c, v);
#pragma unroll
                for (int k = 0; k < EV; ++k) {
                    s_l[k] += g[k] * (v[k] + b[k]);
                    s_b[k] += g[k];
                }
            }
        }
    }
    if (!part) return;
#pragma unroll
    for (int k = 0; k < EV; ++k) { red[0][rl][cl * EV + k] = s_l[k]; red[1][rl][cl * EV + k] = s_b[k]; }
    __syncthreads();
    for (int s = LS_RL / 2; s > 0; s >>= 1) {
        if (rl < s) {
#pragma unroll
            for (int k = 0; k < EV; ++k) {
                red[0][rl][cl * EV + k] += red[0][rl + s][cl * EV + k];
                red[1][rl][cl * EV + k] += red[1][rl + s][cl * EV + k];
            }
        }
        __syncthreads();
    }
    if (rl == 0 && live) {
#pragma unroll
        for (int k = 0; k < EV; ++k) {
            part[((size_t)blockIdx.y * 2 + 0) * N + c + k] = red[0][0][cl * EV + k];
            part[((size_t)blockIdx.y * 2 + 1) * N + c + k] = red[1][0][cl * EV + k];
        }
    }
}

// dlam[c] += sum over the slabs, in slab order; dbias[c] += lam[c] * the same of the second sums
__global__ __launch_bounds__(256) void layerscale_fold_kernel(const float* __restrict__ part, const float* __restrict__ lam,
                                                              float* __restrict__ dlam, float* __restrict__ dbias, int n_slab, int N) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    float sl = 0.f, sb = 0.f;
    for (int s = 0; s < n_slab; ++s) {
        sl += part[((size_t)s * 2 + 0) * N + c];
        sb += part[((size_t)s * 2 + 1) * N + c];
    }
    if (dlam) dlam[c] += sl;
    if (dbias) dbias[c] += lam[c] * sb;
}

// ---- mean-pool head: out[n] = mean over the patch tokens (rows 1 .. Tn - 1) of image n; [CLS] (row 0) is not part of the mean
template <typename T>
__global__ __launch_bounds__(256) void beit_pool_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, int n_img, int Tn, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_img * vpr) return;
    const int n = e / vpr, c = (e - n * vpr) * EV;
    float acc[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) acc[k] = 0.f;
    for (int t = 1; t < Tn; ++t) {
        float v[EV];
        vio<T>::load(x + ((size_t)n * Tn + t) * C + c, v);
#pragma unroll
        for (int k = 0; k < EV; ++k) acc[k] += v[k];
    }
    const float inv = 1.0f / (float)(Tn - 1);
#pragma unroll
    for (int k = 0; k < EV; ++k) acc[k] *= inv;
    vio<T>::store(out + (size_t)n * C + c, acc);
}
template <typename T>
__global__ __launch_bounds__(256) void beit_pool_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dx, int n_img, int Tn, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = (size_t)n_img * Tn * vpr;
    const float inv = 1.0f / (float)(Tn - 1);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        float v[EV];
        vio<T>::load(dout + (row / Tn) * C + c, v);
        const float f = (row % Tn) ? inv : 0.f;
#pragma unroll
        for (int k = 0; k < EV; ++k) v[k] *= f;
        vio<T>::store(dx + row * C + c, v);
    }
}

// ---- x[img, 0] = cls_token (fp32, rounded to the storage type), x[img, 1 + j] = e[img * N + j]
template <typename T>
__global__ __launch_bounds__(256) void beit_assemble_fwd_kernel(const T* __restrict__ e, const float* __restrict__ cls, T* __restrict__ x,
                                                                int n_img, int N, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = (size_t)n_img * (N + 1) * vpr;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t row = idx / vpr;
        const int c = (int)(idx - row * vpr) * EV;
        const size_t img = row / (N + 1), t = row - img * (N + 1);
        if (t == 0) {
            float v[EV];
            load_f32v<EV>(cls + c, v);
            vio<T>::store(x + row * C + c, v);
        } else {
            *reinterpret_cast<uint4*>(x + row * C + c) = vio<T>::load_raw(e + (img * N + t - 1) * C + c);
        }
    }
}

int check_rows(size_t M, int N, int dtype) {
    if (M == 0 || N <= 0) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (N % 8) return MOREC_E_ALIGN;      // one width rule for the three storage types: whole 16-byte lanes of the 16-bit ones
    return MOREC_OK;
}
}  // namespace

extern "C" int morec_beit_bias_expand(const float* table, float* pos_bias, int g, int heads, void* stream) {
    if (!table || !pos_bias || g <= 0 || heads <= 0) return MOREC_E_ARG;
    if (g * g + 1 > 1024) return MOREC_E_UNSUPPORTED;
    const int T = g * g + 1, n = heads * T * beit_tp(T);
    hipLaunchKernelGGL(beit_bias_expand_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), table, pos_bias, g,
                       heads);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_beit_bias_reduce(const float* d_pos_bias, float* dtable, int g, int heads, void* stream) {
    if (!d_pos_bias || !dtable || g <= 0 || heads <= 0) return MOREC_E_ARG;
    if (g * g + 1 > 1024) return MOREC_E_UNSUPPORTED;
    const int n = heads * ((2 * g - 1) * (2 * g - 1) + 3);
    hipLaunchKernelGGL(beit_bias_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_pos_bias, dtable,
                       g, heads);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_layerscale_res_fwd(const void* a, const float* bias, const float* lam, const void* res, const float* rowscale,
                                        int rows_per_scale, void* h, long M, int N, int dtype, void* stream) {
    if (!a || !bias || !lam || !res || !h || M <= 0) return MOREC_E_ARG;
    if (rowscale && (rows_per_scale <= 0 || M % rows_per_scale)) return MOREC_E_ARG;
    const int rc = check_rows((size_t)M, N, dtype);
    if (rc) return rc;
    if (!aligned16(a) || !aligned16(bias) || !aligned16(lam) || !aligned16(res) || !aligned16(h)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t total = (size_t)M * (N / (16 / elt_size(dtype)));
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((layerscale_res_fwd_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)a, bias, lam, (const T*)res,
                           rowscale, rowscale ? rows_per_scale : 1, (T*)h, (size_t)M, N);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_layerscale_res_bwd(const void* dh, const void* a, const float* bias, const float* lam, const float* rowscale,
                                        int rows_per_scale, void* da, float* dlam, float* dbias, long M, int N, int dtype, void* stream) {
    if (!dh || !lam || !da || M <= 0) return MOREC_E_ARG;
    const bool sums = dlam || dbias;
    if (sums && (!a || !bias)) return MOREC_E_ARG;
    if (rowscale && (rows_per_scale <= 0 || M % rows_per_scale)) return MOREC_E_ARG;
    const int rc = check_rows((size_t)M, N, dtype);
    if (rc) return rc;
    if (!aligned16(dh) || !aligned16(a) || !aligned16(bias) || !aligned16(lam) || !aligned16(da)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ev = 16 / elt_size(dtype);
    const int n_slab = (int)((M + LS_SLAB - 1) / LS_SLAB);
    float* part = nullptr;
    if (sums) {
        part = morec_det_scratch(s, (size_t)n_slab * 2 * N);
        if (!part) return (int)hipErrorOutOfMemory;
    }
    dim3 grid((N / ev + LS_CL - 1) / LS_CL, n_slab);
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((layerscale_res_bwd_kernel<T>), grid, dim3(256), 0, s, (const T*)dh, (const T*)a, bias, lam, rowscale,
                           rowscale ? rows_per_scale : 1, (T*)da, part, (size_t)M, N);
    });
    MOREC_CHECK_LAUNCH();
    if (sums) {
        hipLaunchKernelGGL(layerscale_fold_kernel, dim3((N + 255) / 256), dim3(256), 0, s, part, lam, dlam, dbias, n_slab, N);
        MOREC_CHECK_LAUNCH();
    }
    return MOREC_OK;
}

extern "C" int morec_beit_pool_fwd(const void* x, void* out, int n_img, int T, int C, int dtype, void* stream) {
    if (!x || !out || n_img <= 0 || T < 2) return MOREC_E_ARG;
    const int rc = check_rows((size_t)n_img, C, dtype);
    if (rc) return rc;
    const int n = n_img * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
        using Ty = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((beit_pool_fwd_kernel<Ty>), dim3((n + 255) / 256), dim3(256), 0, s, (const Ty*)x, (Ty*)out, n_img, T, C);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_beit_pool_bwd(const void* dpool, void* dx, int n_img, int T, int C, int dtype, void* stream) {
    if (!dpool || !dx || n_img <= 0 || T < 2) return MOREC_E_ARG;
    const int rc = check_rows((size_t)n_img, C, dtype);
    if (rc) return rc;
    const size_t total = (size_t)n_img * T * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
        using Ty = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((beit_pool_bwd_kernel<Ty>), dim3(grid_for(total)), dim3(256), 0, s, (const Ty*)dpool, (Ty*)dx, n_img, T, C);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_beit_assemble_fwd(const void* e, const float* cls_token, void* x, int n_img, int N, int C, int dtype, void* stream) {
    if (!e || !cls_token || !x || n_img <= 0 || N <= 0) return MOREC_E_ARG;
    const int rc = check_rows((size_t)n_img, C, dtype);
    if (rc) return rc;
    if (!aligned16(e) || !aligned16(cls_token) || !aligned16(x)) return MOREC_E_ALIGN;
    const size_t total = (size_t)n_img * (N + 1) * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
        using Ty = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((beit_assemble_fwd_kernel<Ty>), dim3(grid_for(total)), dim3(256), 0, s, (const Ty*)e, cls_token, (Ty*)x, n_img, N, C);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
