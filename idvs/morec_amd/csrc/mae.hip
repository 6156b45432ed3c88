// mae.hip -- the front of the MAE (ViT) item tower: HF ViTMAEEmbeddings (modeling_vit_mae.py:182-327) for the KEPT patches only.
//   * keep_ids        random_masking's argsort(noise)[:, :len_keep] (:297-327), one workgroup per image           (ranking in LDS)
//   * patchify_keep   the im2col of swin.hip's patchify, rows of the kept patches only (from uint8 images: image_front.hip)
//   * assemble        [CLS] + position row 0, kept patch embeddings + their position rows (:259-267); backward
// HF projects every patch and gathers len_keep of them afterwards; here only the kept patches get an im2col row and a row of the
// patch GEMM.  No atomics, every output element is written exactly once, the same bits on every run.
#include <algorithm>
#include "common.hpp"

namespace {

// ---- keep_ids ----------------------------------------------------------------------------------------------------------------
// Order-preserving map of an fp32 value to uint32 (-0 counts as +0, as in a float comparison).
__device__ __forceinline__ uint32_t noise_key(float v) {
    if (v == 0.f) v = 0.f;
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

constexpr int KEEP_NT = 256;
constexpr int KEEP_NMAX = 1024;

// keep[img, r] = the patch whose (key, index) pair is the r-th smallest of the image, r < len_keep.  The ranks of an image are a
// permutation of 0 .. N-1, so every keep slot has exactly one writer.  noise == nullptr: key = drop_hash(seed; img * N + patch),
// the counter-based generator of the dropout masks (32 uniform bits; equal draws fall back to the lower index like any tie).
__global__ __launch_bounds__(KEEP_NT) void mae_keep_ids_kernel(const float* __restrict__ noise, DropRng d, int32_t* __restrict__ keep,
                                                               int N, int len_keep) {
    __shared__ uint32_t key[KEEP_NMAX];
    const int img = blockIdx.x;
    for (int p = threadIdx.x; p < N; p += KEEP_NT)
        key[p] = noise ? noise_key(noise[(size_t)img * N + p]) : drop_hash(d, (uint64_t)img * (uint64_t)N + (uint64_t)p);
    __syncthreads();
    for (int p = threadIdx.x; p < N; p += KEEP_NT) {
        const uint32_t k = key[p];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const uint32_t kj = key[j];      // the same address in every lane: an LDS broadcast
            rank += (kj < k || (kj == k && j < p)) ? 1 : 0;
        }
        if (rank < len_keep) keep[(size_t)img * len_keep + rank] = p;
    }
}

// ---- patchify_keep -------------------------------------------------------------------------------------------------------------
// out[img * len_keep + j, (c, i, jj)] = pixels[img, c, py * ps + i, px * ps + jj] with (py, px) = patch keep[img, j]; thread = EV
// consecutive output elements (one 16-byte store), i.e. EV / 4 runs of 4 pixels (one 16-byte load each; ps % 4 == 0).  A keep entry
// outside [0, G * G) reads nothing and leaves a zero row.
template <typename T>
__global__ __launch_bounds__(256) void mae_patchify_keep_kernel(const float* __restrict__ px, const int32_t* __restrict__ keep,
                                                                T* __restrict__ out, int n_img, int Cin, int R, int ps, int len_keep,
                                                                int ld_out) {
    constexpr int EV = vio<T>::EV;
    const int G = R / ps;
    const int K = Cin * ps * ps;
    const int chunks = K / EV;
    const size_t total = (size_t)n_img * len_keep * chunks;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / chunks;
        const int k0 = (int)(e - row * chunks) * EV;
        const int n = (int)(row / len_keep);
        const int patch = keep[row];
        float v[EV];
        if ((unsigned)patch < (unsigned)(G * G)) {
            const int py = patch / G, pxx = patch - py * G;
#pragma unroll
            for (int q = 0; q < EV / 4; ++q) {
                const int k = k0 + 4 * q;
                const int ci = k / ps, jj = k - ci * ps;           // ci = c * ps + i
                const int c = ci / ps, i = ci - c * ps;
                float t[4];
                io<float>::load4(px + (((size_t)n * Cin + c) * R + (py * ps + i)) * R + pxx * ps + jj, t);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[4 * q + u] = t[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < EV; ++u) v[u] = 0.f;
        }
        vio<T>::store(out + row * ld_out + k0, v);
    }
}

// ---- assemble ------------------------------------------------------------------------------------------------------------------
// x[img, 0] = cls + pos[0]; x[img, 1 + j] = e[img * len_keep + j] + pos[1 + keep[img, j]]: one fp32 add, one rounding to T.
template <typename T>
__global__ __launch_bounds__(256) void mae_assemble_fwd_kernel(const T* __restrict__ e, const float* __restrict__ cls,
                                                               const float* __restrict__ pos, const int32_t* __restrict__ keep,
                                                               T* __restrict__ x, int n_img, int len_keep, int N, int C) {
    constexpr int EV = vio<T>::EV;
    const int chunks = C / EV;
    const int Tn = len_keep + 1;
    const size_t total = (size_t)n_img * Tn * chunks;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t row = idx / chunks;
        const int c0 = (int)(idx - row * chunks) * EV;
        const int img = (int)(row / Tn), t = (int)(row - (size_t)img * Tn);
        float a[EV], b[EV];
        if (t == 0) {
            load_f32v<EV>(cls + c0, a);
            load_f32v<EV>(pos + c0, b);
        } else {
            const size_t er = (size_t)img * len_keep + (t - 1);
            const int patch = keep[er];
            vio<T>::load(e + er * C + c0, a);
            if ((unsigned)patch < (unsigned)N) {
                load_f32v<EV>(pos + (size_t)(1 + patch) * C + c0, b);
            } else {
#pragma unroll
                for (int u = 0; u < EV; ++u) b[u] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < EV; ++u) a[u] += b[u];
        vio<T>::store(x + row * C + c0, a);
    }
}

constexpr int CLS_NT = 256;

// Blocks [0, copy_blocks): de[img * len_keep + j] = dx[img, 1 + j] (16-byte copies).  Blocks behind them, one per EV columns:
// d_cls[c] = sum over img of dx[img, 0, c] in fp32 -- thread t adds the images t, t + 256, ... in ascending order, then a fixed
// binary tree over the 256 partials: the same order, hence the same bits, on every run.
template <typename T>
__global__ __launch_bounds__(CLS_NT) void mae_assemble_bwd_kernel(const T* __restrict__ dx, T* __restrict__ de, float* __restrict__ d_cls,
                                                                  int n_img, int len_keep, int C, int copy_blocks) {
    constexpr int EV = vio<T>::EV;
    const int chunks = C / EV;
    const int Tn = len_keep + 1;
    if ((int)blockIdx.x < copy_blocks) {
        const size_t total = (size_t)n_img * len_keep * chunks;
        for (size_t idx = (size_t)blockIdx.x * CLS_NT + threadIdx.x; idx < total; idx += (size_t)copy_blocks * CLS_NT) {
            const size_t er = idx / chunks;
            const int c0 = (int)(idx - er * chunks) * EV;
            const size_t img = er / len_keep, j = er - img * len_keep;
            *reinterpret_cast<uint4*>(de + er * C + c0) = vio<T>::load_raw(dx + (img * Tn + 1 + j) * C + c0);
        }
        return;
    }
    __shared__ float part[CLS_NT][EV];
    const int c0 = ((int)blockIdx.x - copy_blocks) * EV;
    float acc[EV];
#pragma unroll
    for (int u = 0; u < EV; ++u) acc[u] = 0.f;
    for (int img = threadIdx.x; img < n_img; img += CLS_NT) {
        float v[EV];
        vio<T>::load(dx + (size_t)img * Tn * C + c0, v);
#pragma unroll
        for (int u = 0; u < EV; ++u) acc[u] += v[u];
    }
#pragma unroll
    for (int u = 0; u < EV; ++u) part[threadIdx.x][u] = acc[u];
    __syncthreads();
    for (int s = CLS_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int u = 0; u < EV; ++u) part[threadIdx.x][u] += part[threadIdx.x + s][u];
        }
        __syncthreads();
    }
    if (threadIdx.x < EV) d_cls[c0 + threadIdx.x] = part[0][threadIdx.x];
}

}  // namespace

extern "C" int morec_mae_keep_ids(const float* noise, uint64_t seed, int32_t* keep, int n_img, int N, int len_keep, void* stream) {
    if (!keep || n_img <= 0 || N <= 0 || len_keep <= 0 || len_keep > N) return MOREC_E_ARG;
    if (N > KEEP_NMAX) return MOREC_E_UNSUPPORTED;
    DropRng d{};
    d.s0 = (uint32_t)seed;
    d.s1 = (uint32_t)(seed >> 32);
    d.src = nullptr;
    hipLaunchKernelGGL(mae_keep_ids_kernel, dim3(n_img), dim3(KEEP_NT), 0, reinterpret_cast<hipStream_t>(stream), noise, d, keep, N, len_keep);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_mae_patchify_keep(const float* pixels, const int32_t* keep, void* out, int n_img, int channels, int R, int patch,
                                       int len_keep, int ld_out, int dtype, void* stream) {
    const int rc = check_patchify(pixels, keep, out, n_img, channels, R, patch, len_keep, ld_out, dtype);
    if (rc != MOREC_OK) return rc;
    if (!aligned16(pixels)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t total = (size_t)n_img * len_keep * (channels * patch * patch / (16 / elt_size(dtype)));
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((mae_patchify_keep_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, pixels, keep, (T*)out, n_img, channels, R,
                           patch, len_keep, ld_out);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_mae_assemble_fwd(const void* e, const float* cls_token, const float* pos, const int32_t* keep, void* x, int n_img,
                                      int len_keep, int N, int C, int dtype, void* stream) {
    if (!e || !cls_token || !pos || !keep || !x || n_img <= 0 || len_keep <= 0 || N <= 0 || C <= 0 || len_keep > N) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    // one width rule for the three storage types: whole 16-byte lanes of the 16-bit ones
    if (C % 8 || !aligned16(e) || !aligned16(cls_token) || !aligned16(pos) || !aligned16(x)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t total = (size_t)n_img * (len_keep + 1) * (C / (16 / elt_size(dtype)));
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((mae_assemble_fwd_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)e, cls_token, pos, keep, (T*)x,
                           n_img, len_keep, N, C);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_mae_assemble_bwd(const void* dx, void* de, float* d_cls, int n_img, int len_keep, int C, int dtype, void* stream) {
    if (!dx || !de || !d_cls || n_img <= 0 || len_keep <= 0 || C <= 0) return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (C % 8 || !aligned16(dx) || !aligned16(de)) return MOREC_E_ALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ev = 16 / elt_size(dtype);
    const int copy_blocks = grid_for((size_t)n_img * len_keep * (C / ev));
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        hipLaunchKernelGGL((mae_assemble_bwd_kernel<T>), dim3(copy_blocks + C / ev), dim3(CLS_NT), 0, s, (const T*)dx, (T*)de, d_cls, n_img,
                           len_keep, C, copy_blocks);
    });
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
