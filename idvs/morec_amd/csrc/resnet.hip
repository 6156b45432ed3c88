// resnet.hip -- the kernels of the ResNet item tower that are not convolutions (resnet_engine.py), over NHWC activations viewed as
// [rows, C] with rows = N H W: BatchNorm2d and the 3 x 3 stride-2 max pool (the pixel layout change in front of the stem: image_front.hip).
//
// BatchNorm statistics are (count, mean, M2) partials per slab of BN_SLAB rows and per channel: the slab mean first, then the squares of the
// deviations from THAT mean -- never E[x^2] - mean^2, which loses the digits of a post-ReLU activation (mean ~ std) in the fp32 parity
// mode.  The partials are merged in slab order with Chan's formula (morec_bn_merge: one thread per channel; resnet_engine.merge_bn_partials
// is the same arithmetic on the host, the form a later change merges across ranks).  The backward sums are per-slab partials folded in slab
// order too.  Nothing here uses atomics: every call repeats its bits.
//
// Synchronised BatchNorm (data-parallel ranks; resnet_engine._bn_fwd / _bn_bwd with a sync context) is the same kernels over one more level:
// a rank merges its slabs into one [3, C] partial, the ranks' partials are all-gathered rank-major and morec_bn_merge runs once more over
// those "W slabs" in rank order (that launch updates the running statistics with the global count); the backward sums [2, C] of the ranks
// are gathered and added in rank order by morec_bn_bwd_fold, and morec_bn_bwd_apply_n divides by the global row count it READS from the
// merged count row on the device -- the host never learns that count.  An all-gather and a fixed-order fold, never an all-reduce, whose
// order of summation belongs to the library: every rank computes the same bits.
#include <algorithm>
#include "common.hpp"

namespace {
constexpr int BN_SLAB = 1024;      // rows per statistics partial
constexpr int BN_RL = 16;          // row lanes of a block: thread = (row lane, channel vector)

// fixed-order sum over the BN_RL row lanes of a block: v[EV] of thread (ry, cx) -> the totals, in every thread of the column
template <int EV>
__device__ __forceinline__ void rl_sum(float (&v)[EV], float* sm, int ry, int cx) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EV; ++k) sm[(ry * 16 + cx) * EV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EV; ++k) {
        float s = 0.f;
        for (int y = 0; y < BN_RL; ++y) s += sm[(y * 16 + cx) * EV + k];
        v[k] = s;
    }
}

// part[slab][0 | 1 | 2][C] = count, mean, M2 of rows [slab BN_SLAB, ...) per channel.  grid (slabs, channel-vector groups of 16)
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, int rows, int C) {
    constexpr int EV = vio<T>::EV;
    __shared__ float sm[BN_RL * 16 * EV];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = (blockIdx.y * 16 + cx) * EV;
    const bool live = c < C;
    const int r0 = blockIdx.x * BN_SLAB, r1 = min(r0 + BN_SLAB, rows);
    const float cnt = (float)(r1 - r0);
    float s[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) s[k] = 0.f;
    if (live)
        for (int r = r0 + ry; r < r1; r += BN_RL) {
            float v[EV];
            vio<T>::load(x + (size_t)r * C + c, v);
#pragma unroll
            for (int k = 0; k < EV; ++k) s[k] += v[k];
        }
    rl_sum<EV>(s, sm, ry, cx);
    float mean[EV], m2[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) mean[k] = s[k] / cnt, m2[k] = 0.f;
    if (live)
        for (int r = r0 + ry; r < r1; r += BN_RL) {
            float v[EV];
            vio<T>::load(x + (size_t)r * C + c, v);
#pragma unroll
            for (int k = 0; k < EV; ++k) {
                const float d = v[k] - mean[k];
                m2[k] = fmaf(d, d, m2[k]);
            }
        }
    rl_sum<EV>(m2, sm, ry, cx);
    if (live && ry == 0) {
        float* p = part + (size_t)blockIdx.x * 3 * C + c;
#pragma unroll
        for (int k = 0; k < EV; ++k) p[k] = cnt, p[C + k] = mean[k], p[2 * C + k] = m2[k];
    }
}

// Chan's pairwise update, slab after slab: merged [3][C]; mean / rstd for the apply kernels; torch's running-statistics rule
// (running = (1 - momentum) running + momentum batch, the variance unbiased) when running_mean is given
__global__ void bn_merge_kernel(const float* __restrict__ part, int nslabs, int C, float eps, float momentum, float* __restrict__ merged,
                                float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ running_mean,
                                float* __restrict__ running_var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float n = part[c], mean = part[C + c], m2 = part[2 * C + c];
    for (int s = 1; s < nslabs; ++s) {
        const float* p = part + (size_t)s * 3 * C + c;
        const float nb = p[0], mb = p[C], m2b = p[2 * C];
        const float tot = n + nb, delta = mb - mean;
        mean = mean + delta * (nb / tot);
        m2 = m2 + m2b + delta * delta * (n * nb / tot);
        n = tot;
    }
    if (merged) merged[c] = n, merged[C + c] = mean, merged[2 * C + c] = m2;
    const float var = m2 / n;
    if (mean_out) mean_out[c] = mean;
    if (rstd_out) rstd_out[c] = 1.0f / sqrtf(var + eps);
    if (running_mean) {
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (m2 / fmaxf(n - 1.0f, 1.0f));
    }
}

// rstd of given (running) variances
__global__ void bn_rstd_kernel(const float* __restrict__ var, float* __restrict__ rstd, int C, float eps) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) rstd[c] = 1.0f / sqrtf(var[c] + eps);
}

// y = relu?(gamma xhat + beta (+ res)), xhat = (x - mean) rstd: fp32, one rounding
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const T* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const T* __restrict__ res, T* __restrict__ y, size_t rows, int C, int relu) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = rows * vpr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        float v[EV], m[EV], r[EV], g[EV], b[EV];
        vio<T>::load(x + row * C + c, v);
        load_f32v<EV>(mean + c, m);
        load_f32v<EV>(rstd + c, r);
        load_f32v<EV>(gamma + c, g);
        load_f32v<EV>(beta + c, b);
#pragma unroll
        for (int k = 0; k < EV; ++k) v[k] = fmaf(g[k], (v[k] - m[k]) * r[k], b[k]);
        if (res) {
            float a[EV];
            vio<T>::load(res + row * C + c, a);
#pragma unroll
            for (int k = 0; k < EV; ++k) v[k] += a[k];
        }
        if (relu) {
#pragma unroll
            for (int k = 0; k < EV; ++k) v[k] = fmaxf(v[k], 0.f);
        }
        vio<T>::store(y + row * C + c, v);
    }
}

// ws[slab][0 | 1][C] = sum dz, sum dz xhat over the slab's rows; dz = dy [y > 0] where a ReLU follows (y given)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ ws, int rows, int C) {
    constexpr int EV = vio<T>::EV;
    __shared__ float sm[BN_RL * 16 * EV];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int c = (blockIdx.y * 16 + cx) * EV;
    const bool live = c < C;
    const int r0 = blockIdx.x * BN_SLAB, r1 = min(r0 + BN_SLAB, rows);
    float s1[EV], s2[EV], m[EV], rs[EV];
#pragma unroll
    for (int k = 0; k < EV; ++k) s1[k] = 0.f, s2[k] = 0.f, m[k] = 0.f, rs[k] = 0.f;
    if (live) {
        load_f32v<EV>(mean + c, m);
        load_f32v<EV>(rstd + c, rs);
        for (int r = r0 + ry; r < r1; r += BN_RL) {
            float d[EV], v[EV];
            vio<T>::load(dy + (size_t)r * C + c, d);
            vio<T>::load(x + (size_t)r * C + c, v);
            if (y) {
                float o[EV];
                vio<T>::load(y + (size_t)r * C + c, o);
#pragma unroll
                for (int k = 0; k < EV; ++k) d[k] = o[k] > 0.f ? d[k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < EV; ++k) {
                s1[k] += d[k];
                s2[k] = fmaf(d[k], (v[k] - m[k]) * rs[k], s2[k]);
            }
        }
    }
    rl_sum<EV>(s1, sm, ry, cx);
    rl_sum<EV>(s2, sm, ry, cx);
    if (live && ry == 0) {
        float* p = ws + (size_t)blockIdx.x * 2 * C + c;
#pragma unroll
        for (int k = 0; k < EV; ++k) p[k] = s1[k], p[C + k] = s2[k];
    }
}
// sums[0 | 1][C] = the slab partials added in slab order
__global__ void bn_bwd_fold_kernel(const float* __restrict__ ws, int nslabs, int C, float* __restrict__ sums) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 2 * C) return;
    float s = 0.f;
    for (int i = 0; i < nslabs; ++i) s += ws[(size_t)i * 2 * C + j];
    sums[j] = s;
}

// dx = gamma rstd (dz - mean(dz) - xhat mean(dz xhat)); with sums == null (running statistics: constants) dx = gamma rstd dz.
// dz_out (optional): dz itself, the gradient of the residual branch.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ sums, float inv_rows,
                                                           T* __restrict__ dx, T* __restrict__ dz_out, size_t rows, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = rows * vpr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        float d[EV], v[EV], m[EV], rs[EV], g[EV], a[EV], b[EV];
        vio<T>::load(dy + row * C + c, d);
        vio<T>::load(x + row * C + c, v);
        load_f32v<EV>(mean + c, m);
        load_f32v<EV>(rstd + c, rs);
        load_f32v<EV>(gamma + c, g);
        if (y) {
            float o[EV];
            vio<T>::load(y + row * C + c, o);
#pragma unroll
            for (int k = 0; k < EV; ++k) d[k] = o[k] > 0.f ? d[k] : 0.f;
        }
        if (dz_out) vio<T>::store(dz_out + row * C + c, d);
        if (sums) {
            load_f32v<EV>(sums + c, a);
            load_f32v<EV>(sums + C + c, b);
#pragma unroll
            for (int k = 0; k < EV; ++k) {
                const float xh = (v[k] - m[k]) * rs[k];
                d[k] = g[k] * rs[k] * (d[k] - a[k] * inv_rows - xh * (b[k] * inv_rows));
            }
        } else {
#pragma unroll
            for (int k = 0; k < EV; ++k) d[k] = g[k] * rs[k] * d[k];
        }
        vio<T>::store(dx + row * C + c, d);
    }
}

// The same with the means divided by the row count of ALL ranks read from device memory: synchronised BatchNorm, whose sums are the
// ranks' folded sums (never null).  count: the merged count row (fp32 [C]); every channel counts the same rows, so count[0] is read, once,
// and 1 / count[0] takes the place of inv_rows -- the correctly rounded division the host does there, and the text after it is that kernel's,
// so that the compiler contracts and pairs the same operations: a count equal to rows gives the kernel above's bits.  A kernel of its own, so that the one above keeps its instruction stream.  An fp32
// count is exact below 2^24 rows and relatively 2^-24 off beyond (704 images x 112^2 x 8 ranks passes it): far inside every bound.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_n_kernel(const T* __restrict__ dy, const T* __restrict__ y, const T* __restrict__ x,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ sums,
                                                             const float* __restrict__ count, T* __restrict__ dx, T* __restrict__ dz_out,
                                                             size_t rows, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = rows * vpr;
    const float inv_rows = 1.0f / count[0];
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        float d[EV], v[EV], m[EV], rs[EV], g[EV], a[EV], b[EV];
        vio<T>::load(dy + row * C + c, d);
        vio<T>::load(x + row * C + c, v);
        load_f32v<EV>(mean + c, m);
        load_f32v<EV>(rstd + c, rs);
        load_f32v<EV>(gamma + c, g);
        if (y) {
            float o[EV];
            vio<T>::load(y + row * C + c, o);
#pragma unroll
            for (int k = 0; k < EV; ++k) d[k] = o[k] > 0.f ? d[k] : 0.f;
        }
        if (dz_out) vio<T>::store(dz_out + row * C + c, d);
        if (sums) {
            load_f32v<EV>(sums + c, a);
            load_f32v<EV>(sums + C + c, b);
#pragma unroll
            for (int k = 0; k < EV; ++k) {
                const float xh = (v[k] - m[k]) * rs[k];
                d[k] = g[k] * rs[k] * (d[k] - a[k] * inv_rows - xh * (b[k] * inv_rows));
            }
        } else {
#pragma unroll
            for (int k = 0; k < EV; ++k) d[k] = g[k] * rs[k] * d[k];
        }
        vio<T>::store(dx + row * C + c, d);
    }
}

// ---- MaxPool2d(3, stride 2, padding 1) over NHWC: among equal values the first tap in (kh, kw) scan order wins; its index is kept
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx, int N, int H,
                                                          int W, int Ho, int Wo, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = (size_t)N * Ho * Wo * vpr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        const int n = (int)(row / ((size_t)Ho * Wo)), rem = (int)(row - (size_t)n * Ho * Wo);
        const int ho = rem / Wo, wo = rem - ho * Wo;
        float best[EV];
        uint8_t tap[EV];
#pragma unroll
        for (int k = 0; k < EV; ++k) best[k] = -INFINITY, tap[k] = 0;
        for (int kh = 0; kh < 3; ++kh) {
            const int h = 2 * ho - 1 + kh;
            if (h < 0 || h >= H) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int w = 2 * wo - 1 + kw;
                if (w < 0 || w >= W) continue;
                float v[EV];
                vio<T>::load(x + ((size_t)(n * H + h) * W + w) * C + c, v);
#pragma unroll
                for (int k = 0; k < EV; ++k)
                    if (v[k] > best[k] || v[k] != v[k]) best[k] = v[k], tap[k] = (uint8_t)(kh * 3 + kw);      // a NaN is taken, as torch does
            }
        }
        vio<T>::store(y + row * C + c, best);
#pragma unroll
        for (int k = 0; k < EV; ++k) idx[row * C + c + k] = tap[k];
    }
}
// dx[n, h, w, c] = sum of dy over the (at most four) windows that contain the pixel and selected it: a gather
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ idx, T* __restrict__ dx, int N,
                                                          int H, int W, int Ho, int Wo, int C) {
    constexpr int EV = vio<T>::EV;
    const int vpr = C / EV;
    const size_t total = (size_t)N * H * W * vpr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / vpr;
        const int c = (int)(e - row * vpr) * EV;
        const int n = (int)(row / ((size_t)H * W)), rem = (int)(row - (size_t)n * H * W);
        const int h = rem / W, w = rem - h * W;
        float acc[EV];
#pragma unroll
        for (int k = 0; k < EV; ++k) acc[k] = 0.f;
        for (int kh = 0; kh < 3; ++kh) {
            const int th = h + 1 - kh;
            if (th < 0 || (th & 1) || (th >> 1) >= Ho) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int tw = w + 1 - kw;
                if (tw < 0 || (tw & 1) || (tw >> 1) >= Wo) continue;
                const size_t o = ((size_t)(n * Ho + (th >> 1)) * Wo + (tw >> 1)) * C + c;
                float d[EV];
                vio<T>::load(dy + o, d);
#pragma unroll
                for (int k = 0; k < EV; ++k)
                    if (idx[o + k] == kh * 3 + kw) acc[k] += d[k];
            }
        }
        vio<T>::store(dx + row * C + c, acc);
    }
}

int vec_check(const void* a, const void* b, long long rows, int C) {
    if (!a || !b || rows <= 0 || C <= 0) return MOREC_E_ARG;
    if (C % 8 || !aligned16(a) || !aligned16(b)) return MOREC_E_ALIGN;
    return MOREC_OK;
}
}  // namespace

extern "C" int morec_bn_slab_rows() { return BN_SLAB; }

extern "C" int morec_bn_stats(const void* x, float* part, int rows, int C, int dtype, void* stream) {
    const int rc = vec_check(x, part, rows, C);
    if (rc) return rc;
    const int ev = 16 / elt_size(dtype);
    const dim3 grid((rows + BN_SLAB - 1) / BN_SLAB, (C / ev + 15) / 16);
    if (grid.y > 65535u) return MOREC_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((bn_stats_kernel<T>), grid, dim3(256), 0, s, (const T*)x, part, rows, C);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_bn_merge(const float* part, int nslabs, int C, float eps, float momentum, float* merged, float* mean, float* rstd,
                              float* running_mean, float* running_var, void* stream) {
    if (!part || nslabs <= 0 || C <= 0 || (!running_mean != !running_var)) return MOREC_E_ARG;
    hipLaunchKernelGGL(bn_merge_kernel, dim3((C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), part, nslabs, C, eps,
                       momentum, merged, mean, rstd, running_mean, running_var);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_bn_rstd(const float* var, float* rstd, int C, float eps, void* stream) {
    if (!var || !rstd || C <= 0) return MOREC_E_ARG;
    hipLaunchKernelGGL(bn_rstd_kernel, dim3((C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), var, rstd, C, eps);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_bn_apply_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* res,
                                  void* y, int rows, int C, int relu, int dtype, void* stream) {
    const int rc = vec_check(x, y, rows, C);
    if (rc) return rc;
    if (!mean || !rstd || !gamma || !beta) return MOREC_E_ARG;
    if (!aligned16(mean) || !aligned16(rstd) || !aligned16(gamma) || !aligned16(beta) || (res && !aligned16(res))) return MOREC_E_ALIGN;
    const size_t total = (size_t)rows * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((bn_apply_fwd_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, mean, rstd, gamma, beta, (const T*)res,
                               (T*)y, (size_t)rows, C, relu);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" size_t morec_bn_bwd_workspace_bytes(int rows, int C) {
    return rows > 0 && C > 0 ? (size_t)((rows + BN_SLAB - 1) / BN_SLAB) * 2 * C * sizeof(float) : 0;
}

extern "C" int morec_bn_bwd_reduce(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, float* ws, float* sums,
                                   int rows, int C, int dtype, void* stream) {
    const int rc = vec_check(dy, x, rows, C);
    if (rc) return rc;
    if (!mean || !rstd || !ws || !sums) return MOREC_E_ARG;
    if (!aligned16(mean) || !aligned16(rstd) || (y && !aligned16(y))) return MOREC_E_ALIGN;
    const int ev = 16 / elt_size(dtype), nslabs = (rows + BN_SLAB - 1) / BN_SLAB;
    const dim3 grid(nslabs, (C / ev + 15) / 16);
    if (grid.y > 65535u) return MOREC_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((bn_bwd_reduce_kernel<T>), grid, dim3(256), 0, s, (const T*)dy, (const T*)y, (const T*)x, mean, rstd, ws, rows, C);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, s, ws, nslabs, C, sums);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_bn_bwd_fold(const float* parts, int n, int C, float* sums, void* stream) {
    if (!parts || !sums || n <= 0 || C <= 0) return MOREC_E_ARG;
    hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), parts, n, C, sums);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

namespace {
int bn_bwd_apply_check(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, const float* sums,
                       const void* dx, const void* dz, int rows, int C) {
    const int rc = vec_check(dy, x, rows, C);
    if (rc) return rc;
    if (!mean || !rstd || !gamma || !dx) return MOREC_E_ARG;
    if (!aligned16(mean) || !aligned16(rstd) || !aligned16(gamma) || !aligned16(dx) || (y && !aligned16(y)) || (dz && !aligned16(dz)) ||
        (sums && !aligned16(sums)))
        return MOREC_E_ALIGN;
    return MOREC_OK;
}
}  // namespace

extern "C" int morec_bn_bwd_apply(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma,
                                  const float* sums, void* dx, void* dz, int rows, int C, int dtype, void* stream) {
    const int rc = bn_bwd_apply_check(dy, y, x, mean, rstd, gamma, sums, dx, dz, rows, C);
    if (rc) return rc;
    const size_t total = (size_t)rows * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((bn_bwd_apply_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)dy, (const T*)y, (const T*)x, mean, rstd,
                               gamma, sums, 1.0f / (float)rows, (T*)dx, (T*)dz, (size_t)rows, C);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_bn_bwd_apply_n(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma,
                                    const float* sums, const float* count, void* dx, void* dz, int rows, int C, int dtype, void* stream) {
    const int rc = bn_bwd_apply_check(dy, y, x, mean, rstd, gamma, sums, dx, dz, rows, C);
    if (rc) return rc;
    if (!sums || !count) return MOREC_E_ARG;
    if (!aligned16(count)) return MOREC_E_ALIGN;
    const size_t total = (size_t)rows * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((bn_bwd_apply_n_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)dy, (const T*)y, (const T*)x, mean,
                               rstd, gamma, sums, count, (T*)dx, (T*)dz, (size_t)rows, C);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int dtype, void* stream) {
    if (N <= 0 || H <= 0 || W <= 0) return MOREC_E_ARG;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int rc = vec_check(x, y, (long long)N * Ho * Wo, C);
    if (rc) return rc;
    if (!idx) return MOREC_E_ARG;
    if ((long long)N * H * W > 0x7fffffffLL) return MOREC_E_UNSUPPORTED;
    const size_t total = (size_t)N * Ho * Wo * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((maxpool_fwd_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)x, (T*)y, idx, N, H, W, Ho, Wo, C);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C, int dtype, void* stream) {
    if (N <= 0 || H <= 0 || W <= 0) return MOREC_E_ARG;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int rc = vec_check(dy, dx, (long long)N * H * W, C);
    if (rc) return rc;
    if (!idx) return MOREC_E_ARG;
    if ((long long)N * H * W > 0x7fffffffLL) return MOREC_E_UNSUPPORTED;
    const size_t total = (size_t)N * H * W * (C / (16 / elt_size(dtype)));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((maxpool_bwd_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, (const T*)dy, idx, (T*)dx, N, H, W, Ho, Wo, C);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

