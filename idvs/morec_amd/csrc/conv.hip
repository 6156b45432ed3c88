// conv.hip -- 2-D convolution over NHWC activations viewed as [N H W, C] rows (the ResNet item tower, resnet_engine.py): an implicit GEMM
//   out[m, d] = sum_{kh, kw, c} src[pixel(m, kh, kw), c] . w[d, kh, kw, c]
// in two forms of ONE kernel.  Forward (GATHER = false): m = (n, ho, wo) and the pixel is (n, ho s - p + kh, wo s - p + kw), zero outside
// the image.  Data gradient (GATHER = true): m = (n, h, w) of dx, src = dy, the pixel is (n, (h + p - kh) / s, (w + p - kw) / s) for the taps
// whose quotients are exact and in range, and w is handed in as [Cin, KH, KW, Cout]: every dx element is gathered by its one owner, nothing
// is scattered.  Every output is written once, no atomics: the same bits on every call.
//
// 16-bit storage with a K channel count Ck % 32 == 0 (every ResNet layer but the stem) runs on v_mfma_f32_16x16x32_{bf16,f16} with the tile,
// fragment and MMA helpers of featproj_core.hpp: a 32-element k-step lies inside one tap, so a lane's 8 k-elements are one 16-byte load of
// one pixel row (or a zero vector) -- featproj's main loop with the looked-up row changing per tap.  Like featproj it stages nothing through
// LDS: operand rows are re-read through L2 by the waves that share them.  fp32 storage and every other Ck (the stem, Cin = 3) run the generic
// kernel below: fp32 FMAs in (kh, kw, c) order, one thread per output row and four output channels.
//
// morec_im2col_nhwc writes the operand rows of an output-row range as a matrix [rows, ld] (k = (kh, kw, c), zero fill outside the image
// and in the pad columns K .. ld): the weight gradient is that matrix under the library's weight-gradient GEMM, chunked by the caller.
#include <algorithm>
#include "featproj_core.hpp"

namespace {
struct ConvGeom {
    int N, Hs, Ws, Ck;      // source grid and its channels (the reduction channel)
    int Hd, Wd, D;          // destination grid and its channels
    int KH, KW, stride, pad;
};
struct ConvPix {
    int n, a, b;            // image, row and column on the destination grid
};

__device__ __forceinline__ ConvPix conv_pix(int r, const ConvGeom& g) {
    ConvPix p;
    const int hw = g.Hd * g.Wd;
    p.n = r / hw;
    const int rem = r - p.n * hw;
    p.a = rem / g.Wd;
    p.b = rem - p.a * g.Wd;
    return p;
}
// the source pixel of tap (kh, kw) for destination pixel p; false = the tap contributes zero
template <bool GATHER>
__device__ __forceinline__ bool conv_src(const ConvPix& p, int kh, int kw, const ConvGeom& g, int& hs, int& ws) {
    if (!GATHER) {
        hs = p.a * g.stride - g.pad + kh;
        ws = p.b * g.stride - g.pad + kw;
        return hs >= 0 && hs < g.Hs && ws >= 0 && ws < g.Ws;
    }
    const int th = p.a + g.pad - kh, tw = p.b + g.pad - kw;      // stride is 1 or 2
    const int m = g.stride - 1, sh = g.stride >> 1;
    hs = th >> sh;
    ws = tw >> sh;
    return th >= 0 && tw >= 0 && !(th & m) && !(tw & m) && hs < g.Hs && ws < g.Ws;
}

// ---- MFMA form ------------------------------------------------------------------------------------------------------------------------
struct ConvTap {      // the 32-element k-step the next load fetches: tap (kh, kw), channels c .. c + 31
    int kh, kw, c;
};
// one K step (two 32-element k-steps) into f, advancing the tap iterator.  Every address is a valid one: a tap outside the image (or
// a k-step past the last tap) loads the start of the source / of the weight row and is replaced by zeros AFTER the load.
template <bool GATHER>
__device__ __forceinline__ void conv_load(FpFrags& f, ConvTap& it, const bf16* const (&wrow)[2], const bf16* __restrict__ src,
                                          const ConvPix (&px)[2], const ConvGeom& g, int q) {
    const bf16x8_t zero = {};
#pragma unroll
    for (int u = 0; u < FP_KU; ++u) {
        const bool live = it.kh < g.KH;
        const int c = (live ? it.c : 0) + 8 * q;
        const int koff = live ? (it.kh * g.KW + it.kw) * g.Ck + c : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int hs, ws;
            const bool ok = conv_src<GATHER>(px[i], it.kh, it.kw, g, hs, ws) && live;
            const size_t off = ok ? ((size_t)(px[i].n * g.Hs + hs) * g.Ws + ws) * g.Ck + c : 0;
            const bf16x8_t wv = *reinterpret_cast<const bf16x8_t*>(wrow[i] + koff);
            const bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(src + off);
            f.w[i][u] = live ? wv : zero;
            f.x[i][u] = ok ? xv : zero;
        }
        it.c += 32;
        if (it.c == g.Ck) {
            it.c = 0;
            if (++it.kw == g.KW) {
                it.kw = 0;
                ++it.kh;
            }
        }
    }
}

template <typename T16, bool GATHER>
__global__ __launch_bounds__(256) void conv_mfma_kernel(const T16* __restrict__ src, const T16* __restrict__ W, T16* __restrict__ out,
                                                        ConvGeom g, int R) {
    const FpTile t = fp_tile(g.D);
    const int Kw = g.KH * g.KW * g.Ck;
    const bf16* wrow[2];
    ConvPix px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int d = min(t.d0 + 16 * i + t.c16, g.D - 1);
        const int r = min(t.r0 + 16 * i + t.c16, R - 1);
        wrow[i] = reinterpret_cast<const bf16*>(W) + (size_t)d * Kw;
        px[i] = conv_pix(r, g);
    }
    f32x4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const bf16* s16 = reinterpret_cast<const bf16*>(src);
    const int KS = (Kw / 32 + FP_KU - 1) / FP_KU;
    ConvTap it = {0, 0, 0};
    FpFrags fa, fb;
    conv_load<GATHER>(fa, it, wrow, s16, px, g, t.q);
    int s = 0;
    for (; s + 2 <= KS; s += 2) {      // as fp_accumulate: the loads of the next step are in flight under the MFMAs of this one
        conv_load<GATHER>(fb, it, wrow, s16, px, g, t.q);
        fp_mma<T16>(acc, fa);
        conv_load<GATHER>(fa, it, wrow, s16, px, g, t.q);      // past the last tap: zeros from a valid address, never used
        fp_mma<T16>(acc, fb);
    }
    if (s < KS) fp_mma<T16>(acc, fa);

    // accumulator (i, j), register e: output row r0 + 16 i + c16, channel d0 + 16 j + 4 q + e (D % 8 == 0: the four are in or out together)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int d = t.d0 + 16 * j + 4 * t.q;
        if (d >= g.D) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = t.r0 + 16 * i + t.c16;
            if (r >= R) continue;
            const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            io<T16>::store4(out + (size_t)r * g.D + d, v);
        }
    }
}

// ---- generic form: fp32 arithmetic for every storage type and channel count ---------------------------------------------------------------
template <typename T, bool GATHER>
__global__ __launch_bounds__(256) void conv_generic_kernel(const T* __restrict__ src, const T* __restrict__ W, T* __restrict__ out,
                                                           ConvGeom g, int R) {
    const int dv = g.D / 4;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)R * dv) return;
    const int r = (int)(e / dv), d = (int)(e - (size_t)r * dv) * 4;
    const ConvPix p = conv_pix(r, g);
    const size_t Kw = (size_t)g.KH * g.KW * g.Ck;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int kh = 0; kh < g.KH; ++kh)
        for (int kw = 0; kw < g.KW; ++kw) {
            int hs, ws;
            if (!conv_src<GATHER>(p, kh, kw, g, hs, ws)) continue;
            const T* xp = src + ((size_t)(p.n * g.Hs + hs) * g.Ws + ws) * g.Ck;
            const T* wp = W + (size_t)d * Kw + (size_t)(kh * g.KW + kw) * g.Ck;
            for (int c = 0; c < g.Ck; ++c) {
                const float xv = io<T>::load1(xp + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fmaf(xv, io<T>::load1(wp + k * Kw + c), acc[k]);
            }
        }
    io<T>::store4(out + (size_t)r * g.D + d, acc);
}

// ---- im2col -----------------------------------------------------------------------------------------------------------------------------
// VEC: Cin is a multiple of the 16-byte vector (and so are K and ld): whole-vector copies.  Otherwise (the stem) element by element.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void im2col_kernel(const T* __restrict__ x, T* __restrict__ col, ConvGeom g, int row0, int nrows, int ld) {
    constexpr int EV = VEC ? vio<T>::EV : 1;
    const int K = g.KH * g.KW * g.Ck;
    const int vpr = ld / EV;
    const size_t total = (size_t)nrows * vpr;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int rr = (int)(e / vpr);
        const int k = (int)(e - (size_t)rr * vpr) * EV;
        bool ok = k < K;
        size_t off = 0;
        if (ok) {
            const int tap = k / g.Ck, c = k - tap * g.Ck;
            const int kh = tap / g.KW, kw = tap - kh * g.KW;
            const ConvPix p = conv_pix(row0 + rr, g);
            int hs, ws;
            ok = conv_src<false>(p, kh, kw, g, hs, ws);
            off = ok ? ((size_t)(p.n * g.Hs + hs) * g.Ws + ws) * g.Ck + c : 0;
        }
        T* dst = col + (size_t)rr * ld + k;
        if (VEC) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + off);
            *reinterpret_cast<uint4*>(dst) = ok ? v : make_uint4(0, 0, 0, 0);
        } else {
            const T v = x[off];
            const T z{};
            *dst = ok ? v : z;
        }
    }
}

int conv_out(int H, int K, int stride, int pad) { return (H + 2 * pad - K) / stride + 1; }

int conv_check(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return MOREC_E_ARG;
    if (!(KH == KW && (KH == 1 || KH == 3 || KH == 7)) || !(stride == 1 || stride == 2) || pad < 0 || pad >= KH) return MOREC_E_UNSUPPORTED;
    if (H + 2 * pad < KH || W + 2 * pad < KW) return MOREC_E_UNSUPPORTED;
    const long long rin = (long long)N * H * W, rout = (long long)N * conv_out(H, KH, stride, pad) * conv_out(W, KW, stride, pad);
    if (rin > 0x7fffffffLL || rout > 0x7fffffffLL || (long long)KH * KW * std::max(Cin, Cout) > 0x7fffffffLL) return MOREC_E_UNSUPPORTED;
    return MOREC_OK;
}

// src [N, Hs, Ws, Ck] and w [D, KH, KW, Ck] -> out [N Hd Wd, D]
template <bool GATHER>
int conv_launch(const void* src, const void* w, void* out, const ConvGeom& g, int dtype, hipStream_t s) {
    if (g.D % 8) return MOREC_E_ALIGN;
    if (!aligned16(src) || !aligned16(w) || !aligned16(out)) return MOREC_E_ALIGN;
    const long long R = (long long)g.N * g.Hd * g.Wd;
    if (is_h16(dtype) && g.Ck % 32 == 0) {
        const long long tiles = ((R + FP_TR - 1) / FP_TR) * ((g.D + FP_TC - 1) / FP_TC);
        if (tiles > 0x7fffffffLL) return MOREC_E_UNSUPPORTED;
        by_h16(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            hipLaunchKernelGGL((conv_mfma_kernel<T, GATHER>), dim3((unsigned)tiles), dim3(256), 0, s, (const T*)src, (const T*)w, (T*)out, g, (int)R);
        });
    } else {
        const long long blocks = (R * (g.D / 4) + 255) / 256;
        if (blocks > 0x7fffffffLL) return MOREC_E_UNSUPPORTED;
        if (!by_dtype(dtype, [&](auto* t) {
                using T = MOREC_TAG_T(t);
                hipLaunchKernelGGL((conv_generic_kernel<T, GATHER>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)src, (const T*)w, (T*)out, g, (int)R);
            }))
            return MOREC_E_DTYPE;
    }
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
}  // namespace

extern "C" int morec_conv2d_uses_mfma(int Ck, int dtype) { return is_h16(dtype) && Ck > 0 && Ck % 32 == 0; }

extern "C" int morec_conv2d_fwd(const void* x, const void* w, void* out, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                                int pad, int dtype, void* stream) {
    const int rc = conv_check(N, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    if (!x || !w || !out) return MOREC_E_ARG;
    const ConvGeom g = {N, H, W, Cin, conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad), Cout, KH, KW, stride, pad};
    return conv_launch<false>(x, w, out, g, dtype, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int morec_conv2d_bwd_data(const void* dy, const void* wt, void* dx, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                     int stride, int pad, int dtype, void* stream) {
    const int rc = conv_check(N, H, W, Cin, Cout, KH, KW, stride, pad);
    if (rc) return rc;
    if (!dy || !wt || !dx) return MOREC_E_ARG;
    const ConvGeom g = {N, conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad), Cout, H, W, Cin, KH, KW, stride, pad};
    return conv_launch<true>(dy, wt, dx, g, dtype, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int morec_im2col_nhwc(const void* x, void* col, int N, int H, int W, int Cin, int KH, int KW, int stride, int pad, int row0,
                                 int row1, int ld, int dtype, void* stream) {
    const int rc = conv_check(N, H, W, Cin, 1, KH, KW, stride, pad);
    if (rc) return rc;
    if (!x || !col) return MOREC_E_ARG;
    const ConvGeom g = {N, H, W, Cin, conv_out(H, KH, stride, pad), conv_out(W, KW, stride, pad), 0, KH, KW, stride, pad};
    const long long R = (long long)N * g.Hd * g.Wd, K = (long long)KH * KW * Cin;
    if (row0 < 0 || row1 <= row0 || row1 > R || ld < K) return MOREC_E_ARG;
    const int ev = 16 / elt_size(dtype);
    if (!aligned16(x) || !aligned16(col) || ld % ev) return MOREC_E_ALIGN;
    const bool vec = Cin % ev == 0;
    const size_t total = (size_t)(row1 - row0) * (vec ? ld / ev : ld);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 256 * 64);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto* t) {
            using T = MOREC_TAG_T(t);
            if (vec)
                hipLaunchKernelGGL((im2col_kernel<T, true>), dim3(blocks), dim3(256), 0, s, (const T*)x, (T*)col, g, row0, row1 - row0, ld);
            else
                hipLaunchKernelGGL((im2col_kernel<T, false>), dim3(blocks), dim3(256), 0, s, (const T*)x, (T*)col, g, row0, row1 - row0, ld);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
