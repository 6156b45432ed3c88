// attention_valu.hpp -- the fp32 register-block helpers of the VALU attention kernels: staging of [rows x d-chunk] tiles into LDS as fp32,
// the 4 x 4 (8 x 8) blocks each lane of a wavefront owns of a 32 x 32 (64 x 64) score tile, and the 32-row tile helpers of the kernels that
// walk longer sequences tile by tile.  Shared by attention.hip (tile and row-strip kernels) and attention_stream.hip (streamgen).
#pragma once
#include "common.hpp"

namespace {
// Tile edge TP = 8 TB: the 8 x 8 lanes of the wavefront own TB x TB blocks of the TP x TP score tile.  TB = 4 (T <= 32: titles of 30 tokens,
// histories of 20 / 10) is the shape everything on the benchmarked path has; TB = 8 (T <= 64) serves the reference's longer inputs --
// abstracts / bodies of 50 tokens (T/parameters.py:43-44), longer behaviour sequences -- on the same code.
template <int TB>
struct Tile {
    static constexpr int TP = 8 * TB;      // padded tile edge
    static constexpr int PP = TP + 4;      // pitch (floats) of the TP x TP probability tiles
};

struct AttnArgs {
    const void* qkv;
    const float* key_keep;
    void* ctx;         // fwd: output; bwd: dctx input
    void* dqkv;        // bwd only
    int n_seq, T, n_heads, dh;
    int causal;
    float scale, mask_value;
    DropRng drop;      // attention-probability dropout (modules.py:30; HF attention_probs_dropout_prob)
    const int32_t* cu; // packed-row offsets (unpadded layout) or nullptr
    int total_rows;    // rows of the packed buffers (>= cu[n_seq]); the spare ones are zero-filled by the blocks behind the grid
};

// stage a [T x DC] chunk (columns col0 + d0 .. of the packed row) into LDS as fp32, zero-padded to TP rows
template <typename T, int DC, int TB>
__device__ __forceinline__ void stage_chunk(const T* __restrict__ src, size_t row0, int pitch, int col0, int d0, int dh,
                                            int Tlen, float* __restrict__ dst) {
    constexpr int P = DC + 4;
    constexpr int VEC = Tile<TB>::TP * DC / 4;  // float4 slots
    const int lane = threadIdx.x;
#pragma unroll
    for (int i = 0; i < VEC / 64; ++i) {
        const int v = lane + i * 64;
        const int r = v / (DC / 4), c = (v % (DC / 4)) * 4;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < Tlen && d0 + c < dh) io<T>::load4(src + (row0 + r) * (size_t)pitch + col0 + d0 + c, o);
        *reinterpret_cast<float4*>(dst + r * P + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// s[r][c] += sum_d X[i0 + r][d] * Y[j0 + c][d] over one staged chunk
template <int DC, int TB>
__device__ __forceinline__ void block_dot(const float* __restrict__ X, const float* __restrict__ Y, int i0, int j0,
                                          float (&s)[TB][TB]) {
    constexpr int P = DC + 4;
#pragma unroll 4
    for (int d = 0; d < DC; d += 4) {
        float4 x[TB], y[TB];
#pragma unroll
        for (int r = 0; r < TB; ++r) x[r] = *reinterpret_cast<const float4*>(X + (i0 + r) * P + d);
#pragma unroll
        for (int c = 0; c < TB; ++c) y[c] = *reinterpret_cast<const float4*>(Y + (j0 + c) * P + d);
#pragma unroll
        for (int r = 0; r < TB; ++r)
#pragma unroll
            for (int c = 0; c < TB; ++c)
                s[r][c] += x[r].x * y[c].x + x[r].y * y[c].y + x[r].z * y[c].z + x[r].w * y[c].w;
    }
}

// masked, scaled softmax of the lane's TB x TB block; rows are shared by the 8 lanes with equal (lane >> 3)
template <int TB>
__device__ __forceinline__ void block_softmax(float (&s)[TB][TB], int i0, int j0, int Tlen, int causal, float scale,
                                              float mask_value, const float* __restrict__ keep_row) {
    float keep[TB];
#pragma unroll
    for (int c = 0; c < TB; ++c) keep[c] = (j0 + c < Tlen) ? keep_row[j0 + c] : 0.f;
#pragma unroll
    for (int r = 0; r < TB; ++r) {
        const int i = i0 + r;
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < TB; ++c) {
            const int j = j0 + c;
            const bool kept = (keep[c] != 0.f) && (!causal || j <= i);
            // reference arithmetic: score * scale + additive mask (the large-magnitude mask absorbs the score)
            const float v = s[r][c] * scale + (kept ? 0.f : mask_value);
            s[r][c] = (j < Tlen) ? v : -INFINITY;
            m = fmaxf(m, s[r][c]);
        }
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        m = fmaxf(m, __shfl_xor(m, 2, 64));
        m = fmaxf(m, __shfl_xor(m, 4, 64));
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < TB; ++c) {
            const float e = (j0 + c < Tlen) ? expf(s[r][c] - m) : 0.f;
            s[r][c] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        sum += __shfl_xor(sum, 4, 64);
        const float inv = (i < Tlen) ? 1.0f / sum : 0.f;   // padded query rows contribute nothing downstream
#pragma unroll
        for (int c = 0; c < TB; ++c) s[r][c] *= inv;
    }
}

// dropout keep-mask of the lane's TB x TB block: element index ((tile * TP + i) * TP + j)  (TP = 32 for T <= 32: the same stream as
// the MFMA kernels of attention_mfma.hip draw)
template <int TB>
__device__ __forceinline__ void block_drop_mask(const DropRng& d, uint64_t tile, int i0, int j0, float (&m)[TB][TB]) {
    constexpr uint64_t TP = Tile<TB>::TP;
#pragma unroll
    for (int r = 0; r < TB; ++r)
#pragma unroll
        for (int c4 = 0; c4 < TB; c4 += 4) {
            bool kp[4];
            drop_keep_vec<4>(d, (tile * TP + (uint64_t)(i0 + r)) * TP + (uint64_t)(j0 + c4), kp);   // j0 + c4 is a multiple of 4: even start
#pragma unroll
            for (int c = 0; c < 4; ++c) m[r][c4 + c] = kp[c] ? d.inv_keep : 0.f;
        }
}

// o[r][0..CW-1] = sum_k W[k][w0 + r] * V[k][c0 .. c0+CW-1]   (W stored [k][TP + pad]: "weights by row k");
// CW = DC / 8 columns per lane so that the 8 x 8 lane grid covers a [TP x DC] output chunk exactly.
template <int DC, int TB>
__device__ __forceinline__ void block_pv(const float* __restrict__ W, const float* __restrict__ V, int w0, int c0,
                                         int klen, float (&o)[TB][DC / 8]) {
    constexpr int P = DC + 4, CW = DC / 8, PP = Tile<TB>::PP;
#pragma unroll
    for (int r = 0; r < TB; ++r)
#pragma unroll
        for (int c = 0; c < CW; ++c) o[r][c] = 0.f;
    for (int k = 0; k < klen; ++k) {
        float wr[TB];
#pragma unroll
        for (int r4 = 0; r4 < TB; r4 += 4) {
            const float4 w = *reinterpret_cast<const float4*>(W + k * PP + w0 + r4);
            wr[r4] = w.x; wr[r4 + 1] = w.y; wr[r4 + 2] = w.z; wr[r4 + 3] = w.w;
        }
#pragma unroll
        for (int q = 0; q < CW / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(V + k * P + c0 + 4 * q);
#pragma unroll
            for (int r = 0; r < TB; ++r) {
                o[r][4 * q + 0] += wr[r] * v.x; o[r][4 * q + 1] += wr[r] * v.y;
                o[r][4 * q + 2] += wr[r] * v.z; o[r][4 * q + 3] += wr[r] * v.w;
            }
        }
    }
}

template <typename T, int CW, int TB>
__device__ __forceinline__ void store_rows(T* __restrict__ dst, size_t row0, int pitch, int col, int r0, int Tlen,
                                           int dcol, int dh, const float (&o)[TB][CW]) {
#pragma unroll
    for (int r = 0; r < TB; ++r) {
        if (r0 + r < Tlen) {
            T* p = dst + (row0 + r0 + r) * (size_t)pitch + col;
#pragma unroll
            for (int q = 0; q < CW / 4; ++q) {
                const float v[4] = {o[r][4 * q], o[r][4 * q + 1], o[r][4 * q + 2], o[r][4 * q + 3]};
                if (dcol + 4 * q < dh) io<T>::store4(p + 4 * q, v);
            }
        }
    }
}

// row r of a TB-wide register block -> TB consecutive floats of an LDS row
template <int TB>
__device__ __forceinline__ void put_row(float* __restrict__ dst, const float (&v)[TB]) {
#pragma unroll
    for (int c = 0; c < TB; c += 4) *reinterpret_cast<float4*>(dst + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
}

constexpr int LDC = 64;                                   // head-width chunk of the long kernels
constexpr int LP = LDC + 4, LPP = Tile<4>::PP, LCW = LDC / 8;

// s[r][c] = sum_d X[qt*32 + i0 + r][d] * Y[kt*32 + j0 + c][d] over the whole head width (chunks restaged per call)
template <typename T>
__device__ __forceinline__ void long_dot(const T* __restrict__ xsrc, int xpitch, int xcol, const T* __restrict__ ysrc, int ypitch, int ycol,
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
        block_dot<LDC, 4>(sX, sY, i0, j0, s);
        __syncthreads();
    }
}

// reference arithmetic of one score: scaled + additive mask; keys >= T never enter (-inf)
__device__ __forceinline__ float long_masked(float s, int i, int j, int Tlen, int causal, float scale, float mask_value, const float* __restrict__ keep_row) {
    if (j >= Tlen) return -INFINITY;
    const bool kept = (keep_row[j] != 0.f) && (!causal || j <= i);
    return s * scale + (kept ? 0.f : mask_value);
}

// o[r][c] += sum_{k < klen} W[k][w0 + r] * V[k][c0 + c]
__device__ __forceinline__ void long_pv_acc(const float* __restrict__ W, const float* __restrict__ V, int w0, int c0, int klen, float (&o)[4][LCW]) {
    for (int k = 0; k < klen; ++k) {
        const float4 w = *reinterpret_cast<const float4*>(W + k * LPP + w0);
        const float wr[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < LCW / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(V + k * LP + c0 + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r][4 * q + 0] += wr[r] * v.x; o[r][4 * q + 1] += wr[r] * v.y;
                o[r][4 * q + 2] += wr[r] * v.z; o[r][4 * q + 3] += wr[r] * v.w;
            }
        }
    }
}
}  // namespace
