// attention_frag.hpp -- MFMA operand fragments of the 16-bit attention kernels (attention_mfma.hip: one score tile per sequence;
// attention_stream.hip: key tiles walked with a running softmax): NT fragments from LDS tiles or straight from global memory, transposed
// fragments by ds_read_b64_tr_b16, register fragments of P / dS, and the d-contiguous row store.
#pragma once
#include "common.hpp"

namespace {
constexpr int DCH = 64;                       // head-width chunk staged per pass (elements)
constexpr int PITCH = DCH * 2 + 32;           // bytes per LDS tile row
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;

// No guarded loads in these kernels.  `if (row < T) v = *p;` -- and equally `ok ? *p : 0`, which the compiler turns back into a
// branch -- makes every load its own basic block that ends in s_waitcnt vmcnt(0): the 12 tile loads, 4 fragment loads and 8
// padding-flag loads of a wavefront then run as two dozen SERIAL memory round trips.  Instead every address is clamped to
// the last valid row of the sequence (T >= 1 is checked at kernel entry) and the duplicate rows are left in place: a row
// >= T is only ever multiplied by a probability / dS entry that is exactly 0 (masked key, or query row with inv = 0), and
// rows >= T of the outputs are never stored.  Columns past the head width (dh = 32 in a 64-wide tile) are never read.
__device__ __forceinline__ uint4 load16(const bf16* p) { return *reinterpret_cast<const uint4*>(p); }

// NT fragment: 8 consecutive d of row (blk*16 + lane&15), d offset ks*32 + (lane>>4)*8
// (lane = lane of the wavefront; pitch_bytes = bytes per tile row: PITCH for the 64-column tiles, the padded head width for whole-row tiles)
__device__ __forceinline__ bf16x8_t frag_nt_pitch(const char* tile, int pitch_bytes, int blk, int ks, int lane) {
    const uint4 v = *reinterpret_cast<const uint4*>(tile + (blk * 16 + (lane & 15)) * pitch_bytes + (ks * 32 + (lane >> 4) * 8) * 2);
    return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t frag_nt(const char* tile, int blk, int ks) { return frag_nt_pitch(tile, PITCH, blk, ks, threadIdx.x); }

// NT fragment straight from global memory (no LDS tile): 8 consecutive d of row (blk*16 + lane&15), rows >= Tlen repeat row Tlen - 1.
// Used for the operands that are only ever consumed d-contiguous (Q / K in the forward scores, V in the backward dP):
// every LDS tile dropped raises the number of resident wavefronts of this latency-bound kernel.
__device__ __forceinline__ bf16x8_t frag_nt_global(const bf16* __restrict__ src, size_t row0, int pitch, int col, int blk, int Tlen) {
    const int lane = threadIdx.x;
    const int r = blk * 16 + (lane & 15);
    const uint4 v = load16(src + (row0 + min(r, Tlen - 1)) * (size_t)pitch + col + (lane >> 4) * 8);
    return __builtin_bit_cast(bf16x8_t, v);
}

// Transposed fragment over the 32 rows of a row-major tile that start at `tile`: lane (c = lane&15, g = lane>>4) receives, for
// its column, the rows 4g .. 4g+3 (elements 0..3) and 16+4g .. 16+4g+3 (elements 4..7).  The 16 columns of the block are spread as
// 4 groups of 4: lane c receives column col0 + qstride * (c >> 2) + (c & 3).
// With col0 = 4 * db and qstride = 4 * ND the MFMA outputs of ND consecutive blocks land d-CONTIGUOUS in a lane
// (d = 4 ND g + 4 db + r): a row is then written as 4 lanes x 8 ND bytes (one full 128-byte line at ND = 4) instead of
// ND separate 32-byte pieces -- the partial-line stores were what bound these kernels (writes at ~1 TB/s).
__device__ __forceinline__ bf16x8_t frag_tr_spread_lane(const char* tile, int pitch_bytes, int col0, int qstride, int lane) {
    const int c = lane & 15, g = lane >> 4;
    const char* p0 = tile + (4 * g + (c >> 2)) * pitch_bytes + (col0 + qstride * (c & 3)) * 2;
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p0));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p0 + 16 * pitch_bytes));
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t frag_tr_spread(const char* tile, int pitch_bytes, int col0, int qstride) {
    return frag_tr_spread_lane(tile, pitch_bytes, col0, qstride, threadIdx.x);
}
// the plain transposed fragment (qstride 4): lane c receives column col0 + c
__device__ __forceinline__ bf16x8_t frag_tr(const char* tile, int pitch_bytes, int col0) { return frag_tr_spread(tile, pitch_bytes, col0, 4); }

// store the 4 * ND consecutive d values of one row held by the lane (ND accumulator blocks, 16-byte pieces)
template <typename T16, int ND>
__device__ __forceinline__ void store_row_d(bf16* dst, size_t row, int pitch, int col, const f32x4_t (&o)[ND]) {
    static_assert(ND % 2 == 0, "pairs of blocks");
    bf16* p = dst + row * (size_t)pitch + col;
#pragma unroll
    for (int h = 0; h < ND / 2; ++h) {
        uint4 v;
        v.x = h16<T16>::pack2(o[2 * h][0], o[2 * h][1]);
        v.y = h16<T16>::pack2(o[2 * h][2], o[2 * h][3]);
        v.z = h16<T16>::pack2(o[2 * h + 1][0], o[2 * h + 1][1]);
        v.w = h16<T16>::pack2(o[2 * h + 1][2], o[2 * h + 1][3]);
        *reinterpret_cast<uint4*>(p + 8 * h) = v;
        store_b128_guard();      // (MFMAs of the next block follow: see common.hpp)
    }
}

// register fragment of a [query][key] quantity over one 32-key k-step: blocks x0 (keys 0..15 of the step), x1 (16..31);
// k-slots (g, e) = keys 4g+e | 16+4g+(e-4)
template <typename T16>
__device__ __forceinline__ bf16x8_t frag_regs(const f32x4_t& x0, const f32x4_t& x1) {
    const uint4 v = make_uint4(h16<T16>::pack2(x0[0], x0[1]), h16<T16>::pack2(x0[2], x0[3]), h16<T16>::pack2(x1[0], x1[1]), h16<T16>::pack2(x1[2], x1[3]));
    return __builtin_bit_cast(bf16x8_t, v);
}
}  // namespace
