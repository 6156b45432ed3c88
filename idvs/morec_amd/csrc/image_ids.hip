// image_ids.hip -- the indexed forms of the three front kernels through which decoded uint8 images enter a vision tower.  The image
// catalogue [n_rows, R, R, 3] stays on the device; a batch is its int32 item ids, and image k of the output is computed from catalogue
// row ids[k] (clamped into [0, n_rows - 1]: a bad id never reads outside the catalogue).
//   * swin_patchify_u8_idx       swin.hip's swin_patchify_u8        (Swin, BEiT)
//   * mae_patchify_keep_u8_idx   mae.hip's mae_patchify_keep_u8     (MAE: patches from keep[k], pixels from row ids[k])
//   * pixels_to_nhwc_idx         resnet.hip's pixels_to_nhwc, uint8 (ResNet)
// The per-element arithmetic is the parents' -- ((float)u8 / 255 - mean) / std in fp32, one rounding to the storage type -- so the
// output is bit-equal to catalogue.index_select(0, ids) followed by the parent.  No atomics, every output element has one writer.
#include <algorithm>
#include "common.hpp"

namespace {

__device__ __forceinline__ int clamp_id(int id, int n_rows) { return min(max(id, 0), n_rows - 1); }

// out[row, (c, i, j)] = norm(cat[ids[n], py * ps + i, px * ps + j, c]); row = n * rows_per_img + r and (py, px) = patch r (KEEP: patch
// keep[row]; outside [0, G * G) leaves a zero row, as the parent).  thread = PW pixels of one (row, i) run: PW == 4 reads the 12 bytes
// of 4 RGB pixels as three dwords and writes one 4-element store per channel (Cin == 3, ps % 4 == 0); PW == 1 moves single elements.
template <typename T, int PW, bool KEEP>
__global__ __launch_bounds__(256) void patch_rows_idx_kernel(const uint8_t* __restrict__ cat, const int32_t* __restrict__ ids, int n_rows,
                                                             const int32_t* __restrict__ keep, T* __restrict__ out, int n_img, int Cin,
                                                             int R, int ps, int rows_per_img, int ld_out, float mean, float std) {
    const int G = R / ps;
    const int gpr = ps / PW;                         // thread groups per run of ps pixels
    const int per_row = ps * gpr;
    const size_t total = (size_t)n_img * rows_per_img * per_row;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / per_row;
        const int t = (int)(e - row * per_row);
        const int i = t / gpr, j0 = (t - i * gpr) * PW;
        const int n = (int)(row / rows_per_img);
        const int patch = KEEP ? keep[row] : (int)(row - (size_t)n * rows_per_img);
        T* dst = out + row * ld_out + i * ps + j0;
        if (KEEP && (unsigned)patch >= (unsigned)(G * G)) {
            if constexpr (PW == 4) {
                const float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 3; ++c) io<T>::store4(dst + c * ps * ps, z);
            } else {
                for (int c = 0; c < Cin; ++c) io<T>::store1(dst + c * ps * ps, 0.f);
            }
            continue;
        }
        const int id = clamp_id(ids[n], n_rows);
        const int py = patch / G, pxx = patch - py * G;
        const uint8_t* src = cat + (((size_t)id * R + (py * ps + i)) * R + pxx * ps + j0) * Cin;
        if constexpr (PW == 4) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);      // a multiple of 12 bytes into a 4-byte aligned catalogue
            const uint32_t w[3] = {s4[0], s4[1], s4[2]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int b = u * 3 + c;
                    v[u] = ((float)((w[b >> 2] >> (8 * (b & 3))) & 0xffu) / 255.0f - mean) / std;
                }
                io<T>::store4(dst + c * ps * ps, v);
            }
        } else {
            for (int c = 0; c < Cin; ++c) io<T>::store1(dst + c * ps * ps, ((float)src[c] / 255.0f - mean) / std);
        }
    }
}

// out[k * per + o] = norm(cat[ids[k] * per + o]), per = H W C bytes of one image; thread = PW consecutive bytes (PW == 4: one dword
// load, one 4-element store; per % 4 == 0).
template <typename T, int PW>
__global__ __launch_bounds__(256) void pixels_idx_kernel(const uint8_t* __restrict__ cat, const int32_t* __restrict__ ids, int n_rows,
                                                         T* __restrict__ out, int n_img, size_t per, float mean, float std) {
    const size_t gpi = per / PW;                     // thread groups per image
    const size_t total = (size_t)n_img * gpi;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t k = e / gpi;
        const size_t o = (e - k * gpi) * PW;
        const uint8_t* src = cat + (size_t)clamp_id(ids[k], n_rows) * per + o;
        T* dst = out + k * per + o;
        if constexpr (PW == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(src);
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ((float)((w >> (8 * u)) & 0xffu) / 255.0f - mean) / std;
            io<T>::store4(dst, v);
        } else {
            io<T>::store1(dst, ((float)src[0] / 255.0f - mean) / std);
        }
    }
}

int idx_grid(size_t total) { return (int)std::min<size_t>((total + 255) / 256, 256 * 32); }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the 4-pixel path: RGB, whole groups of 4 pixels, dword loads and 4-element stores on their natural alignment
bool wide_rows(const void* cat, const void* out, int channels, int patch, int ld_out) {
    return channels == 3 && patch % 4 == 0 && ld_out % 4 == 0 && aligned4(cat) && aligned16(out);
}

template <bool KEEP>
void launch_patch_rows(const uint8_t* cat, const int32_t* ids, int n_rows, const int32_t* keep, void* out, int n_img, int channels, int R,
                       int patch, int rows_per_img, int ld_out, float mean, float std, int dtype, hipStream_t s) {
    const bool wide = wide_rows(cat, out, channels, patch, ld_out);
    const size_t total = (size_t)n_img * rows_per_img * patch * (wide ? patch / 4 : patch);
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        if (wide)
            hipLaunchKernelGGL((patch_rows_idx_kernel<T, 4, KEEP>), dim3(idx_grid(total)), dim3(256), 0, s, cat, ids, n_rows, keep, (T*)out,
                               n_img, channels, R, patch, rows_per_img, ld_out, mean, std);
        else
            hipLaunchKernelGGL((patch_rows_idx_kernel<T, 1, KEEP>), dim3(idx_grid(total)), dim3(256), 0, s, cat, ids, n_rows, keep, (T*)out,
                               n_img, channels, R, patch, rows_per_img, ld_out, mean, std);
    });
}

}  // namespace

extern "C" int morec_swin_patchify_u8_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, void* out, int n_img, int channels,
                                          int R, int patch, int ld_out, float mean, float std, int dtype, void* stream) {
    if (!catalogue || !ids || !out || n_rows <= 0 || n_img <= 0 || channels <= 0 || R <= 0 || patch <= 0 || std == 0.f) return MOREC_E_ARG;
    if (R % patch) return MOREC_E_UNSUPPORTED;
    if (ld_out < channels * patch * patch) return MOREC_E_ALIGN;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    const int G = R / patch;
    launch_patch_rows<false>(catalogue, ids, n_rows, nullptr, out, n_img, channels, R, patch, G * G, ld_out, mean, std, dtype,
                             reinterpret_cast<hipStream_t>(stream));
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_mae_patchify_keep_u8_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, const int32_t* keep, void* out,
                                              int n_img, int channels, int R, int patch, int len_keep, int ld_out, float mean, float std,
                                              int dtype, void* stream) {
    // the parent's rules (mae.hip check_patchify), in its order
    if (!catalogue || !ids || !keep || !out || n_rows <= 0 || n_img <= 0 || channels <= 0 || R <= 0 || patch <= 0 || len_keep <= 0)
        return MOREC_E_ARG;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    if (R % patch) return MOREC_E_UNSUPPORTED;
    if (len_keep > (R / patch) * (R / patch)) return MOREC_E_ARG;
    const int ev = 16 / elt_size(dtype);
    if (patch % 4 || (channels * patch * patch) % ev || ld_out < channels * patch * patch || ld_out % ev || !aligned16(out)) return MOREC_E_ALIGN;
    if (std == 0.f) return MOREC_E_ARG;
    launch_patch_rows<true>(catalogue, ids, n_rows, keep, out, n_img, channels, R, patch, len_keep, ld_out, mean, std, dtype,
                            reinterpret_cast<hipStream_t>(stream));
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_pixels_to_nhwc_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, void* out, int n_img, int C, int H, int W,
                                        float mean, float std, int dtype, void* stream) {
    if (!catalogue || !ids || !out || n_rows <= 0 || n_img <= 0 || C <= 0 || H <= 0 || W <= 0 || !(std > 0.f)) return MOREC_E_ARG;
    const size_t per = (size_t)H * W * C;
    const bool wide = per % 4 == 0 && aligned4(catalogue) && aligned16(out);
    const size_t total = (size_t)n_img * (wide ? per / 4 : per);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto tag) {
            using T = MOREC_TAG_T(tag);
            if (wide)
                hipLaunchKernelGGL((pixels_idx_kernel<T, 4>), dim3(idx_grid(total)), dim3(256), 0, s, catalogue, ids, n_rows, (T*)out, n_img,
                                   per, mean, std);
            else
                hipLaunchKernelGGL((pixels_idx_kernel<T, 1>), dim3(idx_grid(total)), dim3(256), 0, s, catalogue, ids, n_rows, (T*)out, n_img,
                                   per, mean, std);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
