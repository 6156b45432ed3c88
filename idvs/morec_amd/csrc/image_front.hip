// image_front.hip -- the front kernels through which pixels enter a vision tower, and the only place where decoded uint8 images are
// normalised into rows: one kernel per layout, item ids optional.
//   * patch_rows<KEEP = false>   im2col rows of every patch            morec_swin_patchify_u8[_idx]       (Swin, BEiT)
//   * patch_rows<KEEP = true>    im2col rows of the patches keep[k]    morec_mae_patchify_keep_u8[_idx]   (MAE)
//   * pixels                     NHWC rows                             morec_pixels_to_nhwc[_idx]         (ResNet; fp32 NCHW: a plain copy)
// ids == nullptr (the direct entry points): image k of the output is image k of the pixel batch.  With ids (the _idx entry points) the
// pixels are an image catalogue [n_rows, R, R, 3] that stays on the device, a batch is its int32 item ids, and image k is computed from
// catalogue row ids[k] (clamped into [0, n_rows - 1]: a bad id never reads outside the catalogue).  Either way an element is
// ((float)u8 / 255 - mean) / std in fp32 with one rounding to the storage type -- ToTensor and Normalize of V/data_utils/dataset.py:69-73
// in the reference's operation order, at a quarter of the H2D and HBM bytes of fp32 pixels -- so the indexed form is
// bit-equal to catalogue.index_select(0, ids) through the direct one.  No atomics, every output element has one writer.
#include "common.hpp"

namespace {

// IDS is a template flag, not a run-time null test: the indexed instantiations are then the code they were before the direct forms moved
// in (with the run-time test the kept-patch form measured 1 % slower through ids, profiles/image_front.txt).
template <bool IDS>
__device__ __forceinline__ int image_row(const int32_t* __restrict__ ids, int n_rows, int n) {
    if constexpr (IDS) return min(max(ids[n], 0), n_rows - 1);
    return n;
}

// f(std::true_type / std::false_type) by a run-time flag
template <typename F>
void by_flag(bool flag, F&& f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// out[row, (c, i, j)] = norm(px[image n, py * ps + i, px * ps + j, c]); row = n * rows_per_img + r and (py, px) = patch r (KEEP: patch
// keep[row]; outside [0, G * G) leaves a zero row).  thread = PW pixels of one (row, i) run: PW == 4 reads the 12 bytes of 4 RGB pixels
// as three dwords and writes one 4-element store per channel (Cin == 3, ps % 4 == 0); PW == 1 moves single elements.
template <typename T, int PW, bool KEEP, bool IDS>
__global__ __launch_bounds__(256) void patch_rows_kernel(const uint8_t* __restrict__ px, const int32_t* __restrict__ ids, int n_rows,
                                                         const int32_t* __restrict__ keep, T* __restrict__ out, int n_img, int Cin, int R,
                                                         int ps, int rows_per_img, int ld_out, float mean, float std) {
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
        const int py = patch / G, pxx = patch - py * G;
        const uint8_t* src = px + (((size_t)image_row<IDS>(ids, n_rows, n) * R + (py * ps + i)) * R + pxx * ps + j0) * Cin;
        if constexpr (PW == 4) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);      // a multiple of 12 bytes into 4-byte aligned pixels
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

// out[k * per + o] = norm(px[image k, o]), per = H W C bytes of one image; thread = PW consecutive bytes (PW == 4: one dword load, one
// 4-element store; per % 4 == 0).
template <typename T, int PW, bool IDS>
__global__ __launch_bounds__(256) void pixels_kernel(const uint8_t* __restrict__ px, const int32_t* __restrict__ ids, int n_rows,
                                                     T* __restrict__ out, int n_img, size_t per, float mean, float std) {
    const size_t gpi = per / PW;                     // thread groups per image
    const size_t total = (size_t)n_img * gpi;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t k = e / gpi;
        const size_t o = (e - k * gpi) * PW;
        const uint8_t* src = px + (size_t)image_row<IDS>(ids, n_rows, (int)k) * per + o;
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

// fp32 NCHW pixels (normalised already) -> NHWC rows [n H W, C] in the compute type
template <typename T>
__global__ __launch_bounds__(256) void pixels_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ out, int n, int C, int H, int W) {
    const size_t hw = (size_t)H * W, total = (size_t)n * hw * C;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t pix = e / C;
        const int c = (int)(e - pix * C);
        const size_t img = pix / hw;
        io<T>::store1(out + e, src[(img * C + c) * hw + (pix - img * hw)]);
    }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the 4-pixel path: RGB, whole groups of 4 pixels, dword loads and 4-element stores on their natural alignment
bool wide_rows(const void* px, const void* out, int channels, int patch, int ld_out) {
    return channels == 3 && patch % 4 == 0 && ld_out % 4 == 0 && aligned4(px) && aligned16(out);
}

template <bool KEEP>
void launch_patch_rows(const uint8_t* px, const int32_t* ids, int n_rows, const int32_t* keep, void* out, int n_img, int channels, int R,
                       int patch, int rows_per_img, int ld_out, float mean, float std, int dtype, void* stream) {
    const bool wide = wide_rows(px, out, channels, patch, ld_out);
    const size_t total = (size_t)n_img * rows_per_img * patch * (wide ? patch / 4 : patch);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
        using T = MOREC_TAG_T(tag);
        by_flag(ids != nullptr, [&](auto has_ids) {
            constexpr bool IDS = decltype(has_ids)::value;
            if (wide)
                hipLaunchKernelGGL((patch_rows_kernel<T, 4, KEEP, IDS>), dim3(grid_for(total)), dim3(256), 0, s, px, ids, n_rows, keep, (T*)out,
                                   n_img, channels, R, patch, rows_per_img, ld_out, mean, std);
            else
                hipLaunchKernelGGL((patch_rows_kernel<T, 1, KEEP, IDS>), dim3(grid_for(total)), dim3(256), 0, s, px, ids, n_rows, keep, (T*)out,
                                   n_img, channels, R, patch, rows_per_img, ld_out, mean, std);
        });
    });
}

// The argument ladder and launch of each front, shared by its direct (ids == nullptr) and _idx entry point.
int swin_rows(const uint8_t* px, const int32_t* ids, int n_rows, void* out, int n_img, int channels, int R, int patch, int ld_out, float mean,
              float std, int dtype, void* stream) {
    if (!px || !out || n_img <= 0 || channels <= 0 || R <= 0 || patch <= 0 || std == 0.f) return MOREC_E_ARG;
    if (R % patch) return MOREC_E_UNSUPPORTED;
    if (ld_out < channels * patch * patch) return MOREC_E_ALIGN;
    if (dtype != MOREC_F32 && !is_h16(dtype)) return MOREC_E_DTYPE;
    const int G = R / patch;
    launch_patch_rows<false>(px, ids, n_rows, nullptr, out, n_img, channels, R, patch, G * G, ld_out, mean, std, dtype, stream);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

int mae_rows(const uint8_t* px, const int32_t* ids, int n_rows, const int32_t* keep, void* out, int n_img, int channels, int R, int patch,
             int len_keep, int ld_out, float mean, float std, int dtype, void* stream) {
    const int rc = check_patchify(px, keep, out, n_img, channels, R, patch, len_keep, ld_out, dtype);
    if (rc != MOREC_OK) return rc;
    if (std == 0.f) return MOREC_E_ARG;
    launch_patch_rows<true>(px, ids, n_rows, keep, out, n_img, channels, R, patch, len_keep, ld_out, mean, std, dtype, stream);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

int nhwc_rows(const uint8_t* px, const int32_t* ids, int n_rows, void* out, int n_img, int C, int H, int W, float mean, float std, int dtype,
              void* stream) {
    if (!px || !out || n_img <= 0 || C <= 0 || H <= 0 || W <= 0 || !(std > 0.f)) return MOREC_E_ARG;
    const size_t per = (size_t)H * W * C;
    const bool wide = per % 4 == 0 && aligned4(px) && aligned16(out);
    const size_t total = (size_t)n_img * (wide ? per / 4 : per);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!by_dtype(dtype, [&](auto tag) {
            using T = MOREC_TAG_T(tag);
            by_flag(ids != nullptr, [&](auto has_ids) {
                constexpr bool IDS = decltype(has_ids)::value;
                if (wide)
                    hipLaunchKernelGGL((pixels_kernel<T, 4, IDS>), dim3(grid_for(total)), dim3(256), 0, s, px, ids, n_rows, (T*)out, n_img, per,
                                       mean, std);
                else
                    hipLaunchKernelGGL((pixels_kernel<T, 1, IDS>), dim3(grid_for(total)), dim3(256), 0, s, px, ids, n_rows, (T*)out, n_img, per,
                                       mean, std);
            });
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

}  // namespace

extern "C" int morec_swin_patchify_u8(const uint8_t* pixels_hwc, void* out, int n_img, int channels, int R, int patch, int ld_out,
                                      float mean, float std, int dtype, void* stream) {
    return swin_rows(pixels_hwc, nullptr, 0, out, n_img, channels, R, patch, ld_out, mean, std, dtype, stream);
}

extern "C" int morec_swin_patchify_u8_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, void* out, int n_img, int channels,
                                          int R, int patch, int ld_out, float mean, float std, int dtype, void* stream) {
    if (!ids || n_rows <= 0) return MOREC_E_ARG;
    return swin_rows(catalogue, ids, n_rows, out, n_img, channels, R, patch, ld_out, mean, std, dtype, stream);
}

extern "C" int morec_mae_patchify_keep_u8(const uint8_t* pixels_hwc, const int32_t* keep, void* out, int n_img, int channels, int R,
                                          int patch, int len_keep, int ld_out, float mean, float std, int dtype, void* stream) {
    return mae_rows(pixels_hwc, nullptr, 0, keep, out, n_img, channels, R, patch, len_keep, ld_out, mean, std, dtype, stream);
}

extern "C" int morec_mae_patchify_keep_u8_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, const int32_t* keep, void* out,
                                              int n_img, int channels, int R, int patch, int len_keep, int ld_out, float mean, float std,
                                              int dtype, void* stream) {
    if (!ids || n_rows <= 0) return MOREC_E_ARG;
    return mae_rows(catalogue, ids, n_rows, keep, out, n_img, channels, R, patch, len_keep, ld_out, mean, std, dtype, stream);
}

extern "C" int morec_pixels_to_nhwc(const void* src, void* out, int n, int C, int H, int W, int src_u8, float mean, float std, int dtype,
                                    void* stream) {
    if (src_u8) return nhwc_rows(reinterpret_cast<const uint8_t*>(src), nullptr, 0, out, n, C, H, W, mean, std, dtype, stream);
    if (!src || !out || n <= 0 || C <= 0 || H <= 0 || W <= 0) return MOREC_E_ARG;
    const size_t total = (size_t)n * H * W * C;
    if (!by_dtype(dtype, [&](auto tag) {
            using T = MOREC_TAG_T(tag);
            hipLaunchKernelGGL((pixels_to_nhwc_kernel<T>), dim3(grid_for(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                               reinterpret_cast<const float*>(src), (T*)out, n, C, H, W);
        }))
        return MOREC_E_DTYPE;
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_pixels_to_nhwc_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, void* out, int n_img, int C, int H, int W,
                                        float mean, float std, int dtype, void* stream) {
    if (!ids || n_rows <= 0) return MOREC_E_ARG;
    return nhwc_rows(catalogue, ids, n_rows, out, n_img, C, H, W, mean, std, dtype, stream);
}
