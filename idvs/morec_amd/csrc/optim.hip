// optim.hip -- fused AdamW over a flat fp32 arena (one launch per hyper-parameter group) with the bf16
// shadow refresh folded in.  torch.optim.AdamW semantics (T/run.py:159-162,246):
//   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
//   p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// HBM-bound: 16 B read + 12 B written per parameter (+ 2 B shadow).
//
// morec_step_params / morec_adamw_sp: the same update driven by a DEVICE-resident block (step count, bias corrections, loss scale,
// overflow flag) -- the GradScaler protocol of the reference's fp16 step (T/run.py:210,243-247) without a host round trip, and the
// form a captured graph can replay (no per-step host scalars among the kernel arguments).
//
// morec_grad_norm_check / morec_step_decide_ex: global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) and an LR schedule in the
// same block.  The overflow pass over the gradients also leaves one partial sum of squares per workgroup (no floating-point atomics, fixed
// order: bit-reproducible); the decision kernel folds them in double, turns the norm into the clip coefficient, the applied-step count into
// the LR multiplier, and morec_adamw_sp reads both -- when the block's flags word says they are set.  A block whose three formerly spare
// words are zero behaves as it always did.
#include "common.hpp"

// SH16: storage type of the shadow (bf16 | f16).  sp != nullptr: step state from the device block (skip when sp->apply == 0).
template <typename SH16>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    unsigned short* __restrict__ shadow, size_t n4, float lr,
                                                    float b1, float b2, float eps, float wd, float inv_bc1,
                                                    float inv_sqrt_bc2, float gscale, const morec_step_params* __restrict__ sp) {
    if (sp) {
        if (!sp->apply) return;           // a non-finite gradient somewhere in this step: parameters, moments and shadow stay as they are
        inv_bc1 = 1.0f / sp->bc1;
        inv_sqrt_bc2 = rsqrtf(sp->bc2);
        gscale = sp->inv_scale;
        // clip coefficient / LR multiplier of morec_step_decide_ex, when it set them (flags word clear: the update of a plain block, bit for bit)
        if (sp->ctl_flags & MOREC_SP_CLIP) gscale *= sp->clip_coef;
        if (sp->ctl_flags & MOREC_SP_LR_MULT) lr *= sp->lr_mult;
    }
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        float pa[4] = {pp.x, pp.y, pp.z, pp.w};
        const float ga[4] = {gg.x * gscale, gg.y * gscale, gg.z * gscale, gg.w * gscale};
        float ma[4] = {mm.x, mm.y, mm.z, mm.w};
        float va[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pa[k] *= (1.0f - lr * wd);
            ma[k] = b1 * ma[k] + (1.0f - b1) * ga[k];
            va[k] = b2 * va[k] + (1.0f - b2) * ga[k] * ga[k];
            const float denom = sqrtf(va[k]) * inv_sqrt_bc2 + eps;
            pa[k] -= (lr * inv_bc1) * (ma[k] / denom);
        }
        reinterpret_cast<float4*>(p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
        reinterpret_cast<float4*>(m)[i] = make_float4(ma[0], ma[1], ma[2], ma[3]);
        reinterpret_cast<float4*>(v)[i] = make_float4(va[0], va[1], va[2], va[3]);
        if (shadow) {
            uint2 s;
            s.x = h16<SH16>::pack2(pa[0], pa[1]);
            s.y = h16<SH16>::pack2(pa[2], pa[3]);
            reinterpret_cast<uint2*>(shadow)[i] = s;
        }
    }
}

extern "C" int morec_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                           size_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || step < 1) return MOREC_E_ARG;
    if (n == 0) return MOREC_OK;
    if (n % 4 || !aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
        (shadow_bf16 && (reinterpret_cast<uintptr_t>(shadow_bf16) & 7u)))
        return MOREC_E_ALIGN;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(adamw_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), param,
                       grad, exp_avg, exp_avg_sq, reinterpret_cast<unsigned short*>(shadow_bf16), n4, lr, beta1, beta2,
                       eps, weight_decay, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), grad_scale, (const morec_step_params*)nullptr);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

extern "C" int morec_adamw_sp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype,
                              size_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                              const morec_step_params* sp, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !sp) return MOREC_E_ARG;
    if (n == 0) return MOREC_OK;
    if (shadow && !is_h16(shadow_dtype)) return MOREC_E_DTYPE;
    if (n % 4 || !aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
        (shadow && (reinterpret_cast<uintptr_t>(shadow) & 7u)))
        return MOREC_E_ALIGN;
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (shadow && shadow_dtype == MOREC_F16)
        hipLaunchKernelGGL(adamw_kernel<f16>, dim3((unsigned)blocks), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq,
                           reinterpret_cast<unsigned short*>(shadow), n4, lr, beta1, beta2, eps, weight_decay, 1.f, 1.f, 1.f, sp);
    else
        hipLaunchKernelGGL(adamw_kernel<bf16>, dim3((unsigned)blocks), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq,
                           reinterpret_cast<unsigned short*>(shadow), n4, lr, beta1, beta2, eps, weight_decay, 1.f, 1.f, 1.f, sp);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// ---- the device-resident step block ------------------------------------------------------------------------------------------------
__global__ void step_params_init_kernel(morec_step_params* sp, float init_scale, int step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        morec_step_params z = {};
        z.step = step;
        z.loss_scale = init_scale;
        z.inv_scale = 1.0f / init_scale;
        z.bc1 = 1.f; z.bc2 = 1.f;
        z.apply = 1;
        z.drop_seed = 0x9E3779B97F4A7C15ull * (uint64_t)(step + 1);
        uint64_t x = z.drop_seed;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        z.drop_seed_mixed = x ^ (x >> 31);
        *sp = z;
    }
}
extern "C" int morec_step_params_init(morec_step_params* sp, float init_scale, int step, void* stream) {
    if (!sp || !(init_scale > 0.f) || step < 0) return MOREC_E_ARG;
    hipLaunchKernelGGL(step_params_init_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sp, init_scale, step);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// found_inf |= any(!isfinite(grad)): one pass over the fp32 gradients (4 B / parameter), one atomic per wavefront that saw one
__global__ __launch_bounds__(256) void grad_check_kernel(const float* __restrict__ g, size_t n4, morec_step_params* __restrict__ sp) {
    bool bad = false;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        // !(|x| <= FLT_MAX) is true for +-inf and for NaN
        bad |= !(fabsf(v.x) <= 3.4028234663852886e38f) | !(fabsf(v.y) <= 3.4028234663852886e38f) | !(fabsf(v.z) <= 3.4028234663852886e38f) |
               !(fabsf(v.w) <= 3.4028234663852886e38f);
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&sp->found_inf, 1);
}
extern "C" int morec_grad_check_finite(const float* grad, size_t n, morec_step_params* sp, void* stream) {
    if (!grad || !sp) return MOREC_E_ARG;
    if (n == 0) return MOREC_OK;
    if (n % 4 || !aligned16(grad)) return MOREC_E_ALIGN;
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(grad_check_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), grad, n4, sp);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// GradScaler.step + update (torch/amp/grad_scaler.py: step() skips optimizer.step() when an inf / NaN was found; update() multiplies the
// scale by backoff_factor then, and by growth_factor after growth_interval consecutive clean steps) as ONE single-thread kernel between
// the checks and the AdamW launches of a step.  The bias corrections are formed in double like torch's `1 - beta ** step`.
__global__ void step_decide_kernel(morec_step_params* sp, float beta1, float beta2, float growth, float backoff, int interval, int dynamic) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    morec_step_params z = *sp;
    z.inv_scale = 1.0f / z.loss_scale;        // the scale this step's gradients carry
    if (z.found_inf) {
        z.apply = 0;
        z.skipped += 1;
        if (dynamic) { z.loss_scale *= backoff; z.growth_tracker = 0; }
    } else {
        z.apply = 1;
        z.step += 1;
        z.bc1 = (float)(1.0 - pow((double)beta1, (double)z.step));
        z.bc2 = (float)(1.0 - pow((double)beta2, (double)z.step));
        if (dynamic) {
            z.growth_tracker += 1;
            if (z.growth_tracker >= interval) { z.loss_scale *= growth; z.growth_tracker = 0; }
        }
    }
    z.found_inf = 0;
    z.ctl_flags = 0;                          // the plain decision carries no clip coefficient and no LR multiplier (clip_coef / lr_mult keep their bits, unread)
    {   // the dropout seed word of the NEXT forward / backward pair (splitmix64 step): every decide call draws a new one
        uint64_t x = (z.drop_seed += 0x9E3779B97F4A7C15ull);
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        z.drop_seed_mixed = x ^ (x >> 31);
    }
    *sp = z;
}
extern "C" int morec_step_decide(morec_step_params* sp, float beta1, float beta2, float growth_factor, float backoff_factor,
                                 int growth_interval, int dynamic, void* stream) {
    if (!sp || growth_interval < 1 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f)) return MOREC_E_ARG;
    hipLaunchKernelGGL(step_decide_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sp, beta1, beta2, growth_factor,
                       backoff_factor, growth_interval, dynamic);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// ---- global-norm clipping + LR schedule on the device ------------------------------------------------------------------------------
// One pass over a gradient arena: found_inf as grad_check_kernel, plus this block's share of sum((g / S)^2) into partials[blockIdx.x].
// Deterministic: the grid depends on n alone (morec_grad_norm_blocks), a thread adds its float4s in index order ((x^2 + y^2) + (z^2 + w^2) each),
// the 64 lanes of a wave meet in a fixed xor butterfly, lane 0 adds the four wave sums in wave order and stores the slot.  No floating-point atomics.
// Longest chain of fp32 additions into one partial: ceil(n4 / (blocks * 256)) + 1 in the thread, 6 in the wave, 3 in the block.
#define MOREC_NORM_MAX_BLOCKS 2048
static inline size_t grad_norm_blocks(size_t n) {
    size_t blocks = (n / 4 + 255) / 256;
    return blocks > MOREC_NORM_MAX_BLOCKS ? MOREC_NORM_MAX_BLOCKS : blocks;
}
extern "C" size_t morec_grad_norm_blocks(size_t n) { return grad_norm_blocks(n); }

__global__ __launch_bounds__(256) void grad_norm_check_kernel(const float* __restrict__ g, size_t n4, morec_step_params* __restrict__ sp,
                                                              float* __restrict__ partials) {
    __shared__ float wsum[4];
    const float inv = 1.0f / sp->loss_scale;      // the scale THESE gradients carry (morec_step_decide moves loss_scale on afterwards)
    bool bad = false;
    float acc = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        bad |= !(fabsf(v.x) <= 3.4028234663852886e38f) | !(fabsf(v.y) <= 3.4028234663852886e38f) | !(fabsf(v.z) <= 3.4028234663852886e38f) |
               !(fabsf(v.w) <= 3.4028234663852886e38f);
        const float x = v.x * inv, y = v.y * inv, z = v.z * inv, w = v.w * inv;
        acc += (x * x + y * y) + (z * z + w * w);
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&sp->found_inf, 1);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
extern "C" int morec_grad_norm_check(const float* grad, size_t n, morec_step_params* sp, float* partials, size_t slot, size_t n_slots,
                                     void* stream) {
    if (!grad || !sp || !partials) return MOREC_E_ARG;
    if (n == 0) return MOREC_OK;
    if (n % 4 || !aligned16(grad)) return MOREC_E_ALIGN;
    const size_t blocks = grad_norm_blocks(n);
    if (slot > n_slots || blocks > n_slots - slot) return MOREC_E_ARG;      // the partials of this arena would run past the buffer
    hipLaunchKernelGGL(grad_norm_check_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), grad, n / 4, sp,
                       partials + slot);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}

// the multiplier of the optimizer step with 0-based index t (include/morec_hip.h states the formula)
__device__ static float lr_multiplier(int t, morec_lr_schedule s) {
    if (t < s.warmup_steps) return (float)((double)t / (double)s.warmup_steps);
    if (s.kind == MOREC_LR_CONSTANT) return 1.f;
    const int span = s.total_steps - s.warmup_steps;
    double prog = (double)(t - s.warmup_steps) / (double)(span > 1 ? span : 1);
    if (prog > 1.0) prog = 1.0;
    const double shape = s.kind == MOREC_LR_COSINE ? 0.5 * (1.0 + cos(3.14159265358979323846 * prog)) : 1.0 - prog;
    return (float)((double)s.min_ratio + (1.0 - (double)s.min_ratio) * shape);
}

// step_decide_kernel with the gradient norm in front of the verdict and the clip coefficient / LR multiplier behind it.  The 256 threads only
// stage the partials in LDS (coalesced reads); thread 0 alone folds them, in ascending slot order, in double, and takes every decision.
#define MOREC_DECIDE_STAGE 4096
__global__ __launch_bounds__(256) void step_decide_ex_kernel(morec_step_params* sp, float beta1, float beta2, float growth, float backoff, int interval,
                                                             int dynamic, const float* __restrict__ partials, size_t n_partials, float max_norm,
                                                             morec_lr_schedule sched, int has_sched, float* grad_norm_out) {
    __shared__ __attribute__((aligned(16))) float stage[MOREC_DECIDE_STAGE];
    double total = 0.0;
    for (size_t base = 0; base < n_partials; base += MOREC_DECIDE_STAGE) {
        const size_t cnt = n_partials - base < MOREC_DECIDE_STAGE ? n_partials - base : MOREC_DECIDE_STAGE;
        const size_t cnt16 = (cnt + 15) & ~(size_t)15;      // zero fill up to a multiple of 16: + 0.0 changes no sum
        for (size_t i = threadIdx.x; i < cnt16; i += blockDim.x) stage[i] = i < cnt ? partials[base + i] : 0.f;
        __syncthreads();
        if (threadIdx.x == 0) {
            // still one chain of additions in ascending slot order; the LDS reads run 16 slots ahead of it instead of one read per addition
            for (size_t i = 0; i < cnt16; i += 16) {
                float4 q[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const float4*>(&stage[i + 4 * j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    total += (double)q[j].x;
                    total += (double)q[j].y;
                    total += (double)q[j].z;
                    total += (double)q[j].w;
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    morec_step_params z = *sp;
    const double norm = sqrt(total);
    if (n_partials && !(norm <= 3.4028234663852886e38)) z.found_inf = 1;      // inf / NaN total (an overflowing square included): skip the step
    if (grad_norm_out) *grad_norm_out = (float)norm;
    z.inv_scale = 1.0f / z.loss_scale;
    if (z.found_inf) {
        z.apply = 0;
        z.skipped += 1;
        if (dynamic) { z.loss_scale *= backoff; z.growth_tracker = 0; }
    } else {
        z.apply = 1;
        z.step += 1;
        z.bc1 = (float)(1.0 - pow((double)beta1, (double)z.step));
        z.bc2 = (float)(1.0 - pow((double)beta2, (double)z.step));
        if (dynamic) {
            z.growth_tracker += 1;
            if (z.growth_tracker >= interval) { z.loss_scale *= growth; z.growth_tracker = 0; }
        }
    }
    z.found_inf = 0;
    z.ctl_flags = 0;
    z.clip_coef = 1.f;
    z.lr_mult = 1.f;
    if (max_norm > 0.f && n_partials) {
        z.ctl_flags |= MOREC_SP_CLIP;
        if (z.apply) {
            const double c = (double)max_norm / (norm + 1e-6);
            z.clip_coef = (float)(c < 1.0 ? c : 1.0);
        }
    }
    if (has_sched) {       // index of the step being applied, or -- after a skip -- of the next one to be: a skipped step does not advance the schedule
        z.ctl_flags |= MOREC_SP_LR_MULT;
        z.lr_mult = lr_multiplier(z.apply ? z.step - 1 : z.step, sched);
    }
    {
        uint64_t x = (z.drop_seed += 0x9E3779B97F4A7C15ull);
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        z.drop_seed_mixed = x ^ (x >> 31);
    }
    *sp = z;
}
extern "C" int morec_step_decide_ex(morec_step_params* sp, float beta1, float beta2, float growth_factor, float backoff_factor,
                                    int growth_interval, int dynamic, const float* partials, size_t n_partials, float max_norm,
                                    const morec_lr_schedule* sched, float* grad_norm_out, void* stream) {
    if (!sp || growth_interval < 1 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f)) return MOREC_E_ARG;
    if (!partials && (n_partials || max_norm > 0.f)) return MOREC_E_ARG;
    if (max_norm > 0.f && n_partials == 0) return MOREC_E_ARG;
    if (!(max_norm == max_norm)) return MOREC_E_ARG;
    if (partials && (reinterpret_cast<uintptr_t>(partials) & 3u)) return MOREC_E_ALIGN;
    if (grad_norm_out && (reinterpret_cast<uintptr_t>(grad_norm_out) & 3u)) return MOREC_E_ALIGN;
    morec_lr_schedule s = {};
    if (sched) {
        s = *sched;
        if (s.kind < MOREC_LR_CONSTANT || s.kind > MOREC_LR_COSINE || s.warmup_steps < 0 || !(s.min_ratio >= 0.f && s.min_ratio <= 1.f)) return MOREC_E_ARG;
        if (s.kind != MOREC_LR_CONSTANT && s.total_steps < s.warmup_steps) return MOREC_E_ARG;
    }
    hipLaunchKernelGGL(step_decide_ex_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), sp, beta1, beta2, growth_factor,
                       backoff_factor, growth_interval, dynamic, partials, n_partials, max_norm, s, sched ? 1 : 0, grad_norm_out);
    MOREC_CHECK_LAUNCH();
    return MOREC_OK;
}
