/*
 * morec_hip.h -- C-ABI of libmorec_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * end-to-end MoRec in-batch training step (westlake-repl/IDvs.MoRec, inbatch_sasrec_e2e_text).
 *
 * The reference is pure Python over PyTorch/HuggingFace and has NO FFI of its own:
 * every entry point below therefore cites the reference Python call site whose arithmetic it
 * replaces (paths relative to /root/reference, T/ = inbatch_sasrec_e2e_text/), and INTEGRATION.md
 * shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless named h_*;
 *   - the caller owns every buffer (PyTorch caching allocator); every call is asynchronous on `stream` (a hipStream_t passed as
 *     void*) and does no host synchronisation;
 *   - return 0 on success, a negative MOREC_E_* for bad arguments, a positive value = hipError_t;
 *   - dtype codes: MOREC_F32 = 0 (exact-fp32 MFMA, v_mfma_f32_16x16x4_f32), MOREC_BF16 = 1 (bf16 operands, fp32 accumulate:
 *     v_mfma_f32_32x32x16_bf16 in the 256 x 256 eight-phase GEMMs, v_mfma_f32_16x16x32_bf16 in attention, scoring and the
 *     small-problem GEMMs), MOREC_F16 = 2 (IEEE fp16 operands, fp32 accumulate: v_mfma_f32_32x32x16_f16 / 16x16x32_f16 in the same
 *     kernels -- the arithmetic of the reference's `torch.cuda.amp.autocast()` step, T/run.py:242-247, three more significand bits
 *     than bf16 at the same MFMA rate; gradients need the loss scaling of morec_step_params below).  "bf16" in an entry point's
 *     description means either 16-bit type unless it says otherwise (the Swin kernels too, V/run.py's autocast step); morec_split_bf16x3
 *     takes MOREC_BF16 only;
 *   - row-major matrices with explicit leading dimensions in ELEMENTS; every base pointer and
 *     every row pitch must be 16-byte aligned (MOREC_E_ALIGN otherwise);
 *   - item ids are int32 on the device (the host narrows the int64 ids PyTorch provides).
 *
 * State the library keeps (everything else is stateless and re-entrant; first-call set-up of a kernel's launch attributes is
 * behind thread-safe function-local statics).  One process drives one GPU (the reference's process model, T/run.py:305-321):
 *   1. process-wide knobs: ONE table (csrc/tuning.hip; the keys and MOREC_* variables are listed at morec_tuning_set below).  The
 *      environment is read once, thread-safely, the first time the table is touched -- by a launch or by morec_tuning_set --
 *      and supplies the defaults; a morec_tuning_set call wins over it from then on, whichever came first.  (Before, each
 *      variable was read lazily at some first use, so whether a set key or its variable won depended on the order of calls.)
 *      Every selectable kernel computes the same function to the same accuracy; "gemm8p_tail_split" = 1 changes the
 *      fp32 SUMMATION ORDER (and with it the last-bit rounding pattern of 16-bit outputs), which is why it is off unless asked
 *      for.  "gemm8p_mfma" regroups the sum inside the instruction (a K-tile as two MFMAs over 32 products or four over 16):
 *      nothing promises equal rounding there, but on MI355X the two shapes measured bit-identical (profiles/mfma_shape_step.txt).
 *      Set knobs before the first launch or between steps, not concurrently with launches;
 *   2. with "gemm8p_tail_split" = 1 only: one device scratch allocation per stream (the only memory the library ever allocates);
 *   3. morec_comm handles (below): created and destroyed by the caller;
 *   4. the dropout seed source (morec_dropout_seed_source): one device pointer, NULL by default;
 *   5. the ring of 256 events behind morec_stream_wait_stream (created on first use, never destroyed);
 *   6. deterministic mode only (morec_tuning_set("deterministic", 1) / MOREC_DETERMINISTIC=1; the reference sets torch's
 *      deterministic flags, T/run.py:313-314): one partial-sum scratch per (device, stream), grown on demand OUTSIDE graph capture
 *      (morec_det_scratch_reserve).  In this mode no kernel falls back to atomics: a call that cannot run its fixed-order form
 *      (scratch unavailable, no token order, row width outside the vector layout) returns an error instead;
 *   7. deterministic mode only: the deferred-fold scope (morec_fold_defer_begin): one host-side job list and one device scratch that is
 *      sized during the first steps and then kept.
 */
#ifndef MOREC_HIP_H
#define MOREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOREC_F32 0
#define MOREC_BF16 1
#define MOREC_F16 2 /* IEEE half operands / activations, fp32 accumulate: the reference's own GPU arithmetic (fp16 autocast, T/run.py:242) */

#define MOREC_OK 0
#define MOREC_E_ARG (-1)         /* null pointer / non-positive size */
#define MOREC_E_ALIGN (-2)       /* pointer or pitch not 16-byte aligned / size not a multiple of the vector width */
#define MOREC_E_UNSUPPORTED (-3) /* shape outside what the kernel was written for */
#define MOREC_E_DTYPE (-4)
#define MOREC_E_COMM (-5)        /* an RCCL call failed: morec_comm_last_error() */

#define MOREC_ACT_NONE 0
#define MOREC_ACT_GELU 1 /* exact erf GELU (HF BertIntermediate; T/model/encoders.py:59 nn.GELU) */
#define MOREC_ACT_RELU 2 /* T/model/modules.py:12 */
#define MOREC_DACT_MUL 3 /* morec_gemm_desc.dact only: C = acc * dact_in[m,n] (dact_in already holds act'(pre), see aux_deriv) */

const char* morec_strerror(int code);
int morec_version(void);
/* Process-wide knobs (measurement / A-B aid; see "State the library keeps" above).  key | values | environment variable | default.
 * Which NT GEMM kernel runs is decided by one function, gemm_plan() in csrc/gemm_plan.hpp; its rules are tried in the order
 * skinny, skinny_wide, two_w, eight_p, small, generic, and morec_gemm_plan() below answers for a descriptor without a GPU.
 *   "gemm8p"             0 automatic | 1 never | 2 wherever eligible                                   MOREC_GEMM8P              0
 *                        the 256 x 256 eight-phase GEMM (16-bit operands, K % 8 == 0, K > 64, N >= 64, plain stores).  Automatic: at least
 *                        192 tiles of 256 x 256 (160 when K >= 2048) and at most 34 % of the tile columns past N.  Also gemm_tn's eight-phase kernel;
 *   "gemm2w"             0 automatic | 1 never | 2 every eligible product                              MOREC_GEMM2W              0
 *                        the 256 x 128 two-workgroups-per-CU GEMM (16-bit in and out, K % 64 == 0, >= 64 tiles; plain / bias, GELU (+ second
 *                        output), x dact_in (+ column sums)).  Automatic: plain products with M >= 8192, K <= 2048 whose N leaves at least a
 *                        fifth of its 256-wide tiles empty (4 x padding >= N: N = 384, and also 128, 192, 320, 576), and x dact_in products
 *                        with 16384 <= M <= 40000, K <= 768 or M <= 70000, K <= 512.  It is asked BEFORE gemm8p;
 *   "gemm_small"         0 automatic | 1 never | 2 every eligible product                              MOREC_GEMM_SMALL          0
 *                        the 64 x 64 four-stage-ring GEMM (16-bit in and out, K >= 64).  Automatic: at most 128 tiles of 128 x 128, K >= 1024,
 *                        N >= 256, no second output, no column sums (the SASRec layers); outputs bit-identical to the 128 x 128 kernel's;
 *   "gemm_skinny"        0 automatic | 1 never | 2 gemm_skinny only                                    MOREC_GEMM_SKINNY         0
 *                        the streaming kernels, M >= 8192, 16-bit in and out, alpha 1, pitches % 8 == 0.  gemm_skinny: plain / bias products,
 *                        64 <= N <= 128 with K <= 384, or N <= 288 with K <= 96.  gemm_skinny_wide: GELU(product + bias) without a second
 *                        output, 288 < N <= 768, 32 <= K <= 192.  With 1 or 2 morec_mlp_dact_recompute_supported() answers 0;
 *   "ce8p"               0 automatic | 1 always the 128 x 128 kernels | 2 wherever the shapes allow    MOREC_CE8P                0
 *                        scoring kernels on 256 x 256 eight-phase tiles (16-bit, D > 64, D % 8 == Nc % 8 == (B S) % 8 == 0);
 *   "featproj"           0 automatic | 1 never | 2 wherever the rules allow                            MOREC_FEATPROJ            0
 *                        the fused gather + first projection of the two-stage tower (morec_featproj_fwd; 16-bit, Kw % 8 == D % 8 == 0).
 *                        Automatic: R Kw D <= 2^29 (morec_featproj_supported);
 *   "featfuse"           0 automatic | 1 never | 2 wherever the rules allow                            MOREC_FEATFUSE            0
 *                        the fused gather + projection + ID fusion of the two-stage ID (+) modality tower (morec_featfuse_fwd; 16-bit,
 *                        Kw % 8 == D % 8 == 0).  Automatic: R Kw D <= 3 . 2^28 (morec_featfuse_supported);
 *   "gemm8p_tmr"         0 always 256-row tiles | 1 automatic | 224 | 192 (other values: 1)            MOREC_GEMM8P_TMR          1
 *   "gemm8p_ngroup"      tile order: -1 automatic column groups | 0 row-major | n groups of n N-tiles  MOREC_GEMM8P_NGROUP       -1
 *   "gemm8p_reserve_cus" 0..128 CUs (multiple of 8) left out of the persistent grid for a concurrent RCCL kernel   MOREC_GEMM8P_RESERVE_CUS   0
 *   "gemm8p_tail_split"  1 = split the last, partly filled round of tiles along K between two workgroups (K >= 1536)   MOREC_GEMM8P_TAIL_SPLIT   0
 *   "gemm8p_tail_bias"   0..16: share of K the first part takes in that split                          -                         2
 *   "gemm8p_mfma"        MFMA shape of gemm8p's main loop: 0 automatic | 16 (16x16x32) | 32 (32x32x16); other values are     MOREC_GEMM8P_MFMA         0
 *                        refused with MOREC_E_UNSUPPORTED (from the environment: 0).  Tiles, schedule and memory traffic do not depend on it;
 *   "gemm8p_debug"       ablation bits (diagnostics)                                                   MOREC_GEMM8P_DEBUG        0
 *   "gemm8p_stamps_lo", "gemm8p_stamps_hi"  device address of a cycle-stamp buffer, in halves          -                         0
 *   "deterministic"      1 = fixed summation order everywhere (state item 6) | 0 off                   MOREC_DETERMINISTIC       0
 *   "fold_defer"         1 = morec_fold_defer_begin opens a scope (state item 7) | 0 = it never does   MOREC_FOLD_DEFER          1
 *   "attn_stream"        the streaming attention kernels (attention_stream.hip): 0 = for T > 256 only (every T <= 256 call     MOREC_ATTN_STREAM         0
 *                        reaches the kernel it reaches without them) | 1 = never: T > 256 is MOREC_E_UNSUPPORTED | 2 = for every T > 64
 *                        (tests and measurements: the tile edges with small inputs, the strip kernels' range on the matrix cores)
 *   "gemm_tile"          one tile shape for every two-buffer GEMM (csrc/gemm_plan.hpp, rule 6): 0 automatic |       MOREC_GEMM_TILE           0
 *                        129 = 128 x 128, 8 waves | 128 = 128 x 128, 4 waves | 1024 = 256 x 256, 16 waves | 256 = 256 x 256, 8 waves |
 *                        2128 = 256 x 128, 8 waves, 64-byte K stages; other values are refused with MOREC_E_UNSUPPORTED (the environment
 *                        variable is taken as given).  A tuning and test aid: it does not change which products reach these kernels;
 *   "gemm_epi"           epilogue form of the two-buffer GEMMs: 0 block staging | 1 per-wave slices | 2 automatic    MOREC_GEMM_EPI            2
 *                        (wave when N <= 1024 or there is a second output); other values are refused with MOREC_E_UNSUPPORTED.
 *                        The environment variable spells them w... = 1, anything else = 0, unset = automatic
 * Environment only:
 *   MOREC_GEMM2W_STAGGER first-round stagger experiment of gemm2w                                                           0
 *   MOREC_TN8P_SKIP      0 = never the block-skipping variant of gemm_tn's eight-phase kernel                                1
 *   MOREC_ATTN_MFMA64, MOREC_ATTN_F32_MFMA   0 = the VALU attention kernels for 32 < T <= 64 / for fp32                      1
 *   MOREC_SWIN_WPW_MIN   fewest windows per workgroup of the window-attention backward (>= 1)                                8
 *   MOREC_SWIN_BWD_WIDE  0 = the narrow window-attention backward                                                            1
 *   MOREC_QUIET          1 = no once-per-process notes on stderr                                                             0
 * Returns MOREC_E_UNSUPPORTED for an unknown key or a value "gemm8p_mfma", "gemm_tile" or "gemm_epi" does not take.  No reference counterpart (the reference has no kernels,
 * SURVEY.md §2). */
int morec_tuning_set(const char* key, int value);
/* Deterministic mode: make the partial-sum scratch of `stream` hold at least n_floats (call outside graph capture; under capture the
 * scratch cannot grow and a launch that needs more returns hipErrorOutOfMemory).  The largest user of the encoder step is the LayerNorm
 * backward: blocks x 3 x N floats.  No reference counterpart (torch.use_deterministic_algorithms, T/run.py:313-314, has no workspace API). */
int morec_det_scratch_reserve(size_t n_floats, void* stream);
/* Deferred folds (deterministic mode; knob "fold_defer").  The fixed-order folds of the deterministic mode -- the partial rows of the
 * LayerNorm backward, the per-tile / per-sequence column sums behind morec_gemm_nt_colsum and morec_attn_bwd_dbias, morec_colsum, the
 * position / type rows -- all add into PARAMETER gradients, which nothing in a backward pass reads (the per-head bias tiles of the window
 * attention feed morec_swin_bias_reduce and are always folded in place).  Between morec_fold_defer_begin(stream)
 * and morec_fold_defer_end() these calls, when issued on `stream`, launch their producing kernel as usual but only QUEUE the fold;
 * morec_fold_flush(run_on) launches everything queued so far as one kernel per 64 jobs on the stream `run_on` (any stream: the caller orders it
 * behind the producers, e.g. morec_stream_wait_stream(run_on, stream)).  Jobs that add into the same destination run in queue order, and
 * every job sums in the order of the in-place launch: the gradients are bit-identical to those of the same calls outside a scope.
 * RULES: (1) a gradient written through a deferred job is DEFINED only after the flush that holds its job has run; (2) the partial rows live
 * in a library-owned scratch that is rewound by morec_fold_defer_end: call it only where `stream` has been made to wait for every stream a
 * flush ran on (or that stream is `stream` itself), and flush before it -- jobs still queued at the end are dropped.  (The workspace handed to
 * morec_gemm_nt_colsum / morec_mlp_dact_recompute / morec_attn_bwd_dbias / morec_swin_attn_bwd_dbias is not used under a scope: a region of
 * the library's scratch takes its place, so the caller may reuse its buffer at once, as outside a scope.)
 * morec_fold_defer_begin opens nothing -- every call behaves as without it -- when the knob is 0, outside the deterministic mode, or while
 * `stream` is being captured into a graph (a captured step keeps its folds in place); morec_fold_defer_active() tells (1 / 0).  One scope
 * per process at a time (a second stream: MOREC_E_UNSUPPORTED).  The scratch grows by hipMalloc while the first scopes find their size and
 * is merged into one buffer at the end of such a scope (a device synchronisation); afterwards a scope allocates nothing.
 * morec_fold_stats: out4 = {device allocations made for the scratch so far, its size in bytes, jobs queued so far, flush launches so far}.
 * No reference counterpart (torch.use_deterministic_algorithms has no such notion). */
int morec_fold_defer_begin(void* stream);
int morec_fold_defer_active(void);
int morec_fold_flush(void* run_on);
int morec_fold_defer_end(void);
int morec_fold_stats(unsigned long long* out4);

/* ------------------------------------------------------------------------------------------
 * GEMM  C[M,N] (+)= alpha * A[M,K] . B[N,K]^T  (both operands K-contiguous, "NT")
 * Replaces every nn.Linear / torch.matmul on the path (T/model/modules.py:14,56-61;
 * HF modeling_bert.py BertSelfAttention/BertSelfOutput/BertIntermediate/BertOutput;
 * T/model/encoders.py:69; T/model/model.py:49) and, fed with transposed operands, their
 * autograd backward (dX = dY.W, dW = dY^T.X).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, K;
    int lda, ldb, ldc;
    int in_dtype;      /* dtype of A and B */
    int out_dtype;     /* dtype of C (and aux_out / dact_in) */
    int act;           /* MOREC_ACT_*: C = act(acc + bias); aux_out (optional) receives acc + bias */
    int dact;          /* MOREC_ACT_*: C = (acc) * act'(dact_in[m,n]) -- backward through an activation */
    int accumulate;    /* 0: C = v   1: C += v (non-atomic)   2: atomicAdd (fp32 C only; used with split_k) */
    int split_k;       /* >= 1: K is cut into split_k chunks over blockIdx.z (requires accumulate == 2 when > 1) */
    float alpha;
    int aux_deriv;     /* 1: aux_out receives act'(acc + bias) instead of acc + bias -- the backward GEMM then runs with
                        * dact = MOREC_DACT_MUL (one multiply per element instead of re-evaluating erf / exp for GELU') */
} morec_gemm_desc;

int morec_gemm_nt(const morec_gemm_desc* d, const void* A, const void* B, void* C, const float* bias,
                  void* aux_out, const void* dact_in, void* stream);

/* Same, and colsum_out[n] += sum_m C[m, n]: with a dact epilogue C is the pre-activation gradient of the layer below, so
 * this is that layer's bias gradient (autograd of nn.Linear: db = dY.sum(0)) without a second pass over C.  The sums are
 * taken from the output tile while it is staged in LDS (the values as rounded to the output dtype), one partial row per
 * row block of the kernel's epilogue (32 ... 256 rows) into `workspace` (morec_gemm_colsum_workspace_bytes(M, N) bytes, fp32: sized for the
 * smallest block, 32 rows, over whole tiles of up to 256 rows), folded by a second small launch.
 * colsum_out == NULL: plain morec_gemm_nt.  MOREC_E_UNSUPPORTED unless dact != NONE, accumulate == 0, split_k <= 1 and
 * the output rows are 16-byte addressable. */
size_t morec_gemm_colsum_workspace_bytes(int M, int N);
int morec_gemm_nt_colsum(const morec_gemm_desc* d, const void* A, const void* B, void* C, const float* bias,
                         void* aux_out, const void* dact_in, float* colsum_out, float* workspace, void* stream);

/* Which kernel morec_gemm_nt(_colsum) would run for this descriptor, asked of the same function the launch uses (csrc/gemm_plan.hpp)
 * with the knobs as they stand.  has_*: whether bias / aux_out / dact_in / colsum_out would be passed; operands are assumed 16-byte
 * aligned, pitches are those of d.  n_cu: CUs of gemm8p's persistent grid (it enters its tile height); <= 0 asks the current device,
 * > 0 touches no device, so the call works on a machine without a GPU.  Returns what the launch would return before launching
 * (MOREC_OK, or the MOREC_E_* of a refused descriptor, with family MOREC_GEMM_UNSUPPORTED).
 * No reference counterpart (the reference has no kernels to select). */
#define MOREC_GEMM_UNSUPPORTED 0
#define MOREC_GEMM_SKINNY 1      /* gemm_skinny.hip: tile = 32 rows x (32 nbh) columns, nbh = 3 | 4 | 9 */
#define MOREC_GEMM_SKINNY_WIDE 2 /* gemm_skinny_wide.hip: tile = 32 whole rows */
#define MOREC_GEMM_TWO_W 3       /* gemm2w.hip: 256 x 128 */
#define MOREC_GEMM_EIGHT_P 4     /* gemm8p.hip: 256 | 224 | 192 rows x 256 */
#define MOREC_GEMM_SMALL 5       /* gemm_small.hip: 64 x 64 */
#define MOREC_GEMM_GENERIC 6     /* two-buffer kernels: 128 x 128, 256 x 256 (256 x 128 only under MOREC_GEMM_TILE) */
typedef struct {
    int family;        /* MOREC_GEMM_* */
    int mode;          /* epilogue: 0 plain (+ bias), 1 GELU, 2 ReLU, 3 x GELU'(dact_in), 4 x ReLU'(dact_in), 5 x dact_in */
    int tile_rows, tile_cols;
    int ngroup;        /* eight_p, two_w: N-tiles per column group of the tile order, 0 = row-major */
    int colsum_fused;  /* the column sums ride on the epilogue */
    const char* family_name; /* "skinny", "skinny_wide", "two_w", "eight_p", "small", "generic", "unsupported" (static storage) */
} morec_gemm_plan_info;
int morec_gemm_plan(const morec_gemm_desc* d, int has_bias, int has_aux, int has_dact_in, int has_colsum, int n_cu,
                    morec_gemm_plan_info* out);

/* Backward of  g = act(X . W1^T + b1) -> fc2  WITHOUT a stored act'(pre) tensor (GELU only):
 *   dU[M, N] = (dY[M, K] . W2t[N, K]^T) * act'(X[M, K] . W1[N, K]^T + b1[N]),   colsum_out[n] += sum_m dU[m, n]  (= d b1)
 * The pre-activation is recomputed from X (K = C wide) instead of being read back 4 C wide; the matching forward is morec_gemm_nt
 * with act = MOREC_ACT_GELU and aux_out == NULL.  All operands contiguous (pitches K, K, K, K, N), 16-bit (bf16 / f16), 16-byte aligned.
 * Written for the Swin stage-1 / stage-2 MLP (HF modeling_swin.py SwinIntermediate / SwinOutput: 288 < N <= 768, K <= 192 --
 * N <= 384 for K <= 96, N <= 512 for K <= 128 --, M >= 8192);
 * morec_mlp_dact_recompute_supported() says for which of those shapes dropping act' pays (K <= 128: the caller then skips the aux
 * output of the forward GEMM); the call itself also takes the K <= 192 class; anything else returns MOREC_E_UNSUPPORTED.  workspace: morec_mlp_dact_recompute_workspace_bytes(N) bytes of fp32 (per-workgroup
 * column sums, folded in a fixed order), needed when colsum_out != NULL.  autograd reference: torch.nn.functional.gelu backward +
 * nn.Linear backward (db = dY.sum(0)). */
int morec_mlp_dact_recompute_supported(int M, int N, int K, int dtype);
size_t morec_mlp_dact_recompute_workspace_bytes(int N);
int morec_mlp_dact_recompute(const void* dY, const void* W2t, const void* X, const void* W1, const float* b1, void* dU,
                             float* colsum_out, float* workspace, int M, int N, int K, int dtype, void* stream);

/* Weight-gradient GEMM without transposed copies (16-bit operands only; MOREC_E_UNSUPPORTED otherwise):
 * C[N, K] (+)= sum_m DY[m, n] * X[m, k], fp32 C.  split_m > 1 cuts the token range over blockIdx.z; without a workspace that
 * requires accumulate != 0 (fp32 atomicAdd into a caller-zeroed C), with one the partial tiles are folded by a second kernel and
 * accumulate == 0 overwrites C.  Autograd backward of nn.Linear: dW = dY^T X.
 * SINGLE WRITER: with accumulate != 0 the update of C is a plain read-modify-write (the slab fold; with one token chunk the GEMM's own
 * 16-byte lanes), not an atomic.  Every kernel that adds into the same C must therefore be ordered with this call -- the same stream, or
 * an event between the streams.  (The engines issue all weight-gradient GEMMs of a step on ONE stream, engine.WgradStream; a tied weight
 * accumulated from two streams at once would lose updates.) */
int morec_gemm_tn(const void* DY, const void* X, float* C, int M, int N, int K, int ldy, int ldx, int ldc, int dtype,
                  int split_m, int accumulate, float* workspace, void* stream);
/* workspace (optional, fp32): morec_gemm_tn_workspace_bytes(N, K, split_m).  With it the split-m partial tiles are written
 * as plain slabs and summed by a second kernel (deterministic, ~4x cheaper than the atomics); without it fp32 atomicAdd. */
size_t morec_gemm_tn_workspace_bytes(int N, int K, int split_m);
/* What morec_gemm_tn would launch for these arguments, asked of the same function the launch uses (csrc/gemm_tn_plan.hpp) with the knobs
 * as they stand ("gemm8p", MOREC_TN8P_SKIP).  has_workspace: whether a workspace would be passed; pointers are assumed 16-byte aligned
 * (the launch checks its own).  Touches no device.  Returns what the launch would return before launching: MOREC_OK, or the MOREC_E_* of a
 * refused call with kernel MOREC_TN_UNSUPPORTED.
 *   mchunk = ceil(M / max(split_m, 1)) rounded up to 64 tokens; zs = ceil(M / mchunk) chunks are launched (<= split_m);
 *   path: store (one chunk, overwrite) | rmw (one chunk, accumulate) | atomic (several chunks, no workspace) | slabs (several chunks,
 *   workspace: fold != 0, a second kernel sums the slabs into C);
 *   kernel: the eight-phase kernel takes the store and slabs paths when every chunk, the last too, has at least 128 tokens -- and,
 *   unless "gemm8p" = 2, mchunk >= 512; "gemm8p" = 1: never.  eight_p_skip: N % 256 or K % 256 in 8 ... 224 (blocks of some tile lie
 *   outside the matrix and cost no MFMA).
 * No reference counterpart (the reference has no kernels to select). */
#define MOREC_TN_UNSUPPORTED 0
#define MOREC_TN_TWO_BUFFER 1
#define MOREC_TN_EIGHT_P 2
#define MOREC_TN_EIGHT_P_SKIP 3
#define MOREC_TN_PATH_NONE 0
#define MOREC_TN_PATH_STORE 1
#define MOREC_TN_PATH_RMW 2
#define MOREC_TN_PATH_ATOMIC 3
#define MOREC_TN_PATH_SLABS 4
typedef struct {
    int kernel;        /* MOREC_TN_* */
    int mchunk, zs;
    int path;          /* MOREC_TN_PATH_* */
    int fold;          /* the slab fold follows the GEMM */
    const char* kernel_name; /* "two_buffer", "eight_p", "eight_p_skip", "unsupported" (static storage) */
    const char* path_name;   /* "store", "rmw", "atomic", "slabs", "none" */
} morec_gemm_tn_plan_info;
int morec_gemm_tn_plan(int M, int N, int K, int ldy, int ldx, int ldc, int dtype, int split_m, int accumulate, int has_workspace,
                       morec_gemm_tn_plan_info* out);

/* out[c, r] = in[r, c]; in is [R, C] with pitch ld_in, out is [C, R] with pitch ld_out.
 * in_dtype/out_dtype select a fused conversion (f32 -> bf16 weight shadows). */
int morec_transpose(const void* in, void* out, int R, int C, int ld_in, int ld_out, int in_dtype, int out_dtype,
                    void* stream);

/* Many transposes in ONE launch -- the W^T copies of every Linear weight that dX = dY . W needs once per optimisation step
 * (T/run.py:246: the weights change once per step; HF Linear backward reads W itself through cuBLAS' transposed operand).
 * items: DEVICE array of n_items entries sorted by tile0; entry i owns the 64 x 64 tiles [tile0_i, tile0_{i+1}) of the launch's
 * n_tiles blocks, tiles of one matrix row-major over ceil(rows / 64) x ceil(cols / 64).  dst[c][r] = src[r][c]; every matrix:
 * cols % 4 == 0, ld_src % 4 == 0, ld_dst % 4 == 0, ld_dst >= rows rounded up to 4, 16-byte aligned bases (same rules as the
 * vectorised path of morec_transpose; the CALLER checks them -- the table is not readable from the host side of this call). */
typedef struct {
    const void* src;
    void* dst;
    int rows, cols;       /* of src */
    int ld_src, ld_dst;   /* elements */
    int tile0;            /* first block of this matrix */
    int reserved;
} morec_transpose_item;
int morec_transpose_batch(const morec_transpose_item* items, int n_items, int n_tiles, int dtype, void* stream);
/* elementwise convert n elements */
int morec_cast(const void* in, void* out, size_t n, int in_dtype, int out_dtype, void* stream);
/* fp32 rows -> bf16 rows of three column blocks for an fp32-accurate product on the bf16 matrix cores ("bf16x3"):
 * out[r, 0:C] = hi = bf16(in[r, :]); block lo_slot (1 or 2) = lo = bf16(in - hi); the remaining block = hi again.  With
 * A3 = split(A, lo_slot 2) = [hi | hi | lo] and B3 = split(B, lo_slot 1) = [hi | lo | hi], morec_gemm_nt(A3, B3) over K' = 3 C is
 * A.B^T up to the lo.lo term (2^-16 relative), accumulated in fp32 -- the numerics of torch's fp32 nn.Linear (T/model/modules.py:14)
 * to ~1e-5 at three bf16 MFMA passes instead of the 1/16-rate exact-fp32 MFMA.  C % 4 == 0, ld_in >= C, ld_out >= 3 C. */
int morec_split_bf16x3(const float* in, void* out, int R, int C, int ld_in, int ld_out, int lo_slot, void* stream);
/* out = dy * act'(pre), elementwise (act = MOREC_ACT_GELU | MOREC_ACT_RELU); T/model/encoders.py:70 backward */
int morec_act_bwd(const void* dy, const void* pre, void* out, size_t n, int act, int dtype, void* stream);
/* out = scale * (x0 + x1 + x2), elementwise, fp32 arithmetic, one rounding to `dtype` (x1, x2 may be NULL; x2 needs x1): the mean over the text
 * attributes of a news item -- T/model/encoders.py:107-116, torch.mean(torch.stack(text_vectors, dim=1), dim=1) -- and, with one input and
 * scale = 1 / k, the gradient each attribute's encoder pass receives.  n % 4 == 0. */
int morec_scaled_sum(const void* x0, const void* x1, const void* x2, void* out, size_t n, float scale, int dtype, void* stream);
/* out[n] = sum_m in[m, n]  (bias gradients), atomically accumulated into fp32 out */
int morec_colsum(const void* in, float* out, int M, int N, int ld, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm with fused pre-add:  z = drop_in(x (+ bias[n])) (+ res[m,n]) (+ pos[m % pos_period, n]);
 * y = drop_out((z - mean) * rstd * gamma + beta).   (T/model/modules.py:14-17,61-63,93-94; HF BertSelfOutput /
 * BertOutput / BertEmbeddings).  z_out may be NULL (not needed) or alias x.
 * Dropout is counter-based: element e = m*N + n is kept iff the (e & 1)-th 16-bit half of hash(seed, e >> 1) >= floor(p * 2^16),
 * kept values scaled by 1 / (1 - floor(p * 2^16) / 2^16); p = 0 disables.  morec_dropout_keep_mask exports the same stream.
 * drop_in  = the Dropout the reference applies to the sub-layer output before the residual add;
 * drop_out = the Dropout applied to the LayerNorm output of the embedding stages.
 * rowscale (may be NULL): per-sample DropPath scale of the sub-layer branch (HF SwinDropPath, modeling_swin.py:42-60):
 * (x + bias) is multiplied by rowscale[m / rows_per_scale] before the residual add.
 * ------------------------------------------------------------------------------------------ */
int morec_layernorm_fwd(const void* x, const float* bias, const void* res, const float* pos, int pos_period,
                        const float* gamma, const float* beta, float eps, void* z_out, void* y, float* mean,
                        float* rstd, int M, int N, int dtype, float p_in, uint64_t seed_in, float p_out,
                        uint64_t seed_out, const float* rowscale, int rows_per_scale, void* stream);
/* dz = LN'(drop_out'(dy_a + dy_b); z) (+ dres); dzd = rowscale * drop_in'(dz) (required iff p_in > 0 or rowscale, else
 * NULL).  dres (may be NULL) is the gradient that reaches z directly along the residual stream of a pre-LN block
 * (HF SwinLayer, modeling_swin.py:536,560-566).  dgamma/dbeta (and, if given, dbias = column sums of dzd: the gradient of
 * the fused pre-add bias) are atomically accumulated (fp32, [N]).  dy_b, dgamma/dbeta and dbias may be NULL. */
int morec_layernorm_bwd(const void* dy_a, const void* dy_b, const void* z, const float* mean, const float* rstd,
                        const float* gamma, void* dz, void* dzd, float* dgamma, float* dbeta, float* dbias, int M, int N,
                        int dtype, float p_in, uint64_t seed_in, float p_out, uint64_t seed_out, const void* dres,
                        const float* rowscale, int rows_per_scale, void* stream);

/* LayerNorm of the reference's AUTOCAST data flow -- the `*_res32` compute modes.  Under `torch.cuda.amp.autocast()` (T/run.py:242) nn.Linear
 * takes and returns 16-bit tensors while LayerNorm runs and RETURNS fp32 (HF modeling_bert.py BertSelfOutput / BertOutput: LayerNorm(dropout(
 * dense(h)) + input_tensor); T/model/modules.py:14-17,61-63,93-94): the residual stream is fp32, only GEMM operands are rounded.
 *   forward:  z32 = drop_in(x16 (+ bias)) (+ res32) (+ pos[m % pos_period]);  y32 = drop_out(LN(z32) * gamma + beta);  y16 = round(y32).
 *             x16: 16-bit output of the sub-layer's GEMM (dtype16 = MOREC_BF16 | MOREC_F16); z32 (saved for the backward), y32 (the residual
 *             stream: the next LayerNorm's res32) and y16 (the next GEMM's operand) may each be NULL, not all of y32 / y16.
 *   backward: dz32 = LN'(drop_out'(dy16 + dy32); z32)  (dy16: gradient through the GEMM that read y16; dy32: gradient along the residual
 *             stream; either may be NULL);  dzd16 = round(drop_in'(dz32)): the 16-bit gradient of the sub-layer output, what its weight- /
 *             input-gradient GEMMs read.  dgamma / dbeta / dbias (= column sums of dzd16 as stored) are accumulated into, as in
 *             morec_layernorm_bwd.  dz32 or dzd16 may be NULL.
 * N % 8 == 0, N <= 4096, all tensors contiguous and 16-byte aligned.  Dropout streams: as morec_layernorm_fwd. */
int morec_layernorm_fwd_res32(const void* x16, const float* bias, const float* res32, const float* pos, int pos_period, const float* gamma,
                              const float* beta, float eps, float* z32, float* y32, void* y16, float* mean, float* rstd, int M, int N,
                              int dtype16, float p_in, uint64_t seed_in, float p_out, uint64_t seed_out, void* stream);
/* The same forward with the residual stream handed over in PRE-LayerNorm form: res_z32 is the z32 the PREVIOUS LayerNorm saved, and the stream
 * value is (res_z32 - res_mean[m]) * res_rstd[m] * res_gamma + res_beta, recomputed in registers -- the previous call then passes y32 = NULL and
 * never writes the stream (12 instead of 16 bytes per element and call; same numbers as reading y32 back up to fp32 contraction).  No pos, no
 * output dropout (the LayerNorms inside an encoder layer have neither: HF BertSelfOutput / BertOutput, T/model/modules.py:17,63). */
int morec_layernorm_fwd_res32_pre(const void* x16, const float* bias, const float* res_z32, const float* res_mean, const float* res_rstd,
                                  const float* res_gamma, const float* res_beta, const float* gamma, const float* beta, float eps, float* z32,
                                  void* y16, float* mean, float* rstd, int M, int N, int dtype16, float p_in, uint64_t seed_in, void* stream);
int morec_layernorm_bwd_res32(const void* dy16, const float* dy32, const float* z32, const float* mean, const float* rstd, const float* gamma,
                              float* dz32, void* dzd16, float* dgamma, float* dbeta, float* dbias, int M, int N, int dtype16, float p_in,
                              uint64_t seed_in, float p_out, uint64_t seed_out, void* stream);
/* dpos[m % period, n] += dz[m, n]  (position-embedding gradient, fp32 atomics) */
int morec_pos_grad(const void* dz, float* dpos, int M, int N, int period, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Small-tile multi-head attention on packed projections qkv[M, 3*H] = [Q | K | V], M = n_seq*T,
 * H = n_heads*dh, T <= 1024 (beyond: MOREC_E_UNSUPPORTED).  16-bit storage, head width % 32 == 0: the matrix-core kernels for T <= 32 and for 32 < T <= 64 (abstracts /
 * bodies of 50 tokens, T/parameters.py:43-44); fp32 storage, T <= 32, head width % 16 == 0: exact-fp32 MFMA (attention_f32mfma.hip: the
 * parity and fp32x3 modes); other head widths and fp32 up to T = 64: the exact-fp32 VALU tile kernels; 64 < T <= 256 (longer than any
 * launcher of the reference sets, accepted by its command line): the row-strip VALU kernels, every dtype; 256 < T <= 1024 (BERT's 512 positions, long behaviour
 * sequences): the streaming kernels of attention_stream.hip, which walk the keys in tiles of 64 / 32 with a running softmax and never hold
 * a full score row -- stream16 (16-bit storage, head width % 32 == 0 and <= 256: 4 wavefronts per (sequence, head), all five products on
 * the matrix cores) and streamgen (every other shape: fp32 arithmetic, one wavefront per (sequence, head)); the "attn_stream" knob moves
 * their lower edge to 64 or takes them away; T > 1024: MOREC_E_UNSUPPORTED.
 * scores = (q.k) * scale + (key masked ? mask_value : 0), causal option,
 * softmax, ctx = P.V.   SASRec: T/model/encoders.py:24-27 + T/model/modules.py:27-31 (causal,
 * mask_value -1e9, scale 1/sqrt(d_k)).  BERT: HF BertSelfAttention eager (mask_value finfo.min).
 * key_keep: float [n_seq, T], nonzero = attend.  One wavefront per (sequence, head).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int n_seq, T, n_heads, dh;
    int causal;
    float scale, mask_value;
    int dtype;
    float p_drop;      /* dropout on the attention probabilities (0 = off) */
    uint64_t seed;     /* element index = ((seq * n_heads + head) * TP + i) * TP + j, TP = 32 for T <= 32, 64 for T <= 64, 32 * ceil(T / 32) above */
    const int32_t* cu_seqlens;   /* NULL: every sequence owns T rows.  Otherwise int32[n_seq + 1] (device): sequence s owns rows
                                    cu_seqlens[s] .. cu_seqlens[s+1]-1 (<= T of them) -- the unpadded ("varlen") token layout in
                                    which [PAD] positions are not materialised at all; key_keep is then indexed by packed row */
    int total_rows;              /* with cu_seqlens: rows of qkv / ctx / dqkv (>= cu_seqlens[n_seq]), or 0.  The packed buffers may carry SPARE
                                    rows behind the last sequence (a token count padded up to a bucket size, so that one captured graph
                                    serves every batch of the bucket); */
    int spare_rows_max;          /* ... upper bound of their number: the launch appends ceil(spare_rows_max / 16) blocks that write zeros into
                                    the rows cu_seqlens[n_seq] .. total_rows-1 of ctx (forward) / dqkv (backward).  0 = no spare rows. */
} morec_attn_desc;

int morec_attn_fwd(const morec_attn_desc* d, const void* qkv, const float* key_keep, void* ctx, void* stream);
int morec_attn_bwd(const morec_attn_desc* d, const void* qkv, const float* key_keep, const void* dctx, void* dqkv,
                   void* stream);
/* The same backward plus the bias gradient of the fused q|k|v projection (HF BertSelfAttention query/key/value biases;
 * T/model/modules.py:30-32 has none): dbias[3 H] (fp32) += column sums of the `rows` dqkv rows (the bf16 MFMA path sums them in fp32
 * before the rows are rounded to bf16; otherwise the stored rows are summed).  ws: optional
 * scratch of n_seq * 3 H floats -- with it the bf16 path sums inside the attention kernel instead of re-reading dqkv. */
int morec_attn_bwd_dbias(const morec_attn_desc* d, const void* qkv, const float* key_keep, const void* dctx, void* dqkv,
                         int rows, float* dbias, float* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Swin vision tower (V/model/encoders.py:24-31 -> HF SwinForImageClassification, built at V/run.py:47-54;
 * transformers/models/swin/modeling_swin.py).  Token rows are kept in natural (image, y, x) order throughout:
 * window partition (:486-495), cyclic shift (:609-618) and window reverse (:498-505) are index arithmetic
 * inside the attention kernel, never copies.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int n_img, H, W;   /* token grid per image */
    int window;        /* 7 (49 tokens); H, W multiples of it */
    int shift;         /* 0 | window/2 (SW-MSA blocks): adds the -100 region mask of :584-607 */
    int heads, dh;     /* dh = 32 */
    float scale;       /* dh^-0.5 */
    int dtype;
} morec_swin_attn_desc;
/* ctx[row, h*dh..] = softmax(q.k*scale + bias_t[h][j][i] + shift mask) v over the row's window (SwinAttention :401-468).
 * qkv [rows, 3*heads*dh] = [q | k | v]; bias_t fp32 [heads][window^2 (key j)][window^2 (query i)]. */
int morec_swin_attn_fwd(const morec_swin_attn_desc* d, const void* qkv, const float* bias_t, void* ctx, void* stream);
/* dqkv from dctx (P recomputed; ctx = saved forward output); dbias_t (may be NULL) += dS summed over windows. */
int morec_swin_attn_bwd(const morec_swin_attn_desc* d, const void* qkv, const float* bias_t, const void* ctx,
                        const void* dctx, void* dqkv, float* dbias_t, void* stream);
/* The same backward plus the bias gradient of the fused q|k|v projection (modeling_swin.py:407-409): dbqkv[3 heads dh] (fp32) +=
 * column sums of dqkv.  ws: optional scratch (n_windows x 3 heads dh floats is always enough) -- with it the bf16 path sums
 * inside the attention kernel (fp32 sums of the rows BEFORE their bf16 rounding) instead of re-reading dqkv. */
int morec_swin_attn_bwd_dbias(const morec_swin_attn_desc* d, const void* qkv, const float* bias_t, const void* ctx,
                              const void* dctx, void* dqkv, float* dbias_t, float* dbqkv, float* ws, size_t ws_bytes, void* stream);
/* bias_t[h][j][i] = table[rel_index(i, j)][h] (SwinRelativePositionBias :329-370) and its transpose-scatter gradient */
int morec_swin_bias_expand(const float* table, float* bias_t, int window, int heads, void* stream);
int morec_swin_bias_reduce(const float* dbias_t, float* dtable, int window, int heads, void* stream);
/* im2col of the patch-embedding conv (SwinPatchEmbeddings :247-286): out[(n,py,px), (c,i,j)] = pixels[n,c,py*p+i,px*p+j];
 * pixels fp32 NCHW (what V/run.py:201-204 puts on the device), out dtype rows of pitch ld_out. */
int morec_swin_patchify(const float* pixels, void* out, int n_img, int channels, int R, int patch, int ld_out, int dtype,
                        void* stream);
/* the same rows from decoded uint8 HWC images [n, R, R, channels]: ToTensor + Normalize(mean, std) of
 * V/data_utils/dataset.py:69-73 applied in flight (fp32, reference operation order: (x / 255 - mean) / std).  The uint8 fronts --
 * this one, morec_mae_patchify_keep_u8 and the uint8 case of morec_pixels_to_nhwc -- live in csrc/image_front.hip, one kernel per
 * layout shared with their _idx forms (below: "The image catalogue on the device"). */
int morec_swin_patchify_u8(const uint8_t* pixels_hwc, void* out, int n_img, int channels, int R, int patch, int ld_out,
                           float mean, float std, int dtype, void* stream);
/* SwinPatchMerging gather (:309-320): [n,H,W,C] -> [n,H/2,W/2,4C]; reverse != 0 is the inverse copy (backward). */
int morec_swin_merge(const void* in, void* out, int n_img, int H, int W, int C, int reverse, int dtype, void* stream);
/* mean over each image's tokens (AdaptiveAvgPool1d(1), :876-879) and its backward */
int morec_swin_pool_fwd(const void* x, void* out, int n_img, int tokens, int C, int dtype, void* stream);
int morec_swin_pool_bwd(const void* dout, void* dx, int n_img, int tokens, int C, int dtype, void* stream);
/* out = res + rowscale[m / rows_per_scale] * (a + bias)  (bias, rowscale may be NULL) */
int morec_bias_residual(const void* a, const float* bias, const void* res, const float* rowscale, int rows_per_scale,
                        void* out, int M, int N, int dtype, void* stream);
/* DropPath per-sample scales: out[i] = hash(seed, i) kept ? 1/(1-p) : 0  (SwinDropPath :51-57) */
int morec_droppath_scale(float* out, int n, float p, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------------
 * The front of the MAE (ViT) item tower (csrc/mae.hip): HF ViTMAEEmbeddings (modeling_vit_mae.py:182-327) for the KEPT patches only.
 * fp32, bf16 and fp16 storage; 16-byte accesses; no atomics, every output element written once, the same bits on every run.
 *
 * keep[n_img, len_keep] (int32) = the patch indices of each image in ascending order of noise, ties to the lower index --
 * torch.argsort(noise)[:, :len_keep] of random_masking (:297-327) for distinct values.  noise: fp32 [n_img, N] (HF's noise= argument),
 * or NULL: the key of (image, patch) is the counter-based generator of the dropout masks at counter image * N + patch under `seed`
 * (32 uniform bits).  len_keep = int(N * (1 - mask_ratio)) is the caller's (host double arithmetic, as HF); len_keep == N returns the
 * whole shuffled order.  One workgroup per image, the keys in LDS: N <= 1024 (beyond: MOREC_E_UNSUPPORTED). */
int morec_mae_keep_ids(const float* noise, uint64_t seed, int32_t* keep, int n_img, int N, int len_keep, void* stream);
/* morec_swin_patchify / morec_swin_patchify_u8 for the kept patches only: out[i * len_keep + j] = the im2col row of patch keep[i, j] of
 * image i, bit-equal to the full im2col followed by a row gather.  patch % 4 != 0, ld_out not a multiple of a 16-byte lane or a base
 * pointer off 16 bytes: MOREC_E_ALIGN.  A keep entry outside [0, (R / patch)^2) leaves a zero row. */
int morec_mae_patchify_keep(const float* pixels, const int32_t* keep, void* out, int n_img, int channels, int R, int patch, int len_keep,
                            int ld_out, int dtype, void* stream);
int morec_mae_patchify_keep_u8(const uint8_t* pixels_hwc, const int32_t* keep, void* out, int n_img, int channels, int R, int patch,
                               int len_keep, int ld_out, float mean, float std, int dtype, void* stream);
/* x[n_img, 1 + len_keep, C]: x[i, 0] = cls_token + pos[0], x[i, 1 + j] = e[i * len_keep + j] + pos[1 + keep[i, j]] (:259-267; e = the
 * patch GEMM's output, bias included; cls_token fp32 [C], pos fp32 [N + 1, C]): one fp32 add, one rounding to the storage type.
 * Backward: de = the patch rows of dx, d_cls[c] = sum_i dx[i, 0, c] (fp32, fixed order, WRITTEN not accumulated); the position table is
 * frozen (requires_grad=False in HF) and has no gradient.  C % 8 != 0 (every dtype) or a base pointer off 16 bytes: MOREC_E_ALIGN. */
int morec_mae_assemble_fwd(const void* e, const float* cls_token, const float* pos, const int32_t* keep, void* x, int n_img, int len_keep,
                           int N, int C, int dtype, void* stream);
int morec_mae_assemble_bwd(const void* dx, void* de, float* d_cls, int n_img, int len_keep, int C, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * The BEiT item tower (HF modeling_beit.py): attention with a per-head additive position bias (csrc/attention_stream.hip, the BIAS
 * instantiations of the streaming kernels) and the tower's small kernels (csrc/beit.hip).
 *
 * morec_attn_bias_fwd / _bwd: morec_attn_fwd / _bwd with
 *     score = (q.k) * scale + (kept ? 0 : mask_value) + pos_bias[h][i][j]
 * the mask added in the literal rounding order of the plain kernels, the bias after it in fp32.  The streaming kernels run for EVERY
 * T <= 1024 (MOREC_ATTN_STREAM is not consulted): stream16 (matrix cores) for bf16 / fp16 with dh % 32 == 0 and dh <= 256, streamgen (fp32
 * arithmetic) otherwise.  The descriptor is the plain one; causal != 0, p_drop > 0, cu_seqlens != NULL and T > 1024 return
 * MOREC_E_UNSUPPORTED (no caller uses them), and the descriptor is judged before any pointer.
 *
 * pos_bias LAYOUT: fp32 [heads][T][Tp], Tp = 64 * ceil(T / 64): row i of head h holds the bias of query i against the keys 0 .. T-1,
 * padded with zeros to the key-tile width; the same for every sequence; 16-byte aligned.  morec_beit_bias_expand produces it.  The
 * cells j >= T are read (in bounds by the layout) but only ever meet a score that is already -inf.
 *
 * Backward: dqkv as morec_attn_bwd.  dqkv_bias (fp32 [3 H], may be NULL) += the column sums of dqkv, as morec_attn_bwd_dbias forms them
 * off the matrix-core path.  d_pos_bias (fp32, pos_bias's layout, may be NULL = frozen table: nothing more is launched) is WRITTEN,
 * pad cells as zero: d_pos_bias[h][i][j] = sum over the sequences of dS[n, h, i, j], dS = P o (dP - delta) -- the gradient at the score,
 * `scale` not applied.  It needs ws of morec_attn_bias_ws_bytes(desc) bytes (16-byte aligned; too small or NULL: MOREC_E_ARG): the row
 * statistics of the main backward ([n_seq][heads][3][T]) and 8 partial tables.  The sequences are cut into 8 chunks of
 * ceil(n_seq / 8); a workgroup sums one (head, query block, key block) tile over the sequences of its chunk in index order, in fp32
 * registers, and the chunks are added in chunk order: no atomics, one fixed order, two calls on the same inputs give the same bits.
 * morec_attn_bias_ws_bytes returns 0 for a descriptor the entry points refuse. */
size_t morec_attn_bias_ws_bytes(const morec_attn_desc* desc);
int morec_attn_bias_fwd(const morec_attn_desc* desc, const void* qkv, const float* key_keep, const float* pos_bias, void* ctx, void* stream);
int morec_attn_bias_bwd(const morec_attn_desc* desc, const void* qkv, const float* key_keep, const float* pos_bias, const void* dctx,
                        void* dqkv, float* dqkv_bias, float* d_pos_bias, float* ws, size_t ws_bytes, void* stream);
/* table fp32 [(2g-1)^2 + 3, heads] (relative_position_bias_table; g = patches per side, T = g^2 + 1 <= 1024) -> pos_bias in the layout
 * above, with BeitRelativePositionBias.generate_relative_position_index: patch pairs by their 2-D offset, then the three entries
 * cls -> token, token -> cls, cls -> cls.  Reduce: dtable += the sum of the d_pos_bias cells behind each entry; ONE thread owns an entry
 * and adds its cells in a fixed order. */
int morec_beit_bias_expand(const float* table, float* pos_bias, int g, int heads, void* stream);
int morec_beit_bias_reduce(const float* d_pos_bias, float* dtable, int g, int heads, void* stream);
/* Layer scale fused with the residual add: h[r, c] = res[r, c] + rowscale[r / rows_per_scale] * (lam[c] * (a[r, c] + bias[c])), formed
 * in fp32 in exactly this order (HF: lambda * output, DropPath, residual) without contraction and rounded once.  rowscale may be NULL;
 * with it M % rows_per_scale != 0 is MOREC_E_ARG.  N % 8 != 0 or a base pointer off 16 bytes: MOREC_E_ALIGN.
 * Backward from dh: da = dh * rowscale * lam (storage type); dlam[c] += sum_r dh * rowscale * (a + bias); dbias[c] += lam[c] * sum_r
 * dh * rowscale.  dlam / dbias may be NULL (frozen: only da is formed; a / bias may then be NULL too).  The column sums run per slab of
 * 1024 rows in a fixed order and the slabs are added in slab order: no atomics.  Every output is written once. */
int morec_layerscale_res_fwd(const void* a, const float* bias, const float* lam, const void* res, const float* rowscale, int rows_per_scale,
                             void* h, long M, int N, int dtype, void* stream);
int morec_layerscale_res_bwd(const void* dh, const void* a, const float* bias, const float* lam, const float* rowscale, int rows_per_scale,
                             void* da, float* dlam, float* dbias, long M, int N, int dtype, void* stream);
/* The mean-pool head: out[n_img, C] = the mean over rows 1 .. T-1 of every image of x[n_img, T, C] ([CLS], row 0, is not part of it);
 * backward: dx rows 1 .. T-1 = dpool / (T - 1), row 0 = 0. */
int morec_beit_pool_fwd(const void* x, void* out, int n_img, int T, int C, int dtype, void* stream);
int morec_beit_pool_bwd(const void* dpool, void* dx, int n_img, int T, int C, int dtype, void* stream);
/* x[n_img, 1 + N, C]: x[i, 0] = cls_token (fp32 [C], rounded to the storage type), x[i, 1 + j] = e[i * N + j] (row copy; BEiT has no
 * absolute positions).  The backward is morec_mae_assemble_bwd: the row copy and d_cls = the sum over images of row 0 in index order. */
int morec_beit_assemble_fwd(const void* e, const float* cls_token, void* x, int n_img, int N, int C, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * The ResNet item tower (resnet_engine.py; csrc/conv.hip, csrc/resnet.hip).  Activations are NHWC, viewed as [N H W, C] rows of the storage
 * type (any of the three).  No atomics anywhere below: every output element has one writer and every call repeats its bits.
 *
 * Convolution as an implicit GEMM.  KH == KW in {1, 3, 7}, stride 1 or 2, 0 <= pad < KH (anything else: MOREC_E_UNSUPPORTED);
 * Ho = (H + 2 pad - KH) / stride + 1.  fwd: out[(n, ho, wo), co] = sum_{kh, kw, c} x[n, ho s - p + kh, wo s - p + kw, c] w[co, kh, kw, c]
 * (zero outside the image), w as [Cout, KH, KW, Cin], Cout % 8 == 0.  bwd_data: dx[(n, h, w), c] = sum over the taps whose
 * (h + p - kh) / s and (w + p - kw) / s are exact and in range of dy[n, ., ., co] wt[c, kh, kw, co], wt as [Cin, KH, KW, Cout],
 * Cin % 8 == 0; H, W are the INPUT grid in both.  16-bit storage whose reduction channel count (Cin for fwd, Cout for bwd_data) is a
 * multiple of 32 runs on the 16x16x32 MFMAs (morec_conv2d_uses_mfma); everything else on an fp32-FMA kernel, in (kh, kw, c) order. */
int morec_conv2d_uses_mfma(int reduction_channels, int dtype);
int morec_conv2d_fwd(const void* x, const void* w, void* out, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                     int dtype, void* stream);
int morec_conv2d_bwd_data(const void* dy, const void* wt, void* dx, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                          int pad, int dtype, void* stream);
/* col[r - row0, (kh, kw, c)] for output rows row0 <= r < row1, row pitch ld >= KH KW Cin elements (a multiple of the 16-byte vector; the
 * columns past KH KW Cin are zeroed): the operand of the weight gradient, dW[co, (kh, kw, c)] += dy[rows]^T col. */
int morec_im2col_nhwc(const void* x, void* col, int N, int H, int W, int Cin, int KH, int KW, int stride, int pad, int row0, int row1, int ld,
                      int dtype, void* stream);
/* BatchNorm2d over [rows, C], C % 8 == 0.  stats: part fp32 [ceil(rows / morec_bn_slab_rows()), 3, C] = (count, mean, M2) of every slab
 * of rows, the slab mean first and then the squared deviations from it.  merge: the partials combined in slab order by Chan's formula
 * into merged [3, C] (optional), mean and rstd = 1 / sqrt(M2 / count + eps) (optional), and, when running_mean / running_var are given,
 * torch's update running = (1 - momentum) running + momentum batch with the unbiased variance.  rstd: 1 / sqrt(var + eps) of given
 * (running) variances.  apply_fwd: y = relu?(gamma (x - mean) rstd + beta (+ res)), fp32, one rounding.
 * bwd_reduce: sums fp32 [2, C] = sum dz, sum dz xhat with dz = dy [y > 0] when y (the saved output of a ReLU) is given, else dy; per-slab
 * partials in ws (morec_bn_bwd_workspace_bytes) added in slab order.  bwd_apply: dx = gamma rstd (dz - sums[0] / rows - xhat sums[1] /
 * rows), or gamma rstd dz with sums == NULL (running statistics); dz (optional) receives dz itself.
 * Synchronised over data-parallel ranks: bwd_fold adds n gathered [2, C] sums (parts [n, 2, C]) in index order into sums [2, C], no
 * atomics; bwd_apply_n is bwd_apply dividing by count[0] (count: fp32 [C] in device memory, the merged count row of all ranks' rows --
 * every channel counts the same rows; exact below 2^24 rows) instead of by its own rows, so the host never learns that count; with
 * count[0] == rows it writes bwd_apply's bits; sums is required.  The forward merge over ranks is
 * morec_bn_merge itself over the gathered [W, 3, C] partials. */
int morec_bn_slab_rows(void);
int morec_bn_stats(const void* x, float* part, int rows, int C, int dtype, void* stream);
int morec_bn_merge(const float* part, int nslabs, int C, float eps, float momentum, float* merged, float* mean, float* rstd,
                   float* running_mean, float* running_var, void* stream);
int morec_bn_rstd(const float* var, float* rstd, int C, float eps, void* stream);
int morec_bn_apply_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* res, void* y,
                       int rows, int C, int relu, int dtype, void* stream);
size_t morec_bn_bwd_workspace_bytes(int rows, int C);
int morec_bn_bwd_reduce(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, float* ws, float* sums, int rows,
                        int C, int dtype, void* stream);
int morec_bn_bwd_apply(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma,
                       const float* sums, void* dx, void* dz, int rows, int C, int dtype, void* stream);
int morec_bn_bwd_fold(const float* parts, int n, int C, float* sums, void* stream);
int morec_bn_bwd_apply_n(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma,
                         const float* sums, const float* count, void* dx, void* dz, int rows, int C, int dtype, void* stream);
/* MaxPool2d(3, stride 2, padding 1), C % 8 == 0: y [N Ho Wo, C] with Ho = (H - 1) / 2 + 1; idx uint8 [N Ho Wo, C] = the selected tap
 * kh * 3 + kw, the FIRST in scan order among equal values (torch's rule; ties are the normal case on post-ReLU input).  bwd: dx[N H W, C],
 * every pixel gathers dy from the windows that selected it. */
int morec_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int dtype, void* stream);
int morec_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C, int dtype, void* stream);
/* src fp32 [n, C, H, W] (src_u8 == 0; copied), or uint8 [n, H, W, C] (src_u8 != 0; (x / 255 - mean) / std as morec_swin_patchify_u8)
 * -> out [n H W, C] of the storage type (csrc/image_front.hip). */
int morec_pixels_to_nhwc(const void* src, void* out, int n, int C, int H, int W, int src_u8, float mean, float std, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * DeBERTa's disentangled self-attention (HF modeling_deberta.py DisentangledSelfAttention with pos_att_type c2p + p2c; csrc/deberta.hip),
 * T <= 64 (titles): morec_attn_fwd / _bwd with two position terms on every score,
 *     score[i][j] = (q_i . k_j + q_i . PK_h[d] + k_j . PQ_h[d]) * scale,   d = i - j + T  (1 .. 2T-1: row 0 of PK / PQ is never read),
 * `scale` = 1 / sqrt(3 dh) applied once to the fp32 sum.  A score whose query OR key is masked (key_keep[n][i] == 0 or key_keep[n][j] == 0)
 * is REPLACED by `mask_value` (a finite value: finfo.min), not added to -- a query row without a kept key is the uniform average of all T
 * value rows -- and takes no gradient.  Then softmax, dropout on P (p_drop > 0: element index ((seq * n_heads + head) * 64 + i) * 64 + j,
 * TP = 64 for every T), ctx = P V.  The descriptor is the plain one; causal != 0, cu_seqlens != NULL and T > 64 return
 * MOREC_E_UNSUPPORTED, and the descriptor is judged before any pointer (null: MOREC_E_ARG).
 *
 * LAYOUT: qkv [n_seq * T, 3 H] = [Q | K | V] with the projection biases already added; key_keep fp32 [n_seq, T]; PK = pos_proj(R) and
 * PQ = pos_q_proj(R) [2 T, H] in the storage type, unscaled, row d = relative position d - T, the head's columns at h * dh as in Q;
 * the same for every sequence.  ctx [n_seq * T, H].
 *
 * Two paths: mfma16 (bf16 / fp16 storage, dh % 32 == 0, dh <= 128: every product on v_mfma_f32_16x16x32_{bf16,f16}) and gen (fp32 storage
 * or other head widths: fp32 FMAs).  One workgroup per (sequence, head); Q PK^T and K PQ^T are formed once as [T x 2T] fp32 tiles in LDS.
 *
 * Backward: dqkv as morec_attn_bwd.  dqkv_bias (fp32 [3 H], may be NULL) += the column sums of dqkv.  dPK, dPQ (fp32 [2 T, H], both or
 * neither NULL = frozen position projections: nothing more is launched) are WRITTEN, row 0 as zero:
 *     dPK_h[d] = sum_seq sum_{i-j+T=d} dS[i][j] q_i * scale,   dPQ_h[d] = sum_seq sum_{i-j+T=d} dS[i][j] k_j * scale.
 * They need ws of morec_disent_attn_ws_bytes(desc) bytes (8 partial pairs; too small or NULL: MOREC_E_ARG): the sequences are cut into 8
 * chunks of ceil(n_seq / 8), a workgroup per (chunk, head) adds its sequences' contributions in index order in fp32, and the partials of
 * the chunks that hold a sequence are added in chunk order.  No atomics in these kernels, every output written once, two calls on the
 * same inputs give the same bits.  morec_disent_attn_ws_bytes returns 0 for a descriptor the entry points refuse. */
size_t morec_disent_attn_ws_bytes(const morec_attn_desc* desc);
int morec_disent_attn_fwd(const morec_attn_desc* desc, const void* qkv, const float* key_keep, const void* PK, const void* PQ, void* ctx,
                          void* stream);
int morec_disent_attn_bwd(const morec_attn_desc* desc, const void* qkv, const float* key_keep, const void* PK, const void* PQ,
                          const void* dctx, void* dqkv, float* dqkv_bias, float* dPK, float* dPQ, float* ws, size_t ws_bytes, void* stream);
/* DebertaEmbeddings' `embeddings * mask` (modeling_deberta.py), in place: row m of x [M, N] becomes exact zeros where keep[m] == 0 and is
 * left as it is elsewhere.  Its own backward (the mask applied to the gradient). */
int morec_rows_keep(void* x, const float* keep, long M, int N, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * BCE variant, one sampled negative per position (bce_text/main-end2end/model/model.py:30-51).
 * E [B, S+1, 2, D] item vectors (pos at [:, :, 0], neg at [:, :, 1]), P [B, S, D] user states, row_valid u8 [B*S].
 * scores fp32 [2][B*S] (pos | neg) are saved for the backward; loss_sum[0] += sum_valid softplus(-pos) + softplus(neg).
 * The sum is one fp32 atomic per valid row; in the deterministic mode a second one-block launch adds the rows' terms in a fixed order instead.
 * Backward: gscale[0] = dloss / n_valid on the device; writes dP [B, S, D] and EVERY row of dE [B, S+1, 2, D] (no atomics).
 * ------------------------------------------------------------------------------------------ */
int morec_bce_fwd(const void* P, const void* E, const uint8_t* row_valid, float* scores, float* loss_sum, int B, int S, int D,
                  int dtype, void* stream);
int morec_bce_bwd(const void* P, const void* E, const uint8_t* row_valid, const float* scores, const float* gscale, void* dP,
                  void* dE, int B, int S, int D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * DSSM two-tower scoring loss (bce_text/main-end2end(DSSM)/model/model.py): every user vector against its own 1 + neg_num sampled items.
 * n1 = 1 + neg_num, R = B * n1.  U [B, D] and E [R, D] in dtype (user b owns the rows b*n1 .. b*n1 + n1 - 1); labels fp32 [R], any
 * values in [0, 1], or NULL for [1, 0, ..., 0] per user.  fp32 outputs: scores[r] = U[r / n1] . E[r], terms[r] = softplus(s) - y s,
 * loss_sum[0] = sum_r terms[r] (overwritten, not accumulated; the caller divides by R for the BCEWithLogitsLoss mean).
 * Backward: gscale[0] = dloss / R on the device; c_r = g (sigmoid(s_r) - y_r), dE[r] = c_r U[r / n1], dU[b] = sum_j c_{b,j} E[b, j].
 * Few users with many rows each: the backward cuts a user's rows into segments, keeps their fp32 partial dU in library-owned scratch and
 * adds them in segment order in a second launch.
 * No atomics: every element of scores, terms, loss_sum, dU and dE is written exactly once and every sum has a fixed order -- the same
 * bits on every run, in either setting of the deterministic mode.  D % 4 != 0 or a row base off 16 bytes: MOREC_E_ALIGN; null pointers
 * (labels excepted), B, n1 or D < 1: MOREC_E_ARG; all before anything is launched.
 * ------------------------------------------------------------------------------------------ */
int morec_dssm_bce_fwd(const void* U, const void* E, const float* labels, float* scores, float* terms, float* loss_sum, int B, int n1,
                       int D, int dtype, void* stream);
int morec_dssm_bce_bwd(const void* U, const void* E, const float* labels, const float* scores, const float* gscale, void* dU, void* dE,
                       int B, int n1, int D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embeddings
 * ------------------------------------------------------------------------------------------ */
/* BERT embeddings: z = word[ids[m]] + pos[m % T] + type0;  y = LN(z)  (HF BertEmbeddings). */
int morec_bert_embed_fwd(const int32_t* ids, const float* word, const float* pos, const float* type0,
                         const float* gamma, const float* beta, float eps, void* z_out, void* y, float* mean,
                         float* rstd, int M, int T, int H, int dtype, float p_out, uint64_t seed_out, void* stream);
/* scatter dz into dword[ids[m]] (skipping pad_id: nn.Embedding padding_idx), dpos[m % T], dtype0.
 * order (may be NULL): int32[M] permutation of the rows in which EQUAL token ids are adjacent (argsort of ids); a run of equal
 * ids is summed in registers, and a run that lies inside one wavefront's 32 rows is added to its table row by a plain
 * read-modify-write (it is that row's only contribution), the others atomically.  An order that is not grouped by id is a
 * caller error (lost updates); without order every row is added atomically. */
int morec_bert_embed_bwd(const int32_t* ids, const void* dz, float* dword, float* dpos, float* dtype0, int pad_id,
                         int M, int T, int H, int dtype, const int32_t* order, void* stream);
/* RoBERTa embeddings: position ids counted from the pad token (HF create_position_ids_from_input_ids, computed from the ids, never
 * from the attention mask).  Per sequence n of T tokens: pos_ids[n*T + t] = pad_id if ids == pad_id, else pad_id + 1 + k for the
 * k-th (from 0) non-pad token; cnt[n] = number of non-pad tokens; perm[n*T + k] = position of the k-th non-pad token for
 * k < cnt[n], followed by the pad positions in order (a permutation of 0 .. T-1).  All int32 device arrays.  One wavefront per
 * sequence, no LDS, no atomics, no allocation, no host synchronisation.  Null pointers, n_seq or T <= 0, pad_id < 0, or
 * pad_id + T >= n_pos (the largest id written must be a row of the n_pos-row table): MOREC_E_ARG before anything is launched. */
int morec_roberta_pos_ids(const int32_t* ids, int pad_id, int n_seq, int T, int n_pos, int32_t* pos_ids_out, int32_t* perm_out,
                          int32_t* cnt_out, void* stream);
/* morec_bert_embed_fwd with the position row of token m taken from pos_ids[m] instead of m % T (same summation order, LayerNorm and
 * dropout stream). */
int morec_bert_embed_fwd_pos(const int32_t* ids, const int32_t* pos_ids, const float* word, const float* pos, const float* type0,
                             const float* gamma, const float* beta, float eps, void* z_out, void* y, float* mean, float* rstd,
                             int M, int T, int H, int dtype, float p_out, uint64_t seed_out, void* stream);
/* morec_bert_embed_bwd under the pad-relative rule (perm, cnt from morec_roberta_pos_ids): dpos[pos_pad + 1 + k] += the rows
 * n*T + perm[n*T + k] of the sequences with k < cnt[n]; dtype0 += every row; the word scatter as above.  Row pos_pad of dpos and the
 * rows outside pos_pad + 1 .. pos_pad + T are not written.  pos_pad < 0 or pos_pad + T >= n_pos: MOREC_E_ARG.  Row widths outside
 * the 16-byte vector layout (H % (16 / sizeof(dtype)) != 0 or more than 256 vectors per row): MOREC_E_UNSUPPORTED. */
int morec_roberta_embed_bwd(const int32_t* ids, const void* dz, float* dword, float* dpos, float* dtype0, int pad_id, int M, int T,
                            int H, int dtype, const int32_t* order, const int32_t* perm, const int32_t* cnt, int pos_pad, int n_pos,
                            void* stream);
/* OPT text tower (csrc/opt.hip; HF modeling_opt.py, the reference's Text_Encoder_mean).  None of the four uses atomics or LDS hand-offs
 * between workgroups, every output element is written exactly once (no pre-zeroing), and every call computes the same bits in either
 * setting of the deterministic mode.
 * morec_mask_pos_ids: position ids counted from the attention MASK (OPTLearnedPositionalEmbedding), never from the ids.  mask int32
 * [n_seq * T], nonzero = kept.  pos_ids[n*T + t] = offset + k for the k-th (from 0) kept token, offset - 1 for a masked one; cnt[n] =
 * number of kept tokens; perm[n*T + k] = position of the k-th kept token for k < cnt[n], then the masked positions in order (what
 * morec_roberta_embed_bwd walks with pos_pad = offset - 1).  Holes in the mask are legal.  One wavefront per sequence.  Null pointers,
 * n_seq or T <= 0, offset - 1 < 0 or offset + T - 1 >= n_pos: MOREC_E_ARG before anything is launched. */
int morec_mask_pos_ids(const int32_t* mask, int n_seq, int T, int offset, int n_pos, int32_t* pos_ids_out, int32_t* perm_out,
                       int32_t* cnt_out, void* stream);
/* out[m, :] = round(word[ids[m], :] + pos[pos_ids[m], :]): fp32 tables, one fp32 add, one rounding to dtype; 16-byte accesses.  No
 * LayerNorm, token type or dropout (OPTDecoder).  H % (16 / sizeof(dtype)) != 0 or more than 256 vectors per row:
 * MOREC_E_UNSUPPORTED; null pointers, M or H <= 0: MOREC_E_ARG; a base pointer off 16 bytes: MOREC_E_ALIGN. */
int morec_opt_embed_fwd(const int32_t* ids, const int32_t* pos_ids, const float* word, const float* pos, void* out, int M, int H,
                        int dtype, void* stream);
/* Masked mean pooling (Text_Encoder_mean: sum(h * mask) / clamp(sum(mask), 1e-9)).  cu == NULL: the padded layout, title n owns rows
 * n*T .. n*T + T - 1; otherwise the packed rows cu[n] .. cu[n+1] - 1.  keep: the fp32 per-row key mask of the attention kernels
 * (nonzero = kept).  fwd: out[n, :] = (sum of the kept rows of x, fp32, in row order) / max(count, 1e-9), rounded once; a title
 * without a kept row gives zeros.  bwd: dx[row, :] = keep[row] ? g[n, :] / count : 0, written for every row of every title.  The count
 * is taken from keep, never from the packed length.  Errors as morec_opt_embed_fwd. */
int morec_masked_mean_fwd(const void* x, const float* keep, const int32_t* cu, void* out, int n_seq, int T, int H, int dtype,
                          void* stream);
int morec_masked_mean_bwd(const void* g, const float* keep, const int32_t* cu, void* dx, int n_seq, int T, int H, int dtype,
                          void* stream);
/* out[r, :] = table[idx[r], :]  (fp32 table -> dtype out).  T/model/model.py:37 nn.Embedding lookup. */
int morec_gather_rows(const float* table, const int32_t* idx, void* out, int R, int D, int dtype, void* stream);
/* dtable[idx[r], :] += d[r, :] unless idx[r] == pad_id (padding_idx=0, T/model/model.py:27) */
int morec_scatter_add_rows(const void* d, const int32_t* idx, float* dtable, int R, int D, int pad_id, int dtype,
                           void* stream);
/* strided row copy: out[r, :] = in[r*stride_rows, :]  (hidden[:, 0], T/model/encoders.py:69) and its
 * backward (scatter into a zero-filled [R*stride_rows, D]) */
/* out[out_idx ? out_idx[r] : r, :] = in[in_idx ? in_idx[r] : r, :] for r < R (row gather / scatter; indices int32, device);
 * in_idx[r] < 0 writes a zero row (the [PAD] rows when a packed token layout is spread back over the padded one) */
int morec_indexed_rows_copy(const void* in, void* out, const int32_t* in_idx, const int32_t* out_idx, int R, int D, int dtype,
                            void* stream);
int morec_strided_rows_copy(const void* in, void* out, int R, int D, int in_row_stride, int out_row_stride,
                            int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * ID (+) modality fusion of item vectors (bce_text/id_plus_mo-end2end: model/model.py:26-47, model/encoders.py:8-39): each item vector is
 * fc(id_embedding(id), encoder(content)) with fc = ADD (x + y) or CAT (cat([x, y], 1) -> one or three Dropout -> Linear -> GELU layers).
 * table: fp32 [n_rows, D]; idx: int32 [R]; content / out / a / dA / d_content: dtype.  D % 8 (16-bit) or D % 4 (fp32), else
 * MOREC_E_ALIGN; p outside [0, 1): MOREC_E_ARG -- all before anything is launched.  Dropout is the counter-based stream of the LayerNorm
 * kernels (element index = position in the matrix named below; morec_dropout_keep_mask exports it); masks are regenerated, never stored.
 *   morec_fuse_add_fwd:  out[r] = T(table[idx[r]] + float(content[r])): one fp32 add, one rounding.  Row idx == 0 is gathered like any
 *       other.  No backward kernel: d(content) = d(out), d(table) by morec_scatter_add_rows with pad_id = 0.
 *   morec_fuse_cat_fwd:  a[r, 0:D] = drop(table[idx[r]]), a[r, D:2D] = drop(content[r]), one stream over the [R, 2D] matrix, kept values
 *       times 1 / (1 - floor(p 2^16) / 2^16), rounded once; p = 0: gather + concatenation.  a feeds morec_gemm_nt (bias, GELU, aux).
 *   morec_fuse_cat_bwd:  from dA [R, 2D] (that GEMM's input gradient) and the forward's (p, seed):
 *       d_content[r] = mask . inv_keep . dA[r, D:2D] (dtype, overwritten);  d_table[idx[r]] += mask . inv_keep . dA[r, 0:D] (fp32, ADDED,
 *       unrounded) unless idx[r] == pad_id.  fp32 atomics, or in the deterministic mode one writer wave per table row summing its source
 *       rows in row order.
 *   morec_dropout_apply: out[e] = keep(e) ? x[e] . inv_keep : 0 for e < n (out may alias x): the Dropouts between the layers of the
 *       three-layer MLP, forward and (same p, seed) backward.
 * ------------------------------------------------------------------------------------------ */
int morec_fuse_add_fwd(const float* table, const int32_t* idx, const void* content, void* out, int R, int D, int dtype, void* stream);
int morec_fuse_cat_fwd(const float* table, const int32_t* idx, const void* content, void* a_out, int R, int D, int dtype, float p,
                       uint64_t seed, void* stream);
int morec_fuse_cat_bwd(const void* dA, const int32_t* idx, void* d_content, float* d_table, int R, int D, int pad_id, int dtype,
                       float p, uint64_t seed, void* stream);
int morec_dropout_apply(const void* x, void* out, size_t n, float p, uint64_t seed, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Two-stage training on frozen item features (bce_text/main-2stage(SASRec), bce_vision/main-2stage(SASRec): model/encoders.py MLP_Layers.fc
 * over rows of a precomputed feature table, which the reference gathers on the host, data_utils/dataset.py BuildTrainDataset).  The first
 * layer with the gather folded in, one launch (csrc/featproj.hip):
 *     out[r, :] = GELU(table[idx[r], :] . W^T + b),   pre[r, :] = table[idx[r], :] . W^T + b,   r < R
 * table [n_rows, Kw] and W [D, Kw]: the same 16-bit dtype, contiguous;  idx int32 [R];  b fp32 [D] or NULL;  out, and pre unless NULL,
 * [R, D] in dtype.  fp32 accumulation on v_mfma_f32_16x16x32_{f16,bf16}, erf GELU (MOREC_ACT_GELU) on the fp32 sum, one rounding per
 * output.  One writer per element and no atomics: the same bits on every run.  Rows >= R and columns >= D are never written.  idx values
 * are clamped into [0, n_rows) inside the kernel, so a bad id never reads outside the table (the data layer validates ids on the host).
 * Checked in this order, before anything touches the device: R, n_rows, Kw or D < 1: MOREC_E_ARG;  fp32 (or an unknown dtype):
 * MOREC_E_DTYPE -- the fp32, fp32x3 and *_res32 first layers are morec_indexed_rows_copy + morec_gemm_nt;  Kw % 8 or D % 8:
 * MOREC_E_ALIGN (loads and stores are whole 16- / 8-byte lanes; Kw % 32 != 0 is legal, the K tail is zero-filled in registers);
 * a null table, idx, W or out: MOREC_E_ARG;  a base pointer off 16 bytes: MOREC_E_ALIGN.
 * morec_featproj_supported: 1 where the library's callers should take this kernel instead of the two-launch composition.  Knob
 * "featproj" (MOREC_FEATPROJ): 0 automatic | 1 never | 2 wherever the rules above allow.  Automatic: where the rules allow and
 * R Kw D <= 2^29 -- measured (profiles/two_stage_step.txt): ahead of the composition up to 1344 x 768 x 512 and at every R with
 * Kw = 128, D = 64; behind it at 5376 x 768 x 512 (39 us against 21 us), where each wave re-reads its operand rows through L2.
 * ------------------------------------------------------------------------------------------ */
int morec_featproj_fwd(const void* table, const int32_t* idx, const void* W, const float* bias, void* out, void* pre, int R, int n_rows,
                       int Kw, int D, int dtype, void* stream);
int morec_featproj_supported(int R, int Kw, int D, int dtype);

/* ------------------------------------------------------------------------------------------
 * Two-stage ID (+) modality fusion (bce_text/id_plus_mo-2stage, bce_vision/id_plus_mo-2stage: model/model.py:48-50 with mo_dnn_layers = 0):
 * the feature lookup, the projection, the GELU and the fusion with the id row in one launch (csrc/featfuse.hip):
 *     y[r, :] = GELU(table[idx[r], :] . W^T + b),   pre[r, :] = table[idx[r], :] . W^T + b (unless NULL),   r < R
 *     MOREC_FUSE_ADD:  out[r, 0:D] = id_table[idx[r], :] + y[r, :]                                       out [R, D]
 *     MOREC_FUSE_CAT:  out[r, 0:D] = drop(id_table[idx[r], :]),  out[r, D:2D] = drop(y[r, :])            out [R, 2D]
 * table, W, b, pre: as morec_featproj_fwd;  id_table fp32 [n_rows, D];  (p, seed): morec_fuse_cat_fwd's dropout stream over the [R, 2D]
 * matrix (ADD: p is checked and unused).  The main loop is morec_featproj_fwd's; y is rounded to dtype before the add / the dropout
 * scaling, so out and pre carry the bits of morec_featproj_fwd followed by morec_fuse_add_fwd / morec_fuse_cat_fwd with the same inputs, p
 * and seed.  idx is clamped into [0, n_rows) for BOTH tables; rows past R of out / pre are not touched.  Deterministic.
 * Checked in this order, before anything is launched: R, n_rows, Kw or D <= 0: MOREC_E_ARG;  dtype MOREC_F32: MOREC_E_DTYPE;  Kw % 8 or
 * D % 8: MOREC_E_ALIGN;  kind neither MOREC_FUSE_ADD nor MOREC_FUSE_CAT, or p outside [0, 1): MOREC_E_ARG;  a null table, idx, W,
 * id_table or out: MOREC_E_ARG;  a base pointer off 16 bytes: MOREC_E_ALIGN.
 * morec_featfuse_supported: 1 where callers should take this kernel instead of the composition.  Knob "featfuse" (MOREC_FEATFUSE):
 * 0 automatic | 1 never | 2 wherever the rules above allow.  Automatic: where the rules allow and R Kw D <= 3 . 2^28 -- measured
 * (profiles/id_two_stage_step.txt): ahead of the composition up to 2048 x 768 x 512 and at 21504 x 128 x 64, behind it at 5376 x 768 x 512
 * (40 us against 25 us), where each wave re-reads its operand rows through L2 as in morec_featproj_fwd.
 * ------------------------------------------------------------------------------------------ */
#define MOREC_FUSE_ADD 0
#define MOREC_FUSE_CAT 1
int morec_featfuse_fwd(const void* table, const int32_t* idx, const void* W, const float* bias, const float* id_table, void* out, void* pre,
                       int R, int n_rows, int Kw, int D, int dtype, int kind, float p, uint64_t seed, void* stream);
int morec_featfuse_supported(int R, int Kw, int D, int dtype);

/* ------------------------------------------------------------------------------------------
 * In-batch debiased sampled-softmax cross-entropy (T/model/model.py:32-33,45-67), fused:
 * logits never reach HBM.  P [Nr, D] user states (Nr = B*S rows), E [Nc, D] item vectors of the
 * column pool (local: Nc = B*(S+1); pooled over ranks: SURVEY.md §8e), both `dtype`.
 *   row_ids   int32 [B*(S+1)]  ids of this rank's users (reject sets)
 *   col_ids   int32 [Nc]       ids of the pool columns
 *   col_logpop float [Nc]      log(pop_prob[col_ids])
 *   col_valid uint8 [Nc]       slot is not padding (cat(log_mask, 1) != 0)
 *   row_valid uint8 [Nr]       log_mask != 0
 *   col_offset                 column of this rank's slot 0 in the pool
 * fwd: per-(row, 64-column slice) partial (max, sumexp) + positive logit -> row_lse[Nr], row_loss[Nr]
 *      and loss_sum (fp32 scalar, += the sum of the valid rows' losses, added in a fixed order: bit-reproducible; caller zeroes it).
 * bwd: dP[Nr, D] and dE[Nc, D] (dtype, overwritten):
 *      dlogit = gscale * (*gscale_dev if given) * (softmax - onehot) on unmasked cells of valid rows,
 *      0 elsewhere; dP = dlogit . E, dE = dlogit^T . P.
 * workspace (both): morec_inbatch_ce_workspace_bytes().
 * MOREC_E_UNSUPPORTED: S so long that the id lists of the users under one 128-row tile do not fit the tile kernel's 64 KiB of LDS
 * (two users of S > 8015 positions; the reference's launchers use S <= 50).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int B, S, D;
    int Nc;
    int col_offset;
    int dtype;
    int dE_fp32;   /* backward only: dE is written as fp32 [Nc, D] whatever the compute dtype (the pooled-negative step reduce-scatters it
                    * over ranks in fp32); bf16 compute with Nc % 8 == 0 only, MOREC_E_UNSUPPORTED otherwise */
    int ws_from_fwd; /* backward only: 1 = `workspace` is the buffer the matching morec_inbatch_ce_fwd call (same descriptor fields, same
                      * P / E / ids / log-pop / validity) was given and nothing has written to it since: the backward then reuses the
                      * (user, column) flag table and the positive logits the forward left there instead of rebuilding them (the
                      * 256 x 256 kernels; ignored by the 128 x 128 ones; the "ce8p" knob must not change between the two calls).
                      * 0 = the workspace is plain scratch. */
} morec_ce_desc;

size_t morec_inbatch_ce_workspace_bytes(const morec_ce_desc* d);
int morec_inbatch_ce_fwd(const morec_ce_desc* d, const void* P, const void* E, const int32_t* row_ids,
                         const int32_t* col_ids, const float* col_logpop, const uint8_t* col_valid,
                         const uint8_t* row_valid, float* row_lse, float* row_loss, float* loss_sum,
                         void* workspace, void* stream);
int morec_inbatch_ce_bwd(const morec_ce_desc* d, const void* P, const void* E, const int32_t* row_ids,
                         const int32_t* col_ids, const float* col_logpop, const uint8_t* col_valid,
                         const uint8_t* row_valid, const float* row_lse, const float* gscale_dev, float gscale,
                         void* dP, void* dE, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused AdamW over a flat fp32 parameter arena (torch.optim.AdamW semantics, T/run.py:159-162,246).
 * One launch per hyper-parameter group (contiguous range).  Optionally refreshes the bf16 shadow.
 * step = 1-based step count after increment.
 * ------------------------------------------------------------------------------------------ */
int morec_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, size_t n,
                float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident step state: what the reference keeps in `torch.cuda.amp.GradScaler()` and in AdamW's per-parameter `step`
 * (T/run.py:210: scaler = GradScaler(); :243-247: scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()), held in
 * one 64-byte DEVICE block so that a step needs no host round trip and no per-step host scalar among its kernel arguments
 * (a captured graph of the step can be replayed).  Protocol of one step in the fp16 mode:
 *   forward; backward with the loss gradient multiplied by sp->loss_scale (morec_inbatch_ce_bwd: gscale_dev = loss_scale / n_valid);
 *   gradient reduction over ranks; morec_grad_check_finite over every gradient arena; morec_step_decide; morec_adamw_sp per group.
 * A step with a non-finite gradient leaves parameters, moments, shadows and the step count untouched and halves the scale
 * (GradScaler defaults: init 65536, growth 2 every 2000 clean steps, backoff 0.5 -- passed in by the caller).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t step;           /* optimizer steps APPLIED so far (a skipped step does not count, as torch never calls optimizer.step() for it) */
    int32_t found_inf;      /* != 0: a non-finite gradient has been seen since the last morec_step_decide */
    int32_t growth_tracker; /* consecutive clean steps since the scale last changed */
    int32_t skipped;        /* steps skipped so far (diagnostics) */
    float loss_scale;       /* S of the NEXT backward pass */
    float inv_scale;        /* 1 / S of the step being applied: what morec_adamw_sp multiplies the gradients with */
    float bc1, bc2;         /* 1 - beta1^step, 1 - beta2^step of the step being applied */
    int32_t apply;          /* decision of the last morec_step_decide: 1 = update, 0 = skip */
    int32_t ctl_flags;      /* MOREC_SP_* bits: which of clip_coef / lr_mult the last decision set.  0 (every block before morec_step_decide_ex
                             * existed, every checkpoint, morec_step_params_init, morec_step_decide): morec_adamw_sp reads neither */
    uint64_t drop_seed;       /* splitmix64 state, advanced by every morec_step_decide */
    uint64_t drop_seed_mixed; /* its output: the word morec_dropout_seed_source(&sp->drop_seed_mixed) feeds to the dropout kernels */
    float clip_coef;        /* min(1, max_norm / (grad_norm + 1e-6)) of the step being applied; read only under MOREC_SP_CLIP */
    float lr_mult;          /* LR multiplier of the step being applied (0 is a legitimate value); read only under MOREC_SP_LR_MULT */
} morec_step_params;
#define MOREC_SP_CLIP 1
#define MOREC_SP_LR_MULT 2
/* ZERO-WORDS RULE: ctl_flags, clip_coef and lr_mult occupy the three words that used to be padding.  A block in which they are zero behaves
 * exactly as it did before they had names; size (64 bytes) and the offset of every other field are unchanged. */

/* LR schedule of morec_step_decide_ex.  The multiplier of the optimizer step with 0-based index t (t = steps APPLIED before it: a skipped
 * step does not advance the schedule; the first step has t = 0, as torch's LambdaLR numbers them), W = warmup_steps, T = total_steps,
 * r = min_ratio:
 *     t < W                  : t / W
 *     otherwise, CONSTANT    : 1
 *     otherwise              : q = min(1, (t - W) / max(1, T - W));
 *                    LINEAR  : r + (1 - r) (1 - q)
 *                    COSINE  : r + (1 - r) (1 + cos(pi q)) / 2
 * (it holds at r from t = T on).  Evaluated in double, stored as float. */
#define MOREC_LR_CONSTANT 0
#define MOREC_LR_LINEAR 1
#define MOREC_LR_COSINE 2
typedef struct {
    int32_t kind;          /* MOREC_LR_* */
    int32_t warmup_steps;  /* >= 0 */
    int32_t total_steps;   /* >= warmup_steps for LINEAR / COSINE; unused for CONSTANT */
    float min_ratio;       /* in [0, 1] */
} morec_lr_schedule;
/* Process-wide dropout seed source (state item 4 of the list at the top of this file): dev_u64 = a DEVICE uint64 (8-byte aligned) that every
 * dropout / DropPath kernel XORs into the two halves of its seed argument at kernel entry, NULL = none (the default).  The mask of a launch
 * is then a function of (seed argument, *dev_u64): a captured graph of the step -- whose seed arguments are frozen at capture -- draws
 * fresh masks at every replay when the word changes between replays (morec_step_decide advances sp->drop_seed_mixed).  The word must not
 * change between the forward and the backward launch that regenerate the same mask.  Stands where torch's global CUDA RNG state stands in
 * the reference (nn.Dropout under T/run.py:307-314 `setup_seed`). */
int morec_dropout_seed_source(const void* dev_u64);
/* Stream `waiting` runs nothing issued after this call before the work issued to stream `signal` so far has finished (event record + stream
 * wait on an internal ring of 256 events; capturable; one device per process).  torch.cuda.Stream.wait_stream in one foreign call: orders the
 * weight-gradient stream behind the backward chain per dW launch.  No reference counterpart (autograd runs its backward on one stream). */
int morec_stream_wait_stream(void* waiting, void* signal);
/* *sp = {step, loss_scale = init_scale, everything else clear} (init_scale = 1: no scaling, bf16 / fp32 modes) */
int morec_step_params_init(morec_step_params* sp, float init_scale, int step, void* stream);
/* sp->found_inf |= any element of grad[0 .. n) is inf or NaN   (GradScaler.unscale_'s found_inf; the division by S is left to AdamW) */
int morec_grad_check_finite(const float* grad, size_t n, morec_step_params* sp, void* stream);
/* GradScaler.step + update on the device: apply = !found_inf; on apply: ++step, bias corrections (formed in double), growth
 * bookkeeping; on skip: ++skipped, scale *= backoff_factor; found_inf is cleared.  dynamic == 0 keeps the scale fixed.  ctl_flags is
 * cleared (no clip coefficient, no LR multiplier: morec_step_decide_ex sets them). */
int morec_step_decide(morec_step_params* sp, float beta1, float beta2, float growth_factor, float backoff_factor,
                      int growth_interval, int dynamic, void* stream);
/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) and an LR schedule without a host scalar in the step.  Protocol:
 * morec_grad_norm_check per gradient arena in place of morec_grad_check_finite, morec_step_decide_ex in place of morec_step_decide.
 *
 * morec_grad_norm_blocks(n): slots of `partials` an arena of n elements fills -- a function of n alone.
 * morec_grad_norm_check: found_inf exactly as morec_grad_check_finite, and partials[slot + b] = block b's share of sum((grad[i] / S)^2), S =
 * sp->loss_scale (the gradients are unscaled BEFORE squaring).  Bit-reproducible: no floating-point atomics, fixed order of additions in the
 * thread, the wavefront and the block, every slot written by one lane.  Padding inside the arena must be zero.  n_slots = capacity of
 * `partials`; slot + morec_grad_norm_blocks(n) > n_slots, or a NULL pointer: MOREC_E_ARG; n % 4 or grad off 16 bytes: MOREC_E_ALIGN; all
 * before anything is launched. */
size_t morec_grad_norm_blocks(size_t n);
int morec_grad_norm_check(const float* grad, size_t n, morec_step_params* sp, float* partials, size_t slot, size_t n_slots, void* stream);
/* morec_step_decide plus: total = partials[0] + ... + partials[n_partials - 1] (ascending, in double); grad_norm = sqrt(total), written to
 * *grad_norm_out (DEVICE float, may be NULL: logging only).  A non-finite total counts as found_inf -- the step is skipped and the scale
 * backs off (torch's clip_grad_norm_ would scale the gradients by NaN / 0 instead; under GradScaler the step is skipped there too).
 * max_norm > 0: clip_coef = min(1, max_norm / (grad_norm + 1e-6)) and MOREC_SP_CLIP; max_norm <= 0: no clipping (partials may then be NULL
 * with n_partials 0).  sched != NULL (HOST struct, read during the call): lr_mult by the formula at morec_lr_schedule, with t = sp->step
 * before this step's increment, and MOREC_SP_LR_MULT; NULL: no schedule.  With max_norm <= 0, sched NULL and no partials it decides what
 * morec_step_decide decides. */
int morec_step_decide_ex(morec_step_params* sp, float beta1, float beta2, float growth_factor, float backoff_factor, int growth_interval,
                         int dynamic, const float* partials, size_t n_partials, float max_norm, const morec_lr_schedule* sched,
                         float* grad_norm_out, void* stream);
/* morec_adamw with step count / bias corrections / gradient scale (1 / S) read from *sp; does nothing when sp->apply == 0.
 * Under MOREC_SP_CLIP the gradient scale is clip_coef / S; under MOREC_SP_LR_MULT the step size AND the weight decay use lr * lr_mult (as
 * torch under a scheduler).  Flags clear, or both factors 1.0f: the same bits as without them.
 * shadow (may be NULL): 16-bit copy of the updated parameters in shadow_dtype (MOREC_BF16 | MOREC_F16). */
int morec_adamw_sp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype, size_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, const morec_step_params* sp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation (T/data_utils/metrics.py:96-102,49-57): rank of the target among all items after
 * masking the history -- count-greater instead of a full argsort.
 * scores = prec[U, D] . item_emb[item_num+1, D]^T are formed tile by tile; rank[u] = 1 + #{items i>=1,
 * i not in history(u), score[u,i] > score[u,target[u]]}.
 * hist: int32 [U, Hmax] padded with -1, any length; repeats and ids outside [1, n_items_plus1) are harmless.
 * ------------------------------------------------------------------------------------------ */
int morec_eval_rank(const float* prec, const float* item_emb, const int32_t* hist, int Hmax, const int32_t* target,
                    int32_t* rank, float* tscore_ws /* float[U] scratch */, int U, int n_items_plus1, int D,
                    void* stream);
/* Cold-start / new-item evaluation (T/data_utils/special.py, eval_model_special): the target is a NEW item, a row of a separate
 * candidate table, ranked against the whole catalogue (the reference appends it to the [item_num+1, D] table per user and
 * argsorts).  rank[u] = 1 + #{items i in [1, n_items_plus1), i not in history(u) : score[u,i] > prec[u] . cand_emb[cand_idx[u]]}.
 * The candidate is never masked and no catalogue column is excluded; ties do not count (as in morec_eval_rank).
 * cand_emb: f32 [n_cand_rows, D]; cand_idx: int32 [U], row reads clamped into [0, n_cand_rows). */
int morec_eval_rank_cand(const float* prec, const float* item_emb, const int32_t* hist, int Hmax, const float* cand_emb,
                         int n_cand_rows, const int32_t* cand_idx, int32_t* rank, float* tscore_ws /* float[U] scratch */, int U,
                         int n_items_plus1, int D, void* stream);
/* Top-K recommendation lists (T/data_utils/metrics.py:96-102 -- score every item, set the history to -inf, argsort -- read for the
 * first K positions instead of the target's): row u of out_ids / out_scores holds the K best ELIGIBLE items of user u, where item i
 * is eligible when 1 <= i < n_items_plus1 and i does not occur in hist[u, :], in a strict total order: score descending, item id
 * ascending among equal scores.  score = prec[u] . item_emb[i] on the exact-fp32 MFMA main loop of morec_eval_rank.  Fewer than K
 * eligible items: the remaining slots hold id -1 and score -inf.  A NaN score is never returned (ordered comparisons only).
 * hist: int32 [U, Hmax] as for morec_eval_rank; NULL or Hmax == 0: nobody masks anything.
 * strips: column strips the catalogue is cut into (0 = automatic, values above the number of 128-column tiles are clamped); the
 * result does not depend on it, on the grid or on the device.  ws: scratch of at least morec_eval_topk_ws_bytes(...) bytes for the
 * same (U, n_items_plus1, K, strips), 8-byte aligned.  K < 1, null outputs or a short workspace: MOREC_E_ARG;
 * K > morec_eval_topk_max_k(): MOREC_E_UNSUPPORTED; D % 4 or misaligned operands: MOREC_E_ALIGN -- all before anything is launched. */
int morec_eval_topk(const float* prec, const float* item_emb, const int32_t* hist, int Hmax, int K, int strips,
                    int32_t* out_ids /* [U, K] */, float* out_scores /* [U, K] */, void* ws, size_t ws_bytes, int U,
                    int n_items_plus1, int D, void* stream);
/* Host-only queries for morec_eval_topk (no device needed; T/data_utils/metrics.py:96-102 has no counterpart: torch allocates the
 * score matrix).  ws_bytes: 0 for arguments morec_eval_topk rejects, else positive and monotone in U, K and strips. */
size_t morec_eval_topk_ws_bytes(int U, int n_items_plus1, int K, int strips);
/* Largest K of morec_eval_topk (T/data_utils/metrics.py:49-57 uses 10): one list entry per lane of a wave, and 128 rows x K x 8 B of
 * lists beside the 64 KiB score tile in one CU's 160 KiB of LDS -- 64. */
int morec_eval_topk_max_k(void);

/* test hook: out[i] = 1 iff the dropout hash keeps element index i for (p, seed) */
int morec_dropout_keep_mask(uint8_t* out, size_t n, float p, uint64_t seed, void* stream);

/* diagnostics: dumps MFMA fragment layouts and ds_read_b64_tr_b16 semantics into out (int32[4096]) */
int morec_probe(int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Vision input pipeline, device half: n decoded uint8 HWC images of arbitrary sizes, packed back to back
 * in `src`, -> uint8 [n, R, R, 3], bit for bit the reference's host-side tv.transforms.Resize((R, R)) on the PIL image
 * (V/data_utils/dataset.py:68-73,91-98 = Pillow's two-pass BILINEAR resampler).  meta: int64 [n][5] = byte offset in src, H, W,
 * offset (in int32 words) of the horizontal and of the vertical tap table in `tables`; a table = ksize, then R rows of
 * (first input index, tap count, taps[ksize]) in Pillow's 2^22 fixed point (host: data_utils/images.py::resize_table).
 * ToTensor + Normalize(0.5, 0.5) are fused into morec_swin_patchify_u8.
 * ------------------------------------------------------------------------------------------ */
int morec_image_resize_u8(const uint8_t* src, const int64_t* meta, const int32_t* tables, uint8_t* out, int n, int R, void* stream);

/* ------------------------------------------------------------------------------------------
 * The image catalogue on the device, a batch as its item ids (csrc/image_front.hip): the indexed forms of the three entry points
 * through which decoded uint8 images enter a vision tower -- morec_swin_patchify_u8, morec_mae_patchify_keep_u8 and the uint8 case
 * of morec_pixels_to_nhwc, the direct forms.  One kernel per layout serves both: the direct form reads image k of the pixel batch,
 * the indexed form catalogue row ids[k].  catalogue: uint8 [n_rows, R, R, channels] ([n_rows, H, W, C] for the NHWC form); ids:
 * int32 [n_img] on the device; the remaining arguments are the direct form's.  ids[k] is clamped into [0, n_rows - 1] (a bad id
 * never reads outside the catalogue; hosts reject it before it gets here).  The output is bit-equal to a row gather of the catalogue
 * followed by the direct form.  The MAE form takes its kept patches from keep[k] and its pixels from row ids[k].  In both forms RGB
 * images with patch % 4 == 0 and ld_out % 4 == 0 (NHWC: H W C % 4 == 0), a source on 4 bytes and an output on 16 move 4 pixels
 * (4 bytes) per thread; anything else moves single elements.  No atomics, one writer per output element.
 * Errors as the direct forms', judged before any launch; ids == NULL, n_rows <= 0 or n_img <= 0: MOREC_E_ARG.
 * ------------------------------------------------------------------------------------------ */
int morec_swin_patchify_u8_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, void* out, int n_img, int channels, int R,
                               int patch, int ld_out, float mean, float std, int dtype, void* stream);
int morec_mae_patchify_keep_u8_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, const int32_t* keep, void* out, int n_img,
                                   int channels, int R, int patch, int len_keep, int ld_out, float mean, float std, int dtype,
                                   void* stream);
int morec_pixels_to_nhwc_idx(const uint8_t* catalogue, const int32_t* ids, int n_rows, void* out, int n_img, int C, int H, int W,
                             float mean, float std, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Collectives of the data-parallel step on the CALLER's stream (RCCL over xGMI, resolved with dlopen from the
 * librccl.so.1 already mapped in the process -- PyTorch's -- and never linked).  They replace, stream-ordered with the kernels
 * around them, what the reference gets from DistributedDataParallel's NCCL hooks (T/run.py:148,321) plus the exchange the
 * pooled-negative step adds:  all-gather of the encoded item vectors E [Nc, D] and of the packed (ids | log-pop | validity |
 * n_valid) record, reduce-scatter(SUM) of dE_pool [world Nc, D] in fp32, all-reduce(SUM) of a gradient bucket in fp32.
 * h_id128: HOST buffer of 128 bytes (ncclUniqueId): rank 0 fills it with morec_comm_unique_id and hands it to the other ranks
 * out of band (torch.distributed store / broadcast, MPI, a file); morec_comm_create is collective over the `world` ranks and
 * needs this process's device to be current.  One handle per (process, device); calls on one handle must not overlap in time
 * on different streams.  Errors: MOREC_E_UNSUPPORTED = no RCCL library found, MOREC_E_COMM = RCCL reported a failure.
 * ------------------------------------------------------------------------------------------ */
typedef struct morec_comm morec_comm;
int morec_comm_available(void);                       /* 1 when librccl.so.1 and every entry point needed were found */
int morec_comm_unique_id(void* h_id128);
int morec_comm_create(morec_comm** out, const void* h_id128, int rank, int world);
int morec_comm_destroy(morec_comm* comm);
const char* morec_comm_last_error(const morec_comm* comm);
/* recv[r * bytes_per_rank ...] = rank r's send[0 .. bytes_per_rank)   (ncclAllGather, byte-typed) */
int morec_comm_all_gather(morec_comm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
/* recv[i] = sum_r send_r[rank * count_per_rank + i]                   (ncclReduceScatter, fp32 SUM) */
int morec_comm_reduce_scatter_f32(morec_comm* comm, const float* send, float* recv, size_t count_per_rank, void* stream);
/* buf[i] = sum_r buf_r[i], in place                                   (ncclAllReduce, fp32 SUM) */
int morec_comm_all_reduce_f32(morec_comm* comm, float* buf, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOREC_HIP_H */
