"""Tensor-level wrappers over the C-ABI (``include/morec_hip.h``): they marshal ``torch`` device tensors
into raw pointers + sizes and launch on torch's current HIP stream.  PyTorch is plumbing here (memory,
streams); all arithmetic happens in ``libmorec_hip.so``.  Every wrapper raises on a non-zero return code.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU, BF16, F16, F32, AttnDesc, CeDesc, GemmDesc, SwinAttnDesc, check

FLT_MIN_MASK = -3.4028234663852886e38  # torch.finfo(torch.float32).min: HF eager additive key mask


# Deterministic mode (``MOREC_DETERMINISTIC=1`` in the environment, or ``set_deterministic(True)``): the library's kernels that end in
# fp32 atomics (LayerNorm / bias column sums, the embedding-table scatters) fold per-block partials in a fixed order instead, and the
# engines keep the split-K of the exact-fp32 weight-gradient GEMMs at one -- two runs of the same step give the same bits.  The
# reference sets torch's deterministic flags (``T/run.py:313-314``).  Covers the text / ID towers; see DESIGN.md §3.
DETERMINISTIC = _lib.env_flag("MOREC_DETERMINISTIC")      # the library is told the same at load (_lib.lib)


def set_deterministic(on: bool = True):
    global DETERMINISTIC
    check(_lib.lib().morec_tuning_set(b"deterministic", int(bool(on))), "morec_tuning_set(deterministic)")
    DETERMINISTIC = bool(on)


def code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16
    raise _lib.MorecError(f"unsupported dtype {dt}")


def _p(t):
    """Raw device address (an int: every pointer parameter is declared ``c_void_p`` in ``_lib._SIGS``, ctypes converts; no wrapper object per argument)."""
    return None if t is None else t.data_ptr()


# the handle without building a torch.cuda.Stream object per launch (MOREC_STREAM_OBJ=1: the object path, for A/B timing of the host side)
_raw_stream = None if os.environ.get("MOREC_STREAM_OBJ") == "1" else getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """torch's CURRENT stream on the current device as a ``hipStream_t`` (every launch goes there; ~700 calls per training step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def stream_wait_stream(waiting, signal=None):
    """``waiting`` (raw handle) runs nothing issued later before what ``signal`` (default: torch's current stream) holds now has finished."""
    check(_lib.lib().morec_stream_wait_stream(waiting, _stream() if signal is None else signal), "morec_stream_wait_stream")


def fold_defer_begin() -> bool:
    """Open the library's deferred-fold scope on torch's current stream (``morec_fold_defer_begin``): until ``fold_defer_end`` the
    fixed-order folds of the deterministic mode issued on that stream are queued, and ``fold_flush`` launches them.  False: nothing was
    opened (knob off, atomic mode, stream under graph capture) and every call behaves as usual."""
    h = _lib.lib()
    check(h.morec_fold_defer_begin(_stream()), "morec_fold_defer_begin")
    return bool(h.morec_fold_defer_active())


def fold_flush(stream=None):
    """Launch the folds queued so far on ``stream`` (raw handle; default: torch's current stream).  The caller orders that stream behind the producers."""
    check(_lib.lib().morec_fold_flush(_stream() if stream is None else stream), "morec_fold_flush")


def fold_defer_end():
    check(_lib.lib().morec_fold_defer_end(), "morec_fold_defer_end")


def fold_stats() -> dict:
    out = (C.c_ulonglong * 4)()
    check(_lib.lib().morec_fold_stats(out), "morec_fold_stats")
    return {"allocations": out[0], "scratch_bytes": out[1], "jobs": out[2], "launches": out[3]}


def _dev(t):
    if not t.is_cuda:
        raise _lib.MorecError("libmorec_hip needs device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise _lib.MorecError("tensor must be contiguous")
    return t


def is16(dt: torch.dtype) -> bool:
    """bf16 or fp16: the two 16-bit storage types of the MFMA paths (``MOREC_BF16`` / ``MOREC_F16``)."""
    return dt in (torch.bfloat16, torch.float16)


def pad8(n: int) -> int:
    return (n + 7) & ~7


# ---------------------------------------------------------------------------------------------------------
# How products of fp32 operands run: "exact" = the exact-fp32 MFMA (the parity mode pinned to the reference goldens), "bf16x3" = both
# operands split into bf16 hi / lo parts and ONE bf16 GEMM over [hi | hi | lo] x [hi | lo | hi] (fp32 accumulation; the lo.lo term,
# 2^-16 relative, is dropped).  Set per step / forward by whoever owns the model (``compute_dtype`` "fp32" / "fp32x3").
FP32_GEMM = "exact"


class fp32_gemm_mode:
    """``with ops.fp32_gemm_mode("bf16x3"): ...`` -- sets ``FP32_GEMM`` for the block and restores it (also drops the per-step split cache
    on both ends).  ``Model.forward`` / ``TrainStep.forward_backward`` run under their model's mode; the autograd shells remember the
    mode of their forward for their backward.  Elsewhere (an encoder called on its own, eval) the process default "exact" applies."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        global FP32_GEMM
        self.prev, FP32_GEMM = FP32_GEMM, self.mode
        _X3_CACHE.clear()
        return self

    def __exit__(self, *exc):
        global FP32_GEMM
        FP32_GEMM = self.prev
        _X3_CACHE.clear()
        return False


def split_bf16x3(t, lo_slot, rows=None, cols=None, ld=None):
    """fp32 [R, C] (row pitch ``ld``) -> bf16 [R, 3 C]: hi | hi | lo (``lo_slot`` 2, A side) or hi | lo | hi (``lo_slot`` 1, B side)."""
    R = t.shape[0] if rows is None else rows
    Cc = t.shape[1] if cols is None else cols
    ld = t.stride(0) if ld is None else ld
    out = torch.empty((R, 3 * Cc), device=t.device, dtype=torch.bfloat16)
    check(_lib.lib().morec_split_bf16x3(_p(t), _p(out), R, Cc, ld, 3 * Cc, lo_slot, _stream()), "morec_split_bf16x3")
    return out


# hi | hi | lo splits of whole activation tensors, kept for the length of one step: the forward's split of x is what the weight-gradient
# product of the same x needs again, the dX product's split of dY likewise.  An entry holds a reference to its source (so the address
# cannot be recycled under it) and the source's version counter (an in-place write invalidates it).
_X3_CACHE = {}


def x3_cache_clear():
    _X3_CACHE.clear()


X3_VERIFY = os.environ.get("MOREC_X3_VERIFY", "0") == "1"
X3_HITS = 0


def split_cached(t):
    """``split_bf16x3(t, 2)`` ([hi | hi | lo], bf16 [R, 3 C]) of a whole contiguous fp32 tensor, computed once per step.
    The entry is keyed by the tensor object; ``t._version`` only sees torch's own in-place writes -- the library's kernels write through raw
    pointers -- so the contract is: no morec op overwrites a tensor between two GEMMs that read it (the engines keep it: the one in-place
    form, ``layernorm_fwd(z_inplace=True)``, overwrites a GEMM OUTPUT that was never an operand).  ``ops.X3_VERIFY`` (env ``MOREC_X3_VERIFY=1``)
    re-splits on every hit and compares: ``tests/test_fp32x3_gpu.py`` runs whole training steps under it."""
    global X3_HITS
    key = id(t)
    hit = _X3_CACHE.get(key)
    if hit is not None and hit[0] is t and hit[1] == t._version:
        if X3_VERIFY:
            X3_HITS += 1
            if not torch.equal(split_bf16x3(t, 2), hit[2]):
                raise RuntimeError("split_cached: the tensor changed since its [hi | hi | lo] split was cached (stale operand)")
        return hit[2]
    s = split_bf16x3(t, 2)
    _X3_CACHE[key] = (t, t._version, s)
    return s


def gemm_tn_x3_(dy3, x3, out, N, K, split_m=1, stream=None):
    """out[N, K] += dy^T x for fp32 dy [M, N], x [M, K] given as their [hi | hi | lo] splits (bf16 [M, 3 N], [M, 3 K]): the three
    products hi.hi + hi.lo + lo.hi on the transposing bf16 GEMM, reading the column blocks in place (row pitch 3 N / 3 K)."""
    _dev(dy3), _dev(x3)
    M = dy3.shape[0]
    ws = None
    if split_m > 1:
        need = _lib.lib().morec_gemm_tn_workspace_bytes(N, K, split_m) // 4
        ws = _scratch(_TN_WS, dy3.device, need, 20 * 1024 * 1024)
    py, px = dy3.data_ptr(), x3.data_ptr()
    for sy, sx in ((0, 0), (0, 2), (2, 0)):      # (hi, hi), (hi, lo), (lo, hi)
        check(_lib.lib().morec_gemm_tn(C.c_void_p(py + 2 * sy * N), C.c_void_p(px + 2 * sx * K), _p(out), M, N, K, 3 * N, 3 * K, out.stride(0),
                                       BF16, split_m, 1, _p(ws), _stream() if stream is None else stream), "morec_gemm_tn")
    return out


_CS_WS = {}      # per-device fp32 scratch of the fused column sums (stream-ordered reuse, like _TN_WS)
# Scratch buffers that have been outgrown are KEPT (never handed back to the allocator): a captured graph of the step
# (TrainStep.step_graphed) has their addresses baked into its kernel arguments and keeps writing there at every replay.
_WS_RETIRED = []


def _scratch(cache, device, need, floor):
    ws = cache.get(device)
    if ws is None or ws.numel() < need:
        grown = 0
        if ws is not None:
            _WS_RETIRED.append(ws)
            grown = ws.numel() + ws.numel() // 2      # geometric growth: everything ever retired stays below twice the live buffer
        ws = torch.empty(max(need, floor, grown), device=device, dtype=torch.float32)
        cache[device] = ws
    return ws


_GEMM_DESCS = {}


def gemm_nt(a, b, *, bias=None, act=ACT_NONE, out=None, out_dtype=None, aux_out=None, dact=ACT_NONE, dact_in=None,
            accumulate=0, split_k=1, alpha=1.0, M=None, N=None, K=None, lda=None, ldb=None, ldc=None, colsum_out=None,
            aux_deriv=False):
    """out[M,N] (+)= alpha * a[M,K] @ b[N,K]^T with the fused epilogues of ``morec_gemm_nt``; ``colsum_out`` (fp32 [N],
    ``dact`` epilogues only) additionally receives ``+= out.sum(0)``: the bias gradient of the layer below."""
    _dev(a), _dev(b)
    M = a.shape[0] if M is None else M
    K = a.shape[1] if K is None else K
    N = b.shape[0] if N is None else N
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=out_dtype or a.dtype)
    ldc = out.stride(0) if ldc is None else ldc
    if FP32_GEMM == "bf16x3" and a.dtype == torch.float32 and b.dtype == torch.float32 and K % 8 == 0:
        whole = a.dim() == 2 and a.is_contiguous() and M == a.shape[0] and K == a.shape[1] and lda == K
        a = split_cached(a) if whole else split_bf16x3(a, 2, M, K, lda)
        b = split_bf16x3(b, 1, N, K, ldb)
        K, lda, ldb = 3 * K, 3 * K, 3 * K
    key = (M, N, K, lda, ldb, ldc, a.dtype, out.dtype, act, dact, accumulate, split_k, alpha, bool(aux_deriv))
    d = _GEMM_DESCS.get(key)
    if d is None:      # the descriptor is read during the call only: one object per distinct launch shape, reused while the cache holds it
        if len(_GEMM_DESCS) >= 8192:      # the unpadded token layout makes M a per-batch number: bound the cache instead of growing with the run
            _GEMM_DESCS.clear()
        d = _GEMM_DESCS[key] = GemmDesc(M, N, K, lda, ldb, ldc, code(a.dtype), code(out.dtype), act, dact, accumulate, split_k, alpha, int(bool(aux_deriv)))
    if colsum_out is not None:
        need = _lib.lib().morec_gemm_colsum_workspace_bytes(M, N) // 4
        ws = _scratch(_CS_WS, a.device, need, 4 * 1024 * 1024)
        check(_lib.lib().morec_gemm_nt_colsum(C.byref(d), _p(a), _p(b), _p(out), _p(bias), _p(aux_out), _p(dact_in),
                                              _p(colsum_out), _p(ws), _stream()), "morec_gemm_nt_colsum")
        return out
    check(_lib.lib().morec_gemm_nt(C.byref(d), _p(a), _p(b), _p(out), _p(bias), _p(aux_out), _p(dact_in), _stream()),
          "morec_gemm_nt")
    return out


_DR_WS = {}


def gemm_plan(M, N, K, dtype=torch.bfloat16, *, out_dtype=None, bias=False, aux=False, dact_in=False, colsum=False, act=ACT_NONE,
              dact=ACT_NONE, accumulate=0, split_k=1, alpha=1.0, lda=None, ldb=None, ldc=None, n_cu=0):
    """Which kernel ``gemm_nt`` would run for this product (``morec_gemm_plan``): a dict of family name, epilogue mode, tile rows / columns,
    ngroup and the fused-column-sum flag.  ``n_cu`` > 0 answers for a chip of that many CUs without touching a device."""
    d = _lib.GemmDesc(M, N, K, lda or K, ldb or K, ldc or N, code(dtype), code(out_dtype or dtype), act, dact, accumulate, split_k, alpha, 0)
    info = _lib.GemmPlanInfo()
    check(_lib.lib().morec_gemm_plan(C.byref(d), int(bias), int(aux), int(dact_in), int(colsum), n_cu, C.byref(info)), "morec_gemm_plan")
    return {"family": info.family_name.decode(), "mode": info.mode, "tile_rows": info.tile_rows, "tile_cols": info.tile_cols,
            "ngroup": info.ngroup, "colsum_fused": bool(info.colsum_fused)}


def mlp_dact_recompute_supported(M, N, K, dtype):
    """Does ``mlp_dact_recompute`` take this shape (Swin stage-1 / stage-2 MLP: 288 < N <= 768, K <= 192, M >= 8192, 16-bit)?  The forward then
    runs fc1 + GELU WITHOUT the act'(pre) output."""
    return dtype in (torch.bfloat16, torch.float16) and bool(_lib.lib().morec_mlp_dact_recompute_supported(M, N, K, code(dtype)))


def mlp_dact_recompute(dy, w2t, x, w1, b1, colsum_out=None):
    """dU = (dy @ w2t^T) * GELU'(x @ w1^T + b1), ``colsum_out += dU.sum(0)``: the backward of ``GELU(fc1(x)) -> fc2`` down to the
    pre-activation gradient, with the pre-activation recomputed from ``x`` instead of read from a saved tensor
    (``morec_mlp_dact_recompute``)."""
    _dev(dy), _dev(x)
    M, K = dy.shape
    N = w2t.shape[0]
    assert dy.is_contiguous() and x.is_contiguous() and w2t.is_contiguous() and w1.is_contiguous()
    assert x.shape == (M, K) and w1.shape == (N, K) and w2t.shape == (N, K)
    out = torch.empty((M, N), device=dy.device, dtype=dy.dtype)
    ws = None
    if colsum_out is not None:
        ws = _scratch(_DR_WS, dy.device, _lib.lib().morec_mlp_dact_recompute_workspace_bytes(N) // 4, 1024 * 1024)
    check(_lib.lib().morec_mlp_dact_recompute(_p(dy), _p(w2t), _p(x), _p(w1), _p(b1), _p(out), _p(colsum_out), _p(ws), M, N, K,
                                              code(dy.dtype), _stream()), "morec_mlp_dact_recompute")
    return out


_TN_WS = {}


def gemm_tn_(dy, x, out, split_m=1, accumulate=True, slabs=True, stream=None, ws_cache=None):
    """out[N, K] (+)= dy[M, N]^T @ x[M, K] (bf16 operands, fp32 out) without transposed copies.  ``slabs``: reduce the
    split-m partials through a reusable fp32 workspace (deterministic) instead of fp32 atomics.  ``stream``: raw handle of the stream to
    launch on (default: torch's current stream) -- the weight-gradient stream, without a ``torch.cuda.stream`` context per launch.
    ``ws_cache``: the per-device slab workspace to use instead of the shared one (launches of ONE stream share a workspace: a caller on
    another stream than the weight-gradient stream brings its own)."""
    _dev(dy), _dev(x)
    M, N = dy.shape
    K = x.shape[1]
    ws = None
    if slabs and split_m > 1:
        need = _lib.lib().morec_gemm_tn_workspace_bytes(N, K, split_m) // 4
        ws = _scratch(_TN_WS if ws_cache is None else ws_cache, dy.device, need, 20 * 1024 * 1024)
    check(_lib.lib().morec_gemm_tn(_p(dy), _p(x), _p(out), M, N, K, dy.stride(0), x.stride(0), out.stride(0), code(dy.dtype),
                                   split_m, int(accumulate), _p(ws), _stream() if stream is None else stream), "morec_gemm_tn")
    return out


def gemm_tn_plan(M, N, K, dtype=torch.bfloat16, *, split_m=1, accumulate=True, workspace=True, ldy=None, ldx=None, ldc=None):
    """What ``morec_gemm_tn`` would launch for these arguments (``morec_gemm_tn_plan``, no device needed): a dict of kernel
    (``two_buffer`` / ``eight_p`` / ``eight_p_skip``), ``mchunk``, ``zs``, path (``store`` / ``rmw`` / ``atomic`` / ``slabs``) and whether
    the slab fold follows.  ``workspace``: whether one would be passed (``gemm_tn_`` passes one when ``slabs`` and ``split_m`` > 1).
    Raises, like the launch, on a refused call."""
    info = _lib.GemmTnPlanInfo()
    check(_lib.lib().morec_gemm_tn_plan(M, N, K, ldy or N, ldx or K, ldc or K, code(dtype), split_m, int(accumulate), int(bool(workspace)),
                                        C.byref(info)), "morec_gemm_tn_plan")
    return {"kernel": info.kernel_name.decode(), "mchunk": info.mchunk, "zs": info.zs, "path": info.path_name.decode(), "fold": bool(info.fold)}


def transpose(x, out=None, out_dtype=None, ld_out=None):
    """[R, C] -> [C, ld_out>=R] (pad columns, if any, are zero)."""
    _dev(x)
    R, Cc = x.shape
    ld_out = pad8(R) if ld_out is None else ld_out
    if out is None:
        alloc = torch.zeros if ld_out != R else torch.empty
        out = alloc((Cc, ld_out), device=x.device, dtype=out_dtype or x.dtype)
    check(_lib.lib().morec_transpose(_p(x), _p(out), R, Cc, x.stride(0), out.stride(0), code(x.dtype), code(out.dtype),
                                     _stream()), "morec_transpose")
    return out


def cast(x, out_dtype, out=None):
    _dev(x)
    if out is None:
        out = torch.empty_like(x, dtype=out_dtype)
    check(_lib.lib().morec_cast(_p(x), _p(out), x.numel(), code(x.dtype), code(out.dtype), _stream()), "morec_cast")
    return out


def act_bwd(dy, pre, act):
    out = torch.empty_like(dy)
    check(_lib.lib().morec_act_bwd(_p(_dev(dy)), _p(_dev(pre)), _p(out), dy.numel(), act, code(dy.dtype), _stream()),
          "morec_act_bwd")
    return out


def scaled_sum(xs, scale, out=None):
    """``scale * (xs[0] + xs[1] + xs[2])`` with fp32 arithmetic and one rounding (``morec_scaled_sum``; one to three same-shaped tensors):
    the mean over the text attributes of an item (``T/model/encoders.py:113-116``) and, with one input, the gradient each attribute's
    encoder pass receives."""
    xs = [_dev(x) for x in xs]
    assert 1 <= len(xs) <= 3 and all(x.shape == xs[0].shape and x.dtype == xs[0].dtype for x in xs)
    if out is None:
        out = torch.empty_like(xs[0])
    ptr = [_p(x) for x in xs] + [None] * (3 - len(xs))
    check(_lib.lib().morec_scaled_sum(ptr[0], ptr[1], ptr[2], _p(out), xs[0].numel(), float(scale), code(xs[0].dtype), _stream()), "morec_scaled_sum")
    return out


def colsum_(x, out, M=None, N=None, ld=None):
    """out[N] += column sums of x[M, N] (fp32 atomics)."""
    _dev(x)
    M = x.shape[0] if M is None else M
    N = x.shape[1] if N is None else N
    ld = x.stride(0) if ld is None else ld
    check(_lib.lib().morec_colsum(_p(x), _p(out), M, N, ld, code(x.dtype), _stream()), "morec_colsum")
    return out


def layernorm_fwd(x, gamma, beta, eps, *, bias=None, res=None, pos=None, pos_period=0, save_z=True, z_inplace=False,
                  p_in=0.0, seed_in=0, p_out=0.0, seed_out=0, rowscale=None, rows_per_scale=0):
    _dev(x)
    M, N = x.shape
    y = torch.empty_like(x)
    need_z = save_z and (bias is not None or res is not None or pos is not None or p_in > 0 or rowscale is not None)
    z = (x if z_inplace else torch.empty_like(x)) if need_z else None
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    check(_lib.lib().morec_layernorm_fwd(_p(x), _p(bias), _p(res), _p(pos), pos_period, _p(gamma), _p(beta), eps, _p(z),
                                         _p(y), _p(mean), _p(rstd), M, N, code(x.dtype), p_in, seed_in, p_out, seed_out,
                                         _p(rowscale), rows_per_scale, _stream()), "morec_layernorm_fwd")
    return y, (z if need_z else x), mean, rstd


class PreLN:
    """The fp32 residual stream in PRE-LayerNorm form: the stream value is ``LN(z) = (z - mean[m]) * rstd[m] * gamma + beta`` of tensors a
    LayerNorm call has saved anyway; the consumer (the next ``layernorm_fwd_res32``) recomputes it in registers, so the stream itself is never
    written or read back (``morec_layernorm_fwd_res32_pre``)."""
    __slots__ = ("z", "mean", "rstd", "gamma", "beta")

    def __init__(self, z, mean, rstd, gamma, beta):
        self.z, self.mean, self.rstd, self.gamma, self.beta = z, mean, rstd, gamma, beta

    def rows(self, idx=None, stride=None, n=None):
        """The same stream restricted to rows ``idx`` (int tensor) or ``0, stride, 2 stride, ...`` (``n`` rows)."""
        if idx is not None:
            i = idx.long()
            return PreLN(self.z.index_select(0, i), self.mean.index_select(0, i), self.rstd.index_select(0, i), self.gamma, self.beta)
        N = self.z.shape[1]
        return PreLN(self.z.view(n, stride, N)[:, 0].contiguous(), self.mean.view(n, stride)[:, 0].contiguous(),
                     self.rstd.view(n, stride)[:, 0].contiguous(), self.gamma, self.beta)

    def materialize(self):
        return ((self.z - self.mean[:, None]) * self.rstd[:, None]) * self.gamma[None, :] + self.beta[None, :]


def layernorm_fwd_res32(x16, gamma, beta, eps, *, bias=None, res=None, pos=None, pos_period=0, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0,
                        lazy_out=False):
    """LayerNorm of the autocast data flow (``morec_layernorm_fwd_res32``; ``*_res32`` compute modes): ``x16`` is the 16-bit output of the
    sub-layer's GEMM, ``res`` the fp32 residual stream (a tensor, or a ``PreLN``).  Returns (y16, y32, z32, mean, rstd): the next GEMM's
    operand, the fp32 residual stream, and what the backward needs.  ``lazy_out``: the stream is NOT written; ``y32`` is a ``PreLN`` over
    (z32, mean, rstd, gamma, beta) for the next call to recompute (needs ``p_out == 0``)."""
    _dev(x16)
    M, N = x16.shape
    z = torch.empty((M, N), device=x16.device, dtype=torch.float32)
    y16 = torch.empty_like(x16)
    mean = torch.empty(M, device=x16.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x16.device, dtype=torch.float32)
    if lazy_out and p_out > 0:
        raise ValueError("layernorm_fwd_res32(lazy_out=True) cannot carry an output dropout")
    if isinstance(res, PreLN):
        if not lazy_out or pos is not None or p_out > 0:
            raise ValueError("a PreLN residual needs lazy_out=True, no pos, no output dropout")
        check(_lib.lib().morec_layernorm_fwd_res32_pre(_p(x16), _p(bias), _p(res.z), _p(res.mean), _p(res.rstd), _p(res.gamma), _p(res.beta),
                                                       _p(gamma), _p(beta), eps, _p(z), _p(y16), _p(mean), _p(rstd), M, N, code(x16.dtype),
                                                       p_in, seed_in, _stream()), "morec_layernorm_fwd_res32_pre")
        return y16, PreLN(z, mean, rstd, gamma, beta), z, mean, rstd
    y32 = None if lazy_out else torch.empty((M, N), device=x16.device, dtype=torch.float32)
    check(_lib.lib().morec_layernorm_fwd_res32(_p(x16), _p(bias), _p(res), _p(pos), pos_period, _p(gamma), _p(beta), eps, _p(z), _p(y32), _p(y16),
                                               _p(mean), _p(rstd), M, N, code(x16.dtype), p_in, seed_in, p_out, seed_out, _stream()),
          "morec_layernorm_fwd_res32")
    return y16, (PreLN(z, mean, rstd, gamma, beta) if lazy_out else y32), z, mean, rstd


def layernorm_bwd_res32(dy16, dy32, z, mean, rstd, gamma, dgamma, dbeta, dtype16, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0, dbias=None, sub16=True):
    """Backward of ``layernorm_fwd_res32``: returns (dz32, dzd16) -- the fp32 gradient along the residual stream and the 16-bit gradient of
    the sub-layer output (None with ``sub16=False``: embedding stages, where nothing 16-bit sits below the LayerNorm)."""
    M, N = z.shape
    dz = torch.empty((M, N), device=z.device, dtype=torch.float32)
    dzd = torch.empty((M, N), device=z.device, dtype=dtype16) if sub16 else None
    check(_lib.lib().morec_layernorm_bwd_res32(_p(dy16), _p(dy32), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dz), _p(dzd), _p(dgamma), _p(dbeta),
                                               _p(dbias), M, N, code(dtype16), p_in, seed_in, p_out, seed_out, _stream()), "morec_layernorm_bwd_res32")
    return dz, dzd


def layernorm_bwd(dy_a, dy_b, z, mean, rstd, gamma, dgamma, dbeta, p_in=0.0, seed_in=0, p_out=0.0, seed_out=0, dbias=None,
                  dres=None, rowscale=None, rows_per_scale=0, sub16=True):
    """Returns (dz, dzd): dz feeds the residual branch, dzd = dropout / DropPath backward of dz feeds the sub-layer (dzd is
    dz when p_in = 0 and there is no rowscale).  ``dres``: gradient arriving at z along a pre-LN residual stream.
    An fp32 ``z`` with a 16-bit ``dy_a`` is the autocast data flow (``layernorm_fwd_res32``): dz is then the fp32 residual-stream gradient
    (``dy_b`` is fp32 too) and dzd the 16-bit sub-layer gradient (``sub16=False``: not wanted, None)."""
    _dev(dy_a)
    if z.dtype == torch.float32 and is16(dy_a.dtype):
        assert dres is None and rowscale is None and (dy_b is None or dy_b.dtype == torch.float32)
        return layernorm_bwd_res32(dy_a, dy_b, z, mean, rstd, gamma, dgamma, dbeta, dy_a.dtype, p_in, seed_in, p_out, seed_out, dbias, sub16)
    M, N = z.shape
    dz = torch.empty_like(z)
    dzd = torch.empty_like(z) if (p_in > 0 or rowscale is not None) else None
    check(_lib.lib().morec_layernorm_bwd(_p(dy_a), _p(dy_b), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dz), _p(dzd),
                                         _p(dgamma), _p(dbeta), _p(dbias), M, N, code(z.dtype), p_in, seed_in, p_out, seed_out,
                                         _p(dres), _p(rowscale), rows_per_scale, _stream()), "morec_layernorm_bwd")
    return dz, (dz if dzd is None else dzd)


class TransposeBatch:
    """dst_i = src_i^T for a fixed list of (src [R, C], dst [C, ld >= R]) pairs in ONE launch (``morec_transpose_batch``).  The
    tensors must stay where they are (the device table holds their addresses): persistent weight shadows and their W^T copies."""

    @staticmethod
    def eligible(src, dst):
        R, C_ = src.shape
        return (src.dim() == 2 and src.is_contiguous() and dst.stride(1) == 1 and src.dtype == dst.dtype and C_ % 4 == 0
                and dst.stride(0) % 4 == 0 and dst.stride(0) >= ((R + 3) & ~3) and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0)

    def __init__(self, pairs):
        assert pairs, "empty transpose batch"
        items = (_lib.TransposeItem * len(pairs))()
        tile0 = 0
        for i, (src, dst) in enumerate(pairs):
            assert TransposeBatch.eligible(src, dst), "morec_transpose_batch: shape / alignment rules (include/morec_hip.h)"
            R, C_ = src.shape
            items[i] = _lib.TransposeItem(src.data_ptr(), dst.data_ptr(), R, C_, C_, dst.stride(0), tile0, 0)
            tile0 += ((R + 63) // 64) * ((C_ + 63) // 64)
        self.n_items, self.n_tiles, self.dtype = len(pairs), tile0, pairs[0][0].dtype
        self.keep = pairs
        host = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
        self.table = host.to(pairs[0][0].device)

    def run(self):
        check(_lib.lib().morec_transpose_batch(_p(self.table), self.n_items, self.n_tiles, code(self.dtype), _stream()), "morec_transpose_batch")


def pos_grad_(dz, dpos, period):
    M, N = dz.shape
    check(_lib.lib().morec_pos_grad(_p(dz), _p(dpos), M, N, period, code(dz.dtype), _stream()), "morec_pos_grad")


# Upper bound of the SPARE rows a packed token layout may carry behind its last sequence (token counts padded up to a multiple of this by
# ``engine.token_packing_host(pad_to=...)`` so that one captured graph serves every batch of the bucket): the attention launches append
# ceil(SPARE_ROWS_MAX / 16) blocks that zero those rows of their outputs.
SPARE_ROWS_MAX = 1024


def attn_desc(n_seq, T, n_heads, dh, causal, scale, mask_value, dtype, p_drop=0.0, seed=0, cu_seqlens=None, total_rows=0):
    """``cu_seqlens``: int32 [n_seq + 1] device tensor for the unpadded token layout (the caller keeps it alive); ``total_rows``: rows of
    the packed buffers (spare rows behind the last sequence are zero-filled in ctx / dqkv)."""
    return AttnDesc(n_seq, T, n_heads, dh, int(causal), scale, mask_value, code(dtype), p_drop, seed,
                    None if cu_seqlens is None else cu_seqlens.data_ptr(), int(total_rows) if cu_seqlens is not None else 0,
                    SPARE_ROWS_MAX if (cu_seqlens is not None and total_rows) else 0)


ATTN_T_MAX = 1024      # longest sequence of morec_attn_fwd / morec_attn_bwd (the streaming kernels, csrc/attention_stream.hip)


def _attn_cap(desc):
    if desc.T > ATTN_T_MAX:
        raise _lib.MorecError(f"attention over {desc.T} positions: the kernels end at {ATTN_T_MAX} positions per sequence "
                              f"(MOREC_E_UNSUPPORTED; 256 with MOREC_ATTN_STREAM=1)")


def attn_fwd(desc, qkv, key_keep):
    _attn_cap(desc)
    _dev(qkv), _dev(key_keep)
    ctx = torch.empty((qkv.shape[0], qkv.shape[1] // 3), device=qkv.device, dtype=qkv.dtype)
    check(_lib.lib().morec_attn_fwd(C.byref(desc), _p(qkv), _p(key_keep), _p(ctx), _stream()), "morec_attn_fwd")
    return ctx


def attn_bwd(desc, qkv, key_keep, dctx, dbias=None):
    """``dbias``: fp32 [3 H] gradient buffer of the fused q|k|v bias, accumulated into (column sums of dqkv)."""
    _attn_cap(desc)
    _dev(dctx)
    dqkv = torch.empty_like(qkv)
    if dbias is None:
        check(_lib.lib().morec_attn_bwd(C.byref(desc), _p(qkv), _p(key_keep), _p(dctx), _p(dqkv), _stream()), "morec_attn_bwd")
    else:
        ws = torch.empty((desc.n_seq, qkv.shape[1]), device=qkv.device, dtype=torch.float32)
        check(_lib.lib().morec_attn_bwd_dbias(C.byref(desc), _p(qkv), _p(key_keep), _p(dctx), _p(dqkv), qkv.shape[0], _p(dbias),
                                              _p(ws), ws.numel() * 4, _stream()), "morec_attn_bwd_dbias")
    return dqkv


def bert_embed_fwd(ids32, word, pos, type0, gamma, beta, eps, T, dtype, p_out=0.0, seed_out=0):
    M = ids32.numel()
    H = word.shape[1]
    z = torch.empty((M, H), device=word.device, dtype=dtype)
    y = torch.empty_like(z)
    mean = torch.empty(M, device=word.device, dtype=torch.float32)
    rstd = torch.empty(M, device=word.device, dtype=torch.float32)
    check(_lib.lib().morec_bert_embed_fwd(_p(ids32), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), eps, _p(z),
                                          _p(y), _p(mean), _p(rstd), M, T, H, code(dtype), p_out, seed_out, _stream()),
          "morec_bert_embed_fwd")
    return y, z, mean, rstd


def bert_embed_bwd_(ids32, dz, dword, dpos, dtype0, pad_id, T, order=None):
    """``order``: int32 argsort of ``ids32`` (integer bookkeeping done by the caller) -- enables the run-length scatter."""
    M, H = dz.shape
    check(_lib.lib().morec_bert_embed_bwd(_p(ids32), _p(dz), _p(dword), _p(dpos), _p(dtype0), pad_id, M, T, H,
                                          code(dz.dtype), _p(order), _stream()), "morec_bert_embed_bwd")


def roberta_pos_ids(ids32, pad_id, T, n_pos):
    """Pad-relative position ids of ``ids32`` (int32 [n_seq * T]): ``(pos_ids, perm, cnt)`` int32 device tensors (``morec_roberta_pos_ids``)."""
    _dev(ids32)
    M = ids32.numel()
    n_seq = M // T if T > 0 else 0
    pos_ids = torch.empty(M, device=ids32.device, dtype=torch.int32)
    perm = torch.empty(M, device=ids32.device, dtype=torch.int32)
    cnt = torch.empty(max(n_seq, 1), device=ids32.device, dtype=torch.int32)
    check(_lib.lib().morec_roberta_pos_ids(_p(ids32), pad_id, n_seq, T, n_pos, _p(pos_ids), _p(perm), _p(cnt), _stream()),
          "morec_roberta_pos_ids")
    return pos_ids, perm, cnt


def bert_embed_fwd_pos(ids32, pos_ids, word, pos, type0, gamma, beta, eps, T, dtype, p_out=0.0, seed_out=0):
    """``bert_embed_fwd`` with the position row of every token given by ``pos_ids`` (int32 [M])."""
    M = ids32.numel()
    H = word.shape[1]
    z = torch.empty((M, H), device=word.device, dtype=dtype)
    y = torch.empty_like(z)
    mean = torch.empty(M, device=word.device, dtype=torch.float32)
    rstd = torch.empty(M, device=word.device, dtype=torch.float32)
    check(_lib.lib().morec_bert_embed_fwd_pos(_p(ids32), _p(pos_ids), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), eps, _p(z),
                                              _p(y), _p(mean), _p(rstd), M, T, H, code(dtype), p_out, seed_out, _stream()),
          "morec_bert_embed_fwd_pos")
    return y, z, mean, rstd


def roberta_embed_bwd_(ids32, dz, dword, dpos, dtype0, pad_id, T, perm, cnt, pos_pad, order=None):
    """``bert_embed_bwd_`` under the pad-relative position rule: ``perm`` / ``cnt`` from ``roberta_pos_ids``; ``dpos`` is the whole table's gradient."""
    M, H = dz.shape
    check(_lib.lib().morec_roberta_embed_bwd(_p(ids32), _p(dz), _p(dword), _p(dpos), _p(dtype0), pad_id, M, T, H, code(dz.dtype),
                                             _p(order), _p(perm), _p(cnt), pos_pad, dpos.shape[0], _stream()), "morec_roberta_embed_bwd")


def mask_pos_ids(mask32, T, offset, n_pos):
    """Position ids counted from the attention mask (int32 [n_seq * T], nonzero = kept): ``(pos_ids, perm, cnt)`` int32 device tensors
    (``morec_mask_pos_ids``); ``perm`` / ``cnt`` are what ``roberta_embed_bwd_`` walks with ``pos_pad = offset - 1``."""
    _dev(mask32)
    M = mask32.numel()
    n_seq = M // T if T > 0 else 0
    pos_ids = torch.empty(M, device=mask32.device, dtype=torch.int32)
    perm = torch.empty(M, device=mask32.device, dtype=torch.int32)
    cnt = torch.empty(max(n_seq, 1), device=mask32.device, dtype=torch.int32)
    check(_lib.lib().morec_mask_pos_ids(_p(mask32), n_seq, T, offset, n_pos, _p(pos_ids), _p(perm), _p(cnt), _stream()),
          "morec_mask_pos_ids")
    return pos_ids, perm, cnt


def opt_embed_fwd(ids32, pos_ids, word, pos, dtype):
    """``round(word[ids] + pos[pos_ids])`` [M, H] in ``dtype`` (``morec_opt_embed_fwd``: no LayerNorm, token type or dropout)."""
    _dev(word), _dev(pos)
    M, H = ids32.numel(), word.shape[1]
    out = torch.empty((M, H), device=word.device, dtype=dtype)
    check(_lib.lib().morec_opt_embed_fwd(_p(ids32), _p(pos_ids), _p(word), _p(pos), _p(out), M, H, code(dtype), _stream()),
          "morec_opt_embed_fwd")
    return out


def masked_mean_fwd(x, keep, n_seq, T, cu=None):
    """Mean of the kept rows of every title ([n_seq, H], ``morec_masked_mean_fwd``): ``keep`` fp32 per row of ``x``; ``cu`` int32
    [n_seq + 1] for the packed layout, None for the padded one ([n_seq * T] rows)."""
    _dev(x), _dev(keep)
    H = x.shape[1]
    out = torch.empty((n_seq, H), device=x.device, dtype=x.dtype)
    check(_lib.lib().morec_masked_mean_fwd(_p(x), _p(keep), _p(cu), _p(out), n_seq, T, H, code(x.dtype), _stream()), "morec_masked_mean_fwd")
    return out


def masked_mean_bwd(g, keep, n_seq, T, rows, cu=None):
    """Backward of ``masked_mean_fwd``: [rows, H] with ``g[n] / count`` on the kept rows of title n and zeros on the others."""
    _dev(g), _dev(keep)
    H = g.shape[1]
    dx = torch.empty((rows, H), device=g.device, dtype=g.dtype)
    check(_lib.lib().morec_masked_mean_bwd(_p(g), _p(keep), _p(cu), _p(dx), n_seq, T, H, code(g.dtype), _stream()), "morec_masked_mean_bwd")
    return dx


def gather_rows(table, idx32, dtype):
    R, D = idx32.numel(), table.shape[1]
    out = torch.empty((R, D), device=table.device, dtype=dtype)
    check(_lib.lib().morec_gather_rows(_p(table), _p(idx32), _p(out), R, D, code(dtype), _stream()), "morec_gather_rows")
    return out


def scatter_add_rows_(d, idx32, dtable, pad_id):
    R, D = d.shape
    check(_lib.lib().morec_scatter_add_rows(_p(_dev(d)), _p(idx32), _p(dtable), R, D, pad_id, code(d.dtype), _stream()),
          "morec_scatter_add_rows")


def fuse_add_fwd(table, idx32, content):
    """``table[idx] + content`` in content's dtype: one fp32 add, one rounding (``morec_fuse_add_fwd``; the ADD fusion tower)."""
    _dev(table), _dev(content)
    R, D = content.shape
    out = torch.empty_like(content)
    check(_lib.lib().morec_fuse_add_fwd(_p(table), _p(idx32), _p(content), _p(out), R, D, code(content.dtype), _stream()), "morec_fuse_add_fwd")
    return out


def fuse_cat_fwd(table, idx32, content, p=0.0, seed=0):
    """``drop(cat([table[idx], content], 1))`` [R, 2D] in content's dtype, one dropout stream over the result (``morec_fuse_cat_fwd``)."""
    _dev(table), _dev(content)
    R, D = content.shape
    a = torch.empty((R, 2 * D), device=content.device, dtype=content.dtype)
    check(_lib.lib().morec_fuse_cat_fwd(_p(table), _p(idx32), _p(content), _p(a), R, D, code(content.dtype), float(p), int(seed), _stream()),
          "morec_fuse_cat_fwd")
    return a


def fuse_cat_bwd(dA, idx32, d_table, pad_id=0, p=0.0, seed=0):
    """Backward of ``fuse_cat_fwd`` with the forward's (p, seed): returns the content gradient [R, D]; the id half of ``dA`` [R, 2D] is
    scatter-ADDED into the fp32 ``d_table`` (rows ``pad_id`` skipped) (``morec_fuse_cat_bwd``)."""
    _dev(dA), _dev(d_table)
    R, D = dA.shape[0], dA.shape[1] // 2
    assert d_table.dtype == torch.float32 and d_table.shape[1] == D
    d_content = torch.empty((R, D), device=dA.device, dtype=dA.dtype)
    check(_lib.lib().morec_fuse_cat_bwd(_p(dA), _p(idx32), _p(d_content), _p(d_table), R, D, pad_id, code(dA.dtype), float(p), int(seed),
                                        _stream()), "morec_fuse_cat_bwd")
    return d_content


def dropout_apply_(x, p, seed):
    """In place: ``x = keep ? x * inv_keep : 0`` with the counter-based stream of (p, seed) over x's elements (``morec_dropout_apply``)."""
    _dev(x)
    check(_lib.lib().morec_dropout_apply(_p(x), _p(x), x.numel(), float(p), int(seed), code(x.dtype), _stream()), "morec_dropout_apply")
    return x


def indexed_rows_copy(src, out, in_idx=None, out_idx=None, R=None):
    """out[out_idx[r]] = src[in_idx[r]] (int32 device index vectors; None = identity)."""
    _dev(src), _dev(out)
    R = (in_idx if in_idx is not None else out_idx).numel() if R is None else R
    check(_lib.lib().morec_indexed_rows_copy(_p(src), _p(out), _p(in_idx), _p(out_idx), R, src.shape[1], code(src.dtype), _stream()),
          "morec_indexed_rows_copy")
    return out


def featproj_supported(R, Kw, D, dtype) -> bool:
    """Does the first layer of the two-stage tower run as ``featproj_fwd`` for this shape (``morec_featproj_supported``: 16-bit,
    ``Kw % 8 == D % 8 == 0``, the knob ``MOREC_FEATPROJ`` / ``set_featproj`` and, when that is automatic, ``R Kw D <= 2^29``: the sizes at
    which one launch measured faster than two, ``profiles/two_stage_step.txt``)?  Otherwise it is ``featproj_composed``."""
    return is16(dtype) and bool(_lib.lib().morec_featproj_supported(int(R), int(Kw), int(D), code(dtype)))


def set_featproj(mode: int):
    """The knob of ``featproj_supported``: 0 automatic | 1 never | 2 wherever the rules allow (``morec_tuning_set("featproj", mode)``)."""
    check(_lib.lib().morec_tuning_set(b"featproj", int(mode)), "morec_tuning_set(featproj)")


def featproj_fwd(table, idx32, w, bias=None, *, need_pre=False, out=None, pre=None, R=None):
    """``GELU(table[idx] @ w^T + bias)`` in ONE launch (``morec_featproj_fwd``): ``table`` [n_rows, Kw] and ``w`` [D, Kw] in the same 16-bit
    dtype, ``idx32`` int32 [R] (clamped into the table by the kernel), ``bias`` fp32 [D] or None.  Returns ``(out, pre)``; ``pre`` (the
    pre-activation, for the backward) is None unless ``need_pre`` or a buffer is given.  Rows past ``R`` of a given buffer stay untouched."""
    _dev(table), _dev(w)
    R = idx32.numel() if R is None else R
    n_rows, Kw = table.shape
    D = w.shape[0]
    assert table.is_contiguous() and w.is_contiguous() and idx32.is_contiguous() and idx32.dtype == torch.int32
    assert w.dtype == table.dtype and w.shape[1] == Kw, "featproj: table and weight must share the 16-bit dtype and the feature width"
    if out is None:
        out = torch.empty((R, D), device=table.device, dtype=table.dtype)
    if pre is None and need_pre:
        pre = torch.empty((R, D), device=table.device, dtype=table.dtype)
    check(_lib.lib().morec_featproj_fwd(_p(table), _p(idx32), _p(w), _p(bias), _p(out), _p(pre), R, n_rows, Kw, D, code(table.dtype),
                                        _stream()), "morec_featproj_fwd")
    return out, pre


def featproj_composed(table, idx32, w, bias=None, *, need_pre=False):
    """The same layer as two launches, in any dtype: ``indexed_rows_copy`` of the looked-up rows, then ``gemm_nt`` with the bias + GELU
    epilogue.  Returns ``(out, pre, x)`` with ``x`` the gathered rows [R, Kw] (the weight gradient's operand)."""
    R = idx32.numel()
    x = indexed_rows_copy(table, torch.empty((R, table.shape[1]), device=table.device, dtype=table.dtype), in_idx=idx32)
    pre = torch.empty((R, w.shape[0]), device=table.device, dtype=table.dtype) if need_pre else None
    out = gemm_nt(x, w, bias=bias, act=ACT_GELU, aux_out=pre)
    return out, pre, x


FUSE_KINDS = {"add": 0, "cat": 1}      # MOREC_FUSE_ADD / MOREC_FUSE_CAT


def featfuse_supported(R, Kw, D, dtype) -> bool:
    """Does the chain lookup -> projection -> GELU -> ID fusion of the id-two-stage tower run as ``featfuse_fwd`` for this shape
    (``morec_featfuse_supported``: 16-bit, ``Kw % 8 == D % 8 == 0``, the knob ``MOREC_FEATFUSE`` / ``set_featfuse`` and, when that is
    automatic, ``R Kw D <= 3 * 2^28``: the sizes at which one launch measured faster, ``profiles/id_two_stage_step.txt``)?  Otherwise it is featproj + ``fuse_add_fwd`` / ``fuse_cat_fwd``."""
    return is16(dtype) and bool(_lib.lib().morec_featfuse_supported(int(R), int(Kw), int(D), code(dtype)))


def set_featfuse(mode: int):
    """The knob of ``featfuse_supported``: 0 automatic | 1 never | 2 wherever the rules allow (``morec_tuning_set("featfuse", mode)``)."""
    check(_lib.lib().morec_tuning_set(b"featfuse", int(mode)), "morec_tuning_set(featfuse)")


def featfuse_fwd(table, idx32, w, bias, id_table, kind, p=0.0, seed=0, *, need_pre=False, out=None, pre=None, R=None):
    """``y = GELU(table[idx] @ w^T + bias)`` fused with the id rows in ONE launch (``morec_featfuse_fwd``): ``kind`` "add" ->
    ``id_table[idx] + y`` [R, D]; "cat" -> ``drop(cat([id_table[idx], y], 1))`` [R, 2D] with ``fuse_cat_fwd``'s stream of (p, seed).
    ``table`` [n_rows, Kw] and ``w`` [D, Kw] in the same 16-bit dtype, ``id_table`` fp32 [n_rows, D], ``idx32`` int32 [R] (clamped into
    the tables by the kernel), ``bias`` fp32 [D] or None.  Returns ``(out, pre)`` with the bits of ``featproj_fwd`` + ``fuse_*_fwd``;
    ``pre`` is None unless ``need_pre`` or a buffer is given.  Rows past ``R`` of a given buffer stay untouched."""
    _dev(table), _dev(w), _dev(id_table)
    R = idx32.numel() if R is None else R
    n_rows, Kw = table.shape
    D = w.shape[0]
    assert table.is_contiguous() and w.is_contiguous() and id_table.is_contiguous() and idx32.is_contiguous() and idx32.dtype == torch.int32
    assert w.dtype == table.dtype and w.shape[1] == Kw, "featfuse: table and weight must share the 16-bit dtype and the feature width"
    assert id_table.dtype == torch.float32 and tuple(id_table.shape) == (n_rows, D), "featfuse: the id table must be fp32 [n_rows, D]"
    if out is None:
        out = torch.empty((R, D if kind == "add" else 2 * D), device=table.device, dtype=table.dtype)
    if pre is None and need_pre:
        pre = torch.empty((R, D), device=table.device, dtype=table.dtype)
    check(_lib.lib().morec_featfuse_fwd(_p(table), _p(idx32), _p(w), _p(bias), _p(id_table), _p(out), _p(pre), R, n_rows, Kw, D,
                                        code(table.dtype), FUSE_KINDS[kind], float(p), int(seed), _stream()), "morec_featfuse_fwd")
    return out, pre


def strided_rows_copy(src, out, R, D, in_stride, out_stride):
    check(_lib.lib().morec_strided_rows_copy(_p(src), _p(out), R, D, in_stride, out_stride, code(src.dtype), _stream()),
          "morec_strided_rows_copy")
    return out


# ---------------------------------------------------------------------------------------------------------
def ce_desc(B, S, D, Nc, col_offset, dtype, dE_fp32=False, ws_from_fwd=False):
    """``ws_from_fwd`` (backward): the workspace is the untouched one of the matching forward call -- its tables are reused."""
    return CeDesc(B, S, D, Nc, col_offset, code(dtype), int(bool(dE_fp32)), int(bool(ws_from_fwd)))


def ce_workspace(desc, device):
    n = _lib.lib().morec_inbatch_ce_workspace_bytes(C.byref(desc))
    return torch.empty(n, device=device, dtype=torch.uint8)


def inbatch_ce_fwd(desc, P, E, row_ids, col_ids, col_logpop, col_valid, row_valid, ws):
    Nr = desc.B * desc.S
    lse = torch.empty(Nr, device=P.device, dtype=torch.float32)
    row_loss = torch.empty(Nr, device=P.device, dtype=torch.float32)
    loss_sum = torch.zeros(1, device=P.device, dtype=torch.float32)
    check(_lib.lib().morec_inbatch_ce_fwd(C.byref(desc), _p(_dev(P)), _p(_dev(E)), _p(row_ids), _p(col_ids), _p(col_logpop),
                                          _p(col_valid), _p(row_valid), _p(lse), _p(row_loss), _p(loss_sum), _p(ws),
                                          _stream()), "morec_inbatch_ce_fwd")
    return loss_sum, lse, row_loss


def inbatch_ce_bwd(desc, P, E, row_ids, col_ids, col_logpop, col_valid, row_valid, lse, gscale_dev, gscale, ws):
    """Returns (dP, dE); dE is fp32 when the descriptor asks for it (``dE_fp32``: the pooled step reduces it over ranks in fp32)."""
    dP = torch.empty_like(P)
    dE = torch.empty_like(E, dtype=torch.float32) if desc.dE_fp32 else torch.empty_like(E)
    check(_lib.lib().morec_inbatch_ce_bwd(C.byref(desc), _p(P), _p(E), _p(row_ids), _p(col_ids), _p(col_logpop),
                                          _p(col_valid), _p(row_valid), _p(lse), _p(gscale_dev), gscale, _p(dP), _p(dE),
                                          _p(ws), _stream()), "morec_inbatch_ce_bwd")
    return dP, dE


def bce_fwd(P, E, row_valid, B, S):
    """BCE variant scoring (``morec_bce_fwd``): returns (loss_sum fp32[1], scores fp32[2, B*S])."""
    _dev(P), _dev(E)
    scores = torch.empty((2, B * S), device=P.device, dtype=torch.float32)
    loss_sum = torch.zeros(1, device=P.device, dtype=torch.float32)
    check(_lib.lib().morec_bce_fwd(_p(P), _p(E), _p(row_valid), _p(scores), _p(loss_sum), B, S, P.shape[-1], code(P.dtype), _stream()),
          "morec_bce_fwd")
    return loss_sum, scores


def bce_bwd(P, E, row_valid, scores, gscale_dev, B, S):
    dP, dE = torch.empty_like(P), torch.empty_like(E)
    check(_lib.lib().morec_bce_bwd(_p(P), _p(E), _p(row_valid), _p(scores), _p(gscale_dev), _p(dP), _p(dE), B, S, P.shape[-1],
                                   code(P.dtype), _stream()), "morec_bce_bwd")
    return dP, dE


def dssm_bce_fwd(U, E, labels, B, n1, *, out=None):
    """DSSM scoring loss (``morec_dssm_bce_fwd``): U [B, D], E [B * n1, D], ``labels`` fp32 [B * n1] or None for [1, 0, ..., 0] per user.
    Returns fp32 ``(scores [B * n1], terms [B * n1], loss_sum [1])``; ``out`` = caller-provided tensors in that order (every element is
    written, so ``torch.empty`` is enough)."""
    _dev(U), _dev(E)
    R, D = B * n1, U.shape[-1]
    if tuple(U.shape) != (B, D) or tuple(E.shape) != (R, D) or E.dtype != U.dtype:
        raise _lib.MorecError(f"dssm_bce_fwd: U {tuple(U.shape)} {U.dtype} / E {tuple(E.shape)} {E.dtype} do not fit B = {B}, n1 = {n1}")
    if labels is not None and (_dev(labels).dtype != torch.float32 or labels.numel() != R):
        raise _lib.MorecError(f"dssm_bce_fwd: labels must be fp32 with {R} elements")
    if out is None:
        out = (torch.empty(R, device=U.device, dtype=torch.float32), torch.empty(R, device=U.device, dtype=torch.float32),
               torch.empty(1, device=U.device, dtype=torch.float32))
    scores, terms, loss_sum = out
    for t, n in ((scores, R), (terms, R), (loss_sum, 1)):
        if _dev(t).dtype != torch.float32 or t.numel() != n:
            raise _lib.MorecError("dssm_bce_fwd: out = (scores [R], terms [R], loss_sum [1]) in fp32")
    check(_lib.lib().morec_dssm_bce_fwd(_p(U), _p(E), _p(labels), _p(scores), _p(terms), _p(loss_sum), B, n1, D, code(U.dtype), _stream()),
          "morec_dssm_bce_fwd")
    return scores, terms, loss_sum


def dssm_bce_bwd(U, E, labels, scores, gscale_dev, B, n1, *, out=None):
    """``morec_dssm_bce_bwd``: returns ``(dU, dE)`` in the dtype of U / E; ``gscale_dev`` fp32 [1] on the device (dloss / R); ``out`` =
    caller-provided ``(dU, dE)``."""
    _dev(U), _dev(E), _dev(scores), _dev(gscale_dev)
    if labels is not None and (_dev(labels).dtype != torch.float32 or labels.numel() != B * n1):
        raise _lib.MorecError(f"dssm_bce_bwd: labels must be fp32 with {B * n1} elements")
    if gscale_dev.dtype != torch.float32 or gscale_dev.numel() < 1:
        raise _lib.MorecError("dssm_bce_bwd: gscale_dev must be an fp32 device tensor")
    if out is None:
        out = (torch.empty_like(U), torch.empty_like(E))
    dU, dE = out
    if _dev(dU).shape != U.shape or _dev(dE).shape != E.shape or dU.dtype != U.dtype or dE.dtype != E.dtype or E.dtype != U.dtype:
        raise _lib.MorecError("dssm_bce_bwd: out = (dU like U, dE like E)")
    if tuple(U.shape) != (B, U.shape[-1]) or E.shape[0] != B * n1 or scores.numel() != B * n1 or scores.dtype != torch.float32:
        raise _lib.MorecError(f"dssm_bce_bwd: shapes do not fit B = {B}, n1 = {n1}")
    check(_lib.lib().morec_dssm_bce_bwd(_p(U), _p(E), _p(labels), _p(scores), _p(gscale_dev), _p(dU), _p(dE), B, n1, U.shape[-1],
                                        code(U.dtype), _stream()), "morec_dssm_bce_bwd")
    return dU, dE


def adamw_(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    check(_lib.lib().morec_adamw(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), param.numel(), lr, beta1,
                                 beta2, eps, wd, step, grad_scale, _stream()), "morec_adamw")


_SEED_SOURCE_OWNER = None      # id() of the StepParams whose seed word the library currently reads (process-wide, like the knob itself)


class StepParams:
    """The device-resident step block (``morec_step_params``: step count, bias corrections, loss scale, overflow flag): what the
    reference keeps in ``GradScaler()`` + AdamW's ``step`` (``T/run.py:210,243-247``).  ``init_scale`` 1.0 = no loss scaling."""

    def __init__(self, device, init_scale=1.0, step=0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, dynamic=True):
        self.buf = torch.zeros(64, device=device, dtype=torch.uint8)
        self.f32 = self.buf.view(torch.float32)       # [16]: loss_scale at index 4
        self.i32 = self.buf.view(torch.int32)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.dynamic = bool(dynamic)
        check(_lib.lib().morec_step_params_init(_p(self.buf), float(init_scale), int(step), _stream()), "morec_step_params_init")

    @property
    def loss_scale_dev(self):
        """fp32 [1] view of the scale the next backward pass multiplies the loss gradient with (no host read)."""
        return self.f32[4:5]

    def use_as_seed_source(self, on: bool = True):
        """Register (or clear) this block's ``drop_seed_mixed`` word as the library's dropout seed source (``morec_dropout_seed_source``):
        every ``decide_`` then changes the masks of the following launches, whatever their seed arguments -- what a replayed graph needs."""
        global _SEED_SOURCE_OWNER
        if not on and _SEED_SOURCE_OWNER not in (None, id(self)):
            return                                   # another block is registered: leave it alone
        ptr = C.c_void_p(self.buf.data_ptr() + _lib.StepParams.drop_seed_mixed.offset) if on else None
        check(_lib.lib().morec_dropout_seed_source(ptr), "morec_dropout_seed_source")
        _SEED_SOURCE_OWNER = id(self) if on else None

    def __del__(self):      # the library must not keep a pointer into a block that is going away
        try:
            if _SEED_SOURCE_OWNER == id(self):
                self.use_as_seed_source(False)
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def check_finite_(self, grad):
        check(_lib.lib().morec_grad_check_finite(_p(grad), grad.numel(), _p(self.buf), _stream()), "morec_grad_check_finite")

    def decide_(self, beta1, beta2):
        check(_lib.lib().morec_step_decide(_p(self.buf), beta1, beta2, self.growth_factor, self.backoff_factor, self.growth_interval,
                                           int(self.dynamic), _stream()), "morec_step_decide")

    # ---- global-norm clipping + LR schedule (morec_grad_norm_check / morec_step_decide_ex) -------------------------------------------
    @staticmethod
    def norm_slots(n: int) -> int:
        """Slots of the partials buffer an arena of ``n`` elements fills (a function of ``n`` alone)."""
        return int(_lib.lib().morec_grad_norm_blocks(int(n)))

    def reserve_partials(self, n_slots: int):
        """fp32 ``[n_slots + 1]`` on the block's device: the per-block sums of squares of a step, and ``grad_norm`` in the tail slot."""
        self.partials = torch.zeros(int(n_slots) + 1, device=self.buf.device, dtype=torch.float32)
        return self.partials

    def norm_check_(self, grad, slot: int):
        """``check_finite_`` plus this arena's share of the sum of squares of the UNSCALED gradients into ``partials[slot : slot + norm_slots(n)]``."""
        pt = getattr(self, "partials", None)
        if pt is None:
            raise _lib.MorecError("norm_check_ before reserve_partials")
        check(_lib.lib().morec_grad_norm_check(_p(grad), grad.numel(), _p(self.buf), _p(pt), int(slot), pt.numel() - 1, _stream()),
              "morec_grad_norm_check")

    def decide_ex_(self, beta1, beta2, n_partials: int = 0, max_norm: float = 0.0, schedule=None):
        """``decide_`` with the gradient norm folded from ``partials[:n_partials]`` in front of the verdict, and the clip coefficient
        (``max_norm`` > 0) / LR multiplier (``schedule``: ``lr_schedule.LrSchedule``) of the step behind it."""
        pt = getattr(self, "partials", None)
        if n_partials and (pt is None or n_partials > pt.numel() - 1):
            raise _lib.MorecError(f"decide_ex_: {n_partials} partials, buffer holds {0 if pt is None else pt.numel() - 1}")
        sched = schedule.c_struct() if schedule is not None else None
        check(_lib.lib().morec_step_decide_ex(_p(self.buf), beta1, beta2, self.growth_factor, self.backoff_factor, self.growth_interval,
                                              int(self.dynamic), _p(pt) if n_partials else None, int(n_partials), float(max_norm),
                                              C.byref(sched) if sched is not None else None,
                                              C.c_void_p(pt.data_ptr() + 4 * (pt.numel() - 1)) if n_partials else None, _stream()),
              "morec_step_decide_ex")

    def grad_norm(self) -> float:
        """Global gradient norm the last ``decide_ex_`` folded (synchronises: logging only)."""
        return float(self.partials[-1].item())

    def clip_coef(self) -> float:
        h = self.host()
        return float(h.clip_coef) if h.ctl_flags & _lib.SP_CLIP else 1.0

    def lr_mult(self) -> float:
        h = self.host()
        return float(h.lr_mult) if h.ctl_flags & _lib.SP_LR_MULT else 1.0

    def host(self):
        """Host copy of the block (synchronises): for logging / checkpoints, never inside the step."""
        raw = bytes(self.buf.cpu().numpy().tobytes())
        return _lib.StepParams.from_buffer_copy(raw)


def adamw_sp_(param, grad, exp_avg, exp_avg_sq, shadow, lr, beta1, beta2, eps, wd, sp: StepParams):
    """``morec_adamw_sp``: AdamW with step count / bias corrections / 1 / loss-scale read from the device block; a no-op when the
    step was marked for skipping (non-finite gradient)."""
    check(_lib.lib().morec_adamw_sp(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(shadow), code(shadow.dtype) if shadow is not None else BF16,
                                    param.numel(), lr, beta1, beta2, eps, wd, _p(sp.buf), _stream()), "morec_adamw_sp")


def eval_rank(prec, item_emb, hist32, target32):
    U, D = prec.shape
    rank = torch.empty(U, device=prec.device, dtype=torch.int32)
    ts = torch.empty(U, device=prec.device, dtype=torch.float32)
    check(_lib.lib().morec_eval_rank(_p(_dev(prec)), _p(_dev(item_emb)), _p(_dev(hist32)), hist32.shape[1], _p(target32),
                                     _p(rank), _p(ts), U, item_emb.shape[0], D, _stream()), "morec_eval_rank")
    return rank


def eval_rank_cand(prec, item_emb, hist32, cand_emb, cand_idx32):
    """``morec_eval_rank_cand``: 1-based rank of each user's candidate ``cand_emb[cand_idx32[u]]`` (a vector outside the catalogue)
    among the catalogue items 1 .. item_num outside the user's history (``special.py``'s new-item evaluation)."""
    U, D = prec.shape
    rank = torch.empty(U, device=prec.device, dtype=torch.int32)
    ts = torch.empty(U, device=prec.device, dtype=torch.float32)
    check(_lib.lib().morec_eval_rank_cand(_p(_dev(prec)), _p(_dev(item_emb)), _p(_dev(hist32)), hist32.shape[1], _p(_dev(cand_emb)),
                                          cand_emb.shape[0], _p(_dev(cand_idx32)), _p(rank), _p(ts), U, item_emb.shape[0], D,
                                          _stream()), "morec_eval_rank_cand")
    return rank


def eval_topk_max_k() -> int:
    """Largest ``k`` of ``eval_topk`` (``morec_eval_topk_max_k``; host code, no device needed)."""
    return int(_lib.lib().morec_eval_topk_max_k())


def eval_topk(prec, item_emb, hist32, k, strips=0):
    """``morec_eval_topk``: for every user the ``k`` best catalogue items 1 .. item_num outside the user's history ``hist32`` (int32
    [U, Hmax] padded with -1, or ``None``: nothing masked), score descending, item id ascending among equal scores -> ``(ids int32
    [U, k], scores float32 [U, k])``; slots past the eligible items hold -1 / -inf.  ``strips`` cuts the catalogue into column strips
    (0 = automatic) and does not change the result.  The workspace comes from torch's caching allocator: a second call of the same
    shape allocates nothing on the device."""
    U, D = prec.shape
    k, strips = int(k), int(strips)
    if k > eval_topk_max_k():
        raise _lib.MorecError(f"eval_topk: k = {k} is above the kernel's cap of {eval_topk_max_k()}")
    h = _lib.lib()
    hmax = 0 if hist32 is None else hist32.shape[1]
    if hist32 is not None and hist32.dtype != torch.int32:
        raise _lib.MorecError("eval_topk: the history must be int32")
    ws_bytes = int(h.morec_eval_topk_ws_bytes(U, item_emb.shape[0], k, strips))
    ids = torch.empty((U, max(k, 0)), device=prec.device, dtype=torch.int32)
    scores = torch.empty((U, max(k, 0)), device=prec.device, dtype=torch.float32)
    ws = torch.empty(max(ws_bytes, 8), device=prec.device, dtype=torch.uint8)
    check(h.morec_eval_topk(_p(_dev(prec)), _p(_dev(item_emb)), _p(None if hist32 is None else _dev(hist32)), hmax, k, strips, _p(ids),
                            _p(scores), _p(ws), ws_bytes, U, item_emb.shape[0], D, _stream()), "morec_eval_topk")
    return ids, scores


# ---------------------------------------------------------------------------------------------------------
# Swin vision tower
# ---------------------------------------------------------------------------------------------------------
def swin_attn_desc(n_img, H, W, window, shift, heads, dh, dtype):
    return SwinAttnDesc(n_img, H, W, window, shift, heads, dh, float(dh) ** -0.5, code(dtype))


def swin_attn_fwd(desc, qkv, bias_t):
    _dev(qkv), _dev(bias_t)
    ctx = torch.empty((qkv.shape[0], qkv.shape[1] // 3), device=qkv.device, dtype=qkv.dtype)
    check(_lib.lib().morec_swin_attn_fwd(C.byref(desc), _p(qkv), _p(bias_t), _p(ctx), _stream()), "morec_swin_attn_fwd")
    return ctx


def swin_attn_bwd(desc, qkv, bias_t, ctx, dctx, dbias_t=None, dbqkv=None):
    """``dbqkv``: fp32 [3 C] gradient buffer of the fused q|k|v bias, accumulated into (column sums of dqkv)."""
    _dev(dctx), _dev(ctx)
    dqkv = torch.empty_like(qkv)
    if dbqkv is None:
        check(_lib.lib().morec_swin_attn_bwd(C.byref(desc), _p(qkv), _p(bias_t), _p(ctx), _p(dctx), _p(dqkv), _p(dbias_t),
                                             _stream()), "morec_swin_attn_bwd")
    else:
        n_win = desc.n_img * (desc.H // desc.window) * (desc.W // desc.window)
        ws = torch.empty(((n_win + 3) // 4 * 4, qkv.shape[1]), device=qkv.device, dtype=torch.float32)     # one row per wavefront slot (4 per block)
        check(_lib.lib().morec_swin_attn_bwd_dbias(C.byref(desc), _p(qkv), _p(bias_t), _p(ctx), _p(dctx), _p(dqkv), _p(dbias_t),
                                                   _p(dbqkv), _p(ws), ws.numel() * 4, _stream()), "morec_swin_attn_bwd_dbias")
    return dqkv


def swin_bias_expand(table, window):
    heads = table.shape[1]
    out = torch.empty((heads, window ** 2, window ** 2), device=table.device, dtype=torch.float32)
    check(_lib.lib().morec_swin_bias_expand(_p(_dev(table)), _p(out), window, heads, _stream()), "morec_swin_bias_expand")
    return out


def swin_bias_reduce_(dbias_t, dtable, window):
    check(_lib.lib().morec_swin_bias_reduce(_p(_dev(dbias_t)), _p(dtable), window, dtable.shape[1], _stream()),
          "morec_swin_bias_reduce")


def swin_patchify(pixels, patch, dtype):
    _dev(pixels)
    if pixels.dtype != torch.float32:
        raise _lib.MorecError("pixels must be fp32 NCHW")
    n, c, R, _ = pixels.shape
    G = R // patch
    out = torch.empty((n * G * G, c * patch * patch), device=pixels.device, dtype=dtype)
    check(_lib.lib().morec_swin_patchify(_p(pixels), _p(out), n, c, R, patch, out.stride(0), code(dtype), _stream()),
          "morec_swin_patchify")
    return out


# ---------------------------------------------------------------------------------------------------------
# uint8 image fronts (csrc/image_front.hip): decoded images in batch order, or -- with ``ids`` -- the rows ``ids[k]`` of an image
# catalogue that stays on the device
# ---------------------------------------------------------------------------------------------------------
def check_catalogue_ids(ids, n_rows):
    """Host-side ids (numpy array or CPU tensor) outside ``[0, n_rows)`` raise here, before anything is uploaded: the kernels only clamp."""
    if isinstance(ids, torch.Tensor):
        if ids.is_cuda or ids.numel() == 0:
            return
        lo, hi = int(ids.min()), int(ids.max())
    else:
        import numpy as np
        a = np.asarray(ids)
        if a.size == 0:
            return
        lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= n_rows:
        raise _lib.MorecError(f"image ids outside the catalogue: [{lo}, {hi}] against {n_rows} rows")


def catalogue_ids(catalogue, ids):
    """(uint8 catalogue [n_rows, ...] on the device, ids of any shape: numpy, CPU or device tensor) -> contiguous int32 ids on the
    catalogue's device, flat.  Ids that come from the host are range-checked there."""
    _dev(catalogue)
    if catalogue.dtype != torch.uint8 or catalogue.dim() != 4 or not catalogue.is_contiguous():
        raise _lib.MorecError("expected a contiguous uint8 [n_rows, H, W, C] catalogue")
    if not isinstance(ids, torch.Tensor):
        import numpy as np
        ids = torch.from_numpy(np.ascontiguousarray(ids))
    check_catalogue_ids(ids, catalogue.shape[0])
    return ids.to(device=catalogue.device, dtype=torch.int32).reshape(-1).contiguous()


def swin_patchify_u8(pixels, patch, dtype, mean=0.5, std=0.5, out=None, ids=None):
    """uint8 [n, R, R, 3] decoded images -> normalised patch rows (ToTensor + Normalize(0.5, 0.5), V/data_utils/dataset.py:69-73).
    ``ids``: ``pixels`` is the image catalogue, image k of the batch its row ``ids[k]`` (``swin_patchify_u8(pixels[ids], ...)`` without the gather).
    ``out``: a caller-owned [n G G, 3 patch^2] buffer of ``dtype`` (the double-buffered input feed, ``data_utils.images.DeviceImageFeed``)."""
    _dev(pixels)
    if pixels.dtype != torch.uint8:
        raise _lib.MorecError("expected uint8 HWC images")
    if ids is not None:
        ids = catalogue_ids(pixels, ids)
    n_rows, R, _, c = pixels.shape
    n = n_rows if ids is None else ids.numel()
    G = R // patch
    if out is None:
        out = torch.empty((n * G * G, c * patch * patch), device=pixels.device, dtype=dtype)
    else:
        assert out.shape == (n * G * G, c * patch * patch) and out.dtype == dtype and out.is_contiguous()
    if ids is None:
        check(_lib.lib().morec_swin_patchify_u8(_p(pixels), _p(out), n, c, R, patch, out.stride(0), mean, std, code(dtype), _stream()),
              "morec_swin_patchify_u8")
    else:
        check(_lib.lib().morec_swin_patchify_u8_idx(_p(pixels), _p(ids), n_rows, _p(out), n, c, R, patch, out.stride(0), mean, std, code(dtype),
                                                    _stream()), "morec_swin_patchify_u8_idx")
    return out


def swin_merge(x, n_img, H, W, Cc, reverse=False):
    _dev(x)
    out = torch.empty((n_img * H * W, Cc) if reverse else (n_img * (H // 2) * (W // 2), 4 * Cc), device=x.device, dtype=x.dtype)
    check(_lib.lib().morec_swin_merge(_p(x), _p(out), n_img, H, W, Cc, int(reverse), code(x.dtype), _stream()), "morec_swin_merge")
    return out


def swin_pool_fwd(x, n_img, tokens):
    out = torch.empty((n_img, x.shape[1]), device=x.device, dtype=x.dtype)
    check(_lib.lib().morec_swin_pool_fwd(_p(_dev(x)), _p(out), n_img, tokens, x.shape[1], code(x.dtype), _stream()), "morec_swin_pool_fwd")
    return out


def swin_pool_bwd(dout, n_img, tokens):
    dx = torch.empty((n_img * tokens, dout.shape[1]), device=dout.device, dtype=dout.dtype)
    check(_lib.lib().morec_swin_pool_bwd(_p(_dev(dout)), _p(dx), n_img, tokens, dout.shape[1], code(dout.dtype), _stream()), "morec_swin_pool_bwd")
    return dx


def bias_residual(a, bias, res, rowscale=None, rows_per_scale=0, inplace=True):
    """res + rowscale[row / rows_per_scale] * (a + bias), written over ``a`` by default."""
    _dev(a), _dev(res)
    out = a if inplace else torch.empty_like(a)
    check(_lib.lib().morec_bias_residual(_p(a), _p(bias), _p(res), _p(rowscale), rows_per_scale, _p(out), a.shape[0], a.shape[1],
                                         code(a.dtype), _stream()), "morec_bias_residual")
    return out


def droppath_scale(n, p, seed, device="cuda"):
    out = torch.empty(n, device=device, dtype=torch.float32)
    check(_lib.lib().morec_droppath_scale(_p(out), n, p, seed, _stream()), "morec_droppath_scale")
    return out


# ---------------------------------------------------------------------------------------------------------
# MAE (ViT) tower front (csrc/mae.hip)
# ---------------------------------------------------------------------------------------------------------
def mae_len_keep(N: int, mask_ratio: float) -> int:
    """HF ``random_masking`` (``modeling_vit_mae.py:308``): Python double arithmetic, truncated."""
    return int(N * (1 - mask_ratio))


def mae_keep_ids(n_img, N, len_keep, *, noise=None, seed=0, device="cuda"):
    """int32 [n_img, len_keep]: ``argsort(noise)[:, :len_keep]`` (ties to the lower index).  ``noise``: fp32 [n_img, N], or None: drawn from
    ``(seed, image, patch)`` by the counter-based generator of the dropout masks."""
    if noise is not None:
        _dev(noise)
        if noise.dtype != torch.float32 or tuple(noise.shape) != (n_img, N):
            raise _lib.MorecError(f"mae noise must be fp32 [{n_img}, {N}], got {noise.dtype} {tuple(noise.shape)}")
        device = noise.device
    keep = torch.empty((n_img, len_keep), device=device, dtype=torch.int32)
    check(_lib.lib().morec_mae_keep_ids(_p(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(keep), n_img, N, len_keep, _stream()), "morec_mae_keep_ids")
    return keep


def mae_patchify_keep(pixels, keep, patch, dtype, mean=0.5, std=0.5, ids=None):
    """The im2col rows of the kept patches only: fp32 NCHW pixels, or uint8 [n, R, R, 3] decoded images (normalised in flight) ->
    [n * len_keep, 3 patch^2] of ``dtype``; bit-equal to ``swin_patchify[_u8]`` followed by a row gather.  ``ids``: ``pixels`` is the uint8
    image catalogue -- patches from ``keep[k]``, pixels from its row ``ids[k]``."""
    _dev(pixels), _dev(keep)
    if ids is not None:
        ids = catalogue_ids(pixels, ids)
    n_img, len_keep = keep.shape
    if keep.dtype != torch.int32 or (pixels.shape[0] if ids is None else ids.numel()) != n_img:
        raise _lib.MorecError("mae keep must be int32 [n_img, len_keep]")
    if pixels.dtype == torch.uint8:
        n_rows, R, _, c = pixels.shape
        out = torch.empty((n_img * len_keep, c * patch * patch), device=pixels.device, dtype=dtype)
        if ids is None:
            check(_lib.lib().morec_mae_patchify_keep_u8(_p(pixels), _p(keep), _p(out), n_img, c, R, patch, len_keep, out.stride(0), mean, std,
                                                        code(dtype), _stream()), "morec_mae_patchify_keep_u8")
        else:
            check(_lib.lib().morec_mae_patchify_keep_u8_idx(_p(pixels), _p(ids), n_rows, _p(keep), _p(out), n_img, c, R, patch, len_keep,
                                                            out.stride(0), mean, std, code(dtype), _stream()), "morec_mae_patchify_keep_u8_idx")
        return out
    if pixels.dtype != torch.float32:
        raise _lib.MorecError("pixels must be fp32 NCHW or uint8 NHWC")
    _, c, R, _ = pixels.shape
    out = torch.empty((n_img * len_keep, c * patch * patch), device=pixels.device, dtype=dtype)
    check(_lib.lib().morec_mae_patchify_keep(_p(pixels), _p(keep), _p(out), n_img, c, R, patch, len_keep, out.stride(0), code(dtype), _stream()),
          "morec_mae_patchify_keep")
    return out


def mae_assemble_fwd(e, cls_token, pos, keep):
    """[n_img * (1 + len_keep), C]: row 0 of an image = cls_token + pos[0], row 1 + j = e[i * len_keep + j] + pos[1 + keep[i, j]]."""
    _dev(e), _dev(keep), _dev(cls_token), _dev(pos)
    n_img, len_keep = keep.shape
    C_ = e.shape[1]
    N = pos.numel() // C_ - 1
    assert e.shape[0] == n_img * len_keep and cls_token.numel() == C_ and cls_token.dtype == pos.dtype == torch.float32
    x = torch.empty((n_img * (1 + len_keep), C_), device=e.device, dtype=e.dtype)
    check(_lib.lib().morec_mae_assemble_fwd(_p(e), _p(cls_token), _p(pos), _p(keep), _p(x), n_img, len_keep, N, C_, code(e.dtype), _stream()),
          "morec_mae_assemble_fwd")
    return x


def mae_assemble_bwd(dx, n_img, len_keep, d_cls=None):
    """(de [n_img * len_keep, C], d_cls fp32 [C]): the patch rows of ``dx`` and the fixed-order sum of its [CLS] rows (written into ``d_cls``)."""
    _dev(dx)
    C_ = dx.shape[1]
    assert dx.shape[0] == n_img * (1 + len_keep)
    de = torch.empty((n_img * len_keep, C_), device=dx.device, dtype=dx.dtype)
    if d_cls is None:
        d_cls = torch.empty(C_, device=dx.device, dtype=torch.float32)
    assert d_cls.dtype == torch.float32 and d_cls.numel() == C_ and d_cls.is_contiguous()
    check(_lib.lib().morec_mae_assemble_bwd(_p(dx), _p(de), _p(d_cls), n_img, len_keep, C_, code(dx.dtype), _stream()), "morec_mae_assemble_bwd")
    return de, d_cls


# ---------------------------------------------------------------------------------------------------------
# BEiT tower (csrc/beit.hip; attention with a position bias: csrc/attention_stream.hip)
# ---------------------------------------------------------------------------------------------------------
def beit_bias_pitch(T: int) -> int:
    """Row pitch of the expanded position bias [heads, T, Tp]: T rounded up to the key-tile width (include/morec_hip.h)."""
    return (T + 63) // 64 * 64


def beit_relative_position_index(g: int) -> torch.Tensor:
    """int64 [g*g + 1, g*g + 1]: ``BeitRelativePositionBias.generate_relative_position_index`` on the host -- patch pairs by their 2-D
    offset, then the entries cls -> token, token -> cls, cls -> cls.  What ``beit_bias_expand`` gathers by."""
    R = 2 * g - 1
    nrd = R * R + 3
    ys, xs = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    idx = torch.zeros((g * g + 1, g * g + 1), dtype=torch.int64)
    idx[1:, 1:] = (ys[:, None] - ys[None, :] + g - 1) * R + (xs[:, None] - xs[None, :] + g - 1)
    idx[0, :] = nrd - 3
    idx[:, 0] = nrd - 2
    idx[0, 0] = nrd - 1
    return idx


def beit_bias_expand(table, g):
    """``relative_position_bias_table`` fp32 [(2g-1)^2 + 3, heads] -> the position bias of ``attn_bias_fwd``: fp32 [heads, T, Tp]."""
    _dev(table)
    heads, T = table.shape[1], g * g + 1
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[0] == (2 * g - 1) ** 2 + 3
    out = torch.empty((heads, T, beit_bias_pitch(T)), device=table.device, dtype=torch.float32)
    check(_lib.lib().morec_beit_bias_expand(_p(table), _p(out), g, heads, _stream()), "morec_beit_bias_expand")
    return out


def beit_bias_reduce_(d_pos_bias, dtable, g):
    """``dtable`` fp32 [(2g-1)^2 + 3, heads] += the sum of the ``d_pos_bias`` cells behind each entry (fixed order)."""
    assert d_pos_bias.shape == (dtable.shape[1], g * g + 1, beit_bias_pitch(g * g + 1)) and dtable.is_contiguous()
    check(_lib.lib().morec_beit_bias_reduce(_p(_dev(d_pos_bias)), _p(dtable), g, dtable.shape[1], _stream()), "morec_beit_bias_reduce")


def attn_bias_fwd(desc, qkv, key_keep, pos_bias):
    """``attn_fwd`` with ``+ pos_bias[h, i, j]`` on every score (``pos_bias``: fp32 [heads, T, Tp], ``beit_bias_expand``'s layout)."""
    _dev(qkv), _dev(key_keep), _dev(pos_bias)
    assert pos_bias.dtype == torch.float32 and tuple(pos_bias.shape) == (desc.n_heads, desc.T, beit_bias_pitch(desc.T)) and pos_bias.is_contiguous()
    ctx = torch.empty((qkv.shape[0], qkv.shape[1] // 3), device=qkv.device, dtype=qkv.dtype)
    check(_lib.lib().morec_attn_bias_fwd(C.byref(desc), _p(qkv), _p(key_keep), _p(pos_bias), _p(ctx), _stream()), "morec_attn_bias_fwd")
    return ctx


def attn_bias_bwd(desc, qkv, key_keep, pos_bias, dctx, dbias=None, need_dpos=True):
    """(dqkv, d_pos_bias): ``attn_bwd`` of the biased scores.  ``dbias``: fp32 [3 H], accumulated into (column sums of dqkv).
    ``d_pos_bias`` fp32 [heads, T, Tp] = the sum over the sequences of dS (the gradient at the score), or None with ``need_dpos=False``
    (a frozen table: no extra launch)."""
    _dev(dctx), _dev(pos_bias)
    dqkv = torch.empty_like(qkv)
    dpos = ws = None
    nbytes = 0
    if need_dpos:
        dpos = torch.empty_like(pos_bias)
        nbytes = int(_lib.lib().morec_attn_bias_ws_bytes(C.byref(desc)))
        ws = torch.empty(nbytes // 4, device=qkv.device, dtype=torch.float32)
    check(_lib.lib().morec_attn_bias_bwd(C.byref(desc), _p(qkv), _p(key_keep), _p(pos_bias), _p(dctx), _p(dqkv), _p(dbias), _p(dpos), _p(ws),
                                         nbytes, _stream()), "morec_attn_bias_bwd")
    return dqkv, dpos


DISENT_T_MAX = 64      # longest sequence of morec_disent_attn_fwd / _bwd (csrc/deberta.hip)
DISENT_DROP_TP = 64    # edge of the dropout stream's tile there, whatever T: element ((seq * heads + head) * 64 + i) * 64 + j


def _disent_check(desc, qkv, key_keep, pk, pq):
    _dev(qkv), _dev(key_keep), _dev(pk), _dev(pq)
    H = desc.n_heads * desc.dh
    if desc.T > DISENT_T_MAX:
        raise _lib.MorecError(f"disentangled attention over {desc.T} positions: the kernels end at {DISENT_T_MAX} (MOREC_E_UNSUPPORTED)")
    assert tuple(qkv.shape) == (desc.n_seq * desc.T, 3 * H) and code(qkv.dtype) == desc.dtype
    assert key_keep.dtype == torch.float32 and tuple(key_keep.shape) == (desc.n_seq, desc.T)
    assert tuple(pk.shape) == (2 * desc.T, H) and tuple(pq.shape) == (2 * desc.T, H) and pk.dtype == qkv.dtype and pq.dtype == qkv.dtype


def disent_attn_fwd(desc, qkv, key_keep, pk, pq):
    """DeBERTa's disentangled attention (``morec_disent_attn_fwd``): score (i, j) = (q_i.k_j + q_i.pk[i - j + T] + k_j.pq[i - j + T]) * scale,
    REPLACED by ``mask_value`` where query or key is masked.  ``pk`` / ``pq``: [2 T, H] in the storage type, unscaled."""
    _disent_check(desc, qkv, key_keep, pk, pq)
    ctx = torch.empty((qkv.shape[0], qkv.shape[1] // 3), device=qkv.device, dtype=qkv.dtype)
    check(_lib.lib().morec_disent_attn_fwd(C.byref(desc), _p(qkv), _p(key_keep), _p(pk), _p(pq), _p(ctx), _stream()), "morec_disent_attn_fwd")
    return ctx


def disent_attn_bwd(desc, qkv, key_keep, pk, pq, dctx, dbias=None, need_dpos=True):
    """(dqkv, dpk, dpq).  ``dbias``: fp32 [3 H], accumulated into (column sums of dqkv).  ``dpk`` / ``dpq``: fp32 [2 T, H], written (row 0
    is zero), or None with ``need_dpos=False`` (frozen position projections: no extra launch)."""
    _disent_check(desc, qkv, key_keep, pk, pq)
    _dev(dctx)
    assert tuple(dctx.shape) == (qkv.shape[0], qkv.shape[1] // 3) and dctx.dtype == qkv.dtype
    assert dbias is None or (dbias.dtype == torch.float32 and dbias.numel() == qkv.shape[1] and dbias.is_contiguous())
    dqkv = torch.empty_like(qkv)
    dpk = dpq = ws = None
    nbytes = 0
    if need_dpos:
        dpk = torch.empty(pk.shape, device=qkv.device, dtype=torch.float32)
        dpq = torch.empty_like(dpk)
        nbytes = int(_lib.lib().morec_disent_attn_ws_bytes(C.byref(desc)))
        ws = torch.empty(nbytes // 4, device=qkv.device, dtype=torch.float32)
    check(_lib.lib().morec_disent_attn_bwd(C.byref(desc), _p(qkv), _p(key_keep), _p(pk), _p(pq), _p(dctx), _p(dqkv), _p(dbias), _p(dpk), _p(dpq),
                                           _p(ws), nbytes, _stream()), "morec_disent_attn_bwd")
    return dqkv, dpk, dpq


def rows_keep_(x, keep):
    """In place: the rows of ``x`` [M, N] whose ``keep`` entry (fp32 [M]) is zero become exact zeros (``morec_rows_keep``)."""
    _dev(x), _dev(keep)
    assert x.dim() == 2 and keep.dtype == torch.float32 and keep.numel() == x.shape[0]
    check(_lib.lib().morec_rows_keep(_p(x), _p(keep), x.shape[0], x.shape[1], code(x.dtype), _stream()), "morec_rows_keep")
    return x


def layerscale_res_fwd(a, bias, lam, res, rowscale=None, rows_per_scale=0):
    """``res + rowscale[row / rows_per_scale] * (lam * (a + bias))``: fp32 arithmetic, one rounding."""
    _dev(a), _dev(res)
    h = torch.empty_like(a)
    check(_lib.lib().morec_layerscale_res_fwd(_p(a), _p(bias), _p(lam), _p(res), _p(rowscale), rows_per_scale, _p(h), a.shape[0], a.shape[1],
                                              code(a.dtype), _stream()), "morec_layerscale_res_fwd")
    return h


def layerscale_res_bwd(dh, a, bias, lam, rowscale=None, rows_per_scale=0, dlam=None, dbias=None):
    """da = dh * rowscale * lam; ``dlam`` += column sums of dh * rowscale * (a + bias); ``dbias`` += lam * column sums of dh * rowscale
    (either may be None: frozen)."""
    _dev(dh)
    da = torch.empty_like(dh)
    check(_lib.lib().morec_layerscale_res_bwd(_p(dh), _p(a), _p(bias), _p(lam), _p(rowscale), rows_per_scale, _p(da), _p(dlam), _p(dbias),
                                              dh.shape[0], dh.shape[1], code(dh.dtype), _stream()), "morec_layerscale_res_bwd")
    return da


def beit_pool_fwd(x, n_img, T):
    """[n_img, C]: the mean over the patch tokens (rows 1 .. T-1) of every image."""
    assert x.shape[0] == n_img * T
    out = torch.empty((n_img, x.shape[1]), device=x.device, dtype=x.dtype)
    check(_lib.lib().morec_beit_pool_fwd(_p(_dev(x)), _p(out), n_img, T, x.shape[1], code(x.dtype), _stream()), "morec_beit_pool_fwd")
    return out


def beit_pool_bwd(dpool, n_img, T):
    dx = torch.empty((n_img * T, dpool.shape[1]), device=dpool.device, dtype=dpool.dtype)
    check(_lib.lib().morec_beit_pool_bwd(_p(_dev(dpool)), _p(dx), n_img, T, dpool.shape[1], code(dpool.dtype), _stream()), "morec_beit_pool_bwd")
    return dx


def beit_assemble_fwd(e, cls_token, n_img):
    """[n_img * (1 + N), C]: row 0 of an image = cls_token, row 1 + j = e[i * N + j]."""
    _dev(e), _dev(cls_token)
    N, C_ = e.shape[0] // n_img, e.shape[1]
    assert e.shape[0] == n_img * N and cls_token.numel() == C_ and cls_token.dtype == torch.float32
    x = torch.empty((n_img * (1 + N), C_), device=e.device, dtype=e.dtype)
    check(_lib.lib().morec_beit_assemble_fwd(_p(e), _p(cls_token), _p(x), n_img, N, C_, code(e.dtype), _stream()), "morec_beit_assemble_fwd")
    return x


def dropout_keep_mask(n, p, seed, device="cuda"):
    out = torch.empty(n, device=device, dtype=torch.uint8)
    check(_lib.lib().morec_dropout_keep_mask(_p(out), n, p, seed, _stream()), "morec_dropout_keep_mask")
    return out


def probe(device="cuda"):
    out = torch.zeros(4096, device=device, dtype=torch.int32)
    check(_lib.lib().morec_probe(_p(out), _stream()), "morec_probe")
    return out


def image_resize_u8_packed(flat, meta, tabs, R: int, device, out=None, src_buf=None):
    """``morec_image_resize_u8`` over a batch the HOST has already packed (``data_utils.images.pack_images``; CPU tensors, ideally
    page-locked by a collate thread): three asynchronous H2D copies + the resize kernel on the current stream -> uint8 [n, R, R, 3].
    ``out`` / ``src_buf``: caller-owned device buffers for the result and for the packed source bytes (``DeviceImageFeed``)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.MorecError("libmorec_hip needs device tensors (no CPU fallback)")
    n = meta.shape[0]
    if src_buf is not None:
        assert src_buf.numel() >= flat.numel() and src_buf.dtype == torch.uint8
        src = src_buf[:flat.numel()]
        src.copy_(flat, non_blocking=True)
    else:
        src = flat.to(device, non_blocking=True)
    meta_d = meta.to(device, non_blocking=True)
    tabs_d = tabs.to(device, non_blocking=True)
    if out is None:
        out = torch.empty((n, R, R, 3), device=device, dtype=torch.uint8)
    else:
        assert out.shape == (n, R, R, 3) and out.dtype == torch.uint8 and out.is_contiguous()
    check(_lib.lib().morec_image_resize_u8(_p(src), _p(meta_d), _p(tabs_d), _p(out), n, R, _stream()), "morec_image_resize_u8")
    return out


def image_resize_u8(images, R: int, device=None):
    """Decoded uint8 [H, W, 3] images of arbitrary sizes (numpy arrays) -> uint8 [n, R, R, 3] on the device: one pinned H2D
    copy of the packed bytes + ``morec_image_resize_u8`` (Pillow's BILINEAR resampler, bit for bit -- what the reference's
    dataloader workers do per image with ``tv.transforms.Resize``, ``V/data_utils/dataset.py:68-73``)."""
    from .data_utils.images import pack_images
    device = torch.device("cuda") if device is None else torch.device(device)
    if device.type != "cuda":
        raise _lib.MorecError("libmorec_hip needs device tensors (no CPU fallback)")
    flat, meta, tabs = pack_images(images, R)
    return image_resize_u8_packed(torch.from_numpy(flat).pin_memory(), torch.from_numpy(meta), torch.from_numpy(tabs), R, device)


# ---------------------------------------------------------------------------------------------------------
# The ResNet item tower (csrc/conv.hip, csrc/resnet.hip): NHWC activations as [N H W, C] rows.
def conv_out_size(H: int, K: int, stride: int, pad: int) -> int:
    return (H + 2 * pad - K) // stride + 1


def conv2d_uses_mfma(reduction_channels: int, dtype) -> bool:
    """Does a convolution of this storage type and reduction channel count (Cin forward, Cout for the data gradient) run on the
    matrix cores?  Otherwise it runs the fp32-FMA kernel."""
    return bool(_lib.lib().morec_conv2d_uses_mfma(int(reduction_channels), code(dtype)))


def conv2d_fwd(x, w, N, H, W, stride, pad):
    """x [N H W, Cin] rows, w [Cout, KH, KW, Cin] (both the storage type) -> [N Ho Wo, Cout]."""
    _dev(x), _dev(w)
    Cout, KH, KW, Cin = w.shape
    assert x.shape == (N * H * W, Cin) and x.dtype == w.dtype
    Ho, Wo = conv_out_size(H, KH, stride, pad), conv_out_size(W, KW, stride, pad)
    out = torch.empty((N * Ho * Wo, Cout), device=x.device, dtype=x.dtype)
    check(_lib.lib().morec_conv2d_fwd(_p(x), _p(w), _p(out), N, H, W, Cin, Cout, KH, KW, stride, pad, code(x.dtype), _stream()), "morec_conv2d_fwd")
    return out


def conv2d_bwd_data(dy, wt, N, H, W, stride, pad):
    """dy [N Ho Wo, Cout] rows, wt [Cin, KH, KW, Cout] -> dx [N H W, Cin]; H, W: the convolution's INPUT grid."""
    _dev(dy), _dev(wt)
    Cin, KH, KW, Cout = wt.shape
    Ho, Wo = conv_out_size(H, KH, stride, pad), conv_out_size(W, KW, stride, pad)
    assert dy.shape == (N * Ho * Wo, Cout) and dy.dtype == wt.dtype
    dx = torch.empty((N * H * W, Cin), device=dy.device, dtype=dy.dtype)
    check(_lib.lib().morec_conv2d_bwd_data(_p(dy), _p(wt), _p(dx), N, H, W, Cin, Cout, KH, KW, stride, pad, code(dy.dtype), _stream()),
          "morec_conv2d_bwd_data")
    return dx


def im2col_nhwc(x, N, H, W, KH, KW, stride, pad, row0=0, row1=None, ld=None):
    """The operand rows [row1 - row0, ld] of output rows row0 .. row1 (k = (kh, kw, c); the columns past KH KW Cin are zero)."""
    _dev(x)
    Cin = x.shape[1]
    Ho, Wo = conv_out_size(H, KH, stride, pad), conv_out_size(W, KW, stride, pad)
    row1 = N * Ho * Wo if row1 is None else row1
    ev = 16 // x.element_size()
    ld = (KH * KW * Cin + ev - 1) // ev * ev if ld is None else ld
    col = torch.empty((row1 - row0, ld), device=x.device, dtype=x.dtype)
    check(_lib.lib().morec_im2col_nhwc(_p(x), _p(col), N, H, W, Cin, KH, KW, stride, pad, row0, row1, ld, code(x.dtype), _stream()),
          "morec_im2col_nhwc")
    return col


def bn_slab_rows() -> int:
    return int(_lib.lib().morec_bn_slab_rows())


def bn_stats(x):
    """fp32 [slabs, 3, C]: (count, mean, M2) of every slab of ``bn_slab_rows()`` rows, per channel."""
    _dev(x)
    rows, Cc = x.shape
    part = torch.empty(((rows + bn_slab_rows() - 1) // bn_slab_rows(), 3, Cc), device=x.device, dtype=torch.float32)
    check(_lib.lib().morec_bn_stats(_p(x), _p(part), rows, Cc, code(x.dtype), _stream()), "morec_bn_stats")
    return part


def bn_merge(part, eps, running_mean=None, running_var=None, momentum=0.1, need_merged=False):
    """The partials of ``bn_stats`` merged in slab order (Chan): (mean, rstd, merged [3, C] or None); updates the running statistics in
    place when they are given."""
    _dev(part)
    nslabs, _, Cc = part.shape
    out = torch.empty((2, Cc), device=part.device, dtype=torch.float32)
    merged = torch.empty((3, Cc), device=part.device, dtype=torch.float32) if need_merged else None
    check(_lib.lib().morec_bn_merge(_p(part), nslabs, Cc, float(eps), float(momentum), _p(merged), _p(out[0]), _p(out[1]), _p(running_mean),
                                    _p(running_var), _stream()), "morec_bn_merge")
    return out[0], out[1], merged


def bn_merged(part):
    """fp32 [n, 3, C] -> [3, C]: the (count, mean, M2) partials merged in index order and nothing else written (one ``morec_bn_merge``
    launch: a rank's own slabs in front of the gather of synchronised BatchNorm)."""
    _dev(part)
    n, three, Cc = part.shape
    assert three == 3 and part.dtype == torch.float32 and part.is_contiguous()
    merged = torch.empty((3, Cc), device=part.device, dtype=torch.float32)
    check(_lib.lib().morec_bn_merge(_p(part), n, Cc, 0.0, 0.0, _p(merged), None, None, None, None, _stream()), "morec_bn_merge")
    return merged


def bn_rstd(var, eps):
    out = torch.empty_like(var)
    check(_lib.lib().morec_bn_rstd(_p(_dev(var)), _p(out), var.numel(), float(eps), _stream()), "morec_bn_rstd")
    return out


def bn_apply_fwd(x, mean, rstd, gamma, beta, res=None, relu=False):
    _dev(x)
    y = torch.empty_like(x)
    check(_lib.lib().morec_bn_apply_fwd(_p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(res), _p(y), x.shape[0], x.shape[1], int(relu),
                                        code(x.dtype), _stream()), "morec_bn_apply_fwd")
    return y


def bn_bwd_reduce(dy, y, x, mean, rstd):
    """fp32 [2, C]: sum dz, sum dz xhat (dz = dy [y > 0] when ``y``, the output of the ReLU behind the BatchNorm, is given)."""
    _dev(dy), _dev(x)
    rows, Cc = x.shape
    ws = torch.empty(_lib.lib().morec_bn_bwd_workspace_bytes(rows, Cc) // 4, device=x.device, dtype=torch.float32)
    sums = torch.empty((2, Cc), device=x.device, dtype=torch.float32)
    check(_lib.lib().morec_bn_bwd_reduce(_p(dy), _p(y), _p(x), _p(mean), _p(rstd), _p(ws), _p(sums), rows, Cc, code(x.dtype), _stream()),
          "morec_bn_bwd_reduce")
    return sums


def bn_bwd_fold(parts):
    """fp32 [n, 2, C] -> [2, C]: the backward sums of n ranks (or slabs) added in index order."""
    _dev(parts)
    n, two, Cc = parts.shape
    assert two == 2 and parts.dtype == torch.float32 and parts.is_contiguous()
    sums = torch.empty((2, Cc), device=parts.device, dtype=torch.float32)
    check(_lib.lib().morec_bn_bwd_fold(_p(parts), n, Cc, _p(sums), _stream()), "morec_bn_bwd_fold")
    return sums


def bn_bwd_apply(dy, y, x, mean, rstd, gamma, sums, need_dz=False, count=None):
    """(dx, dz or None); ``sums`` None: the statistics were constants (evaluation mode), dx = gamma rstd dz.  ``count`` (fp32 [C] on the
    device, the merged count row of every rank's rows; one value for all channels): the means of ``sums`` divide by it instead of by ``x.shape[0]``
    (``morec_bn_bwd_apply_n``; synchronised BatchNorm, whose ``sums`` are the ranks' folded sums)."""
    _dev(dy), _dev(x)
    dx = torch.empty_like(x)
    dz = torch.empty_like(x) if need_dz else None
    if count is not None:
        assert sums is not None and count.dtype == torch.float32 and count.shape == (x.shape[1],) and count.is_contiguous()
        check(_lib.lib().morec_bn_bwd_apply_n(_p(dy), _p(y), _p(x), _p(mean), _p(rstd), _p(gamma), _p(sums), _p(_dev(count)), _p(dx), _p(dz),
                                              x.shape[0], x.shape[1], code(x.dtype), _stream()), "morec_bn_bwd_apply_n")
        return dx, dz
    check(_lib.lib().morec_bn_bwd_apply(_p(dy), _p(y), _p(x), _p(mean), _p(rstd), _p(gamma), _p(sums), _p(dx), _p(dz), x.shape[0], x.shape[1],
                                        code(x.dtype), _stream()), "morec_bn_bwd_apply")
    return dx, dz


def maxpool3x3s2_fwd(x, N, H, W):
    """MaxPool2d(3, 2, 1) over [N H W, C] rows -> (y [N Ho Wo, C], tap uint8 [N Ho Wo, C])."""
    _dev(x)
    Cc = x.shape[1]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N * Ho * Wo, Cc), device=x.device, dtype=x.dtype)
    idx = torch.empty((N * Ho * Wo, Cc), device=x.device, dtype=torch.uint8)
    check(_lib.lib().morec_maxpool3x3s2_fwd(_p(x), _p(y), _p(idx), N, H, W, Cc, code(x.dtype), _stream()), "morec_maxpool3x3s2_fwd")
    return y, idx


def maxpool3x3s2_bwd(dy, idx, N, H, W):
    _dev(dy), _dev(idx)
    dx = torch.empty((N * H * W, dy.shape[1]), device=dy.device, dtype=dy.dtype)
    check(_lib.lib().morec_maxpool3x3s2_bwd(_p(dy), _p(idx), _p(dx), N, H, W, dy.shape[1], code(dy.dtype), _stream()), "morec_maxpool3x3s2_bwd")
    return dx


def pixels_to_nhwc(pixels, dtype, mean=0.5, std=0.5, ids=None):
    """fp32 [n, C, H, W] (normalised already) or uint8 [n, H, W, C] (decoded: ``(x / 255 - mean) / std`` is applied) -> [n H W, C] rows.
    ``ids``: ``pixels`` is the uint8 image catalogue, image k of the batch its row ``ids[k]``."""
    _dev(pixels)
    if ids is not None:
        ids = catalogue_ids(pixels, ids)
        n_rows, H, W, Cc = pixels.shape
        out = torch.empty((ids.numel() * H * W, Cc), device=pixels.device, dtype=dtype)
        check(_lib.lib().morec_pixels_to_nhwc_idx(_p(pixels), _p(ids), n_rows, _p(out), ids.numel(), Cc, H, W, float(mean), float(std),
                                                  code(dtype), _stream()), "morec_pixels_to_nhwc_idx")
        return out
    u8 = pixels.dtype == torch.uint8
    if not u8 and pixels.dtype != torch.float32:
        raise _lib.MorecError("pixels must be fp32 NCHW or uint8 NHWC")
    n, Cc, H, W = (pixels.shape[0], pixels.shape[3], pixels.shape[1], pixels.shape[2]) if u8 else pixels.shape
    out = torch.empty((n * H * W, Cc), device=pixels.device, dtype=dtype)
    check(_lib.lib().morec_pixels_to_nhwc(_p(pixels), _p(out), n, Cc, H, W, int(u8), float(mean), float(std), code(dtype), _stream()),
          "morec_pixels_to_nhwc")
    return out
