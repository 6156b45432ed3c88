"""``torch.autograd.Function`` shells around ``engine``: they make the HIP forward/backward a node of
PyTorch's autograd graph so that the reference driver's ``scaler.scale(loss).backward()``, ``DDP`` gradient
hooks and ``optim.AdamW`` (``T/run.py:243-247``) keep working unchanged on the drop-in ``Model``.
Gradients are computed by the hand-written backward kernels, never by autograd tracing of torch ops.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import engine, ops


def _zeros_like_params(names, params, skip=()):
    return {n: torch.zeros_like(p, dtype=torch.float32) for n, p in zip(names, params) if n not in skip}


class SasrecFn(torch.autograd.Function):
    """``User_Encoder.forward`` (``T/model/encoders.py:23-28``).  ``call``: an ``engine.TowerCall`` with ``kw`` = heads, n_layers, res32
    (the autocast data flow: fp32 residual stream, ``engine.LayerCfg.res32``)."""

    @staticmethod
    def forward(ctx, x_in, log_mask, call, *params):
        kw = call.kw
        p = dict(zip(call.names, params))
        need = any(ctx.needs_input_grad)
        x = x_in.contiguous()
        if x.dtype != call.dtype:
            x = ops.cast(x, call.dtype)
        prep = engine.sasrec_prepare(p, kw["n_layers"], call.dtype, call.prefix)
        out, saved = engine.sasrec_forward(p, prep, x, log_mask, kw["heads"], need, call.prefix, call.drop, res32=kw["res32"])
        ctx.stuff = (p, prep, saved, call, x_in.dtype, tuple(x_in.shape))
        ctx.fp32_gemm = ops.FP32_GEMM
        return out.view(x_in.shape)

    @staticmethod
    def backward(ctx, dout):
        p, prep, saved, call, in_dtype, in_shape = ctx.stuff
        ctx.stuff = None
        names = call.names
        grads = _zeros_like_params(names, [p[n] for n in names], skip=engine.sasrec_no_buffer(len(prep), call.prefix))
        d = dout.contiguous().view(-1, in_shape[-1])
        with ops.fp32_gemm_mode(ctx.fp32_gemm):
            dx = engine.sasrec_backward(p, prep, saved, d, grads, call.prefix)
            engine.WgradStream.join(d.device)      # autograd consumers (DDP hooks, the optimizer) read the gradients on this stream
        if dx.dtype != in_dtype:
            dx = ops.cast(dx, in_dtype)
        return (dx.view(in_shape), None, None) + tuple(grads[n] for n in names)


class TowerFn(torch.autograd.Function):
    """An item tower as one autograd node: ``TowerFn.apply(x, tower, call, *params)`` with ``tower`` the engine module's ``engine.Tower``
    (``engine.TOWER``: BERT / RoBERTa, ``swin_engine.TOWER``, ...), ``call`` an ``engine.TowerCall`` and ``params`` in the order of
    ``call.names``.  The backward ends where ``tower.plan`` says, given what trains; a parameter without ``requires_grad`` gets None, and
    a trainable one the backward left no gradient for is an error.  ``call.features_only``: the rows in front of the projection head,
    non-differentiable."""

    @staticmethod
    def forward(ctx, x, tower, call, *params):
        p = dict(zip(call.names, params))
        needs = ctx.needs_input_grad[3:]
        need = any(ctx.needs_input_grad) and not call.features_only
        prep = tower.prepare(p, call, need)
        plan = tower.plan([n for n, nd in zip(call.names, needs) if nd], call)
        out, saved = tower.forward(p, prep, x, call, need, **plan)
        ctx.stuff = (tower, call, p, prep, saved, plan, needs)
        ctx.fp32_gemm = ops.FP32_GEMM
        if call.features_only:
            ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, d_out):
        tower, call, p, prep, saved, plan, needs = ctx.stuff
        ctx.stuff = None
        names = call.names
        grads = _zeros_like_params(names, [p[n] for n in names], skip=tower.no_buffer(names, needs, call, plan))
        with ops.fp32_gemm_mode(ctx.fp32_gemm):
            tower.backward(p, prep, saved, d_out.contiguous(), grads, call)
            engine.WgradStream.join(d_out.device)      # autograd consumers (DDP hooks, the optimizer) read the gradients on this stream
        missing = [n for n, nd in zip(names, needs) if nd and n not in grads]
        if missing:
            raise RuntimeError(f"the tower's backward left no gradient for the trainable parameter {missing[0]!r}")
        return (None, None, None) + tuple(grads[n] if nd else None for n, nd in zip(names, needs))


class IdEmbeddingFn(torch.autograd.Function):
    """``nn.Embedding(item_num + 1, D, padding_idx=0)`` lookup (``T/model/model.py:27,37``)."""

    @staticmethod
    def forward(ctx, ids, weight, dtype):
        idx = ids.reshape(-1).to(torch.int32).contiguous()
        out = ops.gather_rows(weight, idx, dtype)
        ctx.save_for_backward(idx)
        ctx.shape = weight.shape
        return out.view(tuple(ids.shape) + (weight.shape[1],))

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        dw = torch.zeros(ctx.shape, device=dout.device, dtype=torch.float32)
        ops.scatter_add_rows_(dout.contiguous().view(-1, ctx.shape[1]), idx, dw, 0)
        return None, dw, None


def _cat_layers_forward(a, fc_params, dtype, drop, need):
    """The Linear + GELU layers behind the CAT fusion's concatenation ``a`` [R, 2D] (dropout already applied, site 0); ``drop.site(l)`` is
    the Dropout in front of layer l.  Returns (output, prepared weights, layer inputs, pre-activations) for ``_cat_layers_backward``."""
    p = float(drop.p_hidden)
    n_layers = len(fc_params) // 2
    lin = [engine.prepare_linear(fc_params[2 * l], dtype) for l in range(n_layers)]
    acts, pres = [], []
    for l in range(n_layers):
        pre = torch.empty((a.shape[0], lin[l].w.shape[0]), device=a.device, dtype=dtype) if need else None
        h = ops.gemm_nt(a, lin[l].w, bias=fc_params[2 * l + 1], act=ops.ACT_GELU, aux_out=pre)
        acts.append(a)
        pres.append(pre)
        if l + 1 < n_layers and p > 0:
            ops.dropout_apply_(h, p, drop.site(l + 1))
        a = h
    return a, lin, acts, pres


def _cat_layers_backward(d, dout, lin, acts, pres, p, drop):
    """Backward of ``_cat_layers_forward`` from the output gradient ``d`` (``dout``: the caller's tensor, never written): returns the gradient
    of the concatenation [R, 2D] and [dW1, db1, ...].  Weight gradients run on the weight-gradient stream: the caller joins it."""
    n_layers = len(lin)
    grads = []
    for l in reversed(range(n_layers)):
        if l + 1 < n_layers and p > 0:      # the mask the forward put on this layer's output
            d = ops.dropout_apply_(d.clone() if d.data_ptr() == dout.data_ptr() else d, p, drop.site(l + 1))
        dv = ops.act_bwd(d, pres[l], ops.ACT_GELU)
        db = torch.zeros(dv.shape[1], device=dv.device, dtype=torch.float32)
        dw = torch.zeros(lin[l].w.shape, device=dv.device, dtype=torch.float32)
        ops.colsum_(dv, db)
        engine.linear_wgrad_(dv, acts[l], dw)
        grads = [dw, db] + grads
        d = ops.gemm_nt(dv, lin[l].wt, K=dv.shape[1], N=acts[l].shape[1])
    return d, grads


class FusionFn(torch.autograd.Function):
    """ID (+) modality fusion ``fc(id_embedding(ids), content)`` (``bce_text/id_plus_mo-end2end/model/model.py:43-47``): ``ADD`` or ``CAT``
    (``model/encoders.py:8-39``).  ``cfg = (kind, dtype, drop, pad_id)``: kind "add" | "cat", the compute dtype, a ``DropCfg`` whose
    ``p_hidden`` is the MLP's drop rate (site 0: the concatenation, site l: the input of layer l), and the table row that receives no
    gradient (0 = ``padding_idx``; -1: none).  ``fc_params`` = (W1, b1[, W2, b2, W3, b3]).  Gradients: content, the id table (dense fp32,
    like ``IdEmbeddingFn``), the fc weights and biases.  Outside the residual stream: the ``*_res32`` modes are plain 16-bit here."""

    @staticmethod
    def forward(ctx, ids, content, table, cfg, *fc_params):
        kind, dtype, drop, pad_id = cfg
        need = any(ctx.needs_input_grad)
        idx = ids.reshape(-1).to(torch.int32).contiguous()
        y = content.contiguous().view(idx.numel(), -1)
        if y.dtype != dtype:
            y = ops.cast(y, dtype)
        tab = table.contiguous()
        if tab.dtype != torch.float32 or tab.shape[1] != y.shape[1]:
            raise ValueError(f"fusion: the id table must be fp32 [n, {y.shape[1]}] (content width), got {tab.dtype} {tuple(tab.shape)}")
        if kind == "cat" and fc_params[0].shape[1] != 2 * y.shape[1]:
            raise ValueError(f"fusion: the first Linear takes {fc_params[0].shape[1]} inputs, the concatenation has {2 * y.shape[1]}")
        ctx.fp32_gemm = ops.FP32_GEMM
        ctx.meta = (kind, pad_id, content.dtype, tuple(content.shape), tuple(table.shape))
        if kind == "add":
            ctx.stuff = (idx,)
            return ops.fuse_add_fwd(tab, idx, y)
        p = float(drop.p_hidden)
        a, lin, acts, pres = _cat_layers_forward(ops.fuse_cat_fwd(tab, idx, y, p, drop.site(0)), fc_params, dtype, drop, need)
        ctx.stuff = (idx, lin, acts, pres, p, drop) if need else None
        return a

    @staticmethod
    def backward(ctx, dout):
        kind, pad_id, in_dtype, in_shape, tshape = ctx.meta
        stuff, ctx.stuff = ctx.stuff, None
        idx = stuff[0]
        d_table = torch.zeros(tshape, device=dout.device, dtype=torch.float32)
        d = dout.contiguous().view(idx.numel(), -1)
        if kind == "add":
            ops.scatter_add_rows_(d, idx, d_table, pad_id)
            dc = d if d.dtype == in_dtype else ops.cast(d, in_dtype)
            return None, dc.view(in_shape), d_table, None
        _, lin, acts, pres, p, drop = stuff
        with ops.fp32_gemm_mode(ctx.fp32_gemm):
            d, grads = _cat_layers_backward(d, dout, lin, acts, pres, p, drop)
            dc = ops.fuse_cat_bwd(d, idx, d_table, pad_id, p, drop.site(0))
            engine.WgradStream.join(dout.device)
        if dc.dtype != in_dtype:
            dc = ops.cast(dc, in_dtype)
        return (None, dc.view(in_shape), d_table, None) + tuple(grads)


class MlpFn(torch.autograd.Function):
    """``MLP_Encoder.forward`` of the DSSM package (``bce_text/main-end2end(DSSM)/model/encoders.py:6-41``): ``len(params) / 2`` triples of
    Dropout -> Linear(D, D) -> GELU over the rows of ``x``.  ``cfg = (dtype, drop)``: the compute dtype and a ``DropCfg`` whose ``p_hidden``
    is the drop rate (site l: the input of layer l); masks are regenerated from the seed in the backward.  ``params`` = (W1, b1, W2, b2, ...).
    Built from the same ops as ``FusionFn``'s CAT branch."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        dtype, drop = cfg
        need = any(ctx.needs_input_grad)
        a = x.contiguous().view(-1, x.shape[-1])
        if a.dtype != dtype:
            a = ops.cast(a, dtype)
        p = float(drop.p_hidden)
        n_layers = len(params) // 2
        if params[0].shape[1] != a.shape[1]:
            raise ValueError(f"mlp: the first Linear takes {params[0].shape[1]} inputs, the rows have {a.shape[1]}")
        ctx.fp32_gemm = ops.FP32_GEMM
        ctx.meta = (x.dtype, tuple(x.shape))
        lin = [engine.prepare_linear(params[2 * l], dtype) for l in range(n_layers)]
        acts, pres = [], []
        for l in range(n_layers):
            if p > 0:       # the layer's own Dropout, on its input (never on the caller's tensor)
                a = ops.dropout_apply_(a.clone() if l == 0 and a.data_ptr() == x.data_ptr() else a, p, drop.site(l))
            pre = torch.empty((a.shape[0], lin[l].w.shape[0]), device=a.device, dtype=dtype) if need else None
            h = ops.gemm_nt(a, lin[l].w, bias=params[2 * l + 1], act=ops.ACT_GELU, aux_out=pre)
            acts.append(a)
            pres.append(pre)
            a = h
        ctx.stuff = (lin, acts, pres, p, drop) if need else None
        return a.view(tuple(x.shape[:-1]) + (a.shape[1],))

    @staticmethod
    def backward(ctx, dout):
        in_dtype, in_shape = ctx.meta
        (lin, acts, pres, p, drop), ctx.stuff = ctx.stuff, None
        d = dout.contiguous().view(-1, dout.shape[-1])
        grads = []
        with ops.fp32_gemm_mode(ctx.fp32_gemm):
            for l in reversed(range(len(lin))):
                dv = ops.act_bwd(d, pres[l], ops.ACT_GELU)
                db = torch.zeros(dv.shape[1], device=dv.device, dtype=torch.float32)
                dw = torch.zeros(lin[l].w.shape, device=dv.device, dtype=torch.float32)
                ops.colsum_(dv, db)
                engine.linear_wgrad_(dv, acts[l], dw)
                grads = [dw, db] + grads
                d = ops.gemm_nt(dv, lin[l].wt, K=dv.shape[1], N=acts[l].shape[1])
                if p > 0:       # the mask the forward put on this layer's input
                    ops.dropout_apply_(d, p, drop.site(l))
            engine.WgradStream.join(dout.device)
        if d.dtype != in_dtype:
            d = ops.cast(d, in_dtype)
        return (d.view(in_shape), None) + tuple(grads)


class FeatProjFn(torch.autograd.Function):
    """The first layer of the two-stage item tower over a FROZEN feature table (``bce_text/main-2stage(SASRec)/model/encoders.py:29-30``:
    ``activate(fc(item_content[ids]))``, with the reference's host-side lookup ``data_utils/dataset.py:39`` folded in):
    ``GELU(table[ids] @ W^T + b)``.  ``table`` [n_rows, Kw] in the compute dtype ``dtype``, ``ids`` any integer tensor.  Forward:
    ``ops.featproj_fwd`` (one launch) where ``ops.featproj_supported`` says so, else ``ops.featproj_composed`` (fp32 modes, odd widths,
    ``MOREC_FEATPROJ=1``).  Backward: act', column sums, the looked-up rows materialised on the weight-gradient stream, the weight-gradient
    GEMM -- and NO input-gradient GEMM: the table receives no gradient."""

    @staticmethod
    def forward(ctx, ids, table, dtype, weight, bias):
        need = any(ctx.needs_input_grad)
        idx = ids.reshape(-1).to(torch.int32).contiguous()
        ctx.fp32_gemm = ops.FP32_GEMM
        out, pre = _featproj_forward(idx, table, dtype, weight, bias, need)
        ctx.stuff = (idx, table, pre, tuple(weight.shape)) if need else None
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx, table, pre, wshape), ctx.stuff = ctx.stuff, None
        d = dout.contiguous().view(idx.numel(), -1)
        with ops.fp32_gemm_mode(ctx.fp32_gemm):
            dw, db = _featproj_backward(d, idx, table, pre, wshape)
            engine.WgradStream.join(d.device)
        return None, None, None, dw, db


def _featproj_forward(idx, table, dtype, weight, bias, need):
    """``FeatProjFn``'s forward from the int32 ids: (out, pre) by ``ops.featproj_fwd`` where supported, else ``ops.featproj_composed``."""
    if table.dtype != dtype or table.dim() != 2 or not table.is_contiguous():
        raise ValueError(f"featproj: the feature table must be a contiguous {dtype} matrix, got {table.dtype} {tuple(table.shape)}")
    if weight.shape[1] != table.shape[1]:
        raise ValueError(f"featproj: fc takes {weight.shape[1]} inputs, the feature table has {table.shape[1]} columns")
    w = weight.contiguous() if weight.dtype == dtype else ops.cast(weight.contiguous(), dtype)
    if ops.featproj_supported(idx.numel(), table.shape[1], w.shape[0], dtype):
        return ops.featproj_fwd(table, idx, w, bias, need_pre=need)
    return ops.featproj_composed(table, idx, w, bias, need_pre=need)[:2]


def _featproj_backward(d, idx, table, pre, wshape):
    """(dW, db) of ``GELU(table[idx] @ W^T + b)`` from the output gradient ``d`` [R, D] and the pre-activation.  The looked-up rows are
    gathered and multiplied on the weight-gradient stream: the caller joins it."""
    dev = d.device
    dv = ops.act_bwd(d, pre, ops.ACT_GELU)
    db = torch.zeros(dv.shape[1], device=dev, dtype=torch.float32)
    dw = torch.zeros(wshape, device=dev, dtype=torch.float32)
    ops.colsum_(dv, db)
    # (the side stream exactly where linear_wgrad_ launches on it: 16-bit operands with whole 16-byte rows)
    side = engine.WgradStream.get(dev) if (ops.is16(dv.dtype) and dv.shape[1] % 8 == 0 and table.shape[1] % 8 == 0) else None
    if side is None:
        x = ops.indexed_rows_copy(table, torch.empty((idx.numel(), table.shape[1]), device=dev, dtype=table.dtype), in_idx=idx)
    else:       # X[idx] is read by the weight gradient alone: gathered on ITS stream (which waits for the main one first)
        ops.stream_wait_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            x = ops.indexed_rows_copy(table, torch.empty((idx.numel(), table.shape[1]), device=dev, dtype=table.dtype), in_idx=idx)
    engine.linear_wgrad_(dv, x, dw)
    return dw, db


class FeatFuseFn(torch.autograd.Function):
    """The item tower of the two-stage ID (+) modality packages with ``mo_dnn_layers == 0``
    (``bce_text/id_plus_mo-2stage/model/model.py:48-50``): ``fc(id_embedding(ids), GELU(turn_dim.fc(features[ids])))`` -- the chain
    ids -> ``FeatProjFn`` -> ``FusionFn`` as one node.  ``cfg = (kind, dtype, drop, pad_id)`` as ``FusionFn``'s; ``table`` [n_rows, W] the
    frozen features in the compute dtype, ``id_table`` fp32 [n_rows, D], ``weight`` / ``bias`` the projection, ``fc_params`` = (W1, b1) of
    the CAT layer.  Forward: ``ops.featfuse_fwd`` (one launch) where ``ops.featfuse_supported`` says so, else featproj +
    ``fuse_add_fwd`` / ``fuse_cat_fwd`` (fp32 modes, odd widths, ``MOREC_FEATFUSE=1``, sizes past the rule) -- the same bits either way.
    Backward: ``FusionFn``'s and ``FeatProjFn``'s, existing kernels only; the feature table receives no gradient."""

    @staticmethod
    def forward(ctx, ids, table, id_table, cfg, weight, bias, *fc_params):
        kind, dtype, drop, pad_id = cfg
        need = any(ctx.needs_input_grad)
        idx = ids.reshape(-1).to(torch.int32).contiguous()
        tab = id_table.contiguous()
        D = weight.shape[0]
        if tab.dtype != torch.float32 or tuple(tab.shape) != (table.shape[0], D):
            raise ValueError(f"featfuse: the id table must be fp32 [{table.shape[0]}, {D}], got {tab.dtype} {tuple(tab.shape)}")
        if kind == "cat" and fc_params[0].shape[1] != 2 * D:
            raise ValueError(f"featfuse: the first Linear takes {fc_params[0].shape[1]} inputs, the concatenation has {2 * D}")
        p = float(drop.p_hidden) if kind == "cat" else 0.0
        ctx.fp32_gemm = ops.FP32_GEMM
        ctx.meta = (kind, pad_id, tuple(id_table.shape), tuple(weight.shape))
        if ops.featfuse_supported(idx.numel(), table.shape[1], D, dtype):
            if table.dtype != dtype or table.dim() != 2 or not table.is_contiguous():
                raise ValueError(f"featfuse: the feature table must be a contiguous {dtype} matrix, got {table.dtype} {tuple(table.shape)}")
            if weight.shape[1] != table.shape[1]:
                raise ValueError(f"featfuse: fc takes {weight.shape[1]} inputs, the feature table has {table.shape[1]} columns")
            w = weight.contiguous() if weight.dtype == dtype else ops.cast(weight.contiguous(), dtype)
            a, pre = ops.featfuse_fwd(table, idx, w, bias, tab, kind, p, drop.site(0) if p > 0 else 0, need_pre=need)
        else:
            y, pre = _featproj_forward(idx, table, dtype, weight, bias, need)
            a = ops.fuse_add_fwd(tab, idx, y) if kind == "add" else ops.fuse_cat_fwd(tab, idx, y, p, drop.site(0))
        if kind == "add":
            ctx.stuff = (idx, table, pre) if need else None
            return a
        a, lin, acts, pres = _cat_layers_forward(a, fc_params, dtype, drop, need)
        ctx.stuff = (idx, table, pre, lin, acts, pres, p, drop) if need else None
        return a

    @staticmethod
    def backward(ctx, dout):
        kind, pad_id, tshape, wshape = ctx.meta
        stuff, ctx.stuff = ctx.stuff, None
        idx, table, pre = stuff[:3]
        d_table = torch.zeros(tshape, device=dout.device, dtype=torch.float32)
        d = dout.contiguous().view(idx.numel(), -1)
        grads = []
        with ops.fp32_gemm_mode(ctx.fp32_gemm):
            if kind == "add":
                ops.scatter_add_rows_(d, idx, d_table, pad_id)
            else:
                lin, acts, pres, p, drop = stuff[3:]
                d, grads = _cat_layers_backward(d, dout, lin, acts, pres, p, drop)
                d = ops.fuse_cat_bwd(d, idx, d_table, pad_id, p, drop.site(0))
            dw, db = _featproj_backward(d, idx, table, pre, wshape)
            engine.WgradStream.join(dout.device)
        return (None, None, d_table, None, dw, db) + tuple(grads)


class DssmBceFn(torch.autograd.Function):
    """The DSSM scoring loss (``bce_text/main-end2end(DSSM)/model/model.py:40-42``): U [B, D] user vectors, E [B * n1, D] item vectors,
    ``labels`` fp32 [B * n1] (or None: [1, 0, ..., 0] per user) -> the mean of BCEWithLogits over all B * n1 scores.
    ``morec_dssm_bce_fwd`` / ``morec_dssm_bce_bwd``."""

    @staticmethod
    def forward(ctx, U, E, labels, B, n1):
        U, E = U.contiguous(), E.contiguous()
        if labels is not None:
            labels = labels.reshape(-1).to(torch.float32).contiguous()
        scores, _, loss_sum = ops.dssm_bce_fwd(U, E, labels, B, n1)
        ctx.stuff = (U, E, labels, scores, B, n1)
        return (loss_sum[0] / (B * n1)).to(torch.float32)

    @staticmethod
    def backward(ctx, dloss):
        U, E, labels, scores, B, n1 = ctx.stuff
        ctx.stuff = None
        g = (dloss.to(torch.float32) / (B * n1)).reshape(1).contiguous()
        dU, dE = ops.dssm_bce_bwd(U, E, labels, scores, g, B, n1)
        return dU, dE, None, None, None


def _all_gather_cat(t: torch.Tensor, world: int, comm=None, group=None) -> torch.Tensor:
    """``group``: the process group (None: the world), of ``world`` ranks."""
    if comm is not None:       # morec_comm_all_gather: RCCL on the compute stream (comm.MorecComm)
        return comm.all_gather(t)
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    if dist.get_backend(group) == "gloo" and t.is_cuda:   # gloo smoke tests on a GPU box: list form, staged through the host
        parts = [torch.empty_like(t, device="cpu") for _ in range(world)]
        dist.all_gather(parts, t.detach().cpu().contiguous(), group=group)
        return torch.cat(parts, 0).to(t.device)
    dist.all_gather_into_tensor(out, t.contiguous(), group=group)
    return out


def pool_exchange(E: torch.Tensor, ci, n_valid: torch.Tensor, world: int, rank: int, comm=None):
    """The forward exchange of the pooled-negative step in TWO collectives instead of five: one all-gather of
    the encoded item vectors, one all-gather of a packed int32 record per rank -- slot ids | log-pop bits | validity | the
    rank's valid-row count -- whose last word also replaces the scalar all-reduce (every rank sums the same ``world`` counts in
    the same order: identical n_valid everywhere, deterministically).  Returns (E_pool, pooled CeInputs, n_valid_global)."""
    Nc = ci.col_ids.shape[0]
    blob = torch.cat((ci.col_ids.to(torch.int32), ci.col_logpop.to(torch.float32).view(torch.int32), ci.col_valid.to(torch.int32),
                      n_valid.reshape(1).to(torch.float32).view(torch.int32))).view(1, -1)
    g = _all_gather_cat(blob, world, comm)                             # [world, 3 Nc + 1]
    Epool = _all_gather_cat(E, world, comm)
    pooled = engine.CeInputs(ci.row_ids, g[:, :Nc].reshape(-1).contiguous(),
                             g[:, Nc:2 * Nc].reshape(-1).contiguous().view(torch.float32).to(ci.col_logpop.dtype),
                             g[:, 2 * Nc:3 * Nc].reshape(-1).to(torch.uint8).contiguous(), ci.row_valid, ci.B, ci.S, rank * E.shape[0])
    n_glob = g[:, 3 * Nc].contiguous().view(torch.float32).sum()
    return Epool, pooled, n_glob


def reduce_scatter_dE(dEpool: torch.Tensor, world: int, rank: int, out_dtype: torch.dtype, comm=None) -> torch.Tensor:
    """The backward exchange: SUM of every rank's gradient w.r.t. the pooled item vectors, each rank keeping the rows it owns.
    Always reduced in fp32 (an 8-way sum in bf16 would round seven times), then returned in the compute dtype."""
    t = dEpool if dEpool.dtype == torch.float32 else (ops.cast(dEpool, torch.float32) if dEpool.is_cuda else dEpool.float())
    d = comm.reduce_scatter_sum(t) if comm is not None else _reduce_scatter_sum(t, world, rank)
    if d.dtype == out_dtype:
        return d
    return ops.cast(d, out_dtype) if d.is_cuda else d.to(out_dtype)


def _reduce_scatter_sum(t: torch.Tensor, world: int, rank: int) -> torch.Tensor:
    n = t.shape[0] // world
    if dist.get_backend() == "gloo":   # gloo has no reduce_scatter: all-reduce and keep our shard (smoke / CPU tests only)
        if t.is_cuda:
            h = t.detach().float().cpu()
            dist.all_reduce(h)
            return h[rank * n:(rank + 1) * n].to(t.device).to(t.dtype).contiguous()
        dist.all_reduce(t)
        return t[rank * n:(rank + 1) * n].contiguous()
    out = torch.empty((n,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    dist.reduce_scatter_tensor(out, t.contiguous())
    return out


class InBatchCEFn(torch.autograd.Function):
    """In-batch debiased CE (``T/model/model.py:32-33,45-67``).  With ``pool=True`` under an initialised
    process group the negatives are pooled over ranks: all-gather of the encoded item
    vectors + slot ids + log-pop + validity forward, reduce-scatter(sum) of dE backward, valid-row count
    all-reduced so that N ranks x B equals the single-process loss at batch N*B.  ``loss_mult`` rescales the
    local share (``world_size`` when a gradient-AVERAGING wrapper such as DDP follows, 1 for sum-reduce)."""

    @staticmethod
    def forward(ctx, P, E, ci, pool, loss_mult, backend):
        P, E = P.contiguous(), E.contiguous()
        world = dist.get_world_size() if (pool and dist.is_available() and dist.is_initialized()) else 1
        n_valid = ci.row_valid.sum(dtype=torch.float32)
        if world > 1:
            rank = dist.get_rank()
            Epool, ci, n_valid = pool_exchange(E, ci, n_valid, world, rank)
        else:
            rank, Epool = 0, E
        loss_sum, saved = backend.ce_forward(ci, P, Epool, world > 1) if backend is engine else backend.ce_forward(ci, P, Epool)
        ctx.stuff = (ci, P, Epool, saved, world, rank, n_valid, loss_mult, backend)
        return (loss_sum[0] * loss_mult / n_valid).to(torch.float32)

    @staticmethod
    def backward(ctx, dloss):
        ci, P, Epool, saved, world, rank, n_valid, loss_mult, backend = ctx.stuff
        ctx.stuff = None
        g = (dloss.to(torch.float32) * loss_mult / n_valid).reshape(1).contiguous()
        dP, dEpool = backend.ce_backward(ci, P, Epool, saved, g, 1.0)
        dE = reduce_scatter_dE(dEpool, world, rank, dEpool.dtype) if world > 1 else dEpool
        return dP, dE, None, None, None, None
