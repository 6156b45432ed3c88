"""Host-side orchestration of the DeBERTa text tower: explicit forward and hand-derived backward of ``Text_Encoder.forward`` =
``GELU(fc(DebertaModel(ids, mask)[0][:, 0]))`` over the installed ``transformers/models/deberta/modeling_deberta.py`` (the reference
selects it in its DSSM package, ``bce_text/main-end2end(DSSM)/run.py:26-31``).

The released v1 configuration: ``relative_attention=True``, ``pos_att_type=["c2p", "p2c"]``, ``position_biased_input=False``,
``type_vocab_size=0``, ``max_relative_positions=-1`` (= ``max_position_embeddings``), ``layer_norm_eps=1e-7``, ``pad_token_id=0``.

* Embedding stage: ``dropout(LN(word[ids]) * mask)`` -- no position row, no token type.  Composed of existing kernels, ``morec_gather_rows``
  and ``morec_layernorm_fwd`` with the dropout as its output dropout (mask and dropout are both factors: they commute exactly), plus
  ``morec_rows_keep`` for the mask: no existing kernel zeroes rows of an output in place.  The word gradient is ``morec_scatter_add_rows``
  (row ``pad_token_id`` skipped: ``padding_idx``).
* Layers: post-LN BERT blocks, kernel for kernel ``engine.layer_forward`` / ``layer_backward``, with ``morec_disent_attn_fwd`` / ``_bwd``
  (``csrc/deberta.hip``) in the place of the plain attention.  ``in_proj.weight`` (rows interleaved per head, ``[h][q|k|v][dh]``) is
  permuted to the library's ``[Q | K | V]`` once per prepare, its gradient permuted back; the fused bias is ``cat(q_bias, 0, v_bias)`` and
  the k third of its gradient is discarded.  Per layer and call ``R = pos_dropout(rel_embeddings[P - T : P + T])`` (2T rows, P =
  ``max_relative_positions``), ``PK = pos_proj(R)``, ``PQ = pos_q_proj(R)`` come from the library's GEMMs; their weight gradients come
  from the kernels' ``dPK`` / ``dPQ``, and ``d rel_embeddings`` accumulates over the layers into rows P-T+1 .. P+T-1 (row P-T belongs to
  d = 0, which never occurs: an exact zero like every other row).
* The scale is 1 / s with s = sqrt(3 dh) taken in fp32, as the installed ``scaled_size_sqrt`` takes it.
* Padded layout only: d(i, j) = i - j + T is defined on the padded T, and a masked query row attends to all T keys, so ``MOREC_UNPAD`` is
  not consulted.  The ``*_res32`` modes run this tower in the plain 16-bit type.

Dropout sites of ``drop``: 0 = embedding output; layer l: 1 + 4l = ``pos_dropout`` on R (a fresh stream per layer), 2 + 4l = attention
probabilities, 3 + 4l = attention sub-layer output, 4 + 4l = FFN output.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass

import numpy as np
import torch

from . import engine, ops
from ._lib import ACT_GELU
from .engine import NO_DROP, DropCfg, linear_wgrad_, prepare_linear

TE = engine.TE
T_MAX = ops.DISENT_T_MAX


def check_deberta_config(config, T: int | None = None):
    """Refuse, by name and before anything touches a device, every ``DebertaConfig`` option this tower is not built for."""
    def no(what):
        raise NotImplementedError(f"DeBERTa tower: {what} is not built")
    name = str(getattr(config, "_name_or_path", "") or getattr(config, "name", "")).lower()
    if getattr(config, "model_type", "deberta") in ("deberta-v2", "deberta_v2") or "v2" in name or "v3" in name:
        no("DeBERTa v2 / v3 (another architecture: conv layer, bucketed positions, shared projections)")
    if not getattr(config, "relative_attention", False):
        no("relative_attention=False")
    pat = getattr(config, "pos_att_type", None) or []
    if sorted(pat) != ["c2p", "p2c"]:
        no(f"pos_att_type={list(pat)!r} (only ['c2p', 'p2c'])")
    if getattr(config, "position_biased_input", True):
        no("position_biased_input=True")
    if int(getattr(config, "type_vocab_size", 0) or 0) > 0:
        no(f"type_vocab_size={config.type_vocab_size}")
    emb = getattr(config, "embedding_size", None)
    if emb is not None and emb != config.hidden_size:
        no(f"embedding_size={emb} != hidden_size={config.hidden_size} (embed_proj)")
    if getattr(config, "talking_head", False):
        no("talking_head=True")
    if int(getattr(config, "z_steps", 0) or 0) > 1:
        no(f"z_steps={config.z_steps}")
    act = getattr(config, "hidden_act", "gelu")
    if act != "gelu":
        no(f"hidden_act={act!r} (only 'gelu')")
    if T is not None:
        if T > T_MAX:
            no(f"T > {T_MAX} (titles of {T} tokens: the disentangled attention kernels end at {T_MAX})")
        mrp = int(getattr(config, "max_relative_positions", -1) or -1)
        if mrp < 1:
            mrp = int(config.max_position_embeddings)
        if mrp < T:
            no(f"max_relative_positions={mrp} below the title length {T} (clamped relative positions)")


@dataclass
class DebertaShape:
    vocab_size: int = 50265
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 512
    layer_norm_eps: float = 1e-7
    pad_token_id: int = 0
    max_relative_positions: int = -1

    @staticmethod
    def named(name: str) -> "DebertaShape":
        """Shapes keyed on ``bert_model_load``; a name that only says "deberta" is deberta-base."""
        key = str(name).lower().replace("-", "_")
        if "v2" in key or "v3" in key:
            raise NotImplementedError(f"DeBERTa tower: {name!r} names DeBERTa v2 / v3, another architecture, which is not built")
        table = {
            "deberta_micro": dict(vocab_size=80, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=96,
                                  max_position_embeddings=40),
            "deberta_large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096),
            "deberta_base": dict(),
        }
        for k, kw in table.items():
            if k in key:
                return DebertaShape(**kw)
        if "deberta" in key:
            return DebertaShape()
        raise ValueError(f"unknown DeBERTa model {name!r}")

    @property
    def rel_positions(self) -> int:
        return self.max_relative_positions if self.max_relative_positions >= 1 else self.max_position_embeddings


def deberta_layer_names(prefix: str, l: int) -> str:
    return prefix + f"bert_model.encoder.layer.{l}."


def deberta_param_shapes(shape: DebertaShape, D: int, prefix: str = TE):
    """``named_parameters`` inventory of ``Text_Encoder`` over the installed ``DebertaModel``, in its registration order
    (``--freeze_paras_before`` counts by it): ``encoder.rel_embeddings.weight`` is LAST inside ``bert_model``, index 3 + 16 L."""
    bm = prefix + "bert_model."
    H, I = shape.hidden_size, shape.intermediate_size
    out = OrderedDict()
    out[bm + "embeddings.word_embeddings.weight"] = (shape.vocab_size, H)
    out[bm + "embeddings.LayerNorm.weight"], out[bm + "embeddings.LayerNorm.bias"] = (H,), (H,)
    for l in range(shape.num_hidden_layers):
        L = deberta_layer_names(prefix, l)
        A = L + "attention.self."
        out[A + "q_bias"], out[A + "v_bias"] = (H,), (H,)
        out[A + "in_proj.weight"] = (3 * H, H)
        out[A + "pos_proj.weight"] = (H, H)
        out[A + "pos_q_proj.weight"], out[A + "pos_q_proj.bias"] = (H, H), (H,)
        out[L + "attention.output.dense.weight"], out[L + "attention.output.dense.bias"] = (H, H), (H,)
        out[L + "attention.output.LayerNorm.weight"], out[L + "attention.output.LayerNorm.bias"] = (H,), (H,)
        out[L + "intermediate.dense.weight"], out[L + "intermediate.dense.bias"] = (I, H), (I,)
        out[L + "output.dense.weight"], out[L + "output.dense.bias"] = (H, I), (H,)
        out[L + "output.LayerNorm.weight"], out[L + "output.LayerNorm.bias"] = (H,), (H,)
    out[bm + "encoder.rel_embeddings.weight"] = (2 * shape.rel_positions, H)
    out[prefix + "fc.weight"], out[prefix + "fc.bias"] = (D, H), (D,)
    return out


def permute_in_proj(w: torch.Tensor, heads: int) -> torch.Tensor:
    """Rows of ``in_proj.weight`` [3H, ...] from HF's interleaved ``[h][q|k|v][dh]`` to the library's ``[Q | K | V]``."""
    H3 = w.shape[0]
    dh = H3 // (3 * heads)
    return w.reshape(heads, 3, dh, *w.shape[1:]).transpose(0, 1).reshape(w.shape).contiguous()


def unpermute_in_proj(w: torch.Tensor, heads: int) -> torch.Tensor:
    """The inverse: rows ``[Q | K | V]`` back to ``[h][q|k|v][dh]``."""
    H3 = w.shape[0]
    dh = H3 // (3 * heads)
    return w.reshape(3, heads, dh, *w.shape[1:]).transpose(0, 1).reshape(w.shape).contiguous()


def deberta_grad_from(trainable_names, n_layers: int, prefix: str = TE) -> int:
    """Lowest point of the tower the backward must reach: -1 = the embedding stage, k >= 0 = encoder layer k, ``n_layers`` = nothing
    inside the layers.  ``encoder.rel_embeddings`` is registered last but feeds EVERY layer: while it trains, layer 0 is reached."""
    bm = prefix + "bert_model."
    lo = n_layers
    for n in trainable_names:
        if n.startswith(bm + "embeddings."):
            return -1
        if n.startswith(bm + "encoder.layer."):
            lo = min(lo, int(n[len(bm + "encoder.layer."):].split(".")[0]))
        elif n == bm + "encoder.rel_embeddings.weight":
            lo = min(lo, 0)
    return lo


def deberta_pos_layers(trainable_names, n_layers: int, prefix: str = TE):
    """The layers whose backward must form dPK / dPQ: all of them while ``rel_embeddings`` trains, else those whose own ``pos_proj`` /
    ``pos_q_proj`` train."""
    bm = prefix + "bert_model."
    names = set(trainable_names)
    if bm + "encoder.rel_embeddings.weight" in names:
        return frozenset(range(n_layers))
    return frozenset(l for l in range(n_layers)
                     if any((deberta_layer_names(prefix, l) + "attention.self." + k) in names
                            for k in ("pos_proj.weight", "pos_q_proj.weight", "pos_q_proj.bias")))


def attn_scale(dh: int) -> float:
    """1 / sqrt(3 dh) with the square root taken in fp32 (the installed ``scaled_size_sqrt``)."""
    return 1.0 / float(np.sqrt(np.float32(3 * dh)))


# ---------------------------------------------------------------------------------------------------------
def deberta_prepare(p: dict, shape: DebertaShape, dtype, prefix: str = TE, features_only: bool = False):
    heads, H = shape.num_attention_heads, shape.hidden_size
    prep = dict(layers=[])
    for l in range(shape.num_hidden_layers):
        L = deberta_layer_names(prefix, l)
        A = L + "attention.self."
        bqkv = torch.cat([p[A + "q_bias"], torch.zeros_like(p[A + "q_bias"]), p[A + "v_bias"]], 0).float().contiguous()
        prep["layers"].append(dict(
            qkv=prepare_linear(permute_in_proj(p[A + "in_proj.weight"].detach(), heads), dtype), bqkv=bqkv,
            pk=prepare_linear(p[A + "pos_proj.weight"], dtype), pq=prepare_linear(p[A + "pos_q_proj.weight"], dtype), bpq=p[A + "pos_q_proj.bias"],
            o=prepare_linear(p[L + "attention.output.dense.weight"], dtype), bo=p[L + "attention.output.dense.bias"],
            ln1_g=p[L + "attention.output.LayerNorm.weight"], ln1_b=p[L + "attention.output.LayerNorm.bias"],
            f1=prepare_linear(p[L + "intermediate.dense.weight"], dtype), b1=p[L + "intermediate.dense.bias"],
            f2=prepare_linear(p[L + "output.dense.weight"], dtype), b2=p[L + "output.dense.bias"],
            ln2_g=p[L + "output.LayerNorm.weight"], ln2_b=p[L + "output.LayerNorm.bias"]))
    if not features_only:
        prep["fc"] = prepare_linear(p[prefix + "fc.weight"], dtype)
    return prep


def deberta_forward(p: dict, prep, shape: DebertaShape, text: torch.Tensor, dtype, need_grad: bool, prefix: str = TE,
                    drop: DropCfg = NO_DROP, features_only: bool = False, grad_from: int = -1, pos_layers=None):
    """text int64 [Nc, 2T] = [input_ids | attention_mask] -> item vectors [Nc, D] = ``GELU(fc(hidden[:, 0]))``.  ``features_only``:
    return ``(cls [Nc, H], None)``, the [CLS] rows in front of ``fc``.  ``grad_from`` (``deberta_grad_from``): layers below it keep
    nothing for a backward that never reaches them; ``pos_layers`` (``deberta_pos_layers``; None = all): the layers whose backward forms
    dPK / dPQ.  Dropout sites: see the module docstring."""
    bm = prefix + "bert_model."
    Nc, T2 = text.shape
    T = T2 // 2
    if T > T_MAX:
        raise NotImplementedError(f"DeBERTa tower: T > {T_MAX} (titles of {T} tokens) is not built")
    H, heads = shape.hidden_size, shape.num_attention_heads
    dh = H // heads
    P = shape.rel_positions
    if P < T:
        raise NotImplementedError(f"DeBERTa tower: max_relative_positions={P} below the title length {T} is not built")
    eps = shape.layer_norm_eps
    n_layers = shape.num_hidden_layers
    ids32 = text[:, :T].to(torch.int32).contiguous().view(-1)
    keep = (text[:, T:] != 0).to(torch.float32).contiguous()
    keep_rows = keep.view(-1)
    ph = drop.p_hidden
    e = ops.gather_rows(p[bm + "embeddings.word_embeddings.weight"], ids32, dtype)
    x, _, mean_e, rstd_e = ops.layernorm_fwd(e, p[bm + "embeddings.LayerNorm.weight"], p[bm + "embeddings.LayerNorm.bias"], eps,
                                             save_z=False, p_out=ph, seed_out=drop.site(0))
    ops.rows_keep_(x, keep_rows)
    rel_idx = torch.arange(P - T, P + T, device=x.device, dtype=torch.int32)
    scale = attn_scale(dh)
    saved_layers = []
    for l, w in enumerate(prep["layers"]):
        ng = need_grad and l >= grad_from
        s_pos, s_attn, s1, s2 = (drop.site(k + 4 * l) for k in (1, 2, 3, 4))
        R = ops.gather_rows(p[bm + "encoder.rel_embeddings.weight"], rel_idx, dtype)
        if ph > 0:
            ops.dropout_apply_(R, ph, s_pos)
        PK = ops.gemm_nt(R, w["pk"].w)
        PQ = ops.gemm_nt(R, w["pq"].w, bias=w["bpq"])
        desc = ops.attn_desc(Nc, T, heads, dh, False, scale, ops.FLT_MIN_MASK, dtype, drop.p_attn, s_attn)
        qkv = ops.gemm_nt(x, w["qkv"].w, bias=w["bqkv"])
        ctx = ops.disent_attn_fwd(desc, qkv, keep, PK, PQ)
        a = ops.gemm_nt(ctx, w["o"].w)
        x1, z1, mean1, rstd1 = ops.layernorm_fwd(a, w["ln1_g"], w["ln1_b"], eps, bias=w["bo"], res=x, z_inplace=True, p_in=ph, seed_in=s1)
        u = torch.empty((x.shape[0], w["f1"].w.shape[0]), device=x.device, dtype=dtype) if ng else None
        g = ops.gemm_nt(x1, w["f1"].w, bias=w["b1"], act=ACT_GELU, aux_out=u, aux_deriv=ng)      # u = gelu'(pre-activation)
        f = ops.gemm_nt(g, w["f2"].w)
        x2, z2, mean2, rstd2 = ops.layernorm_fwd(f, w["ln2_g"], w["ln2_b"], eps, bias=w["b2"], res=x1, z_inplace=True, p_in=ph, seed_in=s2)
        dpos = pos_layers is None or l in pos_layers
        saved_layers.append((desc, x, R, PK, PQ, qkv, ctx, z1, mean1, rstd1, x1, u, g, z2, mean2, rstd2, s_pos, s1, s2, dpos) if ng else None)
        x = x2
    cls = ops.strided_rows_copy(x, torch.empty((Nc, H), device=x.device, dtype=dtype), Nc, H, T, 1)
    if features_only:
        return cls, None
    item, pre = engine.head_forward(cls, prep["fc"], p[prefix + "fc.bias"], need_grad)
    saved = ((shape, Nc, T, ids32, keep, keep_rows, e, mean_e, rstd_e, rel_idx, ph, drop.site(0), saved_layers, cls, pre, grad_from)
             if need_grad else None)
    return item, saved


def deberta_backward(p: dict, prep, saved, d_item: torch.Tensor, grads: dict, prefix: str = TE):
    """grads: name -> fp32 buffer (accumulated into); ``in_proj.weight`` (in HF's interleaved layout), ``q_bias`` and ``v_bias`` are handed
    out as fresh tensors.  The pass ends at the forward's ``grad_from``: nothing below the lowest trainable layer is computed."""
    bm = prefix + "bert_model."
    shape, Nc, T, ids32, keep, keep_rows, e, mean_e, rstd_e, rel_idx, ph, seed_e, saved_layers, cls, pre, grad_from = saved
    H, heads = shape.hidden_size, shape.num_attention_heads
    n_layers = shape.num_hidden_layers
    frozen = grad_from >= n_layers and n_layers > 0      # the whole of bert_model is frozen
    dcls = engine.head_backward(d_item, pre, cls, prep["fc"], grads[prefix + "fc.weight"], grads[prefix + "fc.bias"], H, need_dx=not frozen)
    if frozen:
        return
    da = torch.zeros((Nc * T, H), device=dcls.device, dtype=dcls.dtype)      # only hidden[:, 0] is consumed
    ops.strided_rows_copy(dcls, da, Nc, H, 1, T)
    db = None
    dtype = da.dtype
    for l in reversed(range(max(grad_from, 0), n_layers)):
        L = deberta_layer_names(prefix, l)
        A = L + "attention.self."
        w = prep["layers"][l]
        desc, x0, R, PK, PQ, qkv, ctx, z1, mean1, rstd1, x1, u, gact, z2, mean2, rstd2, s_pos, s1, s2, dpos = saved_layers[l]
        dz2, dzd2 = ops.layernorm_bwd(da, db, z2, mean2, rstd2, w["ln2_g"], grads[L + "output.LayerNorm.weight"],
                                      grads[L + "output.LayerNorm.bias"], p_in=ph, seed_in=s2, dbias=grads[L + "output.dense.bias"])
        dx1 = engine.mlp_backward(dzd2, w, gact, u, x1, grads[L + "output.dense.weight"], grads[L + "intermediate.dense.bias"],
                                  grads[L + "intermediate.dense.weight"], H)
        dz1, dzd1 = ops.layernorm_bwd(dx1, dz2, z1, mean1, rstd1, w["ln1_g"], grads[L + "attention.output.LayerNorm.weight"],
                                      grads[L + "attention.output.LayerNorm.bias"], p_in=ph, seed_in=s1,
                                      dbias=grads[L + "attention.output.dense.bias"])
        linear_wgrad_(dzd1, ctx, grads[L + "attention.output.dense.weight"])
        dctx = ops.gemm_nt(dzd1, w["o"].wt, K=dzd1.shape[1], N=H)
        gw, gb = engine.fused_qkv_grads(H, dctx.device)
        dqkv, dPK, dPQ = ops.disent_attn_bwd(desc, qkv, keep, PK, PQ, dctx, dbias=gb, need_dpos=dpos)
        linear_wgrad_(dqkv, x0, gw)
        engine.WgradStream.join(dqkv.device)      # gw is read (permuted) right below
        grads[A + "in_proj.weight"] = unpermute_in_proj(gw, heads)
        # (k has no bias: the k third of the column sums is discarded)
        grads[A + "q_bias"], grads[A + "v_bias"] = gb[:H].clone(), gb[2 * H:].clone()
        if dpos:
            ops.colsum_(dPQ, grads[A + "pos_q_proj.bias"])
            dPK16 = dPK if dtype == torch.float32 else ops.cast(dPK, dtype)
            dPQ16 = dPQ if dtype == torch.float32 else ops.cast(dPQ, dtype)
            linear_wgrad_(dPK16, R, grads[A + "pos_proj.weight"])
            linear_wgrad_(dPQ16, R, grads[A + "pos_q_proj.weight"])
            dR = ops.scaled_sum([ops.gemm_nt(dPK16, w["pk"].wt, K=H, N=H), ops.gemm_nt(dPQ16, w["pq"].wt, K=H, N=H)], 1.0)
            if ph > 0:
                ops.dropout_apply_(dR, ph, s_pos)
            # rows P-T .. P+T-1 of the table; row P-T (d = 0) receives an exact zero
            ops.scatter_add_rows_(dR, rel_idx, grads[bm + "encoder.rel_embeddings.weight"], -1)
        if grad_from >= 0 and l == grad_from:      # nothing trainable below
            return
        da = ops.gemm_nt(dqkv, w["qkv"].wt, K=dqkv.shape[1], N=H)
        db = dz1
    if grad_from >= 0:
        return
    # embedding stage: x = drop(LN(e)) * mask, e = word[ids]
    ops.rows_keep_(da, keep_rows)
    if db is not None:
        ops.rows_keep_(db, keep_rows)
    de, _ = ops.layernorm_bwd(da, db, e, mean_e, rstd_e, p[bm + "embeddings.LayerNorm.weight"], grads[bm + "embeddings.LayerNorm.weight"],
                              grads[bm + "embeddings.LayerNorm.bias"], p_out=ph, seed_out=seed_e)
    ops.scatter_add_rows_(de, ids32, grads[bm + "embeddings.word_embeddings.weight"], shape.pad_token_id)


def _plan(trainable, c):
    n = c.shape.num_hidden_layers
    return dict(grad_from=deberta_grad_from(trainable, n, c.prefix), pos_layers=deberta_pos_layers(trainable, n, c.prefix))


def _no_buffer(names, needs, c, plan):      # handed out as fresh tensors by ``deberta_backward``
    return {deberta_layer_names(c.prefix, l) + "attention.self." + k for l in range(c.shape.num_hidden_layers)
            for k in ("in_proj.weight", "q_bias", "v_bias")}


TOWER = engine.Tower(
    prepare=lambda p, c, need_grad: deberta_prepare(p, c.shape, c.dtype, c.prefix, features_only=c.features_only),
    plan=_plan,
    forward=lambda p, prep, x, c, need_grad, **plan: deberta_forward(p, prep, c.shape, x, c.dtype, need_grad, c.prefix, c.drop,
                                                                     features_only=c.features_only, **plan),
    backward=lambda p, prep, saved, d, grads, c: deberta_backward(p, prep, saved, d, grads, c.prefix),
    no_buffer=_no_buffer)
