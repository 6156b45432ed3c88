"""Host-side orchestration of the OPT text tower: explicit forward and hand-derived backward of ``Text_Encoder_mean.forward``
(``T/model/encoders.py:31-50``) = ``GELU(fc(masked_mean(OPTModel(ids, mask)[0])))`` over HF ``OPTModel`` (``transformers/models/opt/
modeling_opt.py``; the reference selects it by ``'opt' in bert_model_load``, ``T/run.py:41-47``, ``T/model/encoders.py:96-99``).

OPT is a causal pre-LN decoder (``do_layer_norm_before=True``): ``x += drop(out_proj(attn(LN(x))))``, ``x += drop(fc2(relu(fc1(LN(x)))))``,
a decoder-level ``final_layer_norm`` over all rows.  The blocks are composed as ``mae_engine`` composes its pre-LN blocks -- every residual
sum is formed by the LayerNorm kernel that consumes it, with the sub-layer's dropout as that kernel's ``p_in`` -- on causal, key-masked
attention (``morec_attn_fwd`` / ``_bwd``) and ReLU epilogues with the saved derivative.  The stages no other tower has are in
``csrc/opt.hip``: position ids counted from the attention mask (``2 + k`` for the k-th kept token, row 1 for a masked one), an embedding
stage that is the plain sum of two table rows, and the masked mean pooling.  The embedding backward is ``morec_roberta_embed_bwd`` over
the ``perm`` / ``cnt`` of the mask (``pos_pad = 1``): the word scatter skips id 1 (``padding_idx``), position rows ``2 + k`` are filled,
row 1 and the rows past ``1 + T`` are never written.

Masked-out rows never reach the output (their keys are masked, they are pooled out): their gradient is exactly zero along the whole
backward pass -- the pooling backward writes zeros, every later operator is row-wise or multiplies by a probability that is exactly 0.

The embedding stage runs once in the padded layout; the rows then move to the packed layout (``engine.token_packing``) when every mask is
a run of ones then zeros and ``MOREC_UNPAD`` allows it.  A title without a real token keeps one packed row with ``keep = 0``.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import engine, ops
from ._lib import ACT_RELU
from .engine import NO_DROP, DropCfg, linear_wgrad_, prepare_linear

TE = engine.TE
POS_OFFSET = 2          # OPTLearnedPositionalEmbedding.offset
PAD_ID = 1              # OPTConfig.pad_token_id: embed_tokens.padding_idx

# config options of ``OPTConfig`` outside the supported pre-LN layout: (name, the value the tower is built for)
UNSUPPORTED = (("do_layer_norm_before", True), ("layerdrop", 0.0), ("enable_bias", True), ("layer_norm_elementwise_affine", True),
               ("_remove_final_layer_norm", False))


def check_opt_config(config):
    """Refuse, by name and before anything touches a device, every ``OPTConfig`` option this tower is not built for."""
    for name, want in UNSUPPORTED:
        have = getattr(config, name, want)
        if (float(have) if name == "layerdrop" else bool(have)) != want:
            raise NotImplementedError(f"OPT tower: {name}={have!r} is not built (only {name}={want!r})")
    hidden = getattr(config, "hidden_size", None)
    proj = getattr(config, "word_embed_proj_dim", hidden)
    if proj is not None and hidden is not None and proj != hidden:
        raise NotImplementedError(f"OPT tower: project_in / project_out (word_embed_proj_dim={proj} != hidden_size={hidden}, opt-350m) "
                                  f"is not built")
    act = getattr(config, "activation_function", "relu")
    if act != "relu":
        raise NotImplementedError(f"OPT tower: activation_function={act!r} is not built (only 'relu')")


@dataclass
class OptShape:
    vocab_size: int = 50272
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    ffn_dim: int = 3072
    max_position_embeddings: int = 2048
    layer_norm_eps: float = 1e-5
    pad_token_id: int = PAD_ID

    @staticmethod
    def named(name: str) -> "OptShape":
        """Shapes keyed on ``bert_model_load``; a name that only says "opt" is opt-125m."""
        table = {
            "opt_micro": dict(vocab_size=80, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, ffn_dim=96,
                              max_position_embeddings=40),      # dh = 16: q * dh^-0.5 is an exact scaling
            "opt_1.3b": dict(hidden_size=2048, num_hidden_layers=24, num_attention_heads=32, ffn_dim=8192),
            "opt_125m": dict(),
        }
        key = str(name).lower().replace("-", "_")
        for k, kw in table.items():
            if k in key:
                return OptShape(**kw)
        if "opt" in key:
            return OptShape()
        raise ValueError(f"unknown OPT model {name!r}")

    @property
    def num_positions(self) -> int:
        return self.max_position_embeddings + POS_OFFSET


def opt_layer_names(prefix: str, l: int) -> str:
    return prefix + f"bert_model.decoder.layers.{l}."


def opt_param_shapes(shape: OptShape, D: int, prefix: str = TE):
    """``named_parameters`` inventory of ``Text_Encoder_mean`` over HF ``OPTModel``, in the installed-HF registration order
    (``T/run.py:73-75`` freezes ``bert_model`` parameters by index): the decoder-level ``final_layer_norm`` BEFORE the layers, and
    k, v, q, out inside ``self_attn``; then the encoder's ``fc``."""
    dec = prefix + "bert_model.decoder."
    H, I = shape.hidden_size, shape.ffn_dim
    out = OrderedDict()
    out[dec + "embed_tokens.weight"] = (shape.vocab_size, H)
    out[dec + "embed_positions.weight"] = (shape.num_positions, H)
    out[dec + "final_layer_norm.weight"], out[dec + "final_layer_norm.bias"] = (H,), (H,)
    for l in range(shape.num_hidden_layers):
        L = opt_layer_names(prefix, l)
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out[L + f"self_attn.{n}.weight"], out[L + f"self_attn.{n}.bias"] = (H, H), (H,)
        out[L + "self_attn_layer_norm.weight"], out[L + "self_attn_layer_norm.bias"] = (H,), (H,)
        out[L + "fc1.weight"], out[L + "fc1.bias"] = (I, H), (I,)
        out[L + "fc2.weight"], out[L + "fc2.bias"] = (H, I), (H,)
        out[L + "final_layer_norm.weight"], out[L + "final_layer_norm.bias"] = (H,), (H,)
    out[prefix + "fc.weight"], out[prefix + "fc.bias"] = (D, H), (D,)
    return out


def opt_grad_from(trainable_names, n_layers: int, prefix: str = TE) -> int:
    """Lowest point of the tower that has a trainable parameter (the reference freezes ``bert_model`` parameters by index,
    ``T/run.py:73-75``, and autograd then never walks below the first trainable one): -1 = the embedding tables, k >= 0 = decoder layer
    k, ``n_layers`` = nothing below the decoder-level ``final_layer_norm``, which is registered BEFORE the layers but sits above them."""
    dec = prefix + "bert_model.decoder."
    lo = n_layers
    for n in trainable_names:
        if n.startswith(dec + "embed_"):
            return -1
        if n.startswith(dec + "layers."):
            lo = min(lo, int(n[len(dec + "layers."):].split(".")[0]))
    return lo


# ---------------------------------------------------------------------------------------------------------
def opt_prepare(p: dict, shape: OptShape, dtype, prefix: str = TE, features_only: bool = False):
    prep = dict(layers=[])
    for l in range(shape.num_hidden_layers):
        L = opt_layer_names(prefix, l)
        prep["layers"].append(engine.prepare_block(p, L + "self_attn.", L + "self_attn.out_proj.weight", L + "fc1.weight", L + "fc2.weight", dtype))
    if not features_only:
        prep["fc"] = prepare_linear(p[prefix + "fc.weight"], dtype)
    return prep


def opt_forward(p: dict, prep, shape: OptShape, text: torch.Tensor, dtype, need_grad: bool, prefix: str = TE, drop: DropCfg = NO_DROP,
                unpad: bool | None = None, features_only: bool = False, grad_from: int = -1):
    """text int64 [Nc, 2T] = [input_ids | attention_mask] -> item vectors [Nc, D] = ``GELU(fc(mean))``.  ``features_only``: return
    ``(mean [Nc, H], None)``, the pooled mean in front of ``fc``.  Dropout sites of ``drop``: layer l has 1 + 3l = attention
    probabilities, 2 + 3l = attention sub-layer output, 3 + 3l = FFN output (site 0, the embedding dropout of transformers 4.20.1, is
    not drawn: the installed OPTDecoder has none).  ``unpad`` as ``engine.bert_forward``'s.  ``grad_from`` (``opt_grad_from``): layers
    below it keep nothing for a backward that never reaches them."""
    dec = prefix + "bert_model.decoder."
    Nc, T2 = text.shape
    T = T2 // 2
    H, heads = shape.hidden_size, shape.num_attention_heads
    eps = shape.layer_norm_eps
    ids32 = text[:, :T].to(torch.int32).contiguous().view(-1)
    mask = text[:, T:]
    mask32 = mask.to(torch.int32).contiguous().view(-1)
    keep = (mask != 0).to(torch.float32).contiguous().view(-1)
    word, pos_w = p[dec + "embed_tokens.weight"], p[dec + "embed_positions.weight"]
    pos_ids, perm, cnt = ops.mask_pos_ids(mask32, T, POS_OFFSET, pos_w.shape[0])
    x = ops.opt_embed_fwd(ids32, pos_ids, word, pos_w, dtype)
    cu, tok_idx = None, None
    n_layers = shape.num_hidden_layers
    if (engine.UNPAD_DEFAULT if unpad is None else unpad) and n_layers > 0:
        run_of_ones = bool((mask[:, :-1] >= mask[:, 1:]).all()) if T > 1 else True      # ones, then zeros (one host sync, as bert_forward)
        if run_of_ones:
            cu, tok_idx = engine.token_packing(mask)
            if tok_idx.numel() == Nc * T:
                cu, tok_idx = None, None      # nothing to drop
            else:
                x = ops.indexed_rows_copy(x, torch.empty((tok_idx.numel(), H), device=x.device, dtype=dtype), in_idx=tok_idx)
                # a title without a real token keeps its first position: that row is pooled out and its key masked
                keep = keep.index_select(0, tok_idx.long()).contiguous()
    rows = x.shape[0]
    dh = H // heads
    desc = ops.attn_desc(Nc, T, heads, dh, True, float(dh) ** -0.5, ops.FLT_MIN_MASK, dtype, 0.0, 0, cu, total_rows=rows)
    ph = drop.p_hidden
    pending = None          # (f, b2, h, seed): the previous block's FFN output whose residual sum the next LayerNorm forms
    saved_layers = []
    for l in range(n_layers):
        L = opt_layer_names(prefix, l)
        w = prep["layers"][l]
        s1, s2 = drop.site(2 + 3 * l), drop.site(3 + 3 * l)
        if drop.p_attn > 0:
            desc = ops.attn_desc(Nc, T, heads, dh, True, float(dh) ** -0.5, ops.FLT_MIN_MASK, dtype, drop.p_attn, drop.site(1 + 3 * l), cu,
                                 total_rows=rows)
        g1, b1 = p[L + "self_attn_layer_norm.weight"], p[L + "self_attn_layer_norm.bias"]
        if pending is None:
            xn, _, mean1, rstd1 = ops.layernorm_fwd(x, g1, b1, eps, save_z=False)
        else:
            f, b2, h, sp = pending
            xn, x, mean1, rstd1 = ops.layernorm_fwd(f, g1, b1, eps, bias=b2, res=h, z_inplace=True, p_in=ph, seed_in=sp)
        qkv = ops.gemm_nt(xn, w["qkv"].w, bias=w["bqkv"])
        ctx = ops.attn_fwd(desc, qkv, keep)
        a = ops.gemm_nt(ctx, w["o"].w)
        hn, h, mean2, rstd2 = ops.layernorm_fwd(a, p[L + "final_layer_norm.weight"], p[L + "final_layer_norm.bias"], eps,
                                                bias=p[L + "self_attn.out_proj.bias"], res=x, z_inplace=True, p_in=ph, seed_in=s1)
        ng = need_grad and l >= grad_from
        pre = torch.empty((rows, w["f1"].w.shape[0]), device=x.device, dtype=dtype) if ng else None
        g = ops.gemm_nt(hn, w["f1"].w, bias=p[L + "fc1.bias"], act=ACT_RELU, aux_out=pre, aux_deriv=ng)      # pre = relu'(fc1)
        f = ops.gemm_nt(g, w["f2"].w)
        pending = (f, p[L + "fc2.bias"], h, s2)
        saved_layers.append((desc, x, xn, mean1, rstd1, qkv, ctx, h, hn, mean2, rstd2, pre, g, s1, s2) if ng else None)
    gF, bF = p[dec + "final_layer_norm.weight"], p[dec + "final_layer_norm.bias"]
    if pending is None:
        y, z_last, mean_f, rstd_f = ops.layernorm_fwd(x, gF, bF, eps, save_z=False)
    else:
        f, b2, h, sp = pending
        y, z_last, mean_f, rstd_f = ops.layernorm_fwd(f, gF, bF, eps, bias=b2, res=h, z_inplace=True, p_in=ph, seed_in=sp)
    mean = ops.masked_mean_fwd(y, keep, Nc, T, cu)
    if features_only:
        return mean, None
    item, pre_c = engine.head_forward(mean, prep["fc"], p[prefix + "fc.bias"], need_grad)
    saved = ((shape, Nc, T, rows, ids32, perm, cnt, keep, cu, tok_idx, ph, saved_layers, z_last, mean_f, rstd_f, mean, pre_c, grad_from)
             if need_grad else None)
    return item, saved


def opt_backward(p: dict, prep, saved, d_item: torch.Tensor, grads: dict, prefix: str = TE):
    """grads: name -> fp32 buffer (accumulated into); the q/k/v projections are handed out as row views of a fresh fused buffer.  The
    pass ends at the forward's ``grad_from``: nothing below the lowest trainable layer is computed."""
    dec = prefix + "bert_model.decoder."
    shape, Nc, T, rows, ids32, perm, cnt, keep, cu, tok_idx, ph, saved_layers, z_last, mean_f, rstd_f, mean, pre_c, grad_from = saved
    H = shape.hidden_size
    n_layers = shape.num_hidden_layers
    dmean = engine.head_backward(d_item, pre_c, mean, prep["fc"], grads[prefix + "fc.weight"], grads[prefix + "fc.bias"], H)
    dy = ops.masked_mean_bwd(dmean, keep, Nc, T, rows, cu)      # zeros on the masked rows
    # gradient at the last block's output sum (dres) and behind that block's FFN dropout (dsub); its column sums are that block's fc2.bias
    if n_layers == 0 or grad_from >= n_layers:      # no block below, or none that trains: no FFN dropout / fc2.bias to go through
        dres, _ = ops.layernorm_bwd(dy, None, z_last, mean_f, rstd_f, p[dec + "final_layer_norm.weight"], grads[dec + "final_layer_norm.weight"],
                                    grads[dec + "final_layer_norm.bias"])
        dsub = None
        if grad_from >= n_layers and n_layers > 0:
            return
    else:
        dres, dsub = ops.layernorm_bwd(dy, None, z_last, mean_f, rstd_f, p[dec + "final_layer_norm.weight"],
                                       grads[dec + "final_layer_norm.weight"], grads[dec + "final_layer_norm.bias"], p_in=ph,
                                       seed_in=saved_layers[-1][-1], dbias=grads[opt_layer_names(prefix, n_layers - 1) + "fc2.bias"])
    for l in reversed(range(max(grad_from, 0), n_layers)):
        L = opt_layer_names(prefix, l)
        A = L + "self_attn."
        w = prep["layers"][l]
        desc, x, xn, mean1, rstd1, qkv, ctx, h, hn, mean2, rstd2, pre, g, s1, s2 = saved_layers[l]
        # FFN branch: out = h + drop(fc2(relu(fc1(LN2(h)))) + b2)
        dhn = engine.mlp_backward(dsub, w, g, pre, hn, grads[L + "fc2.weight"], grads[L + "fc1.bias"], grads[L + "fc1.weight"], H)
        # h = x + drop(out_proj(ctx) + bo): dh = LN2'(dhn) + dres, da = drop'(dh)
        dh, da = ops.layernorm_bwd(dhn, None, h, mean2, rstd2, p[L + "final_layer_norm.weight"], grads[L + "final_layer_norm.weight"],
                                   grads[L + "final_layer_norm.bias"], p_in=ph, seed_in=s1, dbias=grads[A + "out_proj.bias"], dres=dres)
        linear_wgrad_(da, ctx, grads[A + "out_proj.weight"])
        dctx = ops.gemm_nt(da, w["o"].wt, K=da.shape[1], N=H)
        gw, gb = engine.fused_qkv_grads(H, dctx.device)
        dqkv = ops.attn_bwd(desc, qkv, keep, dctx, dbias=gb)      # + d(q|k|v bias) = column sums of dqkv
        linear_wgrad_(dqkv, xn, gw)
        engine.hand_out_qkv(grads, A, gw, gb, H, key_bias="zero")
        dxn = ops.gemm_nt(dqkv, w["qkv"].wt, K=dqkv.shape[1], N=H)
        if 0 < l == grad_from:      # nothing trainable below: only this LayerNorm's own gradients are wanted
            ops.layernorm_bwd(dxn, None, x, mean1, rstd1, p[L + "self_attn_layer_norm.weight"], grads[L + "self_attn_layer_norm.weight"],
                              grads[L + "self_attn_layer_norm.bias"], dres=dh)
            return
        if l > 0:      # x is the previous block's output sum: behind its FFN dropout sits the previous fc2.bias
            dres, dsub = ops.layernorm_bwd(dxn, None, x, mean1, rstd1, p[L + "self_attn_layer_norm.weight"],
                                           grads[L + "self_attn_layer_norm.weight"], grads[L + "self_attn_layer_norm.bias"], p_in=ph,
                                           seed_in=saved_layers[l - 1][-1], dbias=grads[opt_layer_names(prefix, l - 1) + "fc2.bias"], dres=dh)
        else:          # x is the embedding sum
            dres, _ = ops.layernorm_bwd(dxn, None, x, mean1, rstd1, p[L + "self_attn_layer_norm.weight"],
                                        grads[L + "self_attn_layer_norm.weight"], grads[L + "self_attn_layer_norm.bias"], dres=dh)
    if grad_from >= 0:      # frozen embedding tables
        return
    if tok_idx is not None:      # back to the padded layout the embedding stage lives in: dropped rows get zero
        pa = torch.zeros((Nc * T, H), device=dres.device, dtype=dres.dtype)
        ops.indexed_rows_copy(dres, pa, out_idx=tok_idx)
        dres = pa
    order = torch.argsort(ids32, stable=ops.DETERMINISTIC).to(torch.int32)
    # word rows (id 1 = padding_idx skipped whatever the mask says) and position rows 2 + k; no token-type table
    ops.roberta_embed_bwd_(ids32, dres, grads[dec + "embed_tokens.weight"], grads[dec + "embed_positions.weight"], None, PAD_ID, T, perm, cnt,
                           POS_OFFSET - 1, order)


def _no_buffer(names, needs, c, plan):
    return {n for l in range(c.shape.num_hidden_layers) for n in engine.qkv_names(opt_layer_names(c.prefix, l) + "self_attn.")}


TOWER = engine.Tower(
    prepare=lambda p, c, need_grad: opt_prepare(p, c.shape, c.dtype, c.prefix, features_only=c.features_only),
    # the backward stops at the lowest trainable point of the tower (T/run.py:73-75 freezes a prefix by parameter index)
    plan=lambda trainable, c: dict(grad_from=opt_grad_from(trainable, c.shape.num_hidden_layers, c.prefix)),
    forward=lambda p, prep, x, c, need_grad, **plan: opt_forward(p, prep, c.shape, x, c.dtype, need_grad, c.prefix, c.drop,
                                                                 features_only=c.features_only, **c.kw, **plan),
    backward=lambda p, prep, saved, d, grads, c: opt_backward(p, prep, saved, d, grads, c.prefix),
    no_buffer=_no_buffer)
