"""Host-side orchestration of the BEiT item tower: explicit forward and hand-derived backward of ``Vit_Encoder.forward``
(``V/model/encoders.py:24-31``) = ``GELU(image_net(x)[0])`` with ``image_net`` a HF ``BeitForImageClassification`` whose ``classifier``
was replaced by ``Linear(hidden, embedding_dim)`` (``V/run.py:47-54``; the reference selects it by ``'beit' in CV_model_load``,
``V/model/model.py:26-27``).  Arithmetic of HF ``transformers/models/beit/modeling_beit.py`` with eager attention.

The blocks are the pre-LN blocks of ``mae_engine`` with three differences: every attention score carries a per-head relative-position
bias (one learned table per layer, expanded once per forward to the [heads, T, Tp] layout of ``morec_attn_bias_fwd``); each sub-layer
output is scaled per channel (``lambda_1`` / ``lambda_2``) and per image (DropPath, training only) before the residual add
(``morec_layerscale_res_fwd``: one extra pass per sub-layer, the LayerNorm kernels then normalise the sum they are given); and the head is
``classifier(LN(mean of the patch tokens))`` -- ``BeitModel.layernorm`` is the identity under mean pooling and [CLS] is not in the mean.
There are no absolute positions and no mask token; ``k_proj`` has no bias.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import engine, ops
from ._lib import ACT_GELU
from .engine import NO_DROP, DropCfg, linear_wgrad_, prepare_linear

IN = "image_net."


@dataclass
class BeitShape:
    image_size: int = 224
    patch_size: int = 16
    num_channels: int = 3
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    layer_norm_eps: float = 1e-12
    drop_path_rate: float = 0.1
    layer_scale_init_value: float = 0.1

    @staticmethod
    def named(name: str) -> "BeitShape":
        """Shapes keyed on ``CV_model_load`` the way ``SwinShape.named`` is; a name that only says "beit" (``V/model/model.py:26``) is the
        base model."""
        table = {
            "beit_micro": dict(image_size=16, patch_size=4, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256),
            "beit_large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096),
            "beit_base": dict(),
        }
        for key, kw in table.items():
            if key in name:
                return BeitShape(**kw)
        if "beit" in name:
            return BeitShape()
        raise ValueError(f"unknown CV_model_load {name!r}")

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid ** 2

    @property
    def num_relative_distance(self) -> int:
        return (2 * self.grid - 1) ** 2 + 3

    def drop_path_rates(self):
        n = self.num_hidden_layers
        return [self.drop_path_rate * i / max(n - 1, 1) for i in range(n)]


def beit_layer_names(prefix: str, l: int) -> str:
    return prefix + f"beit.layers.{l}."


TABLE = "relative_position_bias.relative_position_bias_table"


def beit_param_shapes(shape: BeitShape, D: int, prefix: str = IN):
    """``named_parameters`` inventory of the installed HF ``BeitForImageClassification`` (``classifier`` replaced), in registration
    order: ``V/run.py:58-60`` freezes by parameter index."""
    net = prefix + "beit."
    C, I = shape.hidden_size, shape.intermediate_size
    out = OrderedDict()
    out[net + "embeddings.cls_token"] = (1, 1, C)
    out[net + "embeddings.patch_embeddings.projection.weight"] = (C, shape.num_channels, shape.patch_size, shape.patch_size)
    out[net + "embeddings.patch_embeddings.projection.bias"] = (C,)
    for l in range(shape.num_hidden_layers):
        L = beit_layer_names(prefix, l)
        out[L + "lambda_1"], out[L + "lambda_2"] = (C,), (C,)
        out[L + "attention.q_proj.weight"], out[L + "attention.q_proj.bias"] = (C, C), (C,)
        out[L + "attention.k_proj.weight"] = (C, C)
        out[L + "attention.v_proj.weight"], out[L + "attention.v_proj.bias"] = (C, C), (C,)
        out[L + "attention.o_proj.weight"], out[L + "attention.o_proj.bias"] = (C, C), (C,)
        for n in ("layernorm_before", "layernorm_after"):
            out[L + n + ".weight"], out[L + n + ".bias"] = (C,), (C,)
        out[L + "mlp.fc1.weight"], out[L + "mlp.fc1.bias"] = (I, C), (I,)
        out[L + "mlp.fc2.weight"], out[L + "mlp.fc2.bias"] = (C, I), (C,)
        out[L + TABLE] = (shape.num_relative_distance, shape.num_attention_heads)
    out[net + "pooler.layernorm.weight"], out[net + "pooler.layernorm.bias"] = (C,), (C,)
    out[prefix + "classifier.weight"], out[prefix + "classifier.bias"] = (D, C), (D,)
    return out


# ---------------------------------------------------------------------------------------------------------
def beit_prepare(p: dict, shape: BeitShape, dtype, prefix: str = IN, features_only: bool = False):
    net = prefix + "beit."
    pw = p[net + "embeddings.patch_embeddings.projection.weight"]
    prep = dict(patch=prepare_linear(pw.reshape(pw.shape[0], -1), dtype), layers=[])
    for l in range(shape.num_hidden_layers):
        L = beit_layer_names(prefix, l)      # (k_proj has no bias: zeros in the fused one)
        prep["layers"].append(engine.prepare_block(p, L + "attention.", L + "attention.o_proj.weight", L + "mlp.fc1.weight",
                                                   L + "mlp.fc2.weight", dtype))
    if not features_only:
        prep["cls"] = prepare_linear(p[prefix + "classifier.weight"], dtype)
    return prep


def beit_droppath_scales(shape: BeitShape, n_img: int, drop: DropCfg, training: bool, device):
    """[(scale_attn, scale_mlp)] per layer: fp32 [n_img] DropPath factors (0 or 1 / (1 - rate)) or None where the rate is 0.  Each
    (layer, sub-layer) draws from a stream of its own (``drop.site(2 l + sub-layer)``), as ``swin_engine`` keys its blocks."""
    out = []
    for l, rate in enumerate(shape.drop_path_rates()):
        if not training or rate <= 0:
            out.append((None, None))
        else:
            out.append(tuple(ops.droppath_scale(n_img, rate, drop.site(2 * l + k), device) for k in range(2)))
    return out


def beit_forward(p: dict, prep, shape: BeitShape, pixels: torch.Tensor, dtype, need_grad: bool, prefix: str = IN, drop: DropCfg = NO_DROP,
                 training: bool = False, features_only: bool = False):
    """pixels fp32 [n_img, 3, R, R] (normalised) or uint8 [n_img, R, R, 3] (decoded) -> item vectors [n_img, D]
    (``GELU(classifier(LN(mean of the patch tokens)))``).  ``training``: apply DropPath with ``shape.drop_path_rates()`` and the streams of
    ``drop``.  ``features_only``: return ``(pooled [n_img, hidden], None)``, the pooler output = the classifier's input."""
    net = prefix + "beit."
    n_img = pixels.shape[0]
    eps = shape.layer_norm_eps
    C, heads, g = shape.hidden_size, shape.num_attention_heads, shape.grid
    engine.check_image_size(pixels, shape.image_size)
    T = shape.num_patches + 1
    patches = engine.patch_rows(pixels, shape.patch_size, dtype)
    e = ops.gemm_nt(patches, prep["patch"].w, bias=p[net + "embeddings.patch_embeddings.projection.bias"])
    x = ops.beit_assemble_fwd(e, p[net + "embeddings.cls_token"].reshape(-1), n_img)
    key_keep = torch.ones((n_img, T), device=x.device, dtype=torch.float32)
    desc = ops.attn_desc(n_img, T, heads, C // heads, False, float(C // heads) ** -0.5, ops.FLT_MIN_MASK, dtype)
    scales = beit_droppath_scales(shape, n_img, drop, training, x.device)
    saved_layers = []
    for l in range(shape.num_hidden_layers):
        L = beit_layer_names(prefix, l)
        w = prep["layers"][l]
        sc1, sc2 = scales[l]
        pos_bias = ops.beit_bias_expand(p[L + TABLE], g)
        xn, _, mean1, rstd1 = ops.layernorm_fwd(x, p[L + "layernorm_before.weight"], p[L + "layernorm_before.bias"], eps, save_z=False)
        qkv = ops.gemm_nt(xn, w["qkv"].w, bias=w["bqkv"])
        ctx = ops.attn_bias_fwd(desc, qkv, key_keep, pos_bias)
        a = ops.gemm_nt(ctx, w["o"].w)
        h = ops.layerscale_res_fwd(a, p[L + "attention.o_proj.bias"], p[L + "lambda_1"], x, sc1, T)
        hn, _, mean2, rstd2 = ops.layernorm_fwd(h, p[L + "layernorm_after.weight"], p[L + "layernorm_after.bias"], eps, save_z=False)
        pre = torch.empty((x.shape[0], w["f1"].w.shape[0]), device=x.device, dtype=dtype) if need_grad else None
        gl = ops.gemm_nt(hn, w["f1"].w, bias=p[L + "mlp.fc1.bias"], act=ACT_GELU, aux_out=pre, aux_deriv=need_grad)   # pre = GELU'(fc1)
        f = ops.gemm_nt(gl, w["f2"].w)
        out = ops.layerscale_res_fwd(f, p[L + "mlp.fc2.bias"], p[L + "lambda_2"], h, sc2, T)
        saved_layers.append((x, xn, mean1, rstd1, qkv, ctx, pos_bias, a, h, hn, mean2, rstd2, pre, gl, f, sc1, sc2))
        x = out
    pooled_raw = ops.beit_pool_fwd(x, n_img, T)
    pooled, _, mean_f, rstd_f = ops.layernorm_fwd(pooled_raw, p[net + "pooler.layernorm.weight"], p[net + "pooler.layernorm.bias"], eps,
                                                  save_z=False)
    if features_only:
        return pooled, None
    item, pre_c = engine.head_forward(pooled, prep["cls"], p[prefix + "classifier.bias"], need_grad)
    saved = (shape, n_img, T, desc, key_keep, patches, saved_layers, pooled_raw, mean_f, rstd_f, pooled, pre_c) if need_grad else None
    return item, saved


def beit_backward(p: dict, prep, saved, d_item: torch.Tensor, grads: dict, prefix: str = IN):
    """grads: name -> fp32 buffer (accumulated into; ``embeddings.cls_token`` is written); the q/k/v projections are handed out as row
    views of a fresh fused buffer (``k_proj`` has no bias: that third of the fused bias gradient is discarded).  A name that is missing
    from ``grads`` is frozen: a table or a lambda without a buffer skips its gradient work."""
    net = prefix + "beit."
    shape, n_img, T, desc, key_keep, patches, saved_layers, pooled_raw, mean_f, rstd_f, pooled, pre_c = saved
    C, g = shape.hidden_size, shape.grid
    dpooled = engine.head_backward(d_item, pre_c, pooled, prep["cls"], grads[prefix + "classifier.weight"], grads[prefix + "classifier.bias"], C)
    dpr, _ = ops.layernorm_bwd(dpooled, None, pooled_raw, mean_f, rstd_f, p[net + "pooler.layernorm.weight"],
                               grads[net + "pooler.layernorm.weight"], grads[net + "pooler.layernorm.bias"])
    dout = ops.beit_pool_bwd(dpr, n_img, T)
    for l in reversed(range(shape.num_hidden_layers)):
        L = beit_layer_names(prefix, l)
        A = L + "attention."
        w = prep["layers"][l]
        x, xn, mean1, rstd1, qkv, ctx, pos_bias, a, h, hn, mean2, rstd2, pre, gl, f, sc1, sc2 = saved_layers[l]
        # out = h + dp2 * lambda_2 * (fc2(gelu(fc1(LN2(h)))) + b2)
        df = ops.layerscale_res_bwd(dout, f, p[L + "mlp.fc2.bias"], p[L + "lambda_2"], sc2, T, dlam=grads.get(L + "lambda_2"),
                                    dbias=grads[L + "mlp.fc2.bias"])
        dhn = engine.mlp_backward(df, w, gl, pre, hn, grads[L + "mlp.fc2.weight"], grads[L + "mlp.fc1.bias"], grads[L + "mlp.fc1.weight"], C)
        dh, _ = ops.layernorm_bwd(dhn, None, h, mean2, rstd2, p[L + "layernorm_after.weight"], grads[L + "layernorm_after.weight"],
                                  grads[L + "layernorm_after.bias"], dres=dout)
        # h = x + dp1 * lambda_1 * (o_proj(ctx) + bo)
        da = ops.layerscale_res_bwd(dh, a, p[A + "o_proj.bias"], p[L + "lambda_1"], sc1, T, dlam=grads.get(L + "lambda_1"),
                                    dbias=grads[A + "o_proj.bias"])
        linear_wgrad_(da, ctx, grads[A + "o_proj.weight"])
        dctx = ops.gemm_nt(da, w["o"].wt, K=da.shape[1], N=C)
        gw, gb = engine.fused_qkv_grads(C, dctx.device)
        dtable = grads.get(L + TABLE)
        dqkv, dpos = ops.attn_bias_bwd(desc, qkv, key_keep, pos_bias, dctx, dbias=gb, need_dpos=dtable is not None)
        if dtable is not None:
            ops.beit_bias_reduce_(dpos, dtable, g)
        linear_wgrad_(dqkv, xn, gw)
        engine.hand_out_qkv(grads, A, gw, gb, C, key_bias="absent")
        dxn = ops.gemm_nt(dqkv, w["qkv"].wt, K=dqkv.shape[1], N=C)
        dout, _ = ops.layernorm_bwd(dxn, None, x, mean1, rstd1, p[L + "layernorm_before.weight"], grads[L + "layernorm_before.weight"],
                                    grads[L + "layernorm_before.bias"], dres=dh)
    engine.patch_embed_backward(dout, n_img, T - 1, patches, grads, net + "embeddings.")


def _no_buffer(names, needs, c, plan):
    skip = {n for l in range(c.shape.num_hidden_layers) for n in engine.qkv_names(beit_layer_names(c.prefix, l) + "attention.", key_bias="absent")}
    # a frozen bias table or layer scale gets no buffer: its gradient work is skipped (``beit_backward``)
    return skip | {n for n, nd in zip(names, needs) if not nd and n.endswith((TABLE, ".lambda_1", ".lambda_2"))}


TOWER = engine.Tower(
    prepare=lambda p, c, need_grad: beit_prepare(p, c.shape, c.dtype, c.prefix, features_only=c.features_only),
    plan=engine.no_plan,
    forward=lambda p, prep, x, c, need_grad: beit_forward(p, prep, c.shape, x, c.dtype, need_grad, c.prefix, c.drop, c.training,
                                                          features_only=c.features_only),
    backward=lambda p, prep, saved, d, grads, c: beit_backward(p, prep, saved, d, grads, c.prefix),
    no_buffer=_no_buffer)
