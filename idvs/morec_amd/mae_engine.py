"""Host-side orchestration of the MAE (ViT) item tower: explicit forward and hand-derived backward of
``MAE_Encoder.forward`` (``V/model/encoders.py:7-21``) = ``GELU(cv_proj(ViTMAEModel(x)[0][:, 0]))`` (HF
``transformers/models/vit_mae/modeling_vit_mae.py``; the reference selects it by ``'mae' in CV_model_load or "checkpoint" in
CV_model_load``, ``V/model/model.py:28-29``).

``ViTMAEModel`` masks ``mask_ratio`` of the patches in EVERY forward, evaluation included (``random_masking``, ``:297-327``): ViT-B/16 at
224 px runs its encoder over 1 + 49 = 50 tokens per image.  The front of the tower (``csrc/mae.hip``) therefore ranks the noise first and
builds im2col rows, patch-GEMM rows and position sums for the kept patches only.  The blocks are the pre-LN blocks ``swin_engine`` runs
(every residual sum is formed by the LayerNorm kernel that consumes it) without windows, relative bias, DropPath or merging; attention is
global, unmasked and non-causal: ``morec_attn_fwd`` / ``_bwd`` with a ``key_keep`` of ones.  The final LayerNorm is per-row and only the
[CLS] row is read, so it runs on the [CLS] rows alone.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass

import torch

from . import engine, ops
from ._lib import ACT_GELU
from .engine import linear_wgrad_, prepare_linear

ENC = "cv_encoder."
MAE_SEED_TRAIN = 0x6D61655F6B656570       # XOR-ed into the step's dropout base seed: the masking stream of a training step
MAE_SEED_EVAL = 0x6D61655F6576616C        # the fixed seed of evaluation passes (keyed by the row within the call)


@dataclass
class MaeShape:
    image_size: int = 224
    patch_size: int = 16
    num_channels: int = 3
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    layer_norm_eps: float = 1e-12
    mask_ratio: float = 0.75

    @staticmethod
    def named(name: str) -> "MaeShape":
        """Shapes keyed on ``CV_model_load`` the way ``SwinShape.named`` is; a name that only says "mae" / "checkpoint" (the reference's
        ``V/model/model.py:28``) is the base model, the only one whose width its ``MAE_Encoder`` fits."""
        table = {
            "mae_micro": dict(image_size=32, patch_size=4, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256),
            "mae_large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096),
            "mae_base": dict(),
        }
        for key, kw in table.items():
            if key in name:
                return MaeShape(**kw)
        if "mae" in name or "checkpoint" in name:
            return MaeShape()
        raise ValueError(f"unknown CV_model_load {name!r}")

    @property
    def num_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2

    def len_keep(self, mask_ratio=None) -> int:
        return ops.mae_len_keep(self.num_patches, self.mask_ratio if mask_ratio is None else mask_ratio)


def mae_layer_names(prefix: str, l: int) -> str:
    return prefix + f"image_net.layers.{l}."


def mae_param_shapes(shape: MaeShape, D: int, prefix: str = ENC):
    """``named_parameters`` inventory of ``MAE_Encoder`` over HF ``ViTMAEModel``, in the installed-HF registration order
    (``V/run.py:58-60`` freezes by parameter index, and the frozen ``position_embeddings`` counts), then the encoder's ``cv_proj``."""
    net = prefix + "image_net."
    C, I = shape.hidden_size, shape.intermediate_size
    out = OrderedDict()
    out[net + "embeddings.cls_token"] = (1, 1, C)
    out[net + "embeddings.position_embeddings"] = (1, shape.num_patches + 1, C)
    out[net + "embeddings.patch_embeddings.projection.weight"] = (C, shape.num_channels, shape.patch_size, shape.patch_size)
    out[net + "embeddings.patch_embeddings.projection.bias"] = (C,)
    for l in range(shape.num_hidden_layers):
        L = mae_layer_names(prefix, l)
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            out[L + f"attention.{n}.weight"], out[L + f"attention.{n}.bias"] = (C, C), (C,)
        for n in ("layernorm_before", "layernorm_after"):
            out[L + n + ".weight"], out[L + n + ".bias"] = (C,), (C,)
        out[L + "mlp.fc1.weight"], out[L + "mlp.fc1.bias"] = (I, C), (I,)
        out[L + "mlp.fc2.weight"], out[L + "mlp.fc2.bias"] = (C, I), (C,)
    out[net + "layernorm.weight"], out[net + "layernorm.bias"] = (C,), (C,)
    out[prefix + "cv_proj.weight"], out[prefix + "cv_proj.bias"] = (D, C), (D,)
    return out


# ---------------------------------------------------------------------------------------------------------
def mae_prepare(p: dict, shape: MaeShape, dtype, prefix: str = ENC, features_only: bool = False):
    net = prefix + "image_net."
    pw = p[net + "embeddings.patch_embeddings.projection.weight"]
    prep = dict(patch=prepare_linear(pw.reshape(pw.shape[0], -1), dtype), layers=[])
    for l in range(shape.num_hidden_layers):
        L = mae_layer_names(prefix, l)
        prep["layers"].append(engine.prepare_block(p, L + "attention.", L + "attention.o_proj.weight", L + "mlp.fc1.weight",
                                                   L + "mlp.fc2.weight", dtype))
    if not features_only:
        prep["cls"] = prepare_linear(p[prefix + "cv_proj.weight"], dtype)
    return prep


def mae_keep(shape: MaeShape, n_img: int, device, noise=None, seed: int = 0, mask_ratio=None):
    """int32 [n_img, len_keep] kept-patch ids of a forward: from ``noise`` (HF's ``noise=`` argument) or drawn from ``seed``."""
    return ops.mae_keep_ids(n_img, shape.num_patches, shape.len_keep(mask_ratio), noise=noise, seed=seed, device=device)


def mae_forward(p: dict, prep, shape: MaeShape, pixels: torch.Tensor, dtype, need_grad: bool, prefix: str = ENC, noise=None,
                seed: int = 0, mask_ratio=None, features_only: bool = False):
    """pixels fp32 [n_img, 3, R, R] (normalised) or uint8 [n_img, R, R, 3] (decoded) -> item vectors [n_img, D]
    (``GELU(cv_proj(LN(encoder(embed(x)))[:, 0]))``).  ``noise`` fp32 [n_img, N] decides the kept patches as HF's ``noise=`` does; without
    it they are drawn from ``seed``.  ``mask_ratio``: override of ``shape.mask_ratio`` (0 keeps every patch, in shuffled order).
    ``features_only``: return ``(LN(x)[:, 0] [n_img, hidden], None)`` = ``image_net(x)[0][:, 0]``, the input of ``cv_proj``."""
    net = prefix + "image_net."
    n_img = pixels.shape[0]
    eps = shape.layer_norm_eps
    C, heads = shape.hidden_size, shape.num_attention_heads
    engine.check_image_size(pixels, shape.image_size)
    keep = mae_keep(shape, n_img, pixels.device, noise, seed, mask_ratio)
    Lk = keep.shape[1]
    T = Lk + 1
    src, ids = engine.image_source(pixels)      # ImageIds: kept patches from keep[k], pixels from catalogue row ids[k]
    patches = ops.mae_patchify_keep(src, keep, shape.patch_size, dtype, ids=ids)
    e = ops.gemm_nt(patches, prep["patch"].w, bias=p[net + "embeddings.patch_embeddings.projection.bias"])
    x = ops.mae_assemble_fwd(e, p[net + "embeddings.cls_token"].reshape(-1), p[net + "embeddings.position_embeddings"].reshape(-1, C), keep)
    key_keep = torch.ones((n_img, T), device=x.device, dtype=torch.float32)
    desc = ops.attn_desc(n_img, T, heads, C // heads, False, float(C // heads) ** -0.5, ops.FLT_MIN_MASK, dtype)
    pending = None          # (f, b2, h): the previous block's MLP output whose residual sum the next LayerNorm forms
    saved_layers = []
    for l in range(shape.num_hidden_layers):
        L = mae_layer_names(prefix, l)
        w = prep["layers"][l]
        g1, b1 = p[L + "layernorm_before.weight"], p[L + "layernorm_before.bias"]
        if pending is None:
            xn, _, mean1, rstd1 = ops.layernorm_fwd(x, g1, b1, eps, save_z=False)
        else:
            f, b2, h = pending
            xn, x, mean1, rstd1 = ops.layernorm_fwd(f, g1, b1, eps, bias=b2, res=h, z_inplace=True)
        qkv = ops.gemm_nt(xn, w["qkv"].w, bias=w["bqkv"])
        ctx = ops.attn_fwd(desc, qkv, key_keep)
        a = ops.gemm_nt(ctx, w["o"].w)
        hn, h, mean2, rstd2 = ops.layernorm_fwd(a, p[L + "layernorm_after.weight"], p[L + "layernorm_after.bias"], eps,
                                                bias=p[L + "attention.o_proj.bias"], res=x, z_inplace=True)
        pre = torch.empty((x.shape[0], w["f1"].w.shape[0]), device=x.device, dtype=dtype) if need_grad else None
        g = ops.gemm_nt(hn, w["f1"].w, bias=p[L + "mlp.fc1.bias"], act=ACT_GELU, aux_out=pre, aux_deriv=need_grad)   # pre = GELU'(fc1)
        f = ops.gemm_nt(g, w["f2"].w)
        pending = (f, p[L + "mlp.fc2.bias"], h)
        saved_layers.append((x, xn, mean1, rstd1, qkv, ctx, h, hn, mean2, rstd2, pre, g))
    # final LayerNorm on the [CLS] rows only: the last residual sum is formed for those rows alone
    f, b2, h = pending
    f0 = ops.strided_rows_copy(f, torch.empty((n_img, C), device=x.device, dtype=dtype), n_img, C, T, 1)
    h0 = ops.strided_rows_copy(h, torch.empty((n_img, C), device=x.device, dtype=dtype), n_img, C, T, 1)
    cls_n, z_last, mean_f, rstd_f = ops.layernorm_fwd(f0, p[net + "layernorm.weight"], p[net + "layernorm.bias"], eps, bias=b2, res=h0,
                                                      z_inplace=True)
    if features_only:
        return cls_n, None
    item, pre_c = engine.head_forward(cls_n, prep["cls"], p[prefix + "cv_proj.bias"], need_grad)
    saved = (shape, n_img, T, desc, key_keep, keep, patches, saved_layers, z_last, mean_f, rstd_f, cls_n, pre_c) if need_grad else None
    return item, saved


def mae_backward(p: dict, prep, saved, d_item: torch.Tensor, grads: dict, prefix: str = ENC):
    """grads: name -> fp32 buffer (accumulated into; ``embeddings.cls_token`` is written); the q/k/v projections are handed out as row
    views of a fresh fused buffer.  ``embeddings.position_embeddings`` is frozen in HF (``requires_grad=False``): no gradient."""
    net = prefix + "image_net."
    shape, n_img, T, desc, key_keep, keep, patches, saved_layers, z_last, mean_f, rstd_f, cls_n, pre_c = saved
    C = shape.hidden_size
    n_layers = shape.num_hidden_layers
    dcls_n = engine.head_backward(d_item, pre_c, cls_n, prep["cls"], grads[prefix + "cv_proj.weight"], grads[prefix + "cv_proj.bias"], C)
    # gradient at the last block's output sum, [CLS] rows (every other row: zero); its column sums are that block's fc2.bias gradient
    dz0, _ = ops.layernorm_bwd(dcls_n, None, z_last, mean_f, rstd_f, p[net + "layernorm.weight"], grads[net + "layernorm.weight"],
                               grads[net + "layernorm.bias"], dbias=grads[mae_layer_names(prefix, n_layers - 1) + "mlp.fc2.bias"])
    dout = torch.zeros((n_img * T, C), device=dz0.device, dtype=dz0.dtype)
    ops.strided_rows_copy(dz0, dout, n_img, C, 1, T)
    for l in reversed(range(n_layers)):
        L = mae_layer_names(prefix, l)
        A = L + "attention."
        w = prep["layers"][l]
        x, xn, mean1, rstd1, qkv, ctx, h, hn, mean2, rstd2, pre, g = saved_layers[l]
        # MLP branch: out = h + fc2(gelu(fc1(LN2(h)))) + b2
        dhn = engine.mlp_backward(dout, w, g, pre, hn, grads[L + "mlp.fc2.weight"], grads[L + "mlp.fc1.bias"], grads[L + "mlp.fc1.weight"], C)
        # h = x + o_proj(ctx) + bo: dh = LN2'(dhn) + dout
        dh, da = ops.layernorm_bwd(dhn, None, h, mean2, rstd2, p[L + "layernorm_after.weight"], grads[L + "layernorm_after.weight"],
                                   grads[L + "layernorm_after.bias"], dbias=grads[A + "o_proj.bias"], dres=dout)
        linear_wgrad_(da, ctx, grads[A + "o_proj.weight"])
        dctx = ops.gemm_nt(da, w["o"].wt, K=da.shape[1], N=C)
        gw, gb = engine.fused_qkv_grads(C, dctx.device)
        dqkv = ops.attn_bwd(desc, qkv, key_keep, dctx, dbias=gb)      # + d(q|k|v bias) = column sums of dqkv
        linear_wgrad_(dqkv, xn, gw)
        engine.hand_out_qkv(grads, A, gw, gb, C, key_bias="zero")
        dxn = ops.gemm_nt(dqkv, w["qkv"].wt, K=dqkv.shape[1], N=C)
        # x is the previous block's output sum (or the assembled embeddings): its bias gradient is the previous block's fc2.bias
        prev_b2 = grads[mae_layer_names(prefix, l - 1) + "mlp.fc2.bias"] if l > 0 else None
        dout, _ = ops.layernorm_bwd(dxn, None, x, mean1, rstd1, p[L + "layernorm_before.weight"], grads[L + "layernorm_before.weight"],
                                    grads[L + "layernorm_before.bias"], dbias=prev_b2, dres=dh)
    engine.patch_embed_backward(dout, n_img, T - 1, patches, grads, net + "embeddings.")


def _no_buffer(names, needs, c, plan):
    skip = {n for l in range(c.shape.num_hidden_layers) for n in engine.qkv_names(mae_layer_names(c.prefix, l) + "attention.")}
    return skip | {c.prefix + "image_net.embeddings.position_embeddings"}      # frozen in HF: no gradient


TOWER = engine.Tower(
    prepare=lambda p, c, need_grad: mae_prepare(p, c.shape, c.dtype, c.prefix, features_only=c.features_only),
    plan=engine.no_plan,
    forward=lambda p, prep, x, c, need_grad: mae_forward(p, prep, c.shape, x, c.dtype, need_grad, c.prefix, features_only=c.features_only,
                                                         **c.kw),
    backward=lambda p, prep, saved, d, grads, c: mae_backward(p, prep, saved, d, grads, c.prefix),
    no_buffer=_no_buffer)
