"""``HipViTMAEModel``: parameter container with HuggingFace ``ViTMAEModel``'s module tree, ``state_dict`` keys and parameter order
(the reference loads it as the image network of ``MAE_Encoder``, ``V/model/encoders.py:7-21``, for ``CV_model_load`` names containing
'mae' or 'checkpoint', ``V/model/model.py:28-29``).  Forward arithmetic is in ``libmorec_hip.so`` (``functional.TowerFn`` over ``mae_engine.TOWER``); this
class only owns the weights so that a HF checkpoint loads key for key (``from_hf``), including the reference's pinned
``transformers==4.20.1`` key names (``remap_legacy_mae_keys``).  The MAE decoder is not part of ``ViTMAEModel`` and is not built."""
import math
import re
import types

import torch
import torch.nn as nn

from ..mae_engine import MaeShape


def sincos_position_table(grid: int, dim: int, temperature: float = 10000.0) -> torch.Tensor:
    """fp32 [grid * grid + 1, dim]: the fixed 2-D sin-cos position table of ``ViTMAEEmbeddings.initialize_weights``.  Row 0 ([CLS]) is
    zero; patch (h, w), row-major, gets frequencies ``omega_k = temperature^(-k / (dim / 4))`` as ``[sin(w o) | cos(w o) | sin(h o) |
    cos(h o)]`` -- the two halves in the rotated order the pretrained MAE weights rely on (w first).  fp64 arithmetic, rounded once."""
    if dim % 4:
        raise ValueError(f"hidden size {dim} is not divisible by 4")
    q = dim // 4
    omega = torch.arange(q, dtype=torch.float64) / q
    omega = 1.0 / temperature ** omega
    hh, ww = torch.meshgrid(torch.arange(grid, dtype=torch.float64), torch.arange(grid, dtype=torch.float64), indexing="ij")
    ah, aw = hh.reshape(-1).outer(omega), ww.reshape(-1).outer(omega)
    table = torch.cat([aw.sin(), aw.cos(), ah.sin(), ah.cos()], dim=1)
    return torch.cat([torch.zeros(1, dim, dtype=torch.float64), table], dim=0).to(torch.float32)


class _PatchEmbeddings(nn.Module):
    def __init__(self, s: MaeShape):
        super().__init__()
        self.projection = nn.Conv2d(s.num_channels, s.hidden_size, kernel_size=s.patch_size, stride=s.patch_size)


class _Embeddings(nn.Module):
    def __init__(self, s: MaeShape):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, s.hidden_size))
        self.patch_embeddings = _PatchEmbeddings(s)
        self.position_embeddings = nn.Parameter(torch.zeros(1, s.num_patches + 1, s.hidden_size), requires_grad=False)


class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)


class _MLP(nn.Module):
    def __init__(self, C, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, I), nn.Linear(I, C)


class _Layer(nn.Module):
    def __init__(self, s: MaeShape):
        super().__init__()
        self.attention = _Attention(s.hidden_size)
        self.layernorm_before = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)
        self.layernorm_after = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)
        self.mlp = _MLP(s.hidden_size, s.intermediate_size)


_LEGACY = [   # transformers 4.20.1 (README.md:44) -> installed names (the "ViTModel" entry of transformers/conversion_mapping.py)
    (r"^encoder\.layer\.", "layers."), (r"\.encoder\.layer\.", ".layers."),
    (r"\.attention\.attention\.query\.", ".attention.q_proj."), (r"\.attention\.attention\.key\.", ".attention.k_proj."),
    (r"\.attention\.attention\.value\.", ".attention.v_proj."), (r"\.attention\.output\.dense\.", ".attention.o_proj."),
    (r"\.intermediate\.dense\.", ".mlp.fc1."), (r"(layers\.\d+)\.output\.dense\.", r"\1.mlp.fc2."),
]


def remap_legacy_mae_keys(sd: dict) -> dict:
    """Rename a ``transformers==4.20.1``-era ``ViTMAEModel`` ``state_dict`` (what the reference's checkpoints hold:
    ``encoder.layer.N.attention.attention.{query,key,value}``, ``attention.output.dense``, ``intermediate.dense``, ``output.dense``) to the
    installed layout; names already in that layout pass through."""
    out = {}
    for k, v in sd.items():
        for pat, rep in _LEGACY:
            k = re.sub(pat, rep, k)
        out[k] = v
    return out


class HipViTMAEModel(nn.Module):
    def __init__(self, shape: MaeShape, initializer_range: float = 0.02):
        super().__init__()
        self.shape = shape
        self.config = types.SimpleNamespace(image_size=shape.image_size, patch_size=shape.patch_size, num_channels=shape.num_channels,
                                            hidden_size=shape.hidden_size, num_hidden_layers=shape.num_hidden_layers,
                                            num_attention_heads=shape.num_attention_heads, intermediate_size=shape.intermediate_size,
                                            layer_norm_eps=shape.layer_norm_eps, mask_ratio=shape.mask_ratio, eval_mask_ratio=None,
                                            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        self.embeddings = _Embeddings(shape)
        self.layers = nn.ModuleList([_Layer(shape) for _ in range(shape.num_hidden_layers)])
        self.layernorm = nn.LayerNorm(shape.hidden_size, eps=shape.layer_norm_eps)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=initializer_range)
                nn.init.zeros_(m.bias)
        with torch.no_grad():       # ViTMAEEmbeddings.initialize_weights
            w = self.embeddings.patch_embeddings.projection.weight
            nn.init.xavier_uniform_(w.view(w.shape[0], -1))
            nn.init.zeros_(self.embeddings.patch_embeddings.projection.bias)
            nn.init.normal_(self.embeddings.cls_token, std=initializer_range)
            self.embeddings.position_embeddings.copy_(sincos_position_table(math.isqrt(shape.num_patches), shape.hidden_size)[None])

    @staticmethod
    def from_hf(hf_model) -> "HipViTMAEModel":
        """Adopt a HuggingFace ``ViTMAEModel``: same keys and parameter order, weights (the position table included) copied."""
        c = hf_model.config
        if float(getattr(c, "hidden_dropout_prob", 0.0)) or float(getattr(c, "attention_probs_dropout_prob", 0.0)):
            raise NotImplementedError("MAE hidden / attention dropout (0.0 in every MAE config the reference ships)")
        if not getattr(c, "qkv_bias", True):
            raise NotImplementedError("MAE without q/k/v biases")
        image = c.image_size if isinstance(c.image_size, int) else c.image_size[0]
        patch = c.patch_size if isinstance(c.patch_size, int) else c.patch_size[0]
        shape = MaeShape(image_size=image, patch_size=patch, num_channels=c.num_channels, hidden_size=c.hidden_size,
                         num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                         intermediate_size=c.intermediate_size, layer_norm_eps=c.layer_norm_eps, mask_ratio=c.mask_ratio)
        m = HipViTMAEModel(shape)
        sd = remap_legacy_mae_keys(hf_model.state_dict())
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not missing, missing
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), hf_model.named_parameters()):
            assert n1 == n2, (n1, n2)       # same ORDER too: V/run.py:58-60 freezes parameters by index
            p1.requires_grad = p2.requires_grad
        return m
