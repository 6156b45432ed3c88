"""``HipBeitForImageClassification``: parameter container with HuggingFace ``BeitForImageClassification``'s module tree, ``state_dict``
keys and parameter order (the reference loads it as the image network of ``Vit_Encoder``, ``V/model/encoders.py:24-31``, for
``CV_model_load`` names containing 'beit', ``V/model/model.py:26-27``, and replaces ``.classifier`` by ``Linear(hidden, embedding_dim)``,
``V/run.py:47-54``).  Forward arithmetic is in ``libmorec_hip.so`` (``functional.TowerFn`` over ``beit_engine.TOWER``); this class only owns the weights so
that a HF checkpoint loads key for key (``from_hf``), including the reference's pinned ``transformers==4.20.1`` key names
(``remap_legacy_beit_keys``).

Built: the released fine-tuning configuration -- a relative-position bias table per layer, layer scale, the mean-pool head.  Every
other switch of ``BeitConfig`` raises ``NotImplementedError`` naming it (``check_beit_config``)."""
import re
import types

import torch
import torch.nn as nn

from ..beit_engine import BeitShape


class _PatchEmbeddings(nn.Module):
    def __init__(self, s: BeitShape):
        super().__init__()
        self.projection = nn.Conv2d(s.num_channels, s.hidden_size, kernel_size=s.patch_size, stride=s.patch_size)


class _Embeddings(nn.Module):
    def __init__(self, s: BeitShape):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, s.hidden_size))
        self.patch_embeddings = _PatchEmbeddings(s)


class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = nn.Linear(C, C), nn.Linear(C, C, bias=False), nn.Linear(C, C), nn.Linear(C, C)


class _MLP(nn.Module):
    def __init__(self, C, I):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(C, I), nn.Linear(I, C)


class _RelativePositionBias(nn.Module):
    def __init__(self, s: BeitShape):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(torch.zeros(s.num_relative_distance, s.num_attention_heads))


class _Layer(nn.Module):
    def __init__(self, s: BeitShape):
        super().__init__()
        self.attention = _Attention(s.hidden_size)
        self.layernorm_before = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)
        self.layernorm_after = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)
        self.mlp = _MLP(s.hidden_size, s.intermediate_size)
        self.lambda_1 = nn.Parameter(s.layer_scale_init_value * torch.ones(s.hidden_size))
        self.lambda_2 = nn.Parameter(s.layer_scale_init_value * torch.ones(s.hidden_size))
        self.relative_position_bias = _RelativePositionBias(s)


class _Pooler(nn.Module):
    def __init__(self, s: BeitShape):
        super().__init__()
        self.layernorm = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)


class _Beit(nn.Module):
    def __init__(self, s: BeitShape):
        super().__init__()
        self.embeddings = _Embeddings(s)
        self.layers = nn.ModuleList([_Layer(s) for _ in range(s.num_hidden_layers)])
        self.pooler = _Pooler(s)


_LEGACY = [   # transformers 4.20.1 (README.md:44) -> installed names
    (r"^beit\.encoder\.layer\.", "beit.layers."),
    (r"\.attention\.attention\.query\.", ".attention.q_proj."), (r"\.attention\.attention\.key\.", ".attention.k_proj."),
    (r"\.attention\.attention\.value\.", ".attention.v_proj."),
    (r"\.attention\.attention\.relative_position_bias\.", ".relative_position_bias."),
    (r"\.attention\.output\.dense\.", ".attention.o_proj."),
    (r"\.intermediate\.dense\.", ".mlp.fc1."), (r"(layers\.\d+)\.output\.dense\.", r"\1.mlp.fc2."),
]


def remap_legacy_beit_keys(sd: dict) -> dict:
    """Rename a ``transformers==4.20.1``-era ``BeitForImageClassification`` ``state_dict`` (what the reference's checkpoints hold:
    ``beit.encoder.layer.N.attention.attention.{query,key,value}``, ``attention.attention.relative_position_bias.
    relative_position_bias_table``, ``attention.output.dense``, ``intermediate.dense``, ``output.dense``) to the installed layout; the
    legacy ``relative_position_index`` buffers are dropped (the index is a function of the grid); names already in the installed layout
    pass through."""
    out = {}
    for k, v in sd.items():
        if k.endswith("relative_position_index"):
            continue
        for pat, rep in _LEGACY:
            k = re.sub(pat, rep, k)
        out[k] = v
    return out


def check_beit_config(c) -> None:
    """Raise ``NotImplementedError`` naming the option for every ``BeitConfig`` switch outside the released fine-tuning configuration."""
    def bad(name, why):
        raise NotImplementedError(f"BEiT tower: {name} {why}")
    if getattr(c, "use_shared_relative_position_bias", False):
        bad("use_shared_relative_position_bias", "(one table shared by all layers) is not built: the tower keeps one table per layer")
    if getattr(c, "use_absolute_position_embeddings", False):
        bad("use_absolute_position_embeddings", "is not built: positions enter through the relative-position bias only")
    if getattr(c, "use_mask_token", False):
        bad("use_mask_token", "(masked image modelling) is not built")
    if not getattr(c, "use_mean_pooling", True):
        bad("use_mean_pooling=False", "([CLS] head with a final LayerNorm) is not built: the head is the mean over the patch tokens")
    if not getattr(c, "use_relative_position_bias", True):
        bad("use_relative_position_bias=False", "is not built: every layer owns a relative-position bias table")
    if not float(getattr(c, "layer_scale_init_value", 0.1)) > 0:
        bad("layer_scale_init_value <= 0", "(no layer scale) is not built")
    if float(getattr(c, "hidden_dropout_prob", 0.0)):
        bad("hidden_dropout_prob", "must be 0 (hidden dropout is not built; 0.0 in the released configurations)")
    if float(getattr(c, "attention_probs_dropout_prob", 0.0)):
        bad("attention_probs_dropout_prob", "must be 0 (attention dropout is not built; 0.0 in the released configurations)")


class HipBeitForImageClassification(nn.Module):
    def __init__(self, shape: BeitShape, num_labels: int = 1000, initializer_range: float = 0.02):
        super().__init__()
        self.shape = shape
        self.config = types.SimpleNamespace(model_type="beit", image_size=shape.image_size, patch_size=shape.patch_size,
                                            num_channels=shape.num_channels, hidden_size=shape.hidden_size,
                                            num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
                                            intermediate_size=shape.intermediate_size, layer_norm_eps=shape.layer_norm_eps,
                                            drop_path_rate=shape.drop_path_rate, layer_scale_init_value=shape.layer_scale_init_value,
                                            use_relative_position_bias=True, use_shared_relative_position_bias=False,
                                            use_absolute_position_embeddings=False, use_mask_token=False, use_mean_pooling=True,
                                            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        self.beit = _Beit(shape)
        self.classifier = nn.Linear(shape.hidden_size, num_labels)      # V/run.py:47-54 replaces it by Linear(hidden, embedding_dim)
        for m in self.modules():       # BeitPreTrainedModel._init_weights
            if isinstance(m, (nn.Linear, nn.Conv2d)):
                nn.init.normal_(m.weight, std=initializer_range)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    @staticmethod
    def from_hf(hf_model) -> "HipBeitForImageClassification":
        """Adopt a HuggingFace ``BeitForImageClassification`` (its ``classifier`` as it stands): same keys and parameter order, weights
        copied.  Anything else -- no model, another family -- is refused."""
        c = getattr(hf_model, "config", None)
        if c is None or getattr(c, "model_type", None) != "beit" or not hasattr(hf_model, "classifier"):
            raise NotImplementedError(f"BEiT tower: from_hf adopts a HuggingFace BeitForImageClassification, got {type(hf_model).__name__}")
        check_beit_config(c)
        image = c.image_size if isinstance(c.image_size, int) else c.image_size[0]
        patch = c.patch_size if isinstance(c.patch_size, int) else c.patch_size[0]
        shape = BeitShape(image_size=image, patch_size=patch, num_channels=c.num_channels, hidden_size=c.hidden_size,
                          num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                          intermediate_size=c.intermediate_size, layer_norm_eps=c.layer_norm_eps, drop_path_rate=c.drop_path_rate,
                          layer_scale_init_value=c.layer_scale_init_value)
        m = HipBeitForImageClassification(shape, num_labels=hf_model.classifier.out_features)
        sd = remap_legacy_beit_keys(hf_model.state_dict())
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not missing, missing
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), hf_model.named_parameters()):
            assert n1 == n2, (n1, n2)       # same ORDER too: V/run.py:58-60 freezes parameters by index
            p1.requires_grad = p2.requires_grad
        return m
