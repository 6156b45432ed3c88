"""``HipOPTModel``: parameter container with HuggingFace ``OPTModel``'s module tree, ``state_dict`` keys and parameter order (the
reference builds ``OPTModel.from_pretrained(...)`` at ``T/run.py:41-47`` and wraps it in ``Text_Encoder_mean``, ``T/model/encoders.py:
31-50``).  Forward arithmetic is in ``libmorec_hip.so`` (``functional.TowerFn`` over ``opt_engine.TOWER``); this class only owns the weights, so a HF
checkpoint's ``state_dict`` loads key for key (``from_hf``; keys of an ``OPTForCausalLM`` checkpoint lose their leading ``model.``).
The registration order is the installed transformers': the decoder-level ``final_layer_norm`` before the layers, and k, v, q, out inside
``self_attn`` (``tests/golden/g30_opt_keys.json``) -- ``--freeze_paras_before`` counts by it."""
import types

import torch
import torch.nn as nn

from ..opt_engine import PAD_ID, OptShape, check_opt_config


class _Attention(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H), nn.Linear(H, H)


class _Layer(nn.Module):
    def __init__(self, s: OptShape):
        super().__init__()
        self.self_attn = _Attention(s.hidden_size)
        self.self_attn_layer_norm = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)
        self.fc1 = nn.Linear(s.hidden_size, s.ffn_dim)
        self.fc2 = nn.Linear(s.ffn_dim, s.hidden_size)
        self.final_layer_norm = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)


class _Decoder(nn.Module):
    def __init__(self, s: OptShape):
        super().__init__()
        self.embed_tokens = nn.Embedding(s.vocab_size, s.hidden_size, padding_idx=s.pad_token_id)
        self.embed_positions = nn.Embedding(s.num_positions, s.hidden_size)
        self.final_layer_norm = nn.LayerNorm(s.hidden_size, eps=s.layer_norm_eps)
        self.layers = nn.ModuleList([_Layer(s) for _ in range(s.num_hidden_layers)])


class _OptConfig(types.SimpleNamespace):
    """``OPTConfig`` names its probabilities ``dropout`` / ``attention_dropout``; the models read a text tower's as BERT's are named."""

    @property
    def hidden_dropout_prob(self):
        return self.dropout

    @property
    def attention_probs_dropout_prob(self):
        return self.attention_dropout


def strip_model_prefix(sd: dict) -> dict:
    """Checkpoint keys of ``OPTForCausalLM`` (``model.decoder...``) as ``OPTModel`` names them; ``lm_head`` is dropped."""
    out = {}
    for k, v in sd.items():
        if k.startswith("lm_head."):
            continue
        out[k[len("model."):] if k.startswith("model.") else k] = v
    return out


class HipOPTModel(nn.Module):
    def __init__(self, shape: OptShape, init_std: float = 0.02, dropout: float = 0.1, attention_dropout: float = 0.0):
        super().__init__()
        if shape.pad_token_id != PAD_ID:
            raise NotImplementedError(f"OPT tower: pad_token_id={shape.pad_token_id} (the kernels skip word row {PAD_ID})")
        self.shape = shape
        self.config = _OptConfig(model_type="opt", vocab_size=shape.vocab_size, hidden_size=shape.hidden_size,
                                 word_embed_proj_dim=shape.hidden_size, num_hidden_layers=shape.num_hidden_layers,
                                 num_attention_heads=shape.num_attention_heads, ffn_dim=shape.ffn_dim,
                                 max_position_embeddings=shape.max_position_embeddings, pad_token_id=shape.pad_token_id,
                                 bos_token_id=2, eos_token_id=2, dropout=dropout, attention_dropout=attention_dropout,
                                 activation_function="relu", do_layer_norm_before=True, layerdrop=0.0, enable_bias=True,
                                 layer_norm_elementwise_affine=True, _remove_final_layer_norm=False)
        self.decoder = _Decoder(shape)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=init_std)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=init_std)
                if m.padding_idx is not None:
                    with torch.no_grad():
                        m.weight[m.padding_idx].zero_()

    @staticmethod
    def from_hf(hf_model) -> "HipOPTModel":
        """Adopt a HuggingFace ``OPTModel`` (what ``T/run.py:45`` constructs): same keys in the same order, weights copied."""
        c = hf_model.config
        check_opt_config(c)
        shape = OptShape(vocab_size=c.vocab_size, hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers,
                         num_attention_heads=c.num_attention_heads, ffn_dim=c.ffn_dim, max_position_embeddings=c.max_position_embeddings,
                         pad_token_id=c.pad_token_id)
        m = HipOPTModel(shape, dropout=float(getattr(c, "dropout", 0.1)), attention_dropout=float(getattr(c, "attention_dropout", 0.0)))
        sd = strip_model_prefix(hf_model.state_dict())
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not missing, missing
        hf_named = [(n[len("model."):] if n.startswith("model.") else n, q) for n, q in hf_model.named_parameters()
                    if not n.startswith("lm_head.")]
        for (n1, p1), (n2, p2) in zip(m.named_parameters(), hf_named):
            assert n1 == n2, (n1, n2)       # same ORDER too: T/run.py:73-75 freezes parameters by index
            p1.requires_grad = p2.requires_grad
        return m
