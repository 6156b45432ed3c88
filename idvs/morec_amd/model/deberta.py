"""``HipDebertaModel``: parameter container with HuggingFace ``DebertaModel``'s module tree, ``state_dict`` keys and parameter order (the
reference builds ``DebertaModel.from_pretrained(...)`` in its DSSM package, ``bce_text/main-end2end(DSSM)/run.py:26-31``, and wraps it in
``Text_Encoder``).  Forward arithmetic is in ``libmorec_hip.so`` (``functional.TowerFn`` over ``deberta_engine.TOWER``); this class only owns the weights, so
a HF checkpoint's ``state_dict`` loads key for key (``from_hf``; keys of a ``DebertaFor...`` checkpoint lose their leading ``deberta.``).
The registration order is the installed transformers': per layer ``q_bias``, ``v_bias``, ``in_proj.weight``, ``pos_proj.weight``,
``pos_q_proj.weight``, ``pos_q_proj.bias``, then the output and FFN parameters; ``encoder.rel_embeddings.weight`` LAST
(``tests/golden/g31_deberta_keys.json``) -- ``--freeze_paras_before`` counts by it.  ``in_proj.weight`` keeps HF's interleaved row layout
(``[h][q|k|v][dh]``) in the ``state_dict``; ``deberta_engine`` permutes it for the kernels."""
import types

import torch
import torch.nn as nn

from ..deberta_engine import DebertaShape, check_deberta_config


class _SelfAttention(nn.Module):
    """(``named_parameters`` lists a module's own parameters before its sub-modules': q_bias, v_bias, then the three Linears.)"""

    def __init__(self, H):
        super().__init__()
        self.in_proj = nn.Linear(H, 3 * H, bias=False)
        self.q_bias = nn.Parameter(torch.zeros(H))
        self.v_bias = nn.Parameter(torch.zeros(H))
        self.pos_proj = nn.Linear(H, H, bias=False)
        self.pos_q_proj = nn.Linear(H, H)


class _LayerNorm(nn.Module):
    """``DebertaLayerNorm``: the ordinary LayerNorm computed in fp32 (keys ``weight`` / ``bias``)."""

    def __init__(self, H):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(H))
        self.bias = nn.Parameter(torch.zeros(H))


class _SelfOutput(nn.Module):
    def __init__(self, n_in, H):
        super().__init__()
        self.dense = nn.Linear(n_in, H)
        self.LayerNorm = _LayerNorm(H)


class _Attention(nn.Module):
    def __init__(self, H):
        super().__init__()
        self.self = _SelfAttention(H)
        self.output = _SelfOutput(H, H)


class _Intermediate(nn.Module):
    def __init__(self, H, I):
        super().__init__()
        self.dense = nn.Linear(H, I)


class _Layer(nn.Module):
    def __init__(self, s: DebertaShape):
        super().__init__()
        self.attention = _Attention(s.hidden_size)
        self.intermediate = _Intermediate(s.hidden_size, s.intermediate_size)
        self.output = _SelfOutput(s.intermediate_size, s.hidden_size)


class _Embeddings(nn.Module):
    def __init__(self, s: DebertaShape):
        super().__init__()
        self.word_embeddings = nn.Embedding(s.vocab_size, s.hidden_size, padding_idx=s.pad_token_id)
        self.LayerNorm = _LayerNorm(s.hidden_size)


class _Encoder(nn.Module):
    def __init__(self, s: DebertaShape):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(s) for _ in range(s.num_hidden_layers)])
        self.rel_embeddings = nn.Embedding(2 * s.rel_positions, s.hidden_size)


def strip_deberta_prefix(sd: dict) -> dict:
    """Checkpoint keys of a ``DebertaFor...`` model (``deberta.embeddings...``) as ``DebertaModel`` names them; heads, the frozen
    ``position_embeddings`` some checkpoints carry and buffers are dropped."""
    out = {}
    for k, v in sd.items():
        k = k[len("deberta."):] if k.startswith("deberta.") else k
        if k.startswith(("embeddings.", "encoder.")) and "position_embeddings" not in k and not k.endswith("position_ids"):
            out[k] = v
    return out


class HipDebertaModel(nn.Module):
    def __init__(self, shape: DebertaShape, init_std: float = 0.02, hidden_dropout_prob: float = 0.1,
                 attention_probs_dropout_prob: float = 0.1, name: str = "deberta"):
        super().__init__()
        self.shape = shape
        self.config = types.SimpleNamespace(
            model_type="deberta", name=name, vocab_size=shape.vocab_size, hidden_size=shape.hidden_size,
            num_hidden_layers=shape.num_hidden_layers, num_attention_heads=shape.num_attention_heads,
            intermediate_size=shape.intermediate_size, max_position_embeddings=shape.max_position_embeddings,
            layer_norm_eps=shape.layer_norm_eps, pad_token_id=shape.pad_token_id, max_relative_positions=shape.max_relative_positions,
            relative_attention=True, pos_att_type=["c2p", "p2c"], position_biased_input=False, type_vocab_size=0,
            embedding_size=shape.hidden_size, talking_head=False, z_steps=0, hidden_act="gelu",
            hidden_dropout_prob=hidden_dropout_prob, attention_probs_dropout_prob=attention_probs_dropout_prob)
        check_deberta_config(self.config)
        if shape.pad_token_id != 0:
            raise NotImplementedError(f"DeBERTa tower: pad_token_id={shape.pad_token_id} is not built (the released models pad with 0)")
        self.embeddings = _Embeddings(shape)
        self.encoder = _Encoder(shape)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=init_std)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=init_std)
                if m.padding_idx is not None:
                    with torch.no_grad():
                        m.weight[m.padding_idx].zero_()

    @staticmethod
    def from_hf(hf_model) -> "HipDebertaModel":
        """Adopt a HuggingFace ``DebertaModel``: same keys in the same order, weights copied."""
        c = hf_model.config
        check_deberta_config(c)
        if int(getattr(hf_model, "z_steps", 0) or 0) > 1:
            raise NotImplementedError(f"DeBERTa tower: z_steps={hf_model.z_steps} is not built")
        shape = DebertaShape(vocab_size=c.vocab_size, hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers,
                             num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size,
                             max_position_embeddings=c.max_position_embeddings, layer_norm_eps=c.layer_norm_eps,
                             pad_token_id=int(c.pad_token_id or 0), max_relative_positions=int(getattr(c, "max_relative_positions", -1) or -1))
        m = HipDebertaModel(shape, hidden_dropout_prob=float(c.hidden_dropout_prob),
                            attention_probs_dropout_prob=float(c.attention_probs_dropout_prob))
        sd = strip_deberta_prefix(hf_model.state_dict())
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not missing and not unexpected, (missing, unexpected)
        hf_named = [(n[len("deberta."):] if n.startswith("deberta.") else n, q) for n, q in hf_model.named_parameters()]
        hf_named = [(n, q) for n, q in hf_named if n.startswith(("embeddings.", "encoder."))]
        mine = list(m.named_parameters())
        assert len(mine) == len(hf_named), (len(mine), len(hf_named))
        for (n1, p1), (n2, p2) in zip(mine, hf_named):
            assert n1 == n2, (n1, n2)       # same ORDER too: the drivers freeze parameters by index
            p1.requires_grad = p2.requires_grad
        return m
