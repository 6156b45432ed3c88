"""DeBERTa's disentangled attention without a GPU: the torch restatement the GPU tests compare against (``deberta_ref``) is the installed
``DisentangledSelfAttention`` in fp64, the Toeplitz index stays inside the position tiles, and the new entry points judge the descriptor
before any pointer (nothing is launched)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from idvs.morec_amd import _lib, ops
from deberta_ref import delta_index, disent_attn_ref
from test_opt_kernels_gpu import KINDS, make_mask

E_ARG, E_UNSUPPORTED = -1, -3      # MOREC_E_ARG, MOREC_E_UNSUPPORTED (include/morec_hip.h)
HEADS, DH = 4, 16


def _hf_attention():
    from transformers import DebertaConfig
    from transformers.models.deberta.modeling_deberta import DisentangledSelfAttention
    cfg = DebertaConfig(vocab_size=80, hidden_size=HEADS * DH, num_hidden_layers=1, num_attention_heads=HEADS, intermediate_size=96,
                        max_position_embeddings=40, relative_attention=True, pos_att_type=["c2p", "p2c"], position_biased_input=False,
                        type_vocab_size=0, max_relative_positions=-1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(7)
    att = DisentangledSelfAttention(cfg).double().eval()
    with torch.no_grad():
        for p in att.parameters():      # (q_bias / v_bias start as zeros)
            p.copy_(torch.randn(p.shape, dtype=torch.float64) * 0.3)
    return cfg, att


def permute_in_proj(y, heads):
    """[..., 3H] in HF's interleaved layout [h][q|k|v][dh] -> the library's [Q | K | V]."""
    lead, H3 = y.shape[:-1], y.shape[-1]
    dh = H3 // (3 * heads)
    return y.reshape(*lead, heads, 3, dh).transpose(-2, -3).reshape(*lead, H3)


@pytest.mark.parametrize("T", [1, 7, 30])
def test_ref_is_the_installed_attention_in_fp64(T):
    """All five mask kinds of ``test_opt_kernels_gpu.make_mask`` at once (one sequence each): |diff| <= 1e-12 max|ref|."""
    cfg, att = _hf_attention()
    H, n_seq, maxp = HEADS * DH, len(KINDS), cfg.max_position_embeddings
    mask = make_mask(n_seq, T)
    g = torch.Generator().manual_seed(T)
    hidden = torch.randn(n_seq, T, H, generator=g, dtype=torch.float64)
    rel = torch.randn(2 * maxp, H, generator=g, dtype=torch.float64)
    m = (mask != 0)
    ext = m[:, None, None, :] & m[:, None, :, None]
    i = torch.arange(T)
    want = att(hidden, ext, relative_pos=(i[:, None] - i[None, :])[None], rel_embeddings=rel)[0]
    with torch.no_grad():
        qkv = permute_in_proj(att.in_proj(hidden), HEADS).reshape(n_seq * T, 3 * H).clone()
        qkv[:, :H] += att.q_bias
        qkv[:, 2 * H:] += att.v_bias
        R = rel[maxp - T:maxp + T]
        # (the installed scaled_size_sqrt takes the square root in fp32, whatever the dtype of the model: the fp64 module divides by that value)
        s = float(torch.sqrt(torch.tensor(3 * DH, dtype=torch.float)))
        got = disent_attn_ref(qkv, mask, att.pos_proj(R), att.pos_q_proj(R), HEADS, 1.0 / s)
    want = want.reshape(n_seq * T, H).detach()
    assert torch.isfinite(want).all()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("T", [1, 2, 30, 64, 512])
def test_delta_never_leaves_the_tile(T):
    d = delta_index(T)
    assert int(d.min()) == 1 and int(d.max()) == 2 * T - 1
    # one cell per (i, j): the scatter dS -> [T x 2T] gradient tiles is one-to-one along a row and along a column
    assert all(len(set(row.tolist())) == T for row in d) and all(len(set(col.tolist())) == T for col in d.t())


def test_in_proj_permutation_is_exact():
    g = torch.Generator().manual_seed(0)
    y = torch.randn(5, 3 * HEADS * DH, generator=g)
    z = permute_in_proj(y, HEADS)
    H = HEADS * DH
    for h in range(HEADS):
        for s in range(3):
            assert torch.equal(z[:, s * H + h * DH:s * H + (h + 1) * DH], y[:, (3 * h + s) * DH:(3 * h + s + 1) * DH])


def _desc(**kw):
    base = dict(n_seq=3, T=30, n_heads=2, dh=64, causal=False, dtype=torch.bfloat16)
    base.update(kw)
    return ops.attn_desc(base["n_seq"], base["T"], base["n_heads"], base["dh"], base["causal"], 1.0 / math.sqrt(3 * base["dh"]),
                         ops.FLT_MIN_MASK, base["dtype"], p_drop=base.get("p_drop", 0.0))


def _calls(d):
    h = _lib.lib()
    one = C.c_void_p(16)      # a non-null address: the descriptor is judged before any pointer is followed
    return (h.morec_disent_attn_fwd(C.byref(d), one, one, one, one, one, None),
            h.morec_disent_attn_bwd(C.byref(d), one, one, one, one, one, one, None, None, None, None, 0, None))


@pytest.mark.parametrize("kw", [dict(causal=True), dict(T=65), dict(cu=True)])
def test_entry_points_refuse_on_the_descriptor_alone(kw):
    d = _desc(**{k: v for k, v in kw.items() if k != "cu"})
    if kw.get("cu"):
        d.cu_seqlens = 16
    assert _calls(d) == (E_UNSUPPORTED, E_UNSUPPORTED)
    assert _lib.lib().morec_disent_attn_ws_bytes(C.byref(d)) == 0


def test_entry_points_null_pointers_on_a_good_descriptor():
    h = _lib.lib()
    one = C.c_void_p(16)
    for d in (_desc(), _desc(p_drop=0.1), _desc(dtype=torch.float32, dh=16), _desc(T=64)):
        assert h.morec_disent_attn_fwd(C.byref(d), None, one, one, one, one, None) == E_ARG
        assert h.morec_disent_attn_fwd(C.byref(d), one, one, None, one, one, None) == E_ARG
        assert h.morec_disent_attn_fwd(C.byref(d), one, one, one, one, None, None) == E_ARG
        assert h.morec_disent_attn_bwd(C.byref(d), one, one, one, one, None, one, None, None, None, None, 0, None) == E_ARG
        # one of dPK / dPQ without the other; both without (enough) workspace
        assert h.morec_disent_attn_bwd(C.byref(d), one, one, one, one, one, one, None, one, None, None, 0, None) == E_ARG
        assert h.morec_disent_attn_bwd(C.byref(d), one, one, one, one, one, one, None, one, one, None, 0, None) == E_ARG
        assert h.morec_disent_attn_bwd(C.byref(d), one, one, one, one, one, one, None, one, one, one, 64, None) == E_ARG
        assert h.morec_disent_attn_ws_bytes(C.byref(d)) == 8 * 2 * 2 * d.T * d.n_heads * d.dh * 4
    assert h.morec_disent_attn_fwd(None, one, one, one, one, one, None) == E_ARG


# ------------------------------------------------------------------------------------------------ tower: keys, permutation, refusals
def _keys(golden_dir):
    import json
    import os
    return json.load(open(os.path.join(golden_dir, "g31_deberta_keys.json")))


def test_key_order_and_shapes_are_the_installed_models(golden_dir):
    from transformers import DebertaConfig, DebertaModel
    from idvs.morec_amd.deberta_engine import DebertaShape, deberta_param_shapes
    from idvs.morec_amd.model import HipDebertaModel
    keys = _keys(golden_dir)
    m = HipDebertaModel(DebertaShape.named("deberta_micro"))
    mine = [[k, list(p.shape)] for k, p in m.named_parameters()]
    assert len(mine) == 36 and mine == keys["parameters"]
    assert mine[-1][0] == "encoder.rel_embeddings.weight" and mine[3 + 16 * 2][0] == "encoder.rel_embeddings.weight"
    assert [k for k, _ in mine[3:9]] == ["encoder.layer.0.attention.self." + k for k in
                                         ("q_bias", "v_bias", "in_proj.weight", "pos_proj.weight", "pos_q_proj.weight", "pos_q_proj.bias")]
    hf = DebertaModel(DebertaConfig(**keys["config"]))
    assert mine == [[k, list(p.shape)] for k, p in hf.named_parameters()]
    inv = deberta_param_shapes(m.shape, 64, "")
    assert [[k[len("bert_model."):], list(v)] for k, v in inv.items() if k.startswith("bert_model.")] == mine
    assert list(inv)[-2:] == ["fc.weight", "fc.bias"]
    b, l = DebertaShape.named("deberta_base"), DebertaShape.named("microsoft/deberta-large")
    assert (b.vocab_size, b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.intermediate_size) == (50265, 768, 12, 12, 3072)
    assert (b.rel_positions, b.layer_norm_eps, b.pad_token_id) == (512, 1e-7, 0)
    assert (l.hidden_size, l.num_hidden_layers, l.num_attention_heads, l.intermediate_size) == (1024, 24, 16, 4096)


def test_engine_permutation_and_its_inverse_are_exact():
    from idvs.morec_amd.deberta_engine import permute_in_proj as perm, unpermute_in_proj as unperm
    g = torch.Generator().manual_seed(1)
    w = torch.randn(3 * HEADS * DH, HEADS * DH, generator=g)
    x = torch.randn(5, HEADS * DH, generator=g)
    assert torch.equal(unperm(perm(w, HEADS), HEADS), w) and torch.equal(perm(unperm(w, HEADS), HEADS), w)
    assert torch.equal(x @ perm(w, HEADS).t(), permute_in_proj(x @ w.t(), HEADS))      # the rows move, nothing is recomputed
    b = torch.randn(3 * HEADS * DH, generator=g)
    assert torch.equal(unperm(perm(b, HEADS), HEADS), b)


@pytest.mark.parametrize("field,value,word", [
    ("relative_attention", False, "relative_attention"), ("pos_att_type", ["c2p"], "pos_att_type"), ("pos_att_type", [], "pos_att_type"),
    ("position_biased_input", True, "position_biased_input"), ("type_vocab_size", 2, "type_vocab_size"),
    ("embedding_size", 32, "embedding_size"), ("talking_head", True, "talking_head"), ("z_steps", 2, "z_steps"),
    ("max_relative_positions", 16, "max_relative_positions")])
def test_unsupported_config_raises_naming_the_option(field, value, word):
    from idvs.morec_amd.deberta_engine import DebertaShape, check_deberta_config
    from idvs.morec_amd.model import HipDebertaModel
    m = HipDebertaModel(DebertaShape.named("deberta_micro"))
    check_deberta_config(m.config, 30)
    setattr(m.config, field, value)
    with pytest.raises(NotImplementedError) as e:
        check_deberta_config(m.config, 30)
    assert word in str(e.value)


def test_long_titles_and_other_architectures_are_refused_before_a_device():
    from idvs.morec_amd.deberta_engine import DebertaShape, check_deberta_config
    from idvs.morec_amd.model import HipDebertaModel, Text_Encoder
    m = HipDebertaModel(DebertaShape.named("deberta_base"))
    with pytest.raises(NotImplementedError) as e:
        check_deberta_config(m.config, 65)
    assert "T > 64" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        Text_Encoder(HipDebertaModel(DebertaShape.named("deberta_micro")), 64, 64, torch.float32).encode(torch.zeros(2, 130, dtype=torch.int64))
    assert "T > 64" in str(e.value)      # a CPU tensor: refused before anything touches a device
    for name in ("deberta-v2-xlarge", "microsoft/deberta-v3-base"):
        with pytest.raises(NotImplementedError) as e:
            DebertaShape.named(name)
        assert "v2" in str(e.value)
    from transformers import DebertaV2Config
    with pytest.raises(NotImplementedError) as e:
        check_deberta_config(DebertaV2Config())
    assert "v2" in str(e.value)


def test_flags_and_refusals():
    from idvs.morec_amd.parameters import check_deberta_args, check_opt_args, is_deberta_run, parse_args
    base = ["--item_tower", "modal", "--bert_model_load", "deberta_base"]
    assert check_deberta_args(parse_args(base)) is True and check_opt_args(parse_args(base)) is False
    assert check_deberta_args(parse_args(base + ["--arch", "dssm"])) is True
    assert is_deberta_run(parse_args(["--item_tower", "modal_cat", "--bert_model_load", "deberta_base"]))
    for extra, word in ((["--fused_step"], "--fused_step"), (["--graph"], "--graph"), (["--fused_step", "--graph"], "--fused_step")):
        with pytest.raises(SystemExit) as e:
            check_deberta_args(parse_args(base + extra))
        assert "DeBERTa" in str(e.value) and word in str(e.value)
    # not a DeBERTa run: untouched by the check
    assert check_deberta_args(parse_args(["--item_tower", "modal", "--bert_model_load", "bert_base_uncased", "--fused_step"])) is False
    assert check_deberta_args(parse_args(["--item_tower", "id", "--bert_model_load", "deberta_base", "--fused_step"])) is False


@pytest.mark.parametrize("extra", [["--fused_step"], ["--graph"]])
def test_run_exits_naming_deberta(extra):
    from idvs.morec_amd import run
    with pytest.raises(SystemExit) as e:
        run.main(["--synthetic", "10", "--item_tower", "modal", "--bert_model_load", "deberta_micro"] + extra)
    assert "DeBERTa" in str(e.value)


def test_synthetic_titles_are_debertas():
    from idvs.morec_amd import run
    _, content, *_ = run.synthetic_dataset(12, 20, 6, 30, vocab=80, deberta=True)
    ids, mask = content[:, :30], content[:, 30:]
    assert not ids[0].any() and not mask[0].any()
    assert (ids[1:, 0] == 1).all() and ids.max() < 80 and (ids[mask == 0] == 0).all()
    last = mask[1:].sum(1) - 1
    assert (ids[1:][np.arange(20), last] == 2).all() and ((mask[:, :-1] >= mask[:, 1:]).all())
