"""CPU: the host side of the OPT text tower -- parameter inventory and order, the freeze index, refused configurations, routing, names,
the synthetic titles and the run modes that exit naming OPT.  No device is touched."""
import json
import os
import types

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR
from idvs.morec_amd import _lib
from idvs.morec_amd.model import Bert_Encoder, HipOPTModel, OptShape, Text_Encoder, Text_Encoder_mean
from idvs.morec_amd.opt_engine import check_opt_config, opt_param_shapes

KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g30_opt_keys.json")))
TE = "bert_encoder.text_encoders.title."


def make_args(**kw):
    d = dict(max_seq_len=6, embedding_dim=64, num_attention_heads=2, drop_rate=0.0, transformer_block=2, num_words_title=30,
             num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="opt_micro", word_embedding_dim=64,
             compute_dtype="fp32")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_named_shapes():
    for name in ("opt_125m", "opt-125m", "facebook/opt-125m"):
        s = OptShape.named(name)
        assert (s.vocab_size, s.hidden_size, s.num_hidden_layers, s.num_attention_heads, s.ffn_dim, s.max_position_embeddings) == \
            (50272, 768, 12, 12, 3072, 2048)
        assert s.num_positions == 2050 and s.pad_token_id == 1 and s.layer_norm_eps == 1e-5
    b = OptShape.named("opt_1.3b")
    assert (b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.ffn_dim) == (2048, 24, 32, 8192)
    assert OptShape.named("opt-1.3b") == b
    m = OptShape.named("opt_micro")
    c = KEYS["config"]
    assert (m.vocab_size, m.hidden_size, m.num_hidden_layers, m.num_attention_heads, m.ffn_dim, m.max_position_embeddings) == \
        (c["vocab_size"], c["hidden_size"], c["num_hidden_layers"], c["num_attention_heads"], c["ffn_dim"], c["max_position_embeddings"])
    assert m.hidden_size // m.num_attention_heads in (16, 64)      # q * dh^-0.5 is then an exact scaling
    with pytest.raises(ValueError):
        OptShape.named("bert_base")


def test_key_inventory_equals_the_installed_hf_order():
    shape = OptShape.named("opt_micro")
    want = [[k, list(s)] for k, s in KEYS["parameters"]]
    inv = opt_param_shapes(shape, 64, prefix=TE)
    bm = TE + "bert_model."
    got = [[k[len(bm):], list(s)] for k, s in inv.items() if k.startswith(bm)]
    assert got == want
    assert list(inv)[-2:] == [TE + "fc.weight", TE + "fc.bias"]
    assert [[k, list(p.shape)] for k, p in HipOPTModel(shape).named_parameters()] == want
    names = [k for k, _ in want]
    assert names.index("decoder.final_layer_norm.weight") < names.index("decoder.layers.0.self_attn.k_proj.weight")
    assert [n.split(".")[4] for n in names if n.startswith("decoder.layers.0.self_attn.") and n.endswith(".weight")] == \
        ["k_proj", "v_proj", "q_proj", "out_proj"]
    enc = Text_Encoder_mean(HipOPTModel(shape), 64, 64, torch.float32)
    assert [n for n, _ in enc.named_parameters()] == [k[len(TE):] for k in inv]


def test_freeze_paras_before_indexes_by_the_key_order():
    from idvs.morec_amd import run
    for n_frozen in (0, 4, 7, len(KEYS["parameters"])):
        args = make_args(freeze_paras_before=n_frozen, pretrained_dir="/nonexistent")
        bert = run.build_text_tower(args)
        assert isinstance(bert, HipOPTModel) and args.word_embedding_dim == 64
        flags = [(n, p.requires_grad) for n, p in bert.named_parameters()]
        assert [n for n, _ in flags] == [k for k, _ in KEYS["parameters"]]
        assert [g for _, g in flags] == [i >= n_frozen for i in range(len(flags))]
    # the first four are the two tables and the decoder-level final LayerNorm: index 4 is layer 0's k_proj
    assert KEYS["parameters"][4][0] == "decoder.layers.0.self_attn.k_proj.weight"


def test_grad_from_is_the_lowest_trainable_point():
    from idvs.morec_amd.opt_engine import opt_grad_from
    names = list(opt_param_shapes(OptShape.named("opt_micro"), 64, prefix=TE))
    assert opt_grad_from(names, 2, TE) == -1              # the tables train
    assert opt_grad_from(names[1:], 2, TE) == -1          # the position table alone
    assert opt_grad_from(names[2:], 2, TE) == 0           # decoder.final_layer_norm (indices 2, 3) sits ABOVE the layers
    assert opt_grad_from(names[4:], 2, TE) == 0
    assert opt_grad_from(names[5:], 2, TE) == 0           # part of layer 0
    assert opt_grad_from(names[20:], 2, TE) == 1
    assert opt_grad_from(names[36:], 2, TE) == 2          # fc alone
    assert opt_grad_from(names[2:4] + names[36:], 2, TE) == 2
    assert opt_grad_from([], 2, TE) == 2


@pytest.mark.parametrize("option,value", [("do_layer_norm_before", False), ("layerdrop", 0.1), ("enable_bias", False),
                                          ("layer_norm_elementwise_affine", False), ("_remove_final_layer_norm", True)])
def test_unsupported_options_raise_naming_themselves(option, value):
    cfg = HipOPTModel(OptShape.named("opt_micro")).config
    check_opt_config(cfg)
    setattr(cfg, option, value)
    with pytest.raises(NotImplementedError, match=option):
        check_opt_config(cfg)
    m = HipOPTModel(OptShape.named("opt_micro"))
    setattr(m.config, option, value)
    with pytest.raises(NotImplementedError, match=option):
        Text_Encoder_mean(m, 64, 64, torch.float32)


def test_projections_of_opt_350m_raise():
    from transformers import OPTConfig, OPTModel
    c = dict(KEYS["config"])
    c["word_embed_proj_dim"] = 32
    with pytest.raises(NotImplementedError, match="project_in / project_out"):
        HipOPTModel.from_hf(OPTModel(OPTConfig(**c)))
    with pytest.raises(NotImplementedError, match="do_layer_norm_before"):
        HipOPTModel.from_hf(OPTModel(OPTConfig(do_layer_norm_before=False, **KEYS["config"])))


def test_bert_encoder_routes_opt_names_to_the_mean_encoder():
    enc = Bert_Encoder(make_args(), HipOPTModel(OptShape.named("opt_micro")))
    te = enc.text_encoders["title"]
    assert isinstance(te, Text_Encoder_mean) and not isinstance(te, Text_Encoder)
    assert tuple(te.fc.weight.shape) == (64, 64)
    from idvs.morec_amd.model import BertShape, HipBertModel
    enc = Bert_Encoder(make_args(bert_model_load="roberta_micro"), HipBertModel(BertShape.named("roberta_micro")))
    assert isinstance(enc.text_encoders["title"], Text_Encoder)


def test_config_carries_the_dropout_probabilities_under_both_names():
    m = HipOPTModel(OptShape.named("opt_micro"), dropout=0.25, attention_dropout=0.125)
    assert (m.config.hidden_dropout_prob, m.config.attention_probs_dropout_prob) == (0.25, 0.125)
    m.config.dropout = 0.0
    assert m.config.hidden_dropout_prob == 0.0


def test_checkpoint_keys_lose_a_leading_model_prefix():
    from idvs.morec_amd.model.opt import strip_model_prefix
    m = HipOPTModel(OptShape.named("opt_micro"))
    sd = {"model." + k: v + 1 for k, v in m.state_dict().items()}
    sd["lm_head.weight"] = torch.zeros(2, 2)
    missing, unexpected = m.load_state_dict(strip_model_prefix(sd), strict=True)
    assert not missing and not unexpected


def test_new_entry_points_judge_their_arguments():
    h = _lib.lib()
    for n in ("morec_mask_pos_ids", "morec_opt_embed_fwd", "morec_masked_mean_fwd", "morec_masked_mean_bwd"):
        assert n in _lib.EXPORTS and hasattr(h, n)
    assert h.morec_mask_pos_ids(None, 1, 1, 2, 8, None, None, None, None) == -1
    assert h.morec_opt_embed_fwd(None, None, None, None, None, 4, 8, 1, None) == -1
    assert h.morec_masked_mean_fwd(None, None, None, None, 1, 1, 8, 1, None) == -1
    assert h.morec_masked_mean_bwd(None, None, None, None, 1, 1, 8, 1, None) == -1


def test_synthetic_titles_are_opt_titles():
    from idvs.morec_amd import run
    args = make_args(item_tower="modal", CV_model_load="None")
    vocab = run.synthetic_vocab(args, True)
    assert vocab == OptShape.named("opt_micro").vocab_size
    _, content, *_ = run.synthetic_dataset(12, 40, 6, 30, extra_T=(10,), vocab=vocab, opt=True)
    assert content.shape == (41, 80) and not content[0].any()
    for ids, mask in ((content[1:, :30], content[1:, 30:60]), (content[1:, 60:70], content[1:, 70:])):
        assert (ids[:, 0] == 2).all() and int(ids.max()) < vocab
        assert ((mask[:, :-1] >= mask[:, 1:]).all()) and (mask.sum(1) >= 8).all()
        assert (ids[mask == 0] == 1).all() and (ids[mask == 1] >= 2).all()
    docs = run.synthetic_new_item_docs(args, 40, vocab=vocab)
    for enc in docs.values():
        ids, m = np.array(enc[0]["input_ids"]), np.array(enc[0]["attention_mask"])
        assert ids[0] == 2 and int(ids.max()) < vocab and (ids[m == 0] == 1).all() and len(ids) == 30


@pytest.mark.parametrize("extra,word", [(["--fused_step"], "--fused_step"), (["--fused_step", "--graph"], "--fused_step"),
                                        (["--graph"], "--graph"), (["--fused_step", "--pool_negatives"], "--pool_negatives"),
                                        (["--arch", "dssm"], "--arch dssm")])
def test_modes_outside_the_autograd_path_exit_naming_opt(extra, word):
    from idvs.morec_amd.parameters import check_opt_args, parse_args
    args = parse_args(["--bert_model_load", "opt_micro", "--item_tower", "modal", "--synthetic", "8"] + extra)
    with pytest.raises(SystemExit) as e:
        check_opt_args(args)
    assert "OPT" in str(e.value) and word in str(e.value)
    assert check_opt_args(parse_args(["--bert_model_load", "opt_micro", "--item_tower", "modal"])) is True
    assert check_opt_args(parse_args(["--bert_model_load", "bert_base_uncased", "--item_tower", "modal"] + extra)) is False


def test_tokenizer_selection(tmp_path, monkeypatch):
    import transformers

    from idvs.morec_amd import run
    d = tmp_path / "opt_micro"
    d.mkdir()
    args = make_args(pretrained_dir=str(tmp_path))
    with pytest.raises(SystemExit, match="vocab.json"):
        run.load_text_tokenizer(args)
    (d / "vocab.json").write_text("{}")
    (d / "merges.txt").write_text("#version: 0.2\n")
    seen = []
    monkeypatch.setattr(transformers.GPT2Tokenizer, "from_pretrained", classmethod(lambda cls, path: seen.append(path) or "gpt2"))
    assert run.load_text_tokenizer(args) == "gpt2" and seen == [str(d)]
