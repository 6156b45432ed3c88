"""CPU: surface of the RoBERTa text tower (pad-relative position ids): the named shapes, the parameter order of the installed
``RobertaModel`` (``tests/golden/g29_roberta_keys.json``), ``from_hf``, the CPU restatement (``roberta_ref``) against the golden captured
from the reference packages (``g29_roberta.npz``), the argument checks of the three new C-ABI entry points (nothing is launched), and the
driver's tokenizer selection."""
import json
import os
import types

import numpy as np
import pytest
import torch

import roberta_ref
from helpers import GOLDEN_DIR, det_state, relerr
from idvs.morec_amd import _lib
from idvs.morec_amd.model import BertShape, HipBertModel
from idvs.morec_amd.model.spec import bert_param_shapes, model_param_shapes
from idvs.morec_amd.utils.detgen import det_normal

KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g29_roberta_keys.json")))
P = 4096      # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused before a launch
E_ARG, E_UNSUPPORTED, E_DTYPE = -1, -3, -4
F32, BF16 = 0, 1


def g29():
    return np.load(os.path.join(GOLDEN_DIR, "g29_roberta.npz"))


def test_named_shapes():
    b = BertShape.named("roberta_base")
    assert (b.vocab_size, b.hidden_size, b.num_hidden_layers, b.num_attention_heads, b.intermediate_size) == (50265, 768, 12, 12, 3072)
    l = BertShape.named("roberta_large")
    assert (l.vocab_size, l.hidden_size, l.num_hidden_layers, l.num_attention_heads, l.intermediate_size) == (50265, 1024, 24, 16, 4096)
    m = BertShape.named("roberta_micro")
    assert (m.vocab_size, m.hidden_size, m.num_hidden_layers, m.num_attention_heads, m.intermediate_size) == (512, 64, 2, 2, 256)
    assert m.max_position_embeddings == 66
    for s in (b, l):
        assert s.max_position_embeddings == 514
    for s in (b, l, m):
        assert (s.type_vocab_size, s.layer_norm_eps, s.pad_token_id, s.position_rule) == (1, 1e-5, 1, "pad_relative")
    u = BertShape.named("bert_base_uncased")
    assert u == BertShape() and (u.vocab_size, u.max_position_embeddings, u.type_vocab_size, u.layer_norm_eps) == (30522, 512, 2, 1e-12)
    assert (u.pad_token_id, u.position_rule) == (0, "absolute")
    with pytest.raises(ValueError):
        BertShape.named("roberta_nano")


def test_parameter_order_is_the_installed_hf_order():
    shape = BertShape.named("roberta_micro")
    m = HipBertModel(shape)
    got = [[k, list(p.shape)] for k, p in m.named_parameters()]
    assert got == KEYS["parameters"]
    assert [[k, list(v)] for k, v in bert_param_shapes(shape, prefix="").items()] == KEYS["parameters"]
    e = m.embeddings
    assert e.word_embeddings.padding_idx == 1 and e.position_embeddings.padding_idx == 1
    assert m.config.pad_token_id == 1 and m.config.position_rule == "pad_relative"
    # the BERT tower keeps its order
    names = [k for k, _ in HipBertModel(BertShape.named("micro")).named_parameters()][:5]
    assert [n[len("embeddings."):] for n in names] == ["word_embeddings.weight", "position_embeddings.weight",
                                                         "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"]


def test_from_hf_roberta_round_trip():
    from transformers import RobertaConfig, RobertaModel
    hf = RobertaModel(RobertaConfig(attn_implementation="eager", **KEYS["config"]))
    m = HipBertModel.from_hf(hf)
    assert m.shape == BertShape.named("roberta_micro")
    sd, ref = m.state_dict(), hf.state_dict()
    for k, v in sd.items():
        assert torch.equal(v, ref[k]), k
    assert not [k for k in ref if k not in sd and torch.is_floating_point(ref[k])]
    hf2 = RobertaModel(RobertaConfig(attn_implementation="eager", **KEYS["config"]))
    missing, unexpected = hf2.load_state_dict(sd, strict=False)
    assert not unexpected and all(not torch.is_floating_point(hf2.state_dict()[k]) for k in missing)
    for k, v in hf2.state_dict().items():
        if k in sd:
            assert torch.equal(v, sd[k]), k


def test_position_ids_equal_hf():
    g = g29()
    T = int(g["cfg"][2])
    ids = torch.from_numpy(g["content"][:, :T])
    assert torch.equal(roberta_ref.position_ids(ids, 1), torch.from_numpy(g["position_ids"]).long())
    assert roberta_ref.position_ids(torch.tensor([[0, 5, 1, 7, 2, 1, 1, 1]]), 1).tolist() == [[2, 3, 1, 4, 5, 1, 1, 1]]


def _state(S, D, item_num):
    shapes = model_param_shapes(max_seq_len=S, embedding_dim=D, n_blocks=2, item_num=item_num, use_modal=True,
                                bert=BertShape.named("roberta_micro"))
    return {k: v.requires_grad_(True) for k, v in det_state(shapes).items()}


def test_restatement_reproduces_g29():
    """The fp32 bounds of ``test_oracle_vs_golden.py::test_g5_bert_micro``."""
    g = g29()
    S, D, T, item_num, B = (int(v) for v in g["cfg"])
    p = _state(S, D, item_num)
    items = torch.from_numpy(g["content"][g["ids"].reshape(-1)])
    vec = roberta_ref.text_encoder_forward(p, items, 2)
    assert np.abs(vec.detach().numpy() - g["item_vecs"]).max() < 2e-5
    R = torch.from_numpy(det_normal("g29.R", (B * (S + 1), D)))
    (vec * R).sum().backward()
    for k in [k for k in g.files if k.startswith("enc_grad.") and not k.endswith(".64")]:
        assert relerr(p[k[len("enc_grad."):]].grad.numpy(), g[k]) < 5e-5, k
    pos_g = p[roberta_ref.TE + "bert_model.embeddings.position_embeddings.weight"].grad
    assert float(pos_g[1].abs().max()) == 0.0 and float(pos_g[0].abs().max()) == 0.0      # padding_idx row; row 0 is never read
    assert float(p[roberta_ref.TE + "bert_model.embeddings.word_embeddings.weight"].grad[1].abs().max()) == 0.0
    for k in [k for k in g.files if k.startswith("enc_grad_norm.") and not k.endswith(".64")]:
        name = k[len("enc_grad_norm."):]
        if "pooler" in name:
            continue
        assert abs(p[name].grad.double().norm().item() - float(g[k])) <= 1e-4 * float(g[k]) + 2e-5, name
    for v in p.values():
        v.grad = None
    loss = roberta_ref.model_forward(p, torch.from_numpy(g["ids"]).view(-1), items, torch.from_numpy(g["log_mask"]), g["pop"],
                                     max_seq_len=S, embedding_dim=D, n_heads=2, bert_heads=2)
    assert abs(loss.item() - float(g["loss"])) < 2e-5
    loss.backward()
    for k in [k for k in g.files if k.startswith("grad_norm.") and not k.endswith(".64")]:
        name = k[len("grad_norm."):]
        if "pooler" in name:
            continue
        assert abs(p[name].grad.double().norm().item() - float(g[k])) <= 2e-4 * float(g[k]) + 2e-5, name


def test_restatement_reproduces_g29_bce():
    """The bounds of ``test_bce.py::test_bce_oracle_matches_reference``."""
    g = g29()
    S, D, T, item_num, B = (int(v) for v in g["cfg"])
    p = _state(S, D, item_num)
    x = torch.from_numpy(g["content"][g["bce.items"]]).view(-1, 2 * T)
    loss = roberta_ref.bce_model_forward(p, x, torch.from_numpy(g["bce.log_mask"]), max_seq_len=S, embedding_dim=D, n_heads=2, bert_heads=2)
    ref = float(g["bce.loss"])
    assert abs(float(loss.detach()) - ref) < 2e-5 * max(1.0, abs(ref))
    loss.backward()
    for k in [k for k in g.files if k.startswith("bce.grad_norm.") and not k.endswith(".64")]:
        name = k[len("bce.grad_norm."):]
        if "pooler" in name:
            continue
        r = float(g[k])
        assert abs(float(p[name].grad.double().norm()) - r) <= 5e-4 * r + 1e-7, name


def test_new_entry_points_judge_their_arguments():
    h = _lib.lib()
    for n in ("morec_roberta_pos_ids", "morec_bert_embed_fwd_pos", "morec_roberta_embed_bwd"):
        assert n in _lib.EXPORTS and hasattr(h, n)
    # morec_roberta_pos_ids(ids, pad_id, n_seq, T, n_pos, pos_ids, perm, cnt, stream)
    for k in (0, 5, 6, 7):
        a = [P, 1, 2, 8, 16, P, P, P, None]
        a[k] = None
        assert h.morec_roberta_pos_ids(*a) == E_ARG
    assert h.morec_roberta_pos_ids(P, 1, 0, 8, 16, P, P, P, None) == E_ARG
    assert h.morec_roberta_pos_ids(P, 1, 2, 0, 16, P, P, P, None) == E_ARG
    assert h.morec_roberta_pos_ids(P, -1, 2, 8, 16, P, P, P, None) == E_ARG
    assert h.morec_roberta_pos_ids(P, 1, 2, 8, 9, P, P, P, None) == E_ARG          # pad_id + T = 9 is not a row of a 9-row table
    assert h.morec_roberta_pos_ids(P, 1, 2, 512, 513, P, P, P, None) == E_ARG
    # morec_bert_embed_fwd_pos(ids, pos_ids, word, pos, type0, gamma, beta, eps, z, y, mean, rstd, M, T, H, dtype, p_out, seed, stream)
    for k in (0, 1, 2, 3, 4, 5, 6, 9):
        a = [P] * 7 + [1e-5, P, P, P, P, 16, 8, 64, F32, 0.0, 0, None]
        a[k] = None
        assert h.morec_bert_embed_fwd_pos(*a) == E_ARG, k
    assert h.morec_bert_embed_fwd_pos(*([P] * 7 + [1e-5, P, P, P, P, 0, 8, 64, F32, 0.0, 0, None])) == E_ARG
    assert h.morec_bert_embed_fwd_pos(*([P] * 7 + [1e-5, P, P, P, P, 16, 8, 64, F32, 1.0, 0, None])) == E_ARG
    # morec_roberta_embed_bwd(ids, dz, dword, dpos, dtype0, pad_id, M, T, H, dtype, order, perm, cnt, pos_pad, n_pos, stream)
    def bwd(T=8, H=64, dtype=F32, pos_pad=1, n_pos=16, M=None, null=None):
        a = [P, P, P, P, P, 1, 2 * T if M is None else M, T, H, dtype, None, P, P, pos_pad, n_pos, None]
        if null is not None:
            a[null] = None
        return h.morec_roberta_embed_bwd(*a)
    for k in (0, 1, 2, 3, 11, 12):
        assert bwd(null=k) == E_ARG, k
    assert bwd(M=17) == E_ARG                       # not a whole number of sequences
    assert bwd(pos_pad=-1) == E_ARG
    assert bwd(T=8, n_pos=9) == E_ARG               # slot T - 1 writes row pos_pad + T = 9
    assert bwd(T=512, n_pos=513) == E_ARG
    # T = 512, n_pos = 514, pad = 1 passes the range check: the call gets as far as the checks behind it (still nothing launched)
    assert bwd(T=512, n_pos=514, dtype=99) == E_DTYPE
    assert bwd(T=512, n_pos=514, H=68, dtype=BF16) == E_UNSUPPORTED      # 68 bf16 elements: not a multiple of the 16-byte vector
    assert bwd(H=66) == E_UNSUPPORTED
    assert bwd(H=4 * 257) == E_UNSUPPORTED          # more than 256 vectors per row


class _StubTokenizer:
    """``RobertaTokenizer``'s call signature over a whitespace vocabulary (used only if the installed class cannot be built offline)."""

    def __init__(self, vocab):
        self.vocab = vocab

    @classmethod
    def from_pretrained(cls, d):
        return cls(json.load(open(os.path.join(d, "vocab.json"))))

    def __call__(self, text, max_length, padding, truncation):
        ids = [0] + [self.vocab.get(w, 3) for w in text.split()][:max_length - 2] + [2]
        n = len(ids)
        return {"input_ids": ids + [1] * (max_length - n), "attention_mask": [1] * n + [0] * (max_length - n)}


def test_tokenizer_selection(tmp_path, monkeypatch):
    import transformers

    from idvs.morec_amd import run
    from idvs.morec_amd.data_utils import get_doc_input_bert, read_news_bert
    d = tmp_path / "roberta_micro"
    d.mkdir()
    args = types.SimpleNamespace(pretrained_dir=str(tmp_path), bert_model_load="roberta_micro", num_words_title=12, num_words_abstract=50,
                                 num_words_body=50, news_attributes=["title"])
    with pytest.raises(SystemExit) as e:
        run.load_text_tokenizer(args)
    assert "vocab.json" in str(e.value) and "merges.txt" in str(e.value)
    vocab = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3, "<mask>": 4}
    for i, w in enumerate("a b c d e f g h i j k l m n o p q r s t u v w x y z Ġ".split()):
        vocab[w] = 5 + i
    vocab["Ġa"] = len(vocab)
    (d / "vocab.json").write_text(json.dumps(vocab))
    with pytest.raises(SystemExit) as e:
        run.load_text_tokenizer(args)
    assert "merges.txt" in str(e.value) and "vocab.json" not in str(e.value).split("missing")[0].split(":")[-1]
    (d / "merges.txt").write_text("#version: 0.2\nĠ a\n")
    try:
        tok = run.load_text_tokenizer(args)
        tok("a b", max_length=12, padding="max_length", truncation=True)
    except Exception:      # the installed class cannot be built from these files offline: same call signature, stubbed
        monkeypatch.setattr(transformers, "RobertaTokenizer", _StubTokenizer, raising=False)
        tok = run.load_text_tokenizer(args)
    assert type(tok).__name__ in ("RobertaTokenizer", "RobertaTokenizerFast", "_StubTokenizer")
    news = tmp_path / "news.tsv"
    news.write_text("N1\tA b c\tx\nN2\tD e f g h\tx\n")
    a, b, c = read_news_bert(str(news), args, tok)
    ids, mask = get_doc_input_bert(a, args)[:2]
    assert ids.shape == (3, 12)
    for r in (1, 2):
        n = int(mask[r].sum())
        assert 2 < n < 12 and (mask[r, :n] == 1).all() and (mask[r, n:] == 0).all()
        assert ids[r, 0] == 0 and ids[r, n - 1] == 2 and (ids[r, n:] == 1).all() and (ids[r, :n] != 1).all()
    assert (ids[0] == 0).all() and (mask[0] == 0).all()      # the padding item: <s> tokens, positions 2 .. T + 1 under the rule
    # a BERT name still asks for vocab.txt
    args.bert_model_load = "bert_micro"
    with pytest.raises(SystemExit) as e:
        run.load_text_tokenizer(args)
    assert "vocab.txt" in str(e.value)
