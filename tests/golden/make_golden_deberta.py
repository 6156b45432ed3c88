#!/usr/bin/env python
"""g31: golden vectors for the DeBERTa text tower (disentangled attention).  Run once in the build container:
    python tests/golden/make_golden_deberta.py <reference checkout>
``make_golden_opt.py``'s recipe with the installed HuggingFace ``DebertaModel`` (dropout 0, the micro shape, ``det_param`` into every
parameter, so ``q_bias`` / ``v_bias`` are non-zero: with the default initialisation the padding item comes out as all zeros, which hides
the mask rule) inside the unmodified reference ``Model`` of ``inbatch_sasrec_e2e_text`` (its ``Text_Encoder``: ``hidden[:, 0] -> fc -> GELU``),
plus the loss of the reference ``bce_text/main-end2end`` ``Model`` and of the reference ``bce_text/main-end2end(DSSM)`` ``Model`` -- this
tower's own home -- on the same tower.  Titles are ``[CLS]`` = 1 ... ``[SEP]`` = 2, right-padded with 0 under mask 0: one of length 1
(item 3), one of full length (item 7), and the padding item (row 0): all-zero ids with an all-zero mask, whose every score is replaced by
the fill value, i.e. a uniform average of all T value rows in every layer.  A separate encoder-only case has masks with holes (``holes.*``;
the first token masked in some).  Every stored output has its fp64 run beside it (``*.64``; for the encoder gradients as
``enc_grad_twin_minus_fp32.*``, the fp64 run minus the fp32 one in fp32, half the bytes), and the generator asserts that every stored array
is finite in both dtypes.  ``g31_deberta_keys.json`` holds ``DebertaModel.named_parameters()`` names and shapes in registration
order.  Only numeric inputs and outputs are stored."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REFERENCE = sys.argv[1]
from idvs.morec_amd.utils.detgen import det_normal, det_param, det_randint, det_uniform  # noqa: E402

torch.set_num_threads(8)
MICRO = dict(vocab_size=80, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=96, max_position_embeddings=40,
             relative_attention=True, pos_att_type=["c2p", "p2c"], position_biased_input=False, type_vocab_size=0,
             max_relative_positions=-1, layer_norm_eps=1e-7, pad_token_id=0)
S, D, T, ITEM_NUM, B = 6, 64, 30, 50, 4
N_HOLES = 8
USER_NUM, DSSM_B, DSSM_NEG, DSSM_DNN, DSSM_SCALE = 12, 6, 3, 2, 32.0


def ref_model(package):
    """The reference package's ``Model`` (every variant names its package ``model``: the previous one is dropped first)."""
    for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join(REFERENCE, package))
    try:
        return importlib.import_module("model").Model
    finally:
        sys.path.pop(0)


def make_args(**kw):
    d = dict(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2, num_words_title=T,
             num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="deberta_micro", word_embedding_dim=64,
             num_workers=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def deberta():
    from transformers import DebertaConfig, DebertaModel
    return DebertaModel(DebertaConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **MICRO))


def load_det(m, dtype, scale_tables=()):
    sd = m.state_dict()
    new = {k: torch.from_numpy(det_param(k, tuple(v.shape))) for k, v in sd.items() if v.dtype.is_floating_point}
    for k in scale_tables:
        new[k] = new[k] * DSSM_SCALE
    m.load_state_dict(new, strict=False)
    return m.to(dtype).eval()


def titles():
    content = np.zeros((ITEM_NUM + 1, 2 * T), dtype=np.int64)      # row 0: the padding item, all-zero ids with an all-zero mask
    for i in range(1, ITEM_NUM + 1):
        L = T if i == 7 else 1 if i == 3 else int(det_randint(f"g31.tl{i}", (1,), 2, T + 1)[0])
        toks = det_randint(f"g31.tt{i}", (L,), 3, MICRO["vocab_size"])
        toks[-1] = 2
        toks[0] = 1
        content[i, :L] = toks
        content[i, T:T + L] = 1
    return content


def holes():
    """Encoder-only case: masks with holes; rows 0-1 have their first token masked, row 2 is all ones."""
    c = np.zeros((N_HOLES, 2 * T), dtype=np.int64)
    for i in range(N_HOLES):
        toks = det_randint(f"g31.ht{i}", (T,), 3, MICRO["vocab_size"])
        toks[0] = 1
        m = (det_uniform(f"g31.hm{i}", (T,)) < 0.7).astype(np.int64)
        m[0] = 0 if i < 2 else 1
        if i == 2:
            m[:] = 1
        m[5 + i] = 1      # at least one kept token
        c[i, :T], c[i, T:] = toks, m
    return c


def inbatch_batch():
    ids = np.zeros((B, S + 1), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(det_randint(f"g31.len{b}", (1,), 3, S + 2)[0])
        seq = det_randint(f"g31.seq{b}", (L,), 1, ITEM_NUM + 1)
        if L >= 4:
            seq[-2] = seq[0]
            if b > 0:
                seq[1] = ids[b - 1, -1]
        ids[b, S + 1 - L:] = seq
        lm[b, S - (L - 1):] = 1.0
    ids[0, -1], ids[1, -1] = 3, 7      # the length-1 title and the full one are in the batch (and the padding item: the left padding)
    return ids, lm


def bce_batch():
    items = np.zeros((B, S + 1, 2), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(det_randint(f"g31.blen{b}", (1,), 3, S + 2)[0])
        items[b, S + 1 - L:, 0] = det_randint(f"g31.bseq{b}", (L,), 1, ITEM_NUM + 1)
        items[b, S + 1 - L:S, 1] = det_randint(f"g31.bneg{b}", (L - 1,), 1, ITEM_NUM + 1)
        lm[b, S + 1 - L:] = 1.0
    return items, lm


def zipf_pop():
    w = 1.0 / np.arange(1, ITEM_NUM + 1, dtype=np.float64)
    w = w[np.argsort(det_uniform("pop.g31", (ITEM_NUM,)))]
    return np.append([1.0], w / w.sum())


def inbatch(res, content, hol, ids, lm, pop, dtype, sfx):
    Model = ref_model("inbatch_sasrec_e2e_text")
    m = load_det(Model(make_args(), ITEM_NUM, True, deberta(), pop), dtype)
    if dtype == torch.float64:
        m.pop_prob_list = torch.from_numpy(np.asarray(pop, dtype=np.float64))
    items = torch.from_numpy(content[ids.reshape(-1)])
    R = torch.from_numpy(det_normal("g31.R", (B * (S + 1), D))).to(dtype)
    m.zero_grad()
    vec = m.bert_encoder(items)
    (vec * R).sum().backward()
    res["item_vecs" + sfx] = vec.detach().numpy()
    named = dict(m.named_parameters())
    for k, p in named.items():
        if p.grad is not None:      # every encoder gradient, and its norm
            res[f"enc_grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())
            if sfx:      # the fp64 twin of a gradient is stored as its distance from the fp32 one (fp32: half the bytes, which keeps the file
                # under the committed-file limit): twin = enc_grad + enc_grad_twin_minus_fp32, to ~1e-7 of that distance
                res[f"enc_grad_twin_minus_fp32.{k}"] = (p.grad.numpy() - res[f"enc_grad.{k}"].astype(np.float64)).astype(np.float32)
            else:
                res[f"enc_grad.{k}"] = p.grad.numpy().copy()
    m.zero_grad()
    loss = m(torch.from_numpy(ids).view(-1), items, torch.from_numpy(lm).to(dtype), "cpu")
    loss.backward()
    res["loss" + sfx] = loss.detach().numpy().copy()
    for k, p in named.items():
        if p.grad is not None:
            res[f"grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())
    with torch.no_grad():
        res["table_vecs" + sfx] = m.bert_encoder(torch.from_numpy(content)).numpy()      # the whole content table, the padding item included
        res["holes.vecs" + sfx] = m.bert_encoder(torch.from_numpy(hol)).numpy()
    return m


def bce(res, content, items, lm, dtype, sfx):
    Model = ref_model("bce_text/main-end2end")
    m = load_det(Model(make_args(), ITEM_NUM, True, deberta()), dtype)
    loss = m(torch.from_numpy(content[items]).view(-1, 2 * T), torch.from_numpy(lm).to(dtype), "cpu")
    loss.backward()
    res["bce.loss" + sfx] = loss.detach().numpy().copy()
    for k, p in m.named_parameters():
        if p.grad is not None:
            res[f"bce.grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())


def dssm(res, content, dtype, sfx):
    Model = ref_model("bce_text/main-end2end(DSSM)")
    n1 = 1 + DSSM_NEG
    args = make_args(dnn_layers=DSSM_DNN, neg_num=DSSM_NEG)
    m = load_det(Model(args, USER_NUM, ITEM_NUM, True, deberta()), dtype, scale_tables=("user_embedding.weight",))
    users = (np.argsort(det_randint("g31.dssm.users", (DSSM_B,), 0, 1 << 30), kind="stable") + 1).astype(np.int64)
    users[1] = users[0]
    items = det_randint("g31.dssm.items", (DSSM_B * n1,), 0, ITEM_NUM + 1).astype(np.int64)      # (0: the padding item may be drawn)
    items[2], items[3] = 0, 3
    label = np.zeros((DSSM_B, n1), dtype=np.float32)
    label[:, 0] = 1.0
    loss = m(torch.from_numpy(users), torch.from_numpy(content[items]), torch.from_numpy(label).to(dtype))
    loss.backward()
    res["dssm.cfg"] = np.array([USER_NUM, DSSM_B, DSSM_NEG, DSSM_DNN])
    res["dssm.table_scale"] = np.float64(DSSM_SCALE)
    res["dssm.input_user"], res["dssm.sample_items"], res["dssm.bce_label"] = users, items, label
    res["dssm.loss" + sfx] = loss.detach().numpy().copy()
    for k, p in m.named_parameters():
        if p.grad is not None:
            res[f"dssm.grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())


def main():
    res = {}
    content, hol, (ids, lm), (bitems, blm), pop = titles(), holes(), inbatch_batch(), bce_batch(), zipf_pop()
    res["cfg"] = np.array([S, D, T, ITEM_NUM, B])
    res["content"], res["ids"], res["log_mask"], res["pop"] = content, ids, lm, pop
    res["bce.items"], res["bce.log_mask"] = bitems, blm
    res["holes.content"] = hol
    m = inbatch(res, content, hol, ids, lm, pop, torch.float32, "")
    keys = [[k, list(p.shape)] for k, p in m.bert_encoder.text_encoders["title"].bert_model.named_parameters()]
    inbatch(res, content, hol, ids, lm, pop, torch.float64, ".64")
    for dtype, sfx in ((torch.float32, ""), (torch.float64, ".64")):
        bce(res, content, bitems, blm, dtype, sfx)
        dssm(res, content, dtype, sfx)
    for k, v in res.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    assert float(np.abs(res["table_vecs"][0]).max()) > 0      # the padding item's vector is not hidden behind zero biases
    path = os.path.join(HERE, "g31_deberta.npz")
    np.savez_compressed(path, **res)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    with open(os.path.join(HERE, "g31_deberta_keys.json"), "w") as f:
        json.dump(dict(source="DebertaModel.named_parameters() of the installed transformers", transformers=__import__("transformers").__version__,
                       config=MICRO, parameters=keys), f, indent=1)
    print("g31: loss", float(res["loss"]), "fp64", float(res["loss.64"]), "bce", float(res["bce.loss"]), "fp64", float(res["bce.loss.64"]),
          "dssm", float(res["dssm.loss"]), "fp64", float(res["dssm.loss.64"]), "item vec fp32 vs fp64",
          float(np.abs(res["item_vecs"] - res["item_vecs.64"]).max()), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
