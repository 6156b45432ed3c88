#!/usr/bin/env python
"""g30: golden vectors for the OPT text tower (causal pre-LN decoder, masked mean pooling).  Run once in the build container:
    python tests/golden/make_golden_opt.py
``make_golden_roberta.py``'s recipe with the installed HuggingFace ``OPTModel`` (dropout 0, the micro shape, ``det_param`` into every
parameter) inside the unmodified reference ``Model`` of ``inbatch_sasrec_e2e_text`` (its ``Text_Encoder_mean``), plus the loss of the
reference ``bce_text/main-end2end`` ``Model`` on the same tower.  Titles start with ``</s>`` (id 2): right-padded ones (id 1, mask 0), one
of length 1 (item 3), one of full length (item 7), several with an id 1 INSIDE the kept tokens (the positions count from the mask, so
nothing shifts; word row 1 takes no gradient), and the padding item (row 0): all-zero ids with an all-zero mask.  A separate
encoder-only case has masks with holes (``holes.*``; the first token masked in some).  Also stored: HF's position ids of the whole
content table and of the holes case, and the fp64 run of every stored output (``*.64``).

Attention implementation: with ``eager`` the installed model returns NaN for an all-masked title in fp64 (fp32 stays finite), and
``hidden * 0`` then makes the padding item's vector -- and the fp64 loss -- NaN.  The generator tries ``sdpa`` first, then ``eager``,
keeps the first whose stored arrays are all finite in BOTH dtypes and records it (``attn_implementation``).  Pad rows never reach a stored
quantity, so the choice does not change what is stored.  ``g30_opt_keys.json`` holds ``OPTModel.named_parameters()`` names and shapes in
registration order.  Only numeric inputs and outputs are stored."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from idvs.morec_amd.utils.detgen import det_normal, det_param, det_randint, det_uniform  # noqa: E402

torch.set_num_threads(8)
# dh = 16: HF scales q by dh^-0.5 before the product, the kernels scale the product; a power of two makes the two orders equal in fp32
MICRO = dict(vocab_size=80, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, ffn_dim=96, max_position_embeddings=40,
             word_embed_proj_dim=64, pad_token_id=1, bos_token_id=2, eos_token_id=2)
S, D, T, ITEM_NUM, B = 6, 64, 30, 50, 4
N_HOLES = 8
TE = "bert_encoder.text_encoders.title."
BM = TE + "bert_model."


def ref_model(package):
    """The reference package's ``Model`` (every variant names its package ``model``: the previous one is dropped first)."""
    for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, os.path.join("/root/reference", package))
    try:
        return importlib.import_module("model").Model
    finally:
        sys.path.pop(0)


def make_args():
    return types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="opt_micro", word_embedding_dim=64, num_workers=0)


def opt(impl):
    from transformers import OPTConfig, OPTModel
    return OPTModel(OPTConfig(attn_implementation=impl, dropout=0.0, attention_dropout=0.0, **MICRO))


def load_det(m, dtype):
    sd = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(det_param(k, tuple(v.shape))) for k, v in sd.items() if v.dtype.is_floating_point}, strict=False)
    return m.to(dtype).eval()


def titles():
    content = np.zeros((ITEM_NUM + 1, 2 * T), dtype=np.int64)      # row 0: the padding item, all-zero ids with an all-zero mask
    for i in range(1, ITEM_NUM + 1):
        L = T if i == 7 else 1 if i == 3 else int(det_randint(f"g30.tl{i}", (1,), 2, T + 1)[0])
        toks = det_randint(f"g30.tt{i}", (L,), 3, MICRO["vocab_size"])
        toks[0] = 2
        if i % 6 == 1 and L >= 6:       # id 1 inside the kept tokens
            toks[2] = 1
            if L >= 9:
                toks[L - 3] = 1
        content[i, :T] = 1              # the tokenizer's padding
        content[i, :L] = toks
        content[i, T:T + L] = 1
    return content


def holes():
    """Encoder-only case: masks with holes (padded layout only); rows 0-1 have their first token masked, row 2 is all ones."""
    c = np.zeros((N_HOLES, 2 * T), dtype=np.int64)
    for i in range(N_HOLES):
        toks = det_randint(f"g30.ht{i}", (T,), 3, MICRO["vocab_size"])
        toks[0] = 2
        m = (det_uniform(f"g30.hm{i}", (T,)) < 0.7).astype(np.int64)
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
        L = int(det_randint(f"g30.len{b}", (1,), 3, S + 2)[0])
        seq = det_randint(f"g30.seq{b}", (L,), 1, ITEM_NUM + 1)
        if L >= 4:
            seq[-2] = seq[0]
            if b > 0:
                seq[1] = ids[b - 1, -1]
        ids[b, S + 1 - L:] = seq
        lm[b, S - (L - 1):] = 1.0
    ids[0, -1], ids[1, -1], ids[2, -1] = 3, 7, 13      # the length-1 title, the full one and one with an id 1 inside are in the batch
    return ids, lm


def bce_batch():
    items = np.zeros((B, S + 1, 2), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(det_randint(f"g30.blen{b}", (1,), 3, S + 2)[0])
        items[b, S + 1 - L:, 0] = det_randint(f"g30.bseq{b}", (L,), 1, ITEM_NUM + 1)
        items[b, S + 1 - L:S, 1] = det_randint(f"g30.bneg{b}", (L - 1,), 1, ITEM_NUM + 1)
        lm[b, S + 1 - L:] = 1.0
    return items, lm


def zipf_pop():
    w = 1.0 / np.arange(1, ITEM_NUM + 1, dtype=np.float64)
    w = w[np.argsort(det_uniform("pop.g30", (ITEM_NUM,)))]
    return np.append([1.0], w / w.sum())


def inbatch(res, impl, content, hol, ids, lm, pop, dtype, sfx):
    Model = ref_model("inbatch_sasrec_e2e_text")
    m = load_det(Model(make_args(), ITEM_NUM, True, opt(impl), pop), dtype)
    if dtype == torch.float64:
        m.pop_prob_list = torch.from_numpy(np.asarray(pop, dtype=np.float64))
    items = torch.from_numpy(content[ids.reshape(-1)])
    R = torch.from_numpy(det_normal("g30.R", (B * (S + 1), D))).to(dtype)
    m.zero_grad()
    vec = m.bert_encoder(items)
    (vec * R).sum().backward()
    res["item_vecs" + sfx] = vec.detach().numpy()
    named = dict(m.named_parameters())
    for k, p in named.items():
        if p.grad is not None:      # every encoder gradient, and its norm
            res[f"enc_grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())
            res[f"enc_grad.{k}{sfx}"] = p.grad.numpy().copy()
    m.zero_grad()
    lmt = torch.from_numpy(lm).to(dtype)
    loss = m(torch.from_numpy(ids).view(-1), items, lmt, "cpu")
    loss.backward()
    res["loss" + sfx] = loss.detach().numpy().copy()
    for k, p in named.items():
        if p.grad is not None:
            res[f"grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())
    with torch.no_grad():
        res["table_vecs" + sfx] = m.bert_encoder(torch.from_numpy(content)).numpy()      # the whole content table, the padding item included
        res["holes.vecs" + sfx] = m.bert_encoder(torch.from_numpy(hol)).numpy()
    return m


def bce(res, impl, content, items, lm, dtype, sfx):
    Model = ref_model("bce_text/main-end2end")
    m = load_det(Model(make_args(), ITEM_NUM, True, opt(impl)), dtype)
    loss = m(torch.from_numpy(content[items]).view(-1, 2 * T), torch.from_numpy(lm).to(dtype), "cpu")
    loss.backward()
    res["bce.loss" + sfx] = loss.detach().numpy().copy()
    for k, p in m.named_parameters():
        if p.grad is not None:
            res[f"bce.grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())


def hf_position_ids(m, text):
    """What reaches the position table's lookup for ``text`` [N, 2T] (the module adds its offset to the ids it is handed)."""
    seen = []
    pe = m.bert_encoder.text_encoders["title"].bert_model.decoder.embed_positions
    h = pe.register_forward_pre_hook(lambda mod, a, kw: seen.append((kw.get("position_ids") if kw.get("position_ids") is not None
                                                                       else a[2]).detach().clone() + mod.offset), with_kwargs=True)
    with torch.no_grad():
        m.bert_encoder(torch.from_numpy(text))
    h.remove()
    return seen[0].numpy().astype(np.int32)


def generate(impl):
    res = {}
    content, hol, (ids, lm), (bitems, blm), pop = titles(), holes(), inbatch_batch(), bce_batch(), zipf_pop()
    res["cfg"] = np.array([S, D, T, ITEM_NUM, B])
    res["content"], res["ids"], res["log_mask"], res["pop"] = content, ids, lm, pop
    res["bce.items"], res["bce.log_mask"] = bitems, blm
    res["holes.content"] = hol
    m = inbatch(res, impl, content, hol, ids, lm, pop, torch.float32, "")
    res["position_ids"] = hf_position_ids(m, content)
    res["holes.position_ids"] = hf_position_ids(m, hol)
    assert res["position_ids"].shape == (ITEM_NUM + 1, T)
    keys = [[k, list(p.shape)] for k, p in m.bert_encoder.text_encoders["title"].bert_model.named_parameters()]
    inbatch(res, impl, content, hol, ids, lm, pop, torch.float64, ".64")
    bce(res, impl, content, bitems, blm, torch.float32, "")
    bce(res, impl, content, bitems, blm, torch.float64, ".64")
    return res, keys


def main():
    res = keys = used = None
    for impl in ("sdpa", "eager"):
        res, keys = generate(impl)
        bad = [k for k, v in res.items() if not np.isfinite(np.asarray(v, dtype=np.float64)).all()]
        if not bad:
            used = impl
            break
        print(f"g30: attn_implementation={impl!r} leaves non-finite values in {bad[:4]} ... ({len(bad)} arrays)")
    assert used is not None, "no attention implementation is finite in both dtypes"
    for k, v in res.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    path = os.path.join(HERE, "g30_opt.npz")
    np.savez_compressed(path, **res)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    with open(os.path.join(HERE, "g30_opt_keys.json"), "w") as f:
        json.dump(dict(source="OPTModel.named_parameters() of the installed transformers", transformers=__import__("transformers").__version__,
                       attn_implementation=used, config=MICRO, parameters=keys), f, indent=1)
    print("g30:", used, "loss", float(res["loss"]), "fp64", float(res["loss.64"]), "bce", float(res["bce.loss"]), "fp64",
          float(res["bce.loss.64"]), "item vec fp32 vs fp64", float(np.abs(res["item_vecs"] - res["item_vecs.64"]).max()),
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
