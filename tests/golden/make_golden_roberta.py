#!/usr/bin/env python
"""g29: golden vectors for the RoBERTa text tower (pad-relative position ids).  Run once in the build container:
    python tests/golden/make_golden_roberta.py
The g5 / g8 recipe of ``make_golden.py`` (same S, D, T, item_num, B and the same stored quantities) with the installed HuggingFace
``RobertaModel`` (eager attention, dropout 0, the micro shape, ``det_param`` into every parameter -- position row 1 included) inside
the unmodified reference ``Model`` of ``inbatch_sasrec_e2e_text``, plus the loss of the reference ``bce_text/main-end2end`` ``Model`` on
the same tower (g14's batch recipe).  Titles: ``<s>`` ... ``</s>``; half of them right-padded with id 1 (the tokenizer's padding), several
of those with an id 1 INSIDE the real tokens (the rule counts from the ids, so the positions behind it shift), the other half padded the
way the padding item is (id 0 = ``<s>`` with mask 0: non-pad tokens, positions keep counting), one title of full length.  Also stored:
HF's position ids of the whole content table, and the fp64 run of every stored output (``*.64``; the AdamW step deltas excepted, ``loss_after_step.64`` covers the step).  ``g29_roberta_keys.json`` holds
``RobertaModel.named_parameters()`` names and shapes in registration order.  Only numeric inputs and outputs are stored."""
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
MICRO = dict(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2)
S, D, T, ITEM_NUM, B = 6, 64, 30, 50, 4
BM = "bert_encoder.text_encoders.title.bert_model."


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
                                 bert_model_load="roberta_micro", word_embedding_dim=64, num_workers=0)


def roberta():
    from transformers import RobertaConfig, RobertaModel
    return RobertaModel(RobertaConfig(attn_implementation="eager", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **MICRO))


def load_det(m, dtype):
    sd = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(det_param(k, tuple(v.shape))) for k, v in sd.items() if v.dtype.is_floating_point}, strict=False)
    return m.to(dtype).eval()


def titles():
    content = np.zeros((ITEM_NUM + 1, 2 * T), dtype=np.int64)      # row 0: the padding item, all <s> with mask 0
    for i in range(1, ITEM_NUM + 1):
        L = T if i == 7 else int(det_randint(f"g29.tl{i}", (1,), 4, T + 1)[0])
        toks = det_randint(f"g29.tt{i}", (L,), 5, 512)
        toks[0], toks[-1] = 0, 2
        if i % 2 == 1:                  # the tokenizer's padding
            content[i, :T] = 1
            if i % 6 == 1 and L >= 6:   # pad ids inside the real tokens
                toks[2] = 1
                if L >= 9:
                    toks[L - 3] = 1
        content[i, :L] = toks
        content[i, T:T + L] = 1
    return content


def inbatch_batch():
    ids = np.zeros((B, S + 1), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(det_randint(f"g29.len{b}", (1,), 3, S + 2)[0])
        seq = det_randint(f"g29.seq{b}", (L,), 1, ITEM_NUM + 1)
        if L >= 4:
            seq[-2] = seq[0]
            if b > 0:
                seq[1] = ids[b - 1, -1]
        ids[b, S + 1 - L:] = seq
        lm[b, S - (L - 1):] = 1.0
    return ids, lm


def bce_batch():
    items = np.zeros((B, S + 1, 2), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(det_randint(f"g29.blen{b}", (1,), 3, S + 2)[0])
        items[b, S + 1 - L:, 0] = det_randint(f"g29.bseq{b}", (L,), 1, ITEM_NUM + 1)
        items[b, S + 1 - L:S, 1] = det_randint(f"g29.bneg{b}", (L - 1,), 1, ITEM_NUM + 1)
        lm[b, S + 1 - L:] = 1.0
    return items, lm


def zipf_pop():
    w = 1.0 / np.arange(1, ITEM_NUM + 1, dtype=np.float64)
    w = w[np.argsort(det_uniform("pop.g29", (ITEM_NUM,)))]
    return np.append([1.0], w / w.sum())


ENC_GRADS = ["bert_encoder.text_encoders.title.fc.weight", BM + "encoder.layer.0.attention.self.query.weight",
             BM + "encoder.layer.1.output.dense.bias", BM + "embeddings.position_embeddings.weight",
             BM + "embeddings.LayerNorm.weight"]
STEP = ["bert_encoder.text_encoders.title.fc.weight", BM + "encoder.layer.0.attention.self.query.weight",
        BM + "embeddings.word_embeddings.weight", BM + "embeddings.position_embeddings.weight",
        "user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.w_1.weight", "user_encoder.transformer_encoder.layer_norm.bias"]


def inbatch(res, content, ids, lm, pop, dtype, sfx):
    Model = ref_model("inbatch_sasrec_e2e_text")
    m = load_det(Model(make_args(), ITEM_NUM, True, roberta(), pop), dtype)
    if dtype == torch.float64:
        m.pop_prob_list = torch.from_numpy(np.asarray(pop, dtype=np.float64))
    items = torch.from_numpy(content[ids.reshape(-1)])
    R = torch.from_numpy(det_normal("g29.R", (B * (S + 1), D))).to(dtype)
    m.zero_grad()
    vec = m.bert_encoder(items)
    (vec * R).sum().backward()
    res["item_vecs" + sfx] = vec.detach().numpy()
    named = dict(m.named_parameters())
    for k, p in named.items():
        if p.grad is not None:
            res[f"enc_grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())
    for k in ENC_GRADS:
        res[f"enc_grad.{k}{sfx}"] = named[k].grad.numpy().copy()
    m.zero_grad()
    lmt = torch.from_numpy(lm).to(dtype)
    loss = m(torch.from_numpy(ids).view(-1), items, lmt, "cpu")
    loss.backward()
    res["loss" + sfx] = loss.detach().numpy().copy()
    for k, p in named.items():
        if p.grad is not None:
            res[f"grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())
    pool = [BM + "pooler.dense.weight", BM + "pooler.dense.bias"]
    opt = torch.optim.AdamW([{"params": [p for k, p in named.items() if "bert_model" in k and k not in pool], "lr": 5e-5, "weight_decay": 0.01},
                             {"params": [p for k, p in named.items() if "bert_model" not in k], "lr": 1e-4, "weight_decay": 0.01}])
    before = {k: p.detach().clone() for k, p in named.items()}
    opt.step()
    for k in STEP if not sfx else []:      # (no fp64 twin of the step deltas: +-lr almost everywhere, and two thirds of the file)
        res[f"step_delta.{k}{sfx}"] = (named[k].detach() - before[k]).numpy()
    opt.zero_grad()
    res["loss_after_step" + sfx] = m(torch.from_numpy(ids).view(-1), items, lmt, "cpu").detach().numpy().copy()
    return m


def bce(res, content, items, lm, dtype, sfx):
    Model = ref_model("bce_text/main-end2end")
    m = load_det(Model(make_args(), ITEM_NUM, True, roberta()), dtype)
    loss = m(torch.from_numpy(content[items]).view(-1, 2 * T), torch.from_numpy(lm).to(dtype), "cpu")
    loss.backward()
    res["bce.loss" + sfx] = loss.detach().numpy().copy()
    for k, p in m.named_parameters():
        if p.grad is not None:
            res[f"bce.grad_norm.{k}{sfx}"] = np.float64(p.grad.double().norm().item())


def main():
    res = {}
    content, (ids, lm), (bitems, blm), pop = titles(), inbatch_batch(), bce_batch(), zipf_pop()
    res["cfg"] = np.array([S, D, T, ITEM_NUM, B])
    res["content"], res["ids"], res["log_mask"], res["pop"] = content, ids, lm, pop
    res["bce.items"], res["bce.log_mask"] = bitems, blm
    m = inbatch(res, content, ids, lm, pop, torch.float32, "")
    # HF's own position ids of the whole content table: what reaches the position table's lookup
    seen = []
    emb = m.bert_encoder.text_encoders["title"].bert_model.embeddings
    h = emb.position_embeddings.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach().clone()))
    with torch.no_grad():
        m.bert_encoder(torch.from_numpy(content))
    h.remove()
    res["position_ids"] = seen[0].numpy().astype(np.int32)
    assert res["position_ids"].shape == (ITEM_NUM + 1, T)
    keys = [[k, list(p.shape)] for k, p in m.bert_encoder.text_encoders["title"].bert_model.named_parameters()]
    inbatch(res, content, ids, lm, pop, torch.float64, ".64")
    bce(res, content, bitems, blm, torch.float32, "")
    bce(res, content, bitems, blm, torch.float64, ".64")
    np.savez_compressed(os.path.join(HERE, "g29_roberta.npz"), **res)
    with open(os.path.join(HERE, "g29_roberta_keys.json"), "w") as f:
        json.dump(dict(source="RobertaModel.named_parameters() of the installed transformers", transformers=__import__("transformers").__version__,
                       config=MICRO, parameters=keys), f, indent=1)
    print("g29: loss", float(res["loss"]), "fp64", float(res["loss.64"]), "after step", float(res["loss_after_step"]),
          "bce", float(res["bce.loss"]), "fp64", float(res["bce.loss.64"]),
          "item vec fp32 vs fp64", float(np.abs(res["item_vecs"] - res["item_vecs.64"]).max()))


if __name__ == "__main__":
    main()
