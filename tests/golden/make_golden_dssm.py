#!/usr/bin/env python
"""Golden vectors for the DSSM two-tower model (``--arch dssm``) from the imported reference ``bce_text/main-end2end(DSSM)`` package (its
own script: every reference variant names its packages ``model`` / ``data_utils``).  Run once on the CPU, with the reference tree's
root as the only argument:
    python tests/golden/make_golden_dssm.py <reference root>
Cases: the ID tower with (dnn_layers, neg_num) = (0, 1) and (2, 4), and the text tower (g23's bert_micro configuration, token rows of
``g14_bce.npz``: not stored again) with (2, 4).  Weights are ``det_param``, ``drop_rate = 0``, ``.eval()``.  With raw ``det_param`` tables
every score stays near zero and the loss is ln 2 whatever the model computes, so ``user_embedding.weight`` and ``id_embedding.weight``
are multiplied by ``<case>.table_scale`` (stored; the tests apply the same constant); the script asserts that the captured scores take both
signs and reach |s| >= 2 (behind two GELU layers the vectors are mostly positive: the negative scores stay small).  Stored per case:
the inputs, loss and scores, every parameter's gradient norm (fp64), the full gradients of
the two embedding tables, the user table and the item table, and for an eval split of 20 users with histories the 1-based rank of each
target -- the position of the target in the reference's descending argsort of the masked scores, cross-checked against its
``metrics_topK`` -- with the resulting HR@10 / nDCG@10.  The script also asserts that no unmasked item of an eval user scores within
1e-4 max|score| of the target, so the ranks do not hang on rounding.  ``g24_read_behaviors_dssm.npz``: the reference's ten
``read_behaviors`` outputs on ``g2_users.tsv`` / ``g2_items.tsv``."""
import json
import logging
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], "bce_text", "main-end2end(DSSM)"))
from idvs.morec_amd.utils.detgen import det_param, det_randint  # noqa: E402
from model import Model as RefModel  # noqa: E402  (reference package)
from data_utils.metrics import metrics_topK  # noqa: E402
from data_utils.preprocess import read_behaviors, read_news  # noqa: E402

torch.set_num_threads(8)
USER_NUM, B = 20, 20
# name -> (use_modal, dnn_layers, neg_num, table_scale)
CASES = {"id_0_1": (False, 0, 1, 6.0), "id_2_4": (False, 2, 4, 32.0), "modal_2_4": (True, 2, 4, 32.0)}


def load_det(m, scale):
    sd = m.state_dict()
    new = {k: torch.from_numpy(det_param(k, tuple(v.shape))) for k, v in sd.items() if v.dtype.is_floating_point}
    for k in ("user_embedding.weight", "id_embedding.weight"):
        if k in new:
            new[k] = new[k] * scale
    m.load_state_dict(new, strict=False)
    return m


# seed tag of each case's eval split: changed (never the margin) where a draw put an unmasked item within the tie margin of a target
EVAL_TAG = {"id_0_1": "", "id_2_4": "", "modal_2_4": ".b"}


def eval_split(name, item_num):
    """20 users, each with a history of 1 .. 6 distinct items and a target outside it."""
    name = name + EVAL_TAG[name]
    hist, pairs = {}, []
    for u in range(1, USER_NUM + 1):
        n = int(det_randint(f"g24.{name}.hlen{u}", (1,), 1, 7)[0])
        perm = np.argsort(det_randint(f"g24.{name}.perm{u}", (item_num,), 0, 1 << 30), kind="stable") + 1
        hist[u] = torch.LongTensor(perm[:n].astype(np.int64))
        pairs.append((u, int(perm[n])))
    return hist, np.array(pairs)


def main():
    from transformers import BertConfig, BertModel
    g14 = np.load(os.path.join(HERE, "g14_bce.npz"))
    _, D, item_num, _ = (int(v) for v in g14["cfg"])
    content = g14["content"]
    T = content.shape[1] // 2
    cfg = BertConfig(attn_implementation="eager", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=512,
                     hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
    res = {"cfg": np.array([USER_NUM, item_num, D, B])}
    keys = {}
    for name, (use_modal, dnn, neg, scale) in CASES.items():
        n1 = 1 + neg
        args = types.SimpleNamespace(embedding_dim=D, dnn_layers=dnn, neg_num=neg, drop_rate=0.0, num_words_title=T, num_words_abstract=50,
                                     num_words_body=50, news_attributes=["title"], bert_model_load="bert_micro", word_embedding_dim=64)
        m = load_det(RefModel(args, USER_NUM, item_num, use_modal, BertModel(cfg) if use_modal else None), scale).eval()
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        users = (np.argsort(det_randint(f"g24.{name}.users", (B,), 0, 1 << 30), kind="stable") + 1).astype(np.int64)      # every user once ...
        users[1] = users[0]                                          # ... but one twice: its table row sums two gradients
        items = det_randint(f"g24.{name}.items", (B * n1,), 1, item_num + 1).astype(np.int64)
        label = np.zeros((B, n1), dtype=np.float32)
        label[:, 0] = 1.0
        x = torch.from_numpy(content[items]) if use_modal else torch.from_numpy(items)
        # the scores (model.py:40-41), then the loss through the model's own forward
        with torch.no_grad():
            uf = m.user_encoder(m.user_embedding(torch.from_numpy(users)))
            itf = m.bert_encoder(x) if use_modal else m.id_encoder(m.id_embedding(x))
            scores = torch.bmm(itf.view(-1, n1, D), uf.unsqueeze(-1)).squeeze(-1)
        assert float(scores.max()) > 0 > float(scores.min()) and float(scores.abs().max()) >= 2, (name, float(scores.min()), float(scores.max()))
        loss = m(torch.from_numpy(users), x, torch.from_numpy(label))
        loss.backward()
        res[f"{name}.table_scale"] = np.float64(scale)
        res[f"{name}.dnn_layers"], res[f"{name}.neg_num"] = np.int64(dnn), np.int64(neg)
        res[f"{name}.input_user"], res[f"{name}.sample_items"], res[f"{name}.bce_label"] = users, items, label
        res[f"{name}.loss"] = np.float32(loss.item())
        res[f"{name}.scores"] = scores.numpy().copy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                res[f"{name}.grad_norm.{k}"] = np.float64(p.grad.double().norm().item())
        res[f"{name}.grad.user_embedding.weight"] = m.user_embedding.weight.grad.numpy().copy()
        if not use_modal:
            res[f"{name}.grad.id_embedding.weight"] = m.id_embedding.weight.grad.numpy().copy()
        with torch.no_grad():
            utab = m.user_encoder(m.user_embedding(torch.arange(USER_NUM + 1)))
            itab = m.bert_encoder(torch.from_numpy(content)) if use_modal else m.id_encoder(m.id_embedding(torch.arange(item_num + 1)))
        res[f"{name}.user_table"], res[f"{name}.item_table"] = utab.numpy().copy(), itab.numpy().copy()
        hist, pairs = eval_split(name, item_num)
        item_rank = torch.Tensor(np.arange(item_num) + 1)
        ranks, hits, ndcgs = [], [], []
        for u, target in pairs:
            score = torch.matmul(utab[u], itab.t())
            lim = 1e-4 * float(score[1:].abs().max())
            near = (score - score[target]).abs() <= lim
            near[hist[int(u)]] = False
            near[0] = False
            near[target] = False
            assert not bool(near.any()), (name, int(u), "an unmasked item ties with the target")
            score[hist[int(u)]] = -np.inf
            score = score[1:]
            rank = int((torch.argsort(score, descending=True) == target - 1).nonzero()[0, 0]) + 1
            y = torch.zeros(item_num)
            y[target - 1] = 1.0
            ra = metrics_topK(score, y, item_rank, 10, "cpu")
            assert float(ra[0]) == float(rank <= 10) and abs(float(ra[1]) - (1 / math.log2(rank + 1) if rank <= 10 else 0.0)) < 1e-6
            ranks.append(rank)
            hits.append(float(ra[0]))
            ndcgs.append(float(ra[1]))
        res[f"{name}.eval_pairs"] = pairs.astype(np.int64)
        res[f"{name}.eval_hist"] = np.array([np.pad(hist[u].numpy(), (0, 6 - len(hist[u])), constant_values=-1) for u in range(1, USER_NUM + 1)])
        res[f"{name}.eval_ranks"] = np.array(ranks, dtype=np.int64)
        res[f"{name}.hit10"], res[f"{name}.ndcg10"] = np.float64(np.mean(hits)), np.float64(np.mean(ndcgs))
        print(f"g24 {name}: loss {loss.item():.6f}, scores in [{float(scores.min()):.3f}, {float(scores.max()):.3f}], ranks {ranks}, "
              f"HR@10 {np.mean(hits):.3f}")
    np.savez_compressed(os.path.join(HERE, "g24_dssm.npz"), **res)
    with open(os.path.join(HERE, "g24_dssm_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    a, b = read_news(os.path.join(HERE, "g2_items.tsv"))
    out = read_behaviors(os.path.join(HERE, "g2_users.tsv"), a, b, 5, 8, logging.getLogger("g24"))
    user_num, item_num, id2content, tr, va, train_pairs, valid_pairs, test_pairs, hv, ht = out
    rb = dict(user_num=user_num, item_num=item_num, min_seq_len=5, max_seq_len=8, train_pairs=train_pairs, valid_pairs=valid_pairs,
              test_pairs=test_pairs, content_ids=np.array(sorted(id2content)), content=np.array([id2content[k] for k in sorted(id2content)]))
    for u in tr:
        rb[f"train.{u}"], rb[f"valid.{u}"] = np.array(tr[u]), np.array(va[u])
        rb[f"hv.{u}"], rb[f"ht.{u}"] = hv[u].numpy(), ht[u].numpy()
    np.savez_compressed(os.path.join(HERE, "g24_read_behaviors_dssm.npz"), **rb)
    print("g24 read_behaviors: users", user_num, "items", item_num, "train pairs", len(train_pairs))


if __name__ == "__main__":
    main()
