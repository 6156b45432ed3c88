#!/usr/bin/env python
"""Golden vectors for two-stage training (``--arch two_stage``) from the imported reference ``bce_text/main-2stage(SASRec)`` package (its
own script: every reference variant names its packages ``model`` / ``data_utils``).  Run once on the CPU, with the reference tree's
root as the only argument:
    python tests/golden/make_golden_two_stage.py <reference root>
Cases: ``dnn_layer`` 0 and 2 (``mlp_0``, ``mlp_2``).  Weights are ``det_param``, ``drop_rate = 0``, ``.eval()``.  The frozen features are
a deterministic table ``[item_num + 1, 64]`` (``det_normal`` times ``<case>.table_scale``, stored: with raw ``det_param``-sized inputs
every score stays near zero and the loss is 2 ln 2 whatever the model computes); the script asserts that the captured scores of the
valid positions take both signs and reach |s| >= 2.  The batch is g14's (ids ``[B, L + 1, 2]`` and mask: stored again, so the file
stands alone).  Stored per case: loss, the positive / negative scores, every parameter's gradient norm (fp64), the full gradient of
``fc.fc.weight``, the item-embedding table ``fc(table)``, and for 20 eval users (sequences of 2 .. 7 distinct items, history = the
inputs) the 1-based rank of each target -- the position of the target in the reference's descending argsort of the masked scores,
cross-checked against its ``metrics_topK`` -- with HR@10 / nDCG@10.  The script asserts that no unmasked item of an eval user scores
within 1e-4 max|score| of the target.  ``features``: ``get_item_word_embs`` of the package's ``Bert_Encoder`` (``num_workers = 0``) on
g14's token rows with the bert-micro configuration and ``det_param("bert_encoder." + key)`` weights."""
import json
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
sys.path.insert(0, os.path.join(sys.argv[1], "bce_text", "main-2stage(SASRec)"))
from idvs.morec_amd.utils.detgen import det_normal, det_param, det_randint  # noqa: E402
from model import Model as RefModel  # noqa: E402  (reference package)
from model.encoders import Bert_Encoder as RefBertEncoder  # noqa: E402
from data_utils.metrics import get_item_word_embs, metrics_topK  # noqa: E402

torch.set_num_threads(8)
W, N_EVAL = 64, 20
# name -> (dnn_layer, table_scale)
CASES = {"mlp_0": (0, 0.5), "mlp_2": (2, 2.0)}
# seed tag of each case's eval split: changed (never the margin) where a draw put an unmasked item within the tie margin of a target
EVAL_TAG = {"mlp_0": "", "mlp_2": ""}


def eval_split(name, item_num, S):
    """20 users: a sequence of 2 .. S + 1 distinct items, the last one the target, the others input and history."""
    name = name + EVAL_TAG[name]
    seqs = []
    for u in range(N_EVAL):
        n = int(det_randint(f"g25.{name}.len{u}", (1,), 2, S + 2)[0])
        perm = np.argsort(det_randint(f"g25.{name}.perm{u}", (item_num,), 0, 1 << 30), kind="stable") + 1
        seqs.append([int(i) for i in perm[:n]])
    return seqs


def main():
    from transformers import BertConfig, BertModel
    g14 = np.load(os.path.join(HERE, "g14_bce.npz"))
    S, D, item_num, B = (int(v) for v in g14["cfg"])
    ids, log_mask = g14["items"], g14["log_mask"]
    res = {"cfg": np.array([S, D, item_num, B, W]), "ids": ids.astype(np.int64), "log_mask": log_mask.astype(np.float32)}
    base = det_normal("g25.table", (item_num + 1, W), std=1.0).astype(np.float32)
    keys = {}
    for name, (dnn, scale) in CASES.items():
        args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2, dnn_layer=dnn,
                                     word_embedding_dim=W)
        m = RefModel(args, item_num)
        m.load_state_dict({k: torch.from_numpy(det_param(k, tuple(v.shape))) for k, v in m.state_dict().items()})
        m.eval()
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        table = torch.from_numpy(base * np.float32(scale))
        x = table[torch.from_numpy(ids)].view(-1, W)          # what the reference's dataset ships: [B * (L + 1) * 2, W]
        lm = torch.from_numpy(log_mask)
        with torch.no_grad():      # the scores of model.py:30-41
            e = m.fc(x).view(-1, S + 1, 2, D)
            prec = m.user_encoder(e[:, :-1, 0], lm, "cpu")
            pos, neg = (prec * e[:, 1:, 0]).sum(-1), (prec * e[:, :-1, 1]).sum(-1)
        valid = torch.cat((pos[lm != 0], neg[lm != 0]))
        assert float(valid.max()) > 0 > float(valid.min()) and float(valid.abs().max()) >= 2, (name, float(valid.min()), float(valid.max()))
        loss = m(x, lm, "cpu")
        loss.backward()
        res[f"{name}.table_scale"], res[f"{name}.dnn_layer"] = np.float64(scale), np.int64(dnn)
        res[f"{name}.loss"] = np.float32(loss.item())
        res[f"{name}.pos_score"], res[f"{name}.neg_score"] = pos.numpy().copy(), neg.numpy().copy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                res[f"{name}.grad_norm.{k}"] = np.float64(p.grad.double().norm().item())
        res[f"{name}.grad.fc.fc.weight"] = m.fc.fc.weight.grad.numpy().copy()
        with torch.no_grad():
            itab = m.fc(table)
        res[f"{name}.item_table"] = itab.numpy().copy()
        seqs = eval_split(name, item_num, S)
        item_rank = torch.Tensor(np.arange(item_num) + 1)
        ranks, hits, ndcgs = [], [], []
        for seq in seqs:
            tokens, target = seq[:-1], seq[-1]
            pad = S + 1 - len(seq)
            with torch.no_grad():      # BuildEvalDataset + eval_model of data_utils/metrics.py:88-114
                emb = itab[[0] * pad + tokens][None]
                mask = torch.FloatTensor([0] * pad + [1] * len(tokens))[None]
                score = torch.matmul(m.user_encoder(emb, mask, "cpu")[:, -1], itab.t())[0]
            lim = 1e-4 * float(score[1:].abs().max())
            near = (score - score[target]).abs() <= lim
            near[tokens] = False
            near[0] = False
            near[target] = False
            assert not bool(near.any()), (name, seq, "an unmasked item ties with the target")
            score[torch.LongTensor(tokens)] = -np.inf
            score = score[1:]
            rank = int((torch.argsort(score, descending=True) == target - 1).nonzero()[0, 0]) + 1
            y = torch.zeros(item_num)
            y[target - 1] = 1.0
            ra = metrics_topK(score, y, item_rank, 10, "cpu")
            assert float(ra[0]) == float(rank <= 10) and abs(float(ra[1]) - (1 / math.log2(rank + 1) if rank <= 10 else 0.0)) < 1e-6
            ranks.append(rank)
            hits.append(float(ra[0]))
            ndcgs.append(float(ra[1]))
        res[f"{name}.eval_seqs"] = np.array([np.pad(np.array(s), (0, S + 1 - len(s)), constant_values=-1) for s in seqs], dtype=np.int64)
        res[f"{name}.eval_ranks"] = np.array(ranks, dtype=np.int64)
        res[f"{name}.hit10"], res[f"{name}.ndcg10"] = np.float64(np.mean(hits)), np.float64(np.mean(ndcgs))
        print(f"g25 {name}: loss {loss.item():.6f}, scores in [{float(valid.min()):.3f}, {float(valid.max()):.3f}], ranks {ranks}, "
              f"HR@10 {np.mean(hits):.3f}")

    # stage 1: the package's own get_item_word_embs over g14's token rows (bert-micro, one attribute)
    content = g14["content"]
    T = content.shape[1] // 2
    cfg = BertConfig(attn_implementation="eager", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=512,
                     hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
    bargs = types.SimpleNamespace(embedding_dim=D, num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                  bert_model_load="bert_micro", word_embedding_dim=64, num_workers=0)
    enc = RefBertEncoder(bargs, BertModel(cfg))
    sd = enc.state_dict()
    enc.load_state_dict({k: torch.from_numpy(det_param("bert_encoder." + k, tuple(v.shape))) for k, v in sd.items()
                         if v.dtype.is_floating_point}, strict=False)
    feats = get_item_word_embs(enc, content, 16, bargs, "cpu")
    assert tuple(feats.shape) == (item_num + 1, 64)
    res["features"] = feats.numpy().astype(np.float32)
    print("g25 features:", tuple(feats.shape), "max |f|", float(feats.abs().max()))
    np.savez_compressed(os.path.join(HERE, "g25_two_stage.npz"), **res)
    with open(os.path.join(HERE, "g25_two_stage_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)


if __name__ == "__main__":
    main()
