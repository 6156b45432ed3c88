#!/usr/bin/env python
"""Golden vectors for two-stage ID (+) modality fusion (``--arch id_two_stage``) from the imported reference
``bce_text/id_plus_mo-2stage`` package (its own script: every reference variant names its packages ``model`` / ``data_utils``).  Run once
on the CPU, with the reference tree's root as the only argument:
    python tests/golden/make_golden_id_two_stage.py <reference root>
Cases ``<kind>_<mo_dnn_layers>_<dnn_layers>``: {add, cat} x {(0, 0), (0, 2), (2, 0), (2, 2)} on g14's batch (ids ``[B, L + 1, 2]`` and
mask: stored again, so the file stands alone), W = 64, ``drop_rate = 0``, ``.eval()``.  Weights: ``tests/id_two_stage_ref.golden_state``
-- ``det_param``, the id table ``det_normal`` times ``<case>.table_scale`` like the feature table, the weights of the tower's
Dropout-Linear-GELU layers times ``<case>.mlp_scale`` (both stored: with raw ``det_param``-sized values every score stays near zero and
the loss is 2 ln 2 whatever the model computes).  The script asserts per case that the captured scores of the valid positions take both
signs and reach |s| >= 1.  Stored per case: loss, the positive / negative scores, every parameter's gradient norm (fp64), the full
gradients of ``turn_dim.fc.weight`` and ``id_embedding.weight``, the catalogue table (the package's ``get_item_embeddings`` arithmetic:
``mlp_layers(fc(id_embedding(id), turn_dim(features[id])))`` for every id), and for 20 eval users (sequences of 2 .. 7 distinct items,
history = the inputs) the 1-based rank of each target -- the position of the target in the reference's descending argsort of the masked
scores, cross-checked against its ``metrics_topK`` -- with HR@10 / nDCG@10.  The script asserts that no unmasked item of an eval user
scores within 1e-4 max|score| of the target."""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], "bce_text", "id_plus_mo-2stage"))
from idvs.morec_amd.utils.detgen import det_randint  # noqa: E402
from id_two_stage_ref import feature_table, golden_state  # noqa: E402  (tests/: one definition of the golden's parameters)
from model import Model as RefModel  # noqa: E402  (reference package)
from data_utils.metrics import metrics_topK  # noqa: E402

torch.set_num_threads(8)
W, N_EVAL = 64, 20
# name -> (item_tower, mo_dnn_layers, dnn_layers, table_scale, mlp_scale).  Tried on the CPU: table_scale 0.5, 2, 4 x mlp_scale 1, 2, 3, 4.
# table_scale 0.5 meets the score condition asserted below wherever no Dropout-Linear-GELU layer follows the fusion; with dnn_layers = 2 and
# mlp_scale 1 the scores shrink (add only just meets it: [-0.7, 1.6]; cat does not: below 0.4), mlp_scale 2 brings them to [-4, 15]; larger
# factors push every score of the cat cases above zero (cat_2_2 at 0.5 x 4: [2.8, 96]).
CASES = {
    "add_0_0": ("modal_add", 0, 0, 0.5, 1.0),
    "add_0_2": ("modal_add", 0, 2, 0.5, 2.0),
    "add_2_0": ("modal_add", 2, 0, 0.5, 1.0),
    "add_2_2": ("modal_add", 2, 2, 0.5, 2.0),
    "cat_0_0": ("modal_cat", 0, 0, 0.5, 1.0),
    "cat_0_2": ("modal_cat", 0, 2, 0.5, 2.0),
    "cat_2_0": ("modal_cat", 2, 0, 0.5, 1.0),
    "cat_2_2": ("modal_cat", 2, 2, 0.5, 2.0),
}
# seed tag of each case's eval split: changed (never the margin) where a draw put an unmasked item within the tie margin of a target
EVAL_TAG = {name: "" for name in CASES}


def eval_split(name, item_num, S):
    """20 users: a sequence of 2 .. S + 1 distinct items, the last one the target, the others input and history."""
    name = name + EVAL_TAG[name]
    seqs = []
    for u in range(N_EVAL):
        n = int(det_randint(f"g26.{name}.len{u}", (1,), 2, S + 2)[0])
        perm = np.argsort(det_randint(f"g26.{name}.perm{u}", (item_num,), 0, 1 << 30), kind="stable") + 1
        seqs.append([int(i) for i in perm[:n]])
    return seqs


def build(name, S, D, item_num):
    tower, mo, dnn, scale, mlp_scale = CASES[name]
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2, dnn_layers=dnn,
                                 mo_dnn_layers=mo, word_embedding_dim=W, item_tower=tower)
    m = RefModel(args, item_num, True, None)
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(keys, scale, mlp_scale).items()})
    m.eval()
    return m, keys, torch.from_numpy(feature_table(item_num, W, scale))


def scores(m, table, ids, lm, S, D):
    """The scores of model.py:48-63."""
    flat = torch.from_numpy(ids).reshape(-1)
    with torch.no_grad():
        e = m.mlp_layers(m.fc(m.id_embedding(flat), m.turn_dim(table[flat]))).view(-1, S + 1, 2, D)
        prec = m.user_encoder(e[:, :-1, 0], lm, "cpu")
        return (prec * e[:, 1:, 0]).sum(-1), (prec * e[:, :-1, 1]).sum(-1)


def main():
    g14 = np.load(os.path.join(HERE, "g14_bce.npz"))
    S, D, item_num, B = (int(v) for v in g14["cfg"])
    ids, log_mask = g14["items"], g14["log_mask"]
    res = {"cfg": np.array([S, D, item_num, B, W]), "ids": ids.astype(np.int64), "log_mask": log_mask.astype(np.float32)}
    keys = {}
    for name, (tower, mo, dnn, scale, mlp_scale) in CASES.items():
        m, keys[name], table = build(name, S, D, item_num)
        lm = torch.from_numpy(log_mask)
        pos, neg = scores(m, table, ids, lm, S, D)
        valid = torch.cat((pos[lm != 0], neg[lm != 0]))
        assert float(valid.max()) > 0 > float(valid.min()) and float(valid.abs().max()) >= 1, (name, float(valid.min()), float(valid.max()))
        flat = torch.from_numpy(ids).reshape(-1)
        loss = m(flat, table[flat], lm, "cpu")      # what the reference's dataset ships: the ids and [B * (L + 1) * 2, W] features
        loss.backward()
        res[f"{name}.table_scale"], res[f"{name}.mlp_scale"] = np.float64(scale), np.float64(mlp_scale)
        res[f"{name}.mo_dnn_layers"], res[f"{name}.dnn_layers"] = np.int64(mo), np.int64(dnn)
        res[f"{name}.loss"] = np.float32(loss.item())
        res[f"{name}.pos_score"], res[f"{name}.neg_score"] = pos.numpy().copy(), neg.numpy().copy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                res[f"{name}.grad_norm.{k}"] = np.float64(p.grad.double().norm().item())
        res[f"{name}.grad.turn_dim.fc.weight"] = m.turn_dim.fc.weight.grad.numpy().copy()
        res[f"{name}.grad.id_embedding.weight"] = m.id_embedding.weight.grad.numpy().copy()
        with torch.no_grad():      # get_item_embeddings of data_utils/metrics.py:85-105
            itab = m.mlp_layers(m.fc(m.id_embedding(torch.arange(item_num + 1)), m.turn_dim(table)))
        res[f"{name}.item_table"] = itab.numpy().copy()
        seqs = eval_split(name, item_num, S)
        item_rank = torch.Tensor(np.arange(item_num) + 1)
        ranks, hits, ndcgs = [], [], []
        for seq in seqs:
            tokens, target = seq[:-1], seq[-1]
            pad = S + 1 - len(seq)
            with torch.no_grad():      # BuildEvalDataset + eval_model of data_utils/metrics.py:108-135
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
        print(f"g26 {name}: loss {loss.item():.6f}, scores in [{float(valid.min()):.3f}, {float(valid.max()):.3f}], ranks {ranks}, "
              f"HR@10 {np.mean(hits):.3f}")
    np.savez_compressed(os.path.join(HERE, "g26_id_two_stage.npz"), **res)
    with open(os.path.join(HERE, "g26_id_two_stage_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)


if __name__ == "__main__":
    main()
