#!/usr/bin/env python
"""Golden vectors for the ID (+) modality fusion towers (``--item_tower modal_add | modal_cat | modal_cat_3``) from the imported reference
``bce_text/id_plus_mo-end2end`` package (its own script: every reference variant names its package ``model``).  Run once in the build
container:
    python tests/golden/make_golden_fusion.py
Inputs are g14's (``items``, ``log_mask``, ``content`` of ``g14_bce.npz``: not stored again); weights are ``det_param``; ``drop_rate = 0``,
``.eval()``.  ``id_embedding.weight`` is multiplied by ``<tower>.id_scale`` (stored; the test applies the same constant): 0.25 for
``modal_add``, 1 for the CAT towers.  (The ``modal_add`` loss stays near 20.8 whatever the constant -- 20.79 at 1, 20.90 at 0.25, 20.85 at
0: the logits saturate through the CONTENT vectors, as in g14's own ``modal`` case, loss 20.85 -- so the constant only keeps the id
half from dominating the sum.)  Stored per tower: loss, every parameter's gradient norm (fp64),
the full ``id_embedding.weight`` gradient, the catalogue table ``fc(id_embedding(arange), bert_encoder(content))`` and -- for the 16-bit
bounds, should they be needed -- the reference's own loss under ``torch.autocast("cpu", bfloat16)``.  ``g23_fusion_keys.json``: the
``state_dict`` keys and shapes per tower."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, "/root/reference/bce_text/id_plus_mo-end2end")
from idvs.morec_amd.utils.detgen import det_param  # noqa: E402
from model import Model as RefModel  # noqa: E402  (reference package)

torch.set_num_threads(8)
ID_SCALE = {"modal_add": 0.25, "modal_cat": 1.0, "modal_cat_3": 1.0}
TOWERS = ("modal_add", "modal_cat", "modal_cat_3")


def load_det(m, scale):
    sd = m.state_dict()
    new = {k: torch.from_numpy(det_param(k, tuple(v.shape))) for k, v in sd.items() if v.dtype.is_floating_point}
    new["id_embedding.weight"] = new["id_embedding.weight"] * scale
    m.load_state_dict(new, strict=False)
    return m


def main():
    from transformers import BertConfig, BertModel
    g14 = np.load(os.path.join(HERE, "g14_bce.npz"))
    S, D, item_num, B = (int(v) for v in g14["cfg"])
    items, lm, content = g14["items"], g14["log_mask"], g14["content"]
    T = content.shape[1] // 2
    cfg = BertConfig(attn_implementation="eager", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, vocab_size=512,
                     hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
    res = {}
    keys = {}
    ids = torch.from_numpy(items).view(-1)
    x = torch.from_numpy(content[items]).view(-1, 2 * T)
    for tower in TOWERS:
        args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                     num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                     bert_model_load="bert_micro", word_embedding_dim=64, item_tower=tower)
        m = load_det(RefModel(args, item_num, True, BertModel(cfg)), ID_SCALE[tower]).eval()
        res[f"{tower}.id_scale"] = np.float64(ID_SCALE[tower])
        keys[tower] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        loss = m(ids, x, torch.from_numpy(lm), "cpu")
        loss.backward()
        res[f"{tower}.loss"] = np.float32(loss.item())
        for k, p in m.named_parameters():
            if p.grad is not None:
                res[f"{tower}.grad_norm.{k}"] = np.float64(p.grad.double().norm().item())
        res[f"{tower}.grad.id_embedding.weight"] = m.id_embedding.weight.grad.numpy().copy()
        assert not m.id_embedding.weight.grad[0].any()      # padding_idx = 0
        with torch.no_grad():
            table = m.fc(m.id_embedding(torch.arange(item_num + 1)), m.bert_encoder(torch.from_numpy(content)))
            with torch.autocast("cpu", dtype=torch.bfloat16):
                loss16 = m(ids, x, torch.from_numpy(lm), "cpu")
        res[f"{tower}.table"] = table.float().numpy().copy()
        res[f"{tower}.autocast_bf16_loss"] = np.float32(loss16.item())
        print(f"g23 {tower}: loss {loss.item():.6f} (cpu autocast bf16 {loss16.item():.6f})")
    np.savez_compressed(os.path.join(HERE, "g23_fusion.npz"), **res)
    with open(os.path.join(HERE, "g23_fusion_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)


if __name__ == "__main__":
    main()
