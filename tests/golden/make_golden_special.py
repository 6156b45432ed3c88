#!/usr/bin/env python
"""g22: the cold-start / new-item protocol captured from the imported reference (``T/data_utils/special.py``, ``V/data_utils/special.py``).

    python tests/golden/make_golden_special.py          (build container only: needs /root/reference)

Writes small synthetic cold / new / new-items TSVs (``g22_cold.tsv``, ``g22_new.tsv``, ``g22_new_items.tsv``), the outputs of both
``read_behaviors_special`` shapes (``g22_read_special.json``) and, in ``g22_special.npz``, what ``eval_model_special`` of the text
reference computes: per-user Hit@10 / nDCG@10, the means, and the per-user score margin between the target and its nearest
competitor (as g17).  Cold users run through the ID tower, new-item users through the BERT micro tower of g17 (weights from
``det_param``), the new items' vectors from the reference's ``get_item_embeddings``; world-1 gloo group, ``.module`` wrapper.
Cases: a target inside its own history, one-item lines (empty history), a new item shared by several users.
``V/data_utils`` imports ``torchvision`` and ``lmdb`` at module level; empty stand-in modules are registered for them (the functions
used never touch them).  No reference source text is stored."""
from __future__ import annotations

import importlib.util
import json
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference package and the repo on sys.path)

from idvs.morec_amd.utils.detgen import det_randint  # noqa: E402

S, D, T, ITEM_NUM, N_NEW = 8, 64, 30, 60, 5
VISION_REF = "/root/reference/inbatch_sasrec_e2e_vision/data_utils"


def write_tsvs(out):
    """Lines ``u<k>\\t<names>``; catalogue items N1 .. N60 (text) / v1 .. v60 (vision), new items N61 .. N65 / v61 .. v65."""
    cold, new = [], []
    for u in range(23):
        L = 1 if u in (3, 11) else int(det_randint(f"g22.cl{u}", (1,), 2, S + 2)[0])
        seq = [int(v) for v in det_randint(f"g22.cs{u}", (L,), 1, ITEM_NUM + 1)]
        if u in (5, 17) and L >= 3:
            seq[1] = seq[-1]                          # the target is in its own history
        cold.append(seq)
    for u in range(19):
        L = 1 if u == 4 else int(det_randint(f"g22.nl{u}", (1,), 2, S + 2)[0])
        seq = [int(v) for v in det_randint(f"g22.ns{u}", (L - 1,), 1, ITEM_NUM + 1)]
        tgt = ITEM_NUM + 1 + [3, 0, 3, 1, 4, 2][u % 6]          # first appearance order differs from the id order; 3 is shared
        new.append(seq + [tgt])
    files = {}
    for prefix in ("N", "v"):
        files[prefix] = ("".join("u%d\t%s\n" % (u, " ".join(prefix + str(i) for i in s)) for u, s in enumerate(cold)),
                         "".join("u%d\t%s\n" % (u, " ".join(prefix + str(i) for i in s)) for u, s in enumerate(new)))
    with open(os.path.join(out, "g22_cold.tsv"), "w") as f:
        f.write(files["N"][0])
    with open(os.path.join(out, "g22_new.tsv"), "w") as f:
        f.write(files["N"][1])
    with open(os.path.join(out, "g22_cold_v.tsv"), "w") as f:
        f.write(files["v"][0])
    with open(os.path.join(out, "g22_new_v.tsv"), "w") as f:
        f.write(files["v"][1])
    with open(os.path.join(out, "g22_new_items.tsv"), "w") as f:    # the new-items file lists them in ANOTHER order than first use
        f.write("".join("v%d\n" % (ITEM_NUM + 1 + k) for k in (2, 4, 0, 1, 3)))


def text_maps():
    name_to_id = {"N%d" % i: i for i in range(1, ITEM_NUM + 1)}
    before_name_to_id = {"N%d" % i: 100 + i for i in range(1, ITEM_NUM + N_NEW + 1)}         # the full news list: other ids
    before_id_to_dic = {100 + i: "doc%d" % i for i in range(1, ITEM_NUM + N_NEW + 1)}
    return name_to_id, before_id_to_dic, before_name_to_id


def _plain(out):
    seqs_c, hist_c, seqs_n, hist_n, content = out
    js = lambda d: {str(k): v for k, v in d.items()} if d is not None else None
    h = lambda d: {str(k): [int(x) for x in v.tolist()] for k, v in d.items()} if d is not None else None
    c = None if content is None else {str(k): (v.decode("ascii") if isinstance(v, bytes) else v) for k, v in content.items()}
    return dict(seqs_for_cold=js(seqs_c), history_for_cold=h(hist_c), seqs_for_new=js(seqs_n), history_for_new=h(hist_n),
                new_item_id_to_content=c, history_dtypes=sorted({str(v.dtype) for v in list(hist_c.values()) + list((hist_n or {}).values())}))


def vision_special():
    import transformers  # noqa: F401  (imported before the stand-ins: it probes for torchvision itself)
    for name in ("torchvision", "torchvision.transforms", "lmdb"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    spec = importlib.util.spec_from_file_location("vref_data_utils", os.path.join(VISION_REF, "__init__.py"),
                                                  submodule_search_locations=[VISION_REF])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["vref_data_utils"] = pkg
    spec.loader.exec_module(pkg)
    for name in ("torchvision", "torchvision.transforms", "lmdb"):
        sys.modules.pop(name)
    return sys.modules["vref_data_utils.special"]


def g22(out):
    import torch.distributed as dist
    from data_utils import metrics as ref_metrics
    from data_utils import special as ref_special
    write_tsvs(out)
    log = logging.getLogger("g22")
    name_to_id, before_dic, before_name = text_maps()
    p = lambda n: os.path.join(out, n)
    read = {}
    for use_modal in (True, False):
        read["text.%d" % use_modal] = _plain(ref_special.read_behaviors_special(p("g22_cold.tsv"), p("g22_new.tsv"), name_to_id, before_dic,
                                                                               before_name, log, use_modal))
    vs = vision_special()
    vname = {"v%d" % i: i for i in range(1, ITEM_NUM + 1)}
    for use_modal in (True, False):
        read["vision.%d" % use_modal] = _plain(vs.read_behaviors_special(p("g22_cold_v.tsv"), p("g22_new_v.tsv"), p("g22_new_items.tsv"),
                                                                         vname, log, use_modal))
    with open(p("g22_read_special.json"), "w") as f:
        json.dump(read, f, indent=0, sort_keys=True)

    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:29622", rank=0, world_size=1)
    seqs_c, hist_c, seqs_n, hist_n, new_content = ref_special.read_behaviors_special(p("g22_cold.tsv"), p("g22_new.tsv"), name_to_id,
                                                                                    before_dic, before_name, log, True)
    args = mg.make_args(max_seq_len=S, embedding_dim=D, word_embedding_dim=64)
    pop = mg.zipf_pop(ITEM_NUM, "pop.g22")
    captured, means = [], []
    orig_concat = ref_special.eval_concat

    def cap_concat(eval_list, sampler):
        captured.append([e.clone().numpy() for e in eval_list])
        return orig_concat(eval_list, sampler)

    ref_special.eval_concat = cap_concat
    ref_special.print_metrics = lambda x, lg, v: means.append(list(x))

    def margins(m, emb, seqs, cand=None):
        res = np.zeros(len(seqs))
        with torch.no_grad():
            for u in range(len(seqs)):
                toks = seqs[u][:-1]
                idx = np.zeros(S, dtype=np.int64)
                lm = np.zeros((1, S), dtype=np.float32)
                if toks:
                    idx[S - len(toks):] = toks
                    lm[0, S - len(toks):] = 1
                prec = m.user_encoder(emb[torch.from_numpy(idx)][None], torch.from_numpy(lm), "cpu")[0, -1]
                sc = (emb @ prec).numpy().astype(np.float64)
                sc[np.array(toks, dtype=np.int64)] = -np.inf
                if cand is None:
                    t = sc[seqs[u][-1]]
                    others = np.delete(sc[1:], seqs[u][-1] - 1)
                else:
                    t = float((cand[seqs[u][-1]] @ prec).numpy())
                    others = sc[1:]
                fin = others[np.isfinite(others)]
                res[u] = np.min(np.abs(fin - t)) if (np.isfinite(t) and fin.size) else np.inf
        return res

    res = dict(cfg=np.array([S, D, T, ITEM_NUM]), pop=pop)
    # cold users: ID tower (use_modal False: the reference evaluates the cold users only)
    m_id = mg.RefModel(args, ITEM_NUM, False, None, pop)
    mg.load_det(m_id)
    m_id.eval()
    wrap = types.SimpleNamespace(module=m_id, eval=m_id.eval, train=m_id.train)
    emb = ref_metrics.get_item_embeddings(wrap, np.arange(ITEM_NUM + 1), 16, args, False, "cpu")
    ref_special.eval_model_special(wrap, emb, None, 16, args, ITEM_NUM, log, seqs_c, hist_c, None, None, "cpu", False)
    Uc = len(seqs_c)
    res.update({"id_item_embeddings": emb.numpy(), "cold.hit": captured[-1][0][:Uc], "cold.ndcg": captured[-1][1][:Uc],
                "cold.means": np.array(means[-1], dtype=np.float64), "cold.margins": margins(m_id, emb, seqs_c), "cold.n": Uc})
    # new-item users: BERT micro tower (g17's architecture)
    kw = dict(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64)
    m = mg.build_modal(args, kw, ITEM_NUM, pop)
    wrap = types.SimpleNamespace(module=m, eval=m.eval, train=m.train)
    content = mg.synth_titles("g22", ITEM_NUM, T, 512)
    new_titles = mg.synth_titles("g22new", N_NEW, T, 512)           # new id k (1 ..) -> title row k
    emb = ref_metrics.get_item_embeddings(wrap, content, 16, args, True, "cpu")
    new_emb = ref_metrics.get_item_embeddings(wrap, new_titles, 16, args, True, "cpu")
    ref_special.eval_model_special(wrap, emb, new_emb, 16, args, ITEM_NUM, log, seqs_c, hist_c, seqs_n, hist_n, "cpu", True)
    Un = len(seqs_n)
    res.update({"content": content, "new_content": new_titles, "bert_item_embeddings": emb.numpy(), "new_item_embeddings": new_emb.numpy(),
                "new.hit": captured[-1][0][:Un], "new.ndcg": captured[-1][1][:Un], "new.means": np.array(means[-1], dtype=np.float64),
                "new.margins": margins(m, emb, seqs_n, new_emb), "new.n": Un})
    for u in range(Uc):
        res[f"cold.seq.{u}"] = np.array(seqs_c[u])
    for u in range(Un):
        res[f"new.seq.{u}"] = np.array(seqs_n[u])
    np.savez_compressed(p("g22_special.npz"), **res)
    print("g22 done: cold", res["cold.means"], "new", res["new.means"], "min margins", res["cold.margins"].min(), res["new.margins"].min())


if __name__ == "__main__":
    g22(HERE)
