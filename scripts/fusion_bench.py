#!/usr/bin/env python
"""Fused ID (+) modality kernels (``csrc/fuse.hip``) against the composition of existing ops they replace, on the device:

  add  forward : ``fuse_add_fwd``            vs  ``gather_rows`` + torch add
  cat  forward : ``fuse_cat_fwd`` (p = 0.1)  vs  ``gather_rows`` + ``torch.cat`` + multiply by a stored mask
  cat  backward: ``fuse_cat_bwd`` (p = 0.1)  vs  slice + mask multiply (both halves) + ``scatter_add_rows_``   (atomic and deterministic scatter)

at R = 2688 and 5376 rows (B (S + 1) and 2 B (S + 1) at B = 128, S = 20), D = 512, fp16; and one ``BceModel`` training step on BERT-base with
the plain ``modal`` tower and with ``modal_cat`` (the difference is what the fusion tower costs end to end).  Timing: device events around
windows of ``--iters`` launches, the variants of a pair ALTERNATING window by window, ``--rounds`` windows each; reported: median and
min .. max per launch.  The composition is given its mask ready-made (a stored mask is what it would have to keep for the backward).

    python scripts/fusion_bench.py [--out FILE] [--no-model]
"""
import argparse
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import ops  # noqa: E402

DEV = "cuda"
P, SEED = 0.1, 0x5DEECE66D1234567


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def ab(name, fused, composed, iters, rounds, log):
    for f in (fused, composed):      # warm-up: code objects, allocator
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    t = {"fused": [], "composed": []}
    for _ in range(rounds):
        t["fused"].append(window(fused, iters))
        t["composed"].append(window(composed, iters))
    mf, mc = statistics.median(t["fused"]), statistics.median(t["composed"])
    log(f"{name:44s} fused {mf:8.2f} us ({min(t['fused']):.2f} .. {max(t['fused']):.2f})   composed {mc:8.2f} us "
        f"({min(t['composed']):.2f} .. {max(t['composed']):.2f})   composed / fused = {mc / mf:.2f}")
    return mf, mc


def kernels(R, D, dtype, iters, rounds, log):
    g = torch.Generator(device="cpu").manual_seed(R)
    n_items = 20000
    table = torch.randn(n_items + 1, D, generator=g).to(DEV)
    idx = torch.randint(1, n_items + 1, (R,), generator=g)
    idx[::21] = 0                                               # padded slots
    idx[1::7] = idx[3::7][: idx[1::7].numel()]                  # duplicates, as popular items give
    idx = idx.to(torch.int32).to(DEV)
    content = torch.randn(R, D, generator=g).to(DEV).to(dtype)
    dA = torch.randn(R, 2 * D, generator=g).to(DEV).to(dtype)
    keep = ops.dropout_keep_mask(R * 2 * D, P, SEED).view(R, 2 * D)
    thresh = int(P * 65536)
    mask = (keep.float() / (1.0 - thresh / 65536.0)).to(dtype)      # the stored mask of the composition
    d_table = torch.zeros(n_items + 1, D, device=DEV)

    def add_c():
        return ops.gather_rows(table, idx, dtype) + content

    def cat_c():
        return torch.cat([ops.gather_rows(table, idx, dtype), content], 1) * mask

    def bwd_c():
        dc = dA[:, D:] * mask[:, D:]
        did = (dA[:, :D] * mask[:, :D]).contiguous()
        ops.scatter_add_rows_(did, idx, d_table, 0)
        return dc

    # same results first (the composition rounds the id half once more on the way; dropped elements agree exactly)
    a_f, a_c = ops.fuse_cat_fwd(table, idx, content, P, SEED), cat_c()
    assert torch.equal(a_f == 0, a_c == 0) and float((a_f.float() - a_c.float()).abs().max()) < 0.05
    assert float((ops.fuse_add_fwd(table, idx, content).float() - add_c().float()).abs().max()) < 0.05
    tag = f"R={R} D={D} {str(dtype).replace('torch.', '')}"
    ab(f"add fwd      {tag}", lambda: ops.fuse_add_fwd(table, idx, content), add_c, iters, rounds, log)
    ab(f"cat fwd      {tag}", lambda: ops.fuse_cat_fwd(table, idx, content, P, SEED), cat_c, iters, rounds, log)
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            ab(f"cat bwd {'det   ' if det else 'atomic'} {tag}", lambda: ops.fuse_cat_bwd(dA, idx, d_table, 0, P, SEED), bwd_c, iters, rounds, log)
        finally:
            ops.set_deterministic(False)


def model_step(log, steps, rounds):
    from idvs.morec_amd.model import BertShape, HipBertModel
    from idvs.morec_amd.model.bce import BceModel
    B, S, D, T, item_num = 128, 20, 512, 30, 20000
    rng = np.random.default_rng(0)
    ids = torch.from_numpy(rng.integers(1, item_num + 1, (B * (S + 1) * 2,))).to(DEV)
    lens = rng.integers(8, T + 1, ids.numel())
    tok = rng.integers(5, 30000, (ids.numel(), T)) * (np.arange(T)[None] < lens[:, None])
    x = torch.from_numpy(np.concatenate([tok, (tok != 0).astype(np.int64)], 1)).to(DEV)
    lm = torch.ones(B, S, device=DEV)
    runs = {}
    for tower in ("modal", "modal_cat"):
        args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                     num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                     bert_model_load="bert_base_uncased", word_embedding_dim=768, compute_dtype="bf16", item_tower=tower)
        torch.manual_seed(1)
        m = BceModel(args, item_num, True, HipBertModel(BertShape.named("base"))).to(DEV).train()

        def step(m=m, fused=(tower != "modal")):
            for p in m.parameters():
                p.grad = None
            loss = m(ids, x, lm, DEV) if fused else m(x, lm, DEV)
            loss.backward()

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        runs[tower] = step
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            t[k].append(window(f, steps) / 1e3)
    for k, v in t.items():
        log(f"BceModel {k:10s} BERT-base bf16 B={B} S={S} (R={B * (S + 1) * 2}): {statistics.median(v):8.2f} ms / step ({min(v):.2f} .. {max(v):.2f})")
    log(f"fusion tower end to end: {statistics.median(t['modal_cat']) - statistics.median(t['modal']):+.2f} ms / step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# fusion_bench: {torch.cuda.get_device_name(0)}; us per call, median (min .. max) over {a.rounds} alternating windows of {a.iters} calls")
    for R in (2688, 5376):
        kernels(R, 512, torch.float16, a.iters, a.rounds, log)
    if not a.no_model:
        model_step(log, 5, 5)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
