"""Embedding stage of the text tower under both position rules: BERT's (row t) and RoBERTa's (rows counted from the pad token).
Forward (``morec_bert_embed_fwd`` vs ``morec_roberta_pos_ids`` + ``morec_bert_embed_fwd_pos``) and backward (``morec_bert_embed_bwd`` vs
``morec_roberta_embed_bwd``) at the bench shape (2688 titles x 30 tokens, H = 768, fp16) and at T = 512.  The two rules are timed in
interleaved rounds of one process; per arm the median and the range of the rounds, and the ratio of the medians with the spread of the
per-round ratios.
    python scripts/roberta_embed_bench.py > profiles/roberta_embed.txt"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from idvs.morec_amd import ops  # noqa: E402

DEV, H, V, ROUNDS, ITERS = "cuda", 768, 30522, 11, 20


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS      # us per call


def case(n_seq, T):
    g = torch.Generator().manual_seed(n_seq + T)
    M, n_pos = n_seq * T, 514
    lens = torch.randint(8, T + 1, (n_seq,), generator=g)
    ids = torch.randint(1000, V, (n_seq, T), generator=g)
    real = torch.arange(T)[None, :] < lens[:, None]
    ids_b = torch.where(real, ids, torch.zeros_like(ids)).to(torch.int32).view(-1).to(DEV)      # BERT: padded with 0
    ids_r = torch.where(real, ids, torch.ones_like(ids)).to(torch.int32).view(-1).to(DEV)       # RoBERTa: padded with 1
    word, pos = torch.randn(V, H, generator=g).to(DEV), torch.randn(n_pos, H, generator=g).to(DEV)
    type0, gamma, beta = (torch.randn(H, generator=g).to(DEV) for _ in range(3))
    dz = torch.randn(M, H, generator=g).to(torch.float16).to(DEV)
    order_b, order_r = (torch.argsort(i, stable=True).to(torch.int32) for i in (ids_b, ids_r))
    dword, dpos, dty = torch.zeros(V, H, device=DEV), torch.zeros(n_pos, H, device=DEV), torch.zeros(H, device=DEV)
    _, perm, cnt = ops.roberta_pos_ids(ids_r, 1, T, n_pos)

    def fwd_r():
        p, _, _ = ops.roberta_pos_ids(ids_r, 1, T, n_pos)
        ops.bert_embed_fwd_pos(ids_r, p, word, pos, type0, gamma, beta, 1e-5, T, torch.float16)
    arms = {
        "fwd absolute": lambda: ops.bert_embed_fwd(ids_b, word, pos, type0, gamma, beta, 1e-12, T, torch.float16),
        "fwd pad_relative (ids + embed)": fwd_r,
        "bwd absolute": lambda: ops.bert_embed_bwd_(ids_b, dz, dword, dpos, dty, 0, T, order_b),
        "bwd pad_relative": lambda: ops.roberta_embed_bwd_(ids_r, dz, dword, dpos, dty, 1, T, perm, cnt, 1, order_r),
        "pos_ids alone": lambda: ops.roberta_pos_ids(ids_r, 1, T, n_pos),
    }
    for fn in arms.values():      # warm-up: allocator, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(timed(fn))
    print(f"\n{n_seq} titles x {T} tokens, H = {H}, fp16, {M * H * 2 / 1e6:.1f} MB of dz; {ROUNDS} interleaved rounds x {ITERS} calls, us per call")
    for k, v in rounds.items():
        print(f"  {k:32s} median {statistics.median(v):8.2f}   range {min(v):8.2f} .. {max(v):8.2f}")
    for a, b in (("fwd absolute", "fwd pad_relative (ids + embed)"), ("bwd absolute", "bwd pad_relative")):
        r = [y / x for x, y in zip(rounds[a], rounds[b])]
        print(f"  ratio {b} / {a}: {statistics.median(rounds[b]) / statistics.median(rounds[a]):.3f} "
              f"(per-round ratios {min(r):.3f} .. {max(r):.3f})")


if __name__ == "__main__":
    print("embedding stage, absolute (BERT) vs pad-relative (RoBERTa) position rule; " + torch.cuda.get_device_name(0))
    case(2688, 30)
    case(160, 512)
