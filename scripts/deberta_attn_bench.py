"""DeBERTa's disentangled attention (``morec_disent_attn_fwd`` / ``_bwd``, csrc/deberta.hip), forward and backward, against
  * the torch composition it replaces (three matmuls, two gathers, masked_fill, softmax, matmul, and autograd for the backward), and
  * ``morec_attn_fwd`` / ``_bwd`` at the same shape: what the two position terms cost on top of plain attention;
and the deberta-base tower forward + backward.  fp16, 2688 titles x 30 tokens and 1792 x 50, H = 768, 12 heads; the arms of a group are
timed in interleaved rounds of one process; per arm the median and the range of the rounds.  No ratio is a condition of anything: the
figures are written down as they come out.  Not measured: bf16, fp32 (the gen path), deberta-large, more than one GPU.
    python scripts/deberta_attn_bench.py > profiles/deberta_attn.txt"""
import math
import statistics
import sys

import torch

sys.path.insert(0, ".")
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.model import DebertaShape, HipDebertaModel, Text_Encoder  # noqa: E402

DEV, H, HEADS, V, ROUNDS = "cuda", 768, 12, 50265, 7
DT = torch.float16
SHAPES = ((2688, 30), (1792, 50))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def report(title, arms, iters, pairs=()):
    for fn in arms.values():      # warm-up: allocator, code objects
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(timed(fn, iters))
    print(f"\n{title}; {ROUNDS} interleaved rounds x {iters} calls, us per call")
    for k, v in rounds.items():
        print(f"  {k:44s} median {statistics.median(v):10.2f}   range {min(v):10.2f} .. {max(v):10.2f}")
    for a, b in pairs:
        r = [x / y for x, y in zip(rounds[a], rounds[b])]
        print(f"  ratio {a} / {b}: {statistics.median(rounds[a]) / statistics.median(rounds[b]):.3f} (per-round ratios {min(r):.3f} .. {max(r):.3f})")


def titles(g, n_seq, T):
    lens = torch.randint(min(8, T), T + 1, (n_seq,), generator=g)
    real = torch.arange(T)[None, :] < lens[:, None]
    ids = torch.where(real, torch.randint(3, V, (n_seq, T), generator=g), torch.zeros(n_seq, T, dtype=torch.int64))
    ids[:, 0] = 1
    return ids, real.long()


def torch_attn(qkv, keep_b, pk, pq, idx, idx_t, scale, n_seq, T):
    dh = H // HEADS
    q, k, v = (qkv[:, s * H:(s + 1) * H].view(n_seq, T, HEADS, dh).permute(0, 2, 1, 3) for s in range(3))
    pkh, pqh = (x.view(2 * T, HEADS, dh).permute(1, 0, 2) for x in (pk, pq))
    c2p = torch.gather(torch.matmul(q, pkh.transpose(-1, -2)), -1, idx)
    p2c = torch.gather(torch.matmul(k, pqh.transpose(-1, -2)), -1, idx_t).transpose(-1, -2)
    s = (torch.matmul(q, k.transpose(-1, -2)) + c2p + p2c) * scale
    s = s.masked_fill(~keep_b, torch.finfo(s.dtype).min)
    return torch.matmul(torch.softmax(s, -1), v).permute(0, 2, 1, 3).reshape(n_seq * T, H)


def attention(n_seq, T):
    g = torch.Generator().manual_seed(T)
    dh = H // HEADS
    _, mask = titles(g, n_seq, T)
    keep = mask.float().to(DEV)
    qkv = (torch.randn(n_seq * T, 3 * H, generator=g) * 0.7).to(DT).to(DEV)
    pk, pq = ((torch.randn(2 * T, H, generator=g) * 0.7).to(DT).to(DEV) for _ in range(2))
    dctx = torch.randn(n_seq * T, H, generator=g).to(DT).to(DEV)
    scale = 1.0 / math.sqrt(3 * dh)
    desc = ops.attn_desc(n_seq, T, HEADS, dh, False, scale, ops.FLT_MIN_MASK, DT)
    i = torch.arange(T, device=DEV)
    d = i[:, None] - i[None, :] + T
    idx, idx_t = d.expand(n_seq, HEADS, T, T), d.t().expand(n_seq, HEADS, T, T)
    m = keep != 0
    keep_b = (m[:, :, None] & m[:, None, :])[:, None]
    qg, kg, pg = (x.clone().requires_grad_(True) for x in (qkv, pk, pq))

    def torch_fb():
        qg.grad = kg.grad = pg.grad = None
        torch_attn(qg, keep_b, kg, pg, idx, idx_t, scale, n_seq, T).backward(dctx)
    arms = {
        "disent fwd (morec_disent_attn_fwd)": lambda: ops.disent_attn_fwd(desc, qkv, keep, pk, pq),
        "torch fwd (composition, no autograd)": lambda: torch_attn(qkv, keep_b, pk, pq, idx, idx_t, scale, n_seq, T),
        "plain fwd (morec_attn_fwd)": lambda: ops.attn_fwd(desc, qkv, keep),
        "disent bwd, dPK / dPQ formed": lambda: ops.disent_attn_bwd(desc, qkv, keep, pk, pq, dctx),
        "disent bwd, position projections frozen": lambda: ops.disent_attn_bwd(desc, qkv, keep, pk, pq, dctx, need_dpos=False),
        "torch fwd + bwd (autograd)": torch_fb,
        "plain bwd (morec_attn_bwd)": lambda: ops.attn_bwd(desc, qkv, keep, dctx),
    }
    report(f"attention, {n_seq} titles x {T} tokens, H = {H}, {HEADS} heads, fp16 (mfma16 path)", arms, 3,
           (("disent fwd (morec_disent_attn_fwd)", "torch fwd (composition, no autograd)"),
            ("disent fwd (morec_disent_attn_fwd)", "plain fwd (morec_attn_fwd)"),
            ("disent bwd, dPK / dPQ formed", "plain bwd (morec_attn_bwd)"),
            ("disent bwd, position projections frozen", "plain bwd (morec_attn_bwd)")))


def tower(n_seq, T):
    g = torch.Generator().manual_seed(2)
    ids, mask = titles(g, n_seq, T)
    text = torch.cat((ids, mask), 1).to(DEV)
    torch.manual_seed(0)
    bert = HipDebertaModel(DebertaShape.named("deberta_base"), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    enc = Text_Encoder(bert, 512, 768, DT).to(DEV).train()
    R = torch.randn(n_seq, 512, generator=g).to(DEV)

    def run():
        enc.zero_grad(set_to_none=True)
        (enc.encode(text).float() * R).sum().backward()
    report(f"deberta-base tower forward + backward (every parameter trainable, dropout 0), {n_seq} titles x {T} tokens, fp16, item dim 512",
           {"padded layout": run}, 1)


if __name__ == "__main__":
    print("DeBERTa disentangled attention against the torch composition and against plain attention, and the tower; MI355X ("
          + torch.cuda.get_device_properties(0).gcnArchName.split(":")[0] + ")")
    for n_seq, T in SHAPES:
        attention(n_seq, T)
    for n_seq, T in SHAPES:
        tower(n_seq, T)
