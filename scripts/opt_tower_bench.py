"""The stages of the OPT text tower that are its own, each against the torch composition it replaces, and the whole tower.
  * embedding stage forward (``morec_mask_pos_ids`` + ``morec_opt_embed_fwd``) against ``cumsum`` / two ``index_select`` / add / cast, and
    backward (argsort + ``morec_roberta_embed_bwd`` over the mask's ``perm`` / ``cnt``) against two fp32 ``index_add_``;
  * masked mean pooling forward and backward against ``(h * mask).sum(1) / mask.sum(1).clamp(1e-9)`` and its broadcast backward;
  * opt-125m forward + backward at the same batch in the padded and in the packed layout.
2688 titles x 30 tokens, H = 768, fp16; the arms of a group are timed in interleaved rounds of one process; per arm the median and the
range of the rounds.  Not measured: bf16, larger models, more than one GPU, real checkpoints (random weights, synthetic titles).
    python scripts/opt_tower_bench.py > profiles/opt_tower.txt"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.model import HipOPTModel, OptShape, Text_Encoder_mean  # noqa: E402

DEV, H, V, N_SEQ, T, ROUNDS = "cuda", 768, 50272, 2688, 30, 11
DT = torch.float16


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
        for _ in range(3):
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


def titles(g):
    lens = torch.randint(8, T + 1, (N_SEQ,), generator=g)
    real = torch.arange(T)[None, :] < lens[:, None]
    ids = torch.where(real, torch.randint(3, V, (N_SEQ, T), generator=g), torch.ones(N_SEQ, T, dtype=torch.int64))
    ids[:, 0] = 2
    return ids, real.long()


def stages():
    g = torch.Generator().manual_seed(1)
    ids, mask = titles(g)
    M, n_pos = N_SEQ * T, 2050
    ids32, mask32 = ids.to(torch.int32).view(-1).to(DEV), mask.to(torch.int32).view(-1).to(DEV)
    ids_l, mask_l = ids.to(DEV), mask.to(DEV)
    word, pos = torch.randn(V, H, generator=g).to(DEV), torch.randn(n_pos, H, generator=g).to(DEV)
    dz = (torch.randn(M, H, generator=g) * mask.view(-1, 1)).to(DT).to(DEV)
    dword, dpos = torch.zeros(V, H, device=DEV), torch.zeros(n_pos, H, device=DEV)
    pos_ids, perm, cnt = ops.mask_pos_ids(mask32, T, 2, n_pos)

    def fwd_hip():
        p, _, _ = ops.mask_pos_ids(mask32, T, 2, n_pos)
        ops.opt_embed_fwd(ids32, p, word, pos, DT)

    def fwd_torch():
        p = torch.cumsum(mask_l, 1) * mask_l - 1 + 2
        return (word[ids_l.view(-1)] + pos[p.view(-1)]).to(DT)

    def bwd_hip():
        order = torch.argsort(ids32).to(torch.int32)
        ops.roberta_embed_bwd_(ids32, dz, dword, dpos, None, 1, T, perm, cnt, 1, order)

    pos_l, ids_flat = pos_ids.long(), ids_l.view(-1)
    not_pad = (ids_flat != 1).view(-1, 1)

    def bwd_torch():
        d32 = dz.float()
        dword.index_add_(0, ids_flat, d32 * not_pad)
        dpos.index_add_(0, pos_l, d32)
    report(f"embedding stage, {N_SEQ} titles x {T} tokens, H = {H}, fp16 ({M * H * 2 / 1e6:.1f} MB of rows)",
           {"fwd hip (mask_pos_ids + opt_embed_fwd)": fwd_hip, "fwd torch (cumsum, 2 gathers, add, cast)": fwd_torch,
            "bwd hip (argsort + roberta_embed_bwd)": bwd_hip, "bwd torch (cast + 2 index_add_)": bwd_torch}, 20,
           (("fwd hip (mask_pos_ids + opt_embed_fwd)", "fwd torch (cumsum, 2 gathers, add, cast)"),
            ("bwd hip (argsort + roberta_embed_bwd)", "bwd torch (cast + 2 index_add_)")))

    x = torch.randn(M, H, generator=g).to(DT).to(DEV)
    gm = torch.randn(N_SEQ, H, generator=g).to(DT).to(DEV)
    keep = mask.float().view(-1).to(DEV)
    me = mask_l.unsqueeze(-1).float()

    def pool_torch():
        return ((x.view(N_SEQ, T, H) * me).sum(1) / me.sum(1).clamp(min=1e-9)).to(DT)

    def pool_bwd_torch():
        return ((gm.float() / me.sum(1).clamp(min=1e-9))[:, None, :] * me).to(DT)
    report(f"masked mean pooling, padded layout, {N_SEQ} x {T} x {H}, fp16",
           {"fwd hip (masked_mean_fwd)": lambda: ops.masked_mean_fwd(x, keep, N_SEQ, T),
            "fwd torch (mul, sum, clamp, div, cast)": pool_torch,
            "bwd hip (masked_mean_bwd)": lambda: ops.masked_mean_bwd(gm, keep, N_SEQ, T, M),
            "bwd torch (div, broadcast mul, cast)": pool_bwd_torch}, 20,
           (("fwd hip (masked_mean_fwd)", "fwd torch (mul, sum, clamp, div, cast)"),
            ("bwd hip (masked_mean_bwd)", "bwd torch (div, broadcast mul, cast)")))


def tower():
    g = torch.Generator().manual_seed(2)
    ids, mask = titles(g)
    text = torch.cat((ids, mask), 1).to(DEV)
    torch.manual_seed(0)
    enc = Text_Encoder_mean(HipOPTModel(OptShape.named("opt_125m"), dropout=0.0), 512, 768, DT).to(DEV).train()
    R = torch.randn(N_SEQ, 512, generator=g).to(DEV)

    def step(unpad):
        def run():
            enc.unpad = unpad
            enc.zero_grad(set_to_none=True)
            (enc.encode(text).float() * R).sum().backward()
        return run
    n_tok = int(mask.sum())
    report(f"opt-125m tower forward + backward (every parameter trainable, dropout 0), {N_SEQ} titles x {T} tokens "
           f"({n_tok} real tokens of {N_SEQ * T}), fp16, item dim 512",
           {"padded layout": step(False), "packed layout": step(True)}, 3, (("packed layout", "padded layout"),))


if __name__ == "__main__":
    print("OPT text tower: its own stages against the torch compositions they replace, and the tower; MI355X (" + torch.cuda.get_device_properties(0).gcnArchName.split(":")[0] + ")")
    stages()
    tower()
