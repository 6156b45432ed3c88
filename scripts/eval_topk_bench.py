"""Top-K selection at the bench's eval shape (I = 80 001 items, D = 512, histories of ~23 ids, K = 10), for U = 512 and U = 4096 users:
  (a) ops.eval_topk                    -- score tiles + selection in LDS, no score matrix
  (b) ops.eval_rank on the same inputs -- the same matrix work, a count instead of a selection (the yardstick for the selection's cost)
  (c) the torch data flow (a) replaces -- prec @ emb.T, scatter_ of -inf over the histories, torch.topk
Each variant is warmed up, then the three are timed in turn, REPEATS rounds of ITERS calls each (device events around the ITERS calls),
so that a drift of the clock or a neighbour on the host hits all three alike.  Reports the median and the range over the rounds and
says once for how many users (a) and (c) return the same ids ((c)'s GEMM rounds differently: near-ties may swap).
python scripts/eval_topk_bench.py [--out profiles/eval_topk.txt] [--repeats 7] [--iters 10] [--strips 0]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from idvs.morec_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--strips", type=int, default=0)
ap.add_argument("--items", type=int, default=80001)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--hmax", type=int, default=23)
ap.add_argument("--k", type=int, default=10)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("eval_topk_bench needs the GPU: a CPU run measures nothing")
dev = "cuda"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


say(f"eval_topk_bench: I = {a.items}, D = {a.dim}, Hmax = {a.hmax}, K = {a.k}, strips = {a.strips} (0 = automatic); "
    f"{a.repeats} interleaved rounds x {a.iters} calls, 3 warm-up calls each; {torch.cuda.get_device_name(0)}")
g = torch.Generator(device=dev).manual_seed(1234)
emb = torch.randn(a.items, a.dim, device=dev, generator=g)
for U in (512, 4096):
    prec = torch.randn(U, a.dim, device=dev, generator=g)
    hist = torch.randint(1, a.items, (U, a.hmax), device=dev, generator=g, dtype=torch.int32)
    hist[:, -3:] = -1                                     # padded tails
    target = torch.randint(1, a.items, (U,), device=dev, generator=g, dtype=torch.int32)
    hidx = hist.long().clamp_min(0)                       # scatter index of (c): padding -> column 0, which is dropped anyway

    def f_topk():
        return ops.eval_topk(prec, emb, hist, a.k, a.strips)

    def f_rank():
        return ops.eval_rank(prec, emb, hist, target)

    def f_torch():
        s = prec @ emb.T
        s.scatter_(1, hidx, float("-inf"))
        s[:, 0] = float("-inf")
        return torch.topk(s, a.k, dim=1)

    fns = (("a eval_topk", f_topk), ("b eval_rank", f_rank), ("c torch matmul+scatter+topk", f_torch))
    for _, fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ids, sc = f_topk()
    tv, ti = f_torch()
    tie_free = (tv[:, 1:] < tv[:, :-1]).all(1)
    same = int((ids.long() == ti).all(1)[tie_free].sum())
    close = (sc - tv).abs().max().item()
    say(f"U = {U}: (a) and (c) return the same ids for {same} of the {int(tie_free.sum())} users whose (c) scores are tie-free ({U} users); max |score a - score c| = {close:.3e} "
        f"(c's GEMM is not the exact-fp32 one)")
    times = {n: [] for n, _ in fns}
    for _ in range(a.repeats):
        for n, fn in fns:
            times[n].append(timed(fn, a.iters))
    flop = 2.0 * U * a.items * a.dim
    for n, _ in fns:
        t = times[n]
        med = statistics.median(t)
        say(f"U = {U:5d}  {n:30s} median {med:9.1f} us  (min {min(t):9.1f}, max {max(t):9.1f})  {flop / med / 1e6:7.1f} TFLOP/s of score work")
    ma, mb, mc = (statistics.median(times[n]) for n, _ in fns)
    say(f"U = {U:5d}  a / b = {ma / mb:.2f}   a / c = {ma / mc:.2f}   score matrix of (c): {U * a.items * 4 / 1e6:.0f} MB")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
