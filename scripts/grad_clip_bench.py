#!/usr/bin/env python
"""What global-norm clipping and the LR schedule cost on the device.

Three comparisons, each interleaved in rounds on one GPU so that drift of the box hits both sides alike:

1. kernel: ``morec_grad_norm_check`` against ``morec_grad_check_finite`` on an arena the size of the BERT-base tower's gradient arena
   (device events around ``--iters`` back-to-back launches; both read 4 B / parameter);
2. step: the fp16 ``TrainStep`` at the bench configuration (BERT-base, batch 128, S = 20, T = 30, D = 512) with ``max_grad_norm`` on and off;
3. step: the same with a cosine schedule on and off.

``--baseline_tree DIR`` (a checkout of the PARENT commit with its library built): its check kernel and its step are timed in child processes
that alternate with this tree's, and reported next to them.  Without it the "off" side of this tree stands in (same source for the check
kernel; the AdamW kernel differs by two flag tests).

Prints a table and, with ``--out``, writes it to a file (``profiles/grad_clip.txt``).  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds per comparison")
    ap.add_argument("--iters", type=int, default=50, help="kernel launches per round and side")
    ap.add_argument("--steps", type=int, default=12, help="timed steps per round and side")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--bert", default="base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--item_num", type=int, default=20000)
    ap.add_argument("--baseline_tree", default=None)
    ap.add_argument("--commit", default="unknown", help="what the numbers were taken against (written into the report)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=["kernel", "step"], help="internal: time one side of THIS python path's tree, print JSON")
    ap.add_argument("--variants", default="off", help="internal: comma list of off,clip,sched")
    return ap.parse_args()


def build(a, variant):
    """The bench configuration's model and a TrainStep on it (``variant``: off | clip | sched)."""
    import numpy as np
    import torch

    import bench
    from idvs.morec_amd.model import BertShape, HipBertModel, Model
    from idvs.morec_amd.train_step import TrainStep
    S, T, D = 20, 30, 512
    shape = BertShape.named(a.bert)
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                 num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="bert_" + a.bert, word_embedding_dim=shape.hidden_size, compute_dtype="fp16")
    rng = np.random.default_rng(12345)
    content = bench.synth_catalog(a.item_num, T, rng)
    n = a.warmup + a.steps
    ids_all = bench.synth_batches(n, a.batch, S, a.item_num, np.random.default_rng(12345))
    counts = np.bincount(ids_all.reshape(-1), minlength=a.item_num + 1).astype(np.float64) + 1.0
    pop = counts / counts[1:].sum()
    pop[0] = 1.0
    torch.manual_seed(12345)
    model = Model(args, a.item_num, True, HipBertModel(shape), pop).to("cuda").train()
    kw = {}
    if variant == "clip":
        kw["max_grad_norm"] = 1.0
    elif variant == "sched":
        from idvs.morec_amd.lr_schedule import LrSchedule
        kw["lr_schedule"] = LrSchedule("cosine", 100, 10000, 0.1)
    ts = TrainStep(model, lr=1e-4, fine_tune_lr=5e-5, l2_weight=0.01, fine_tune_l2_weight=0.01, pool_negatives=False, defer_update=True, **kw)
    from idvs.morec_amd import engine
    batches = []
    for i in range(n):
        rows = content[ids_all[i].reshape(-1)]
        pack = tuple(t.to("cuda") for t in engine.token_packing_host(rows[:, T:], rows[:, :T]))
        batches.append((torch.from_numpy(ids_all[i]).to("cuda").view(-1), torch.from_numpy(rows).to("cuda"), torch.ones(a.batch, S, device="cuda"), pack))
    return ts, batches


def time_steps(ts, batches, warm, steps):
    """Milliseconds per step over ``steps`` steps behind ``warm`` untimed ones: host clock around work that ends in a synchronise."""
    import torch
    for b in batches[:warm]:
        ts.step(b[0], b[1], b[2], token_packing=b[3])
    ts.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches[warm:warm + steps]:
        ts.step(b[0], b[1], b[2], token_packing=b[3])
    ts.flush()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def time_kernel(fn, iters):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # microseconds per launch


def child(a):
    """One process = one tree (whatever PYTHONPATH names): kernel -> us per launch of the check kernel(s); step -> ms per step per variant."""
    import torch
    from idvs.morec_amd import ops
    out = {}
    if a.child == "kernel":
        ts, _ = build(a, "off")
        n = ts.groups[0]["arena"].numel
        del ts
        g = torch.randn(n, device="cuda") * 1e-2
        sp = ops.StepParams("cuda", init_scale=65536.0)
        out["n"] = n
        out["check_finite"] = [time_kernel(lambda: sp.check_finite_(g), a.iters) for _ in range(2)]
        if hasattr(sp, "norm_check_"):
            sp.reserve_partials(sp.norm_slots(n))
            rounds = {"check_finite": [], "norm_check": []}
            for _ in range(a.rounds):      # interleaved inside the process as well
                rounds["check_finite"].append(time_kernel(lambda: sp.check_finite_(g), a.iters))
                rounds["norm_check"].append(time_kernel(lambda: sp.norm_check_(g, 0), a.iters))
            out.update(rounds)
    else:
        for v in a.variants.split(","):
            ts, batches = build(a, v)
            out[v] = time_steps(ts, batches, a.warmup, a.steps)
            ts.close()
            del ts, batches
            torch.cuda.empty_cache()
    print("GRADCLIP_JSON " + json.dumps(out), flush=True)


def run_child(a, tree, part, variants="off"):
    env = dict(os.environ, PYTHONPATH=tree + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--variants", variants, "--iters", str(a.iters), "--rounds", str(a.rounds),
           "--steps", str(a.steps), "--warmup", str(a.warmup), "--bert", a.bert, "--batch", str(a.batch), "--item_num", str(a.item_num)]
    r = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("GRADCLIP_JSON "):
            print(f"[{time.strftime('%H:%M:%S')}] {os.path.basename(tree.rstrip('/'))} {part} {variants}: {line[len('GRADCLIP_JSON '):][:200]}", file=sys.stderr, flush=True)
            return json.loads(line[len("GRADCLIP_JSON "):])
    raise RuntimeError(f"child ({tree}, {part}) gave no result: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def main():
    a = parse()
    if a.child:
        return child(a)
    lines = [f"grad_clip_bench: taken against {a.commit}; {a.rounds} interleaved rounds; median [min .. max]"]
    # 1. kernels
    k_new = run_child(a, ROOT, "kernel")
    n = k_new["n"]
    lines.append(f"arena: {n} fp32 gradients ({n * 4 / 2 ** 20:.1f} MiB), the BERT-{a.bert} tower group")
    for name in ("check_finite", "norm_check"):
        med, lo, hi = stats(k_new[name])
        lines.append(f"  this tree   morec_grad_{name:<13s} {med:8.1f} us [{lo:.1f} .. {hi:.1f}]   {n * 4 / med / 1e6:7.2f} TB/s")
    if a.baseline_tree:
        par = []
        for _ in range(2):
            par += run_child(a, a.baseline_tree, "kernel")["check_finite"]
        med, lo, hi = stats(par)
        lines.append(f"  parent tree morec_grad_check_finite  {med:8.1f} us [{lo:.1f} .. {hi:.1f}]   {n * 4 / med / 1e6:7.2f} TB/s")
    # 2. / 3. steps: processes alternate parent, this tree (off, clip, sched), parent, ...
    res = {"off": [], "clip": [], "sched": [], "parent": []}
    order = ["off", "clip", "sched"]
    for rd in range(a.rounds):
        if a.baseline_tree:
            res["parent"].append(run_child(a, a.baseline_tree, "step", "off")["off"])
        r = run_child(a, ROOT, "step", ",".join(order[rd % 3:] + order[:rd % 3]))      # rotated: no variant always runs last in its process
        for k in ("off", "clip", "sched"):
            res[k].append(r[k])
    lines.append(f"fp16 TrainStep, BERT-{a.bert}, batch {a.batch}, S 20, T 30, D 512, deferred update; ms per step over {a.steps} steps")
    for k, label in (("parent", "parent tree"), ("off", "this tree, off"), ("clip", "max_grad_norm = 1"), ("sched", "cosine schedule")):
        if res[k]:
            med, lo, hi = stats(res[k])
            lines.append(f"  {label:<20s} {med:8.2f} ms [{lo:.2f} .. {hi:.2f}]")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
