#!/usr/bin/env python
"""Synchronised BatchNorm of the ResNet item tower on ONE device, fp16 --

  1. the plain path against another build: forward + backward of ``Resnet_Encoder`` over ResNet-50 (unconverted modules, training mode,
     ``--images`` decoded uint8 images of 224 px) in this tree and in the tree given by ``--other-root`` (a checkout of the parent commit
     with its own ``libmorec_hip.so``).  One worker process per tree, both alive, their windows alternating round by round; the check is
     that this tree's median lies within the other tree's own round-to-round range.
  2. what synchronisation adds per BatchNorm layer ON THE DEVICE: the extra launches (the rank's own slabs merged into [3, C], the merge
     over W rank partials, the fold of W backward sums, the apply that reads the count) against the plain ``stats + merge`` and
     ``reduce + apply``, at the stem shape (``images`` x 112 x 112 rows, C = 64) and a layer-4 shape (``images`` x 7 x 7 rows, C = 2048),
     with a stand-in gather: the rank's own partial stacked W = 8 times.

Nothing here measures communication: there is one device and no collective.  RCCL at more than one GPU is unmeasured.

Timing: device events around windows of ``--iters`` calls after a warm-up of every variant, ``--rounds`` windows per variant, the variants
of a group alternating window by window; reported: median and min .. max per call.

    python scripts/resnet_syncbn_bench.py [--out FILE] [--images 704] [--other-root DIR]
"""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 8


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def worker(root, n_img, D):
    """One tree's tower: warm up, print READY, then one window (one forward + backward) per line read from stdin."""
    sys.path.insert(0, root)
    import torch
    from idvs.morec_amd.model.encoders import Resnet_Encoder
    from idvs.morec_amd.model.resnet import HipResNet, ResNetShape
    enc = Resnet_Encoder(HipResNet(ResNetShape.named("resnet50"), D), compute_dtype=torch.float16).to("cuda").train()
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (n_img, 224, 224, 3), generator=g, dtype=torch.uint8).to("cuda")
    d_item = (torch.randn((n_img, D), generator=g) * 1e-2).to("cuda").to(torch.float16)

    def step():
        for p in enc.parameters():
            p.grad = None
        enc.encode(images).backward(d_item)

    step()
    torch.cuda.synchronize()
    print("READY", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        print(f"{a.elapsed_time(b):.4f}", flush=True)


def towers(roots, n_img, D, rounds, log):
    procs = {}
    try:
        for name, root in roots.items():
            procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--images", str(n_img), "--dim", str(D)],
                                           stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        for name, p in procs.items():
            line = p.stdout.readline().strip()
            if line != "READY":
                raise SystemExit(f"worker {name} did not start: {line!r} (exit {p.poll()})")
        t = {k: [] for k in procs}
        for _ in range(rounds):
            for name, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                t[name].append(float(p.stdout.readline()))
    finally:
        for p in procs.values():
            if p.poll() is None:
                try:
                    p.stdin.close()
                    p.wait(60)
                except Exception:
                    p.kill()
    for name in t:
        log(f"ResNet-50 tower, plain path (BatchNorm2d, one process), {n_img} images of 224 px, fp16, training mode, forward + backward, "
            f"{name}: {fmt(t[name])} over {rounds} alternating rounds")
    if len(t) == 2:
        mine, other = statistics.median(t["this tree"]), t["other tree"]
        log(f"this tree's median {mine:.3f} ms is {'within' if min(other) <= mine <= max(other) else 'OUTSIDE'} the other tree's range "
            f"{min(other):.3f} .. {max(other):.3f} ms")


def per_layer(n_img, iters, rounds, log):
    import torch
    sys.path.insert(0, HERE)
    from idvs.morec_amd import ops
    sys.path.insert(0, os.path.join(HERE, "scripts"))
    from resnet_bench import alternate
    torch.manual_seed(5)
    for what, hw, C in (("stem", 112, 64), ("layer 4", 7, 2048)):
        rows = n_img * hw * hw
        x = (torch.randn((rows, C), device="cuda").abs_() + 0.5).half()
        dy = torch.randn((rows, C), device="cuda").half()
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        mean, rstd, merged = ops.bn_merge(ops.bn_stats(x), 1e-5, need_merged=True)
        y = ops.bn_apply_fwd(x, mean, rstd, gamma, beta, relu=True)
        count = merged[0]

        def plain_fwd():
            return ops.bn_merge(ops.bn_stats(x), 1e-5, rm, rv)

        def sync_fwd():
            local = ops.bn_merged(ops.bn_stats(x))
            return ops.bn_merge(local.unsqueeze(0).repeat(W, 1, 1), 1e-5, rm, rv, need_merged=True)      # the stand-in gather

        def plain_bwd():
            return ops.bn_bwd_apply(dy, y, x, mean, rstd, gamma, ops.bn_bwd_reduce(dy, y, x, mean, rstd))

        def sync_bwd():
            sums = ops.bn_bwd_fold(ops.bn_bwd_reduce(dy, y, x, mean, rstd).unsqueeze(0).repeat(W, 1, 1))
            return ops.bn_bwd_apply(dy, y, x, mean, rstd, gamma, sums, count=count)

        def extra_fwd():      # everything behind the stats kernel, on a partial that is already there
            return ops.bn_merge(ops.bn_merged(part).unsqueeze(0).repeat(W, 1, 1), 1e-5, rm, rv, need_merged=True)

        def extra_bwd():
            return ops.bn_bwd_fold(sums0.unsqueeze(0).repeat(W, 1, 1))

        part, sums0 = ops.bn_stats(x), ops.bn_bwd_reduce(dy, y, x, mean, rstd)
        t = alternate({"plain_fwd": plain_fwd, "sync_fwd": sync_fwd, "plain_bwd": plain_bwd, "sync_bwd": sync_bwd, "extra_fwd": extra_fwd,
                       "extra_bwd": extra_bwd}, iters, rounds)
        med = {k: statistics.median(v) for k, v in t.items()}
        log(f"BatchNorm, {what} shape [{rows}, {C}] ({part.shape[0]} slabs), fp16, W = {W} stand-in gather:  forward statistics plain "
            f"(stats + merge) {fmt(t['plain_fwd'])}   synchronised (stats + local merge + stack + rank merge) {fmt(t['sync_fwd'])}   "
            f"difference {med['sync_fwd'] - med['plain_fwd']:+.3f} ms; local merge + stack + rank merge without the stats kernel {fmt(t['extra_fwd'])} "
            "(the local merge takes the place of the plain path's merge launch, serial over the slabs: only the stack and the rank merge over "
            f"{W} partials are added)")
        log(f"BatchNorm, {what} shape [{rows}, {C}], fp16, W = {W} stand-in gather:  backward plain (reduce + apply) {fmt(t['plain_bwd'])}   "
            f"synchronised (reduce + stack + fold + apply with the device count) {fmt(t['sync_bwd'])}   difference "
            f"{med['sync_bwd'] - med['plain_bwd']:+.3f} ms; the added fold (with its stack) alone {fmt(t['extra_bwd'])}")
        del x, dy, y
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=704)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--other-root", default="", help="a checkout of the commit to compare the plain path against, built")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.images, a.dim)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resnet_syncbn_bench.py measures on the device: no GPU here")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:      # written line by line: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    log(f"# scripts/resnet_syncbn_bench.py on {torch.cuda.get_device_name(0)}: median (min .. max) per call over {a.rounds} windows; one "
        "device, no collective: communication (RCCL at more than one GPU) is NOT measured here")
    per_layer(a.images, a.iters, a.rounds, log)
    roots = {"this tree": HERE}
    if a.other_root:
        roots["other tree"] = os.path.abspath(a.other_root)
    towers(roots, a.images, a.dim, a.rounds, log)


if __name__ == "__main__":
    main()
