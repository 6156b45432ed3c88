#!/usr/bin/env python
"""Forward + backward of the DSSM scoring loss: the two library ops (``ops.dssm_bce_fwd`` / ``ops.dssm_bce_bwd``, three launches) against the
torch composition they replace (``torch.bmm`` + ``binary_cross_entropy_with_logits`` and their autograd).  B = 512, neg_num in
{1, 4, 100}, D in {256, 512}, plus two few-user shapes (B = 4 / 8 with 300 / 500 negatives), fp16.  Both versions are warmed up at every shape, timed with device events over windows of about 1.5 s, alternating, three rounds each (the spread is printed).  Also reported: the achieved bytes/s of the library path
against the algorithmic traffic (bytes the algorithm needs over time, not measured HBM traffic: the tensors of a shape are reused from one
repetition to the next and may sit in the last-level cache) -- forward (R + B) D elements read, backward the same read plus (R + B) D written, R = B (1 + neg_num).

    python scripts/dssm_bench.py [--out profiles/dssm_bce.txt]

Needs a GPU (there is no CPU fallback); the table goes to stdout and to ``--out``."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import ops  # noqa: E402

DEV = "cuda"


def time_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dssm_bce.txt"))
    ap.add_argument("--B", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dssm_bench: no GPU")
    B, dtype = args.B, torch.float16
    lines = [f"DSSM scoring loss, forward + backward, fp16, {torch.cuda.get_device_name(0)}",
             "ms per fwd+bwd: median of three rounds (min .. max); library GB/s = algorithmic bytes, 3 (R + B) D elements of 2 bytes, over that time",
             f"{'B':>5} {'neg_num':>7} {'D':>4} {'R':>6} | {'library ms':>24} | {'torch ms':>24} | {'torch/library':>13} | {'library GB/s':>12}"]
    shapes = [(B, neg, D) for neg in (1, 4, 100) for D in (256, 512)] + [(4, 300, 512), (8, 500, 512)]      # the last two: few users, many negatives
    for B, neg, D in shapes:
        if True:
            n1 = 1 + neg
            R = B * n1
            g = torch.Generator(device=DEV).manual_seed(neg * 1000 + D)
            U = (torch.randn(B, D, device=DEV, generator=g) * 0.1).to(dtype)
            E = (torch.randn(R, D, device=DEV, generator=g) * 0.1).to(dtype)
            y = torch.zeros(B, n1, device=DEV)
            y[:, 0] = 1.0
            yf = y.reshape(-1).contiguous()
            gs = torch.full((1,), 1.0 / R, device=DEV)

            def lib():
                scores, _, loss_sum = ops.dssm_bce_fwd(U, E, yf, B, n1)
                return ops.dssm_bce_bwd(U, E, yf, scores, gs, B, n1)

            Ut, Et = U.clone().requires_grad_(True), E.clone().requires_grad_(True)

            def ref():
                Ut.grad = Et.grad = None
                s = torch.bmm(Et.view(B, n1, D), Ut.unsqueeze(-1)).squeeze(-1)
                torch.nn.functional.binary_cross_entropy_with_logits(s.float().view(-1), yf).backward()
                return Ut.grad, Et.grad

            dU, dE = lib()
            rU, rE = ref()
            torch.cuda.synchronize()
            err = max(float((dU.float() - rU.float()).norm() / rU.float().norm()), float((dE.float() - rE.float()).norm() / rE.float().norm()))
            for fn in (lib, ref):       # warm-up at this shape
                time_ms(fn, 20)
            reps = {}
            for name, fn in (("lib", lib), ("ref", ref)):
                reps[name] = max(50, int(1500.0 / max(time_ms(fn, 20), 1e-3)))      # ~1.5 s per timed window
            t = {"lib": [], "ref": []}
            for _ in range(3):          # alternating
                t["lib"].append(time_ms(lib, reps["lib"]))
                t["ref"].append(time_ms(ref, reps["ref"]))
            med = {k: sorted(v)[1] for k, v in t.items()}
            gbs = 3 * (R + B) * D * 2 / (med["lib"] * 1e-3) / 1e9
            fmt = lambda v: f"{sorted(v)[1]:8.4f} ({min(v):.4f} .. {max(v):.4f})"
            lines.append(f"{B:>5} {neg:>7} {D:>4} {R:>6} | {fmt(t['lib']):>24} | {fmt(t['ref']):>24} | {med['ref'] / med['lib']:>13.2f} | {gbs:>12.1f}"
                         f"   (gradients vs torch: rel {err:.1e})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
