"""gemm8p MFMA shape A/B (knob gemm8p_mfma: 16 = 16x16x32, 32 = 32x32x16) at the six NT products of the BERT-base step, M = 54 919 token rows,
fp16 and bf16 operands ~ N(0, 0.5): un-profiled, >= SECONDS of back-to-back launches per cell, the two shapes alternating, ROUNDS times over
(the spread of a cell over its rounds is the run-to-run noise a difference has to beat).

    python scripts/mfma_shape_bench.py [--seconds 2] [--rounds 2] [--shapes 16,32] [--tn | --only-tn] >> profiles/mfma_shape_launches.txt

--shapes 0 times whatever the library picks (a library without the knob: MOREC_HIP_LIB=...).  --tn adds the weight-gradient products on
gemm_tn8p (no shape knob there: a number for comparing two libraries).
"""
import argparse
import math
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import _lib, ops  # noqa: E402
from idvs.morec_amd._lib import ACT_GELU, DACT_MUL  # noqa: E402
from idvs.morec_amd.engine import _splitk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=2.0)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--shapes", default="16,32")
ap.add_argument("--M", type=int, default=54919)
ap.add_argument("--tn", action="store_true")
ap.add_argument("--only-tn", action="store_true")
args = ap.parse_args()
shapes = [int(x) for x in args.shapes.split(",")]
L = _lib.lib()
M = args.M
PRODUCTS = ((768, 768, "plain"), (2304, 768, "plain"), (3072, 768, "gelu+act'"), (768, 3072, "plain"), (3072, 768, "x act'+colsum"), (768, 2304, "plain"))


def timed(fn):
    """us per launch over >= args.seconds of back-to-back launches (count sized from a short run)."""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(10, int(math.ceil(args.seconds * 1e3 / (e0.elapsed_time(e1) / 10))))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


print(f"# box {socket.gethostname()} ({torch.cuda.get_device_name(0)}), library {os.path.basename(_lib.LIB_PATH)}, M = {M}, "
      f">= {args.seconds} s per cell, {args.rounds} rounds, shapes alternate within a round", flush=True)
print("# dtype  N     K     epilogue        mfma   us per launch (each round)   TFLOP/s (mean)   spread   16 vs 32", flush=True)
for dt, dname in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
    for N, K, kind in (() if args.only_tn else PRODUCTS):
        a = (torch.randn(M, K, device="cuda") * 0.5).to(dt)
        b = (torch.randn(N, K, device="cuda") * 0.5).to(dt)
        out = torch.empty(M, N, device="cuda", dtype=dt)
        kw = {}
        if kind.startswith("gelu"):
            kw = dict(act=ACT_GELU, aux_out=torch.empty(M, N, device="cuda", dtype=dt), aux_deriv=True)
        elif kind.startswith("x act'"):
            kw = dict(dact=DACT_MUL, dact_in=torch.randn(M, N, device="cuda").to(dt), colsum_out=torch.zeros(N, device="cuda"))
        us = {s: [] for s in shapes}
        for _ in range(args.rounds):
            for s in shapes:
                if s:
                    assert L.morec_tuning_set(b"gemm8p_mfma", s) == 0
                us[s].append(timed(lambda: ops.gemm_nt(a, b, out=out, **kw)))
        mean = {s: sum(v) / len(v) for s, v in us.items()}
        for s in shapes:
            ratio = f"{mean[32] / mean[16]:.3f} x" if s == 16 and 32 in mean else ""
            print(f"{dname:6s} {N:5d} {K:5d} {kind:15s} {s:4d}   {' '.join(f'{u:8.1f}' for u in us[s]):28s} {2.0 * M * N * K / mean[s] / 1e6:8.0f}"
                  f"   {(max(us[s]) - min(us[s])) / mean[s] * 100:5.2f} %   {ratio}", flush=True)
    if args.tn or args.only_tn:      # out[N, K] += dy[M, N]^T x[M, K]
        for N, K in ((768, 768), (2304, 768), (3072, 768), (768, 3072)):
            dy = (torch.randn(M, N, device="cuda") * 0.5).to(dt)
            x = (torch.randn(M, K, device="cuda") * 0.5).to(dt)
            o = torch.zeros(N, K, device="cuda")
            split = _splitk(N, K, M)
            v = [timed(lambda: ops.gemm_tn_(dy, x, o, split_m=split, accumulate=True)) for _ in range(args.rounds)]
            m = sum(v) / len(v)
            print(f"{dname:6s} {N:5d} {K:5d} {'tn (dW)':15s}    -   {' '.join(f'{u:8.1f}' for u in v):28s} {2.0 * M * N * K / m / 1e6:8.0f}   {(max(v) - min(v)) / m * 100:5.2f} %",
                  flush=True)
if shapes != [0]:
    L.morec_tuning_set(b"gemm8p_mfma", 0)
