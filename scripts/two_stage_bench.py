#!/usr/bin/env python
"""Two-stage training step (``TwoStageModel``: fc over frozen feature rows -> SASRec -> BCE, forward + backward + AdamW) three ways at
B = 128, L = 20, W = 768, D = 512, fp16:

  fused      ids in, the first layer is ``morec_featproj_fwd`` (gather + projection + GELU in one launch; ``MOREC_FEATPROJ=2``);
  composed   ids in, the first layer is ``indexed_rows_copy`` + ``gemm_nt`` (``MOREC_FEATPROJ=1``);
  host       the reference's batch: the feature rows gathered on the host from a CPU table (``item_content[sample_items]``), shipped as
             [B (L + 1) 2, W] fp32 -- gather and H2D copy are inside the timed step, as they are inside the reference's.

and the first layer alone (forward, with the pre-activation output) at R = 5376, fused against composed.  Every version is warmed up, then
timed with device events (the host variant: wall clock around a synchronised step, its work is on the host) in windows of about 1 s,
alternating, three rounds each; median (min .. max) is printed.

    python scripts/two_stage_bench.py [--out profiles/two_stage_step.txt]

Needs a GPU (there is no CPU fallback); the table goes to stdout and to ``--out``."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.model import TwoStageModel  # noqa: E402

DEV = "cuda"


def time_ms(fn, reps, wall=False):
    if wall:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def rounds(variants, window_ms=1000.0, wall=()):
    """{name: fn} -> {name: [three timings]}, alternating between the variants."""
    for name, fn in variants.items():
        time_ms(fn, 10, name in wall)
    reps = {name: max(20, int(window_ms / max(time_ms(fn, 10, name in wall), 1e-3))) for name, fn in variants.items()}
    t = {name: [] for name in variants}
    for _ in range(3):
        for name, fn in variants.items():
            t[name].append(time_ms(fn, reps[name], name in wall))
    return t


def fmt(v):
    return f"{sorted(v)[1]:8.4f} ({min(v):.4f} .. {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "two_stage_step.txt"))
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--dnn_layer", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_bench: no GPU")
    B, L, W, D, dtype = 128, 20, 768, 512, torch.float16
    R = B * (L + 1) * 2
    args = types.SimpleNamespace(max_seq_len=L, embedding_dim=D, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                 dnn_layer=a.dnn_layer, word_embedding_dim=W, compute_dtype="fp16")
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    table_host = torch.from_numpy(rng.standard_normal((a.items + 1, W), dtype=np.float32))
    model = TwoStageModel(args, a.items).to(DEV).train()
    model.set_feature_table(table_host)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    ids_host = torch.from_numpy(rng.integers(1, a.items + 1, (B, L + 1, 2)).astype(np.int32))
    ids_dev = ids_host.to(DEV)
    lm = torch.ones(B, L, device=DEV)

    def step(x):
        opt.zero_grad()
        loss = model(x, lm, DEV)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    def on_device():
        step(ids_dev)

    def host():
        step(table_host[ids_host.long()].view(-1, W).to(DEV, non_blocking=True))

    lines = [f"Two-stage step (fc over frozen features -> SASRec x 2 -> BCE, forward + backward + AdamW), fp16, {torch.cuda.get_device_name(0)}",
             f"B = {B}, L = {L}, W = {W}, D = {D}, dnn_layer = {a.dnn_layer}: R = {R} feature rows per step; ms: median of three rounds (min .. max)"]
    # the knob is read per call: the fused and composed variants alternate inside one process on the same tensors
    t = {"fused": [], "composed": [], "host": []}
    variants = {"fused": (on_device, 2), "composed": (on_device, 1), "host": (host, 0)}      # knob 2: fused wherever the rules allow
    for name, (fn, knob) in variants.items():
        ops.set_featproj(knob)
        time_ms(fn, 10, True)
    reps = {}
    for name, (fn, knob) in variants.items():
        ops.set_featproj(knob)
        reps[name] = max(20, int(1000.0 / max(time_ms(fn, 10, True), 1e-3)))
    for _ in range(3):
        for name, (fn, knob) in variants.items():
            ops.set_featproj(knob)
            t[name].append(time_ms(fn, reps[name], True))
    ops.set_featproj(0)
    lines.append("step, wall clock per synchronised window (the host's launches are part of a launch-bound step):")
    for name in t:
        lines.append(f"  {name:>9}: {fmt(t[name])} ms")
    lines.append(f"  H2D bytes per step: ids {ids_host.numel() * 4 / 1e3:.0f} KB; host-gathered fp32 rows {R * W * 4 / 1e6:.1f} MB")

    table = model.feature_table
    w = model.fc.fc.weight.detach().to(dtype).contiguous()
    bias = model.fc.fc.bias.detach()
    idx = ids_dev.reshape(-1).contiguous()
    out, pre = torch.empty((R, D), device=DEV, dtype=dtype), torch.empty((R, D), device=DEV, dtype=dtype)
    layer = rounds({"fused": lambda: ops.featproj_fwd(table, idx, w, bias, out=out, pre=pre),
                    "composed": lambda: ops.featproj_composed(table, idx, w, bias, need_pre=True)})
    a_out, _ = ops.featproj_fwd(table, idx, w, bias)
    c_out, _, _ = ops.featproj_composed(table, idx, w, bias)
    diff = float((a_out.float() - c_out.float()).abs().max())
    lines.append(f"first layer alone (forward with the pre-activation output), R = {R}, device events:")
    for name in layer:
        lines.append(f"  {name:>9}: {fmt(layer[name])} ms")
    lines.append(f"  fused vs composed output: max |difference| {diff:.3g}")
    # where the automatic rule of morec_featproj_supported comes from: the first layer alone over R and the two widths
    lines.append("first layer alone over R (forward with the pre-activation output), device events, ms:")
    lines.append(f"  {'R':>6} {'W':>5} {'D':>4} | {'fused':>26} | {'composed':>26} | composed/fused")
    g = torch.Generator(device=DEV).manual_seed(1)
    for Ws, Ds in ((W, D), (128, 64)):
        tab = torch.randn(a.items + 1, Ws, device=DEV, generator=g).to(dtype)
        ws = (torch.randn(Ds, Ws, device=DEV, generator=g) * 0.05).to(dtype)
        bs = torch.randn(Ds, device=DEV, generator=g)
        for Rs in (42, 336, 1344, 5376, 21504):
            ix = torch.randint(0, a.items + 1, (Rs,), device=DEV, generator=g, dtype=torch.int32)
            o, q = torch.empty((Rs, Ds), device=DEV, dtype=dtype), torch.empty((Rs, Ds), device=DEV, dtype=dtype)
            r = rounds({"fused": lambda: ops.featproj_fwd(tab, ix, ws, bs, out=o, pre=q),
                        "composed": lambda: ops.featproj_composed(tab, ix, ws, bs, need_pre=True)}, window_ms=300.0)
            lines.append(f"  {Rs:>6} {Ws:>5} {Ds:>4} | {fmt(r['fused']):>26} | {fmt(r['composed']):>26} | {sorted(r['composed'])[1] / sorted(r['fused'])[1]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
