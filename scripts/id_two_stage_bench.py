#!/usr/bin/env python
"""``morec_featfuse_fwd`` against the composition it replaces, and the id-two-stage training step with either, fp16:

  kernels   ``ops.featfuse_fwd`` (lookup + projection + GELU + ID fusion, one launch, with the pre-activation output) against what
            ``FeatFuseFn`` runs otherwise -- the first layer as ``FeatProjFn`` picks it (``morec_featproj_fwd`` or ``indexed_rows_copy`` +
            ``gemm_nt``, automatic rule) followed by ``fuse_add_fwd`` / ``fuse_cat_fwd`` -- add and cat (p = 0.1), at the sizes of
            ``profiles/two_stage_step.txt`` (R in {1344, 5376} x 768 x 512; 21504 x 128 x 64) and at two sizes on either side of the
            rule it started from, R Kw D <= 2^29 (R in {1024, 1344 | 1536, 2048} x 768 x 512).  Device events, windows of about 0.3 s.
  step      ``IdTwoStageModel`` (item tower -> SASRec x 2 -> BCE, forward + backward + AdamW + GradScaler) at B = 128, L = 20, W = 768,
            D = 512 with the ids on the device, ``MOREC_FEATFUSE`` 1 against 2, add and cat, (mo_dnn_layers, dnn_layers) = (0, 0) and
            (4, 2) -- in the second ``FeatFuseFn`` is not on the path and the two columns time the same code: their difference is the
            noise.  Wall clock around synchronised windows of about 1 s.

Every variant is warmed up; the variants of a comparison alternate inside one process, three rounds each; median (min .. max) is printed.

    python scripts/id_two_stage_bench.py [--out profiles/id_two_stage_step.txt]

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
from idvs.morec_amd.model import IdTwoStageModel  # noqa: E402

DEV = "cuda"
SEED = 0x5EED5EED5EED


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


def rounds(variants, window_ms, wall=False, before=None):
    """{name: fn} -> {name: [three timings]}, alternating between the variants; ``before[name]()`` runs ahead of each window (a knob)."""
    before = before or {}
    reps = {}
    for name, fn in variants.items():
        before.get(name, lambda: None)()
        time_ms(fn, 10, wall)
        reps[name] = max(20, int(window_ms / max(time_ms(fn, 10, wall), 1e-3)))
    t = {name: [] for name in variants}
    for _ in range(3):
        for name, fn in variants.items():
            before.get(name, lambda: None)()
            t[name].append(time_ms(fn, reps[name], wall))
    return t


def med(v):
    return sorted(v)[1]


def fmt(v):
    return f"{med(v):8.4f} ({min(v):.4f} .. {max(v):.4f})"


def composition(table, idx, w, bias, id_table, kind, p):
    """What ``FeatFuseFn`` runs where ``featfuse_supported`` says no: the first layer as ``FeatProjFn`` picks it, then the fusion kernel."""
    if ops.featproj_supported(idx.numel(), table.shape[1], w.shape[0], table.dtype):
        y, pre = ops.featproj_fwd(table, idx, w, bias, need_pre=True)
    else:
        y, pre, _ = ops.featproj_composed(table, idx, w, bias, need_pre=True)
    out = ops.fuse_add_fwd(id_table, idx, y) if kind == "add" else ops.fuse_cat_fwd(id_table, idx, y, p, SEED)
    return out, pre


def kernel_table(items, lines):
    dtype = torch.float16
    g = torch.Generator(device=DEV).manual_seed(1)
    lines.append("featfuse_fwd against the composition it replaces (forward with the pre-activation output; cat: p = 0.1), device events, ms:")
    lines.append(f"  {'kind':>4} {'R':>6} {'W':>5} {'D':>4} {'R W D / 2^29':>12} {'first layer':>11} | {'fused':>26} | {'composition':>26} | "
                 "composition/fused | same bits")
    for Ws, Ds, Rs_all in ((768, 512, (1024, 1344, 1536, 2048, 5376)), (128, 64, (21504,))):
        tab = torch.randn(items + 1, Ws, device=DEV, generator=g).to(dtype)
        idt = torch.randn(items + 1, Ds, device=DEV, generator=g)
        ws = (torch.randn(Ds, Ws, device=DEV, generator=g) * 0.05).to(dtype)
        bs = torch.randn(Ds, device=DEV, generator=g)
        for Rs in Rs_all:
            ix = torch.randint(0, items + 1, (Rs,), device=DEV, generator=g, dtype=torch.int32)
            first = "featproj" if ops.featproj_supported(Rs, Ws, Ds, dtype) else "gather+gemm"
            for kind, p in (("add", 0.0), ("cat", 0.1)):
                o = torch.empty((Rs, Ds if kind == "add" else 2 * Ds), device=DEV, dtype=dtype)
                q = torch.empty((Rs, Ds), device=DEV, dtype=dtype)
                r = rounds({"fused": lambda: ops.featfuse_fwd(tab, ix, ws, bs, idt, kind, p, SEED, need_pre=True),      # both allocate their outputs
                            "composition": lambda: composition(tab, ix, ws, bs, idt, kind, p)}, window_ms=300.0)
                c_out, c_pre = composition(tab, ix, ws, bs, idt, kind, p)
                ops.featfuse_fwd(tab, ix, ws, bs, idt, kind, p, SEED, out=o, pre=q)
                # (gather + gemm accumulates in another order than the MFMA loop of featproj: only against featproj are the bits the same)
                same = "yes" if torch.equal(o, c_out) and torch.equal(q, c_pre) else f"no (max |diff| {float((o.float() - c_out.float()).abs().max()):.3g})"
                lines.append(f"  {kind:>4} {Rs:>6} {Ws:>5} {Ds:>4} {Rs * Ws * Ds / 2 ** 29:>12.2f} {first:>11} | {fmt(r['fused']):>26} | "
                             f"{fmt(r['composition']):>26} | {med(r['composition']) / med(r['fused']):>17.2f} | {same}")


def step_table(items, lines):
    B, L, W, D = 128, 20, 768, 512
    R = B * (L + 1) * 2
    rng = np.random.default_rng(0)
    table_host = torch.from_numpy(rng.standard_normal((items + 1, W), dtype=np.float32))
    ids = torch.from_numpy(rng.integers(1, items + 1, (B, L + 1, 2)).astype(np.int32)).to(DEV).reshape(-1)
    lm = torch.ones(B, L, device=DEV)
    lines.append(f"training step (forward + backward + AdamW + GradScaler), B = {B}, L = {L}, W = {W}, D = {D}: R = {R} item rows per step, "
                 f"R W D / 2^29 = {R * W * D / 2 ** 29:.2f}; ids on the device; wall clock per synchronised window, ms:")
    lines.append(f"  {'tower':>9} {'mo':>2} {'dnn':>3} | {'MOREC_FEATFUSE=1':>26} | {'MOREC_FEATFUSE=2':>26} | knob 1 / knob 2")
    for mo, dnn in ((0, 0), (4, 2)):
        for tower in ("modal_add", "modal_cat"):
            args = types.SimpleNamespace(max_seq_len=L, embedding_dim=D, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                         dnn_layers=dnn, mo_dnn_layers=mo, word_embedding_dim=W, item_tower=tower, compute_dtype="fp16")
            torch.manual_seed(0)
            model = IdTwoStageModel(args, items, True).to(DEV).train()
            model.set_feature_table(table_host)
            opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
            scaler = torch.amp.GradScaler("cuda", enabled=True)

            def step():
                opt.zero_grad()
                loss = model(ids, None, lm, DEV)
                scaler.scale(loss).backward()
                scaler.step(opt)
                scaler.update()

            t = rounds({"1": step, "2": step}, window_ms=1000.0, wall=True,
                       before={"1": lambda: ops.set_featfuse(1), "2": lambda: ops.set_featfuse(2)})
            ops.set_featfuse(0)
            lines.append(f"  {tower:>9} {mo:>2} {dnn:>3} | {fmt(t['1']):>26} | {fmt(t['2']):>26} | {med(t['1']) / med(t['2']):.2f}")
            del model, opt, scaler


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "id_two_stage_step.txt"))
    ap.add_argument("--items", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("id_two_stage_bench: no GPU")
    lines = [f"Two-stage ID (+) modality fusion: morec_featfuse_fwd and the training step, fp16, {torch.cuda.get_device_name(0)}",
             "ms: median of three rounds (min .. max); the variants of a row alternate inside one process"]
    kernel_table(a.items, lines)
    step_table(a.items, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
