#!/usr/bin/env python
"""The BEiT item tower on the device, ViT-B/16, 704 images of 224 px (T = 197 tokens), fp16 --

  * attention with the relative-position bias, forward and backward (``morec_attn_bias_fwd`` / ``_bwd``, the bias gradient included),
    against the no-bias streaming kernels at the same shape (``attn_stream`` = 2; ``MOREC_ATTN_STREAM=2`` in the environment) and against
    the torch composition it replaces: ``matmul`` + add + ``softmax`` + ``matmul`` and their autograd;
  * the bias-gradient pass on its own: the backward with ``d_pos_bias`` minus the backward without it (a frozen table launches nothing);
  * the tower: forward + backward of ``Vit_Encoder`` over the BEiT container from decoded uint8 images, training mode (DropPath drawn).

Timing: device events around windows of ``--iters`` calls after a warm-up of every variant, ``--rounds`` windows per variant, the variants
of a group alternating window by window; reported: median and min .. max per call.

    python scripts/beit_bench.py [--out FILE] [--images 704]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import _lib, ops  # noqa: E402
from idvs.morec_amd.beit_engine import BeitShape  # noqa: E402
from idvs.morec_amd.model.beit import HipBeitForImageClassification  # noqa: E402
from idvs.morec_amd.model.encoders import Vit_Encoder  # noqa: E402

DEV = "cuda"


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters      # ms per call


def alternate(variants, iters, rounds, warm=3):
    """{name: fn} -> {name: [ms per call, one per window]}; the windows of the variants alternate."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(window(fn, iters))
    return t


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def knob(v):
    ops.check(_lib.lib().morec_tuning_set(b"attn_stream", v), "morec_tuning_set(attn_stream)")


def attention(n_img, iters, rounds, log):
    shape = BeitShape.named("beit_base")
    heads, C, g = shape.num_attention_heads, shape.hidden_size, shape.grid
    T, dh = g * g + 1, C // heads
    gen = torch.Generator().manual_seed(3)
    qkv = (torch.randn((n_img * T, 3 * C), generator=gen) * 0.7).to(DEV).half()
    dctx = torch.randn((n_img * T, C), generator=gen).to(DEV).half()
    keep = torch.ones((n_img, T), device=DEV)
    table = (torch.randn((shape.num_relative_distance, heads), generator=gen) * 0.5).to(DEV)
    pb = ops.beit_bias_expand(table, g)
    desc = ops.attn_desc(n_img, T, heads, dh, False, dh ** -0.5, ops.FLT_MIN_MASK, torch.float16)
    knob(2)
    try:
        fwd = alternate({"bias": lambda: ops.attn_bias_fwd(desc, qkv, keep, pb), "plain": lambda: ops.attn_fwd(desc, qkv, keep)},
                        iters, rounds)
        bwd = alternate({"bias": lambda: ops.attn_bias_bwd(desc, qkv, keep, pb, dctx),
                         "frozen": lambda: ops.attn_bias_bwd(desc, qkv, keep, pb, dctx, need_dpos=False),
                         "plain": lambda: ops.attn_bwd(desc, qkv, keep, dctx)}, iters, rounds)
    finally:
        knob(0)
    log(f"attention forward, {n_img} x {heads} heads, T = {T}, dh = {dh}, fp16:  with bias {fmt(fwd['bias'])}   no-bias streaming kernels "
        f"{fmt(fwd['plain'])}   bias / plain = {statistics.median(fwd['bias']) / statistics.median(fwd['plain']):.3f}")
    log(f"attention backward, same shape:  with bias + d_pos_bias {fmt(bwd['bias'])}   with bias, frozen table {fmt(bwd['frozen'])}   "
        f"no-bias streaming kernels {fmt(bwd['plain'])}   frozen / plain = {statistics.median(bwd['frozen']) / statistics.median(bwd['plain']):.3f}")
    dpos = [a - b for a, b in zip(bwd["bias"], bwd["frozen"])]
    share = statistics.median(dpos) / statistics.median(bwd["frozen"])
    log(f"d_pos_bias pass (statistics out, tile sums over the sequences, chunk fold; backward with - without it, window by window): "
        f"{fmt(dpos)}   = {share:.3f} of the attention backward")

    # the torch composition: [n, heads, T, T] scores in memory, autograd for the backward
    q, k, v = (qkv[:, i * C:(i + 1) * C].view(n_img, T, heads, dh).transpose(1, 2).contiguous() for i in range(3))
    bias16 = pb[:, :, :T].half().contiguous()
    do = dctx.view(n_img, T, heads, dh).transpose(1, 2).contiguous()

    def torch_fwd():
        return torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * dh ** -0.5 + bias16, -1, dtype=torch.float32).half() @ v

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, bias16)]

    def torch_fwd_bwd():
        for t in leaves:
            t.grad = None
        ql, kl, vl, bl = leaves
        o = torch.softmax(torch.matmul(ql, kl.transpose(-1, -2)) * dh ** -0.5 + bl, -1, dtype=torch.float32).half() @ vl
        o.backward(do)

    tt = alternate({"fwd": torch_fwd, "fwd_bwd": torch_fwd_bwd}, max(1, iters // 4), rounds)
    log(f"torch composition (matmul + add + softmax + matmul), same shape:  forward {fmt(tt['fwd'])}   forward + autograd backward "
        f"{fmt(tt['fwd_bwd'])}   against {statistics.median(fwd['bias']):.3f} + {statistics.median(bwd['bias']):.3f} ms here")
    return share


def tower(n_img, D, iters, rounds, log):
    shape = BeitShape.named("beit_base")
    enc = Vit_Encoder(HipBeitForImageClassification(shape, D), compute_dtype=torch.float16).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (n_img, 224, 224, 3), generator=g, dtype=torch.uint8).to(DEV)
    d_item = (torch.randn((n_img, D), generator=g) * 1e-2).to(DEV).half()

    def step():
        for p in enc.parameters():
            p.grad = None
        enc.encode(images).backward(d_item)

    def forward():
        with torch.no_grad():
            enc.encode(images)

    t = alternate({"step": step, "fwd": forward}, max(1, iters // 3), rounds, warm=2)
    log(f"tower, {n_img} images (T = {shape.num_patches + 1}), fp16, training mode:  forward + backward {fmt(t['step'])}   forward alone "
        f"{fmt(t['fwd'])}   {n_img / statistics.median(t['step']) * 1e3:8.0f} images/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=704)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beit_bench.py measures on the device: no GPU here")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# scripts/beit_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16 BEiT tower, median (min .. max) per call over {a.rounds} windows")
    attention(a.images, a.iters * 20, a.rounds, log)      # sub-millisecond calls: windows of a tenth of a second and more
    tower(a.images, a.dim, a.iters, a.rounds, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
