#!/usr/bin/env python
"""The MAE (ViT) item tower on the device: forward + backward of ``MAE_Encoder`` at ViT-B/16, 704 images of 224 px (the Swin line's image
count), fp16, decoded uint8 images as the driver feeds them --

  * mask ratio 0.75 (T = 50 tokens per image: the matrix-core attention kernels) and mask ratio 0 (T = 197), each with the attention rule
    at its default (``attn_stream`` = 0: 64 < T <= 256 runs on the row-strip kernels) and at ``attn_stream`` = 2 (the streaming kernels
    from T = 65 on; ``MOREC_ATTN_STREAM=2`` in the environment);
  * the front of the tower alone -- ``mae_keep_ids`` + ``mae_patchify_keep`` + the patch GEMM over the kept rows + ``mae_assemble_fwd`` --
    against the composition it replaces: ``torch.rand`` + ``argsort``, the full ``swin_patchify_u8``, the full patch GEMM, the position add,
    ``torch.gather`` and ``torch.cat`` (HF's ``ViTMAEEmbeddings.forward``).

Timing: device events around windows of ``--iters`` calls after a warm-up of every shape, ``--rounds`` windows per variant, the variants of a
pair alternating window by window; reported: median and min .. max per call.

    python scripts/mae_bench.py [--out FILE] [--images 704]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import _lib, ops  # noqa: E402
from idvs.morec_amd.mae_engine import MaeShape  # noqa: E402
from idvs.morec_amd.model.encoders import MAE_Encoder  # noqa: E402
from idvs.morec_amd.model.mae import HipViTMAEModel  # noqa: E402

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


def tower(n_img, D, iters, rounds, log):
    shape = MaeShape.named("mae_base")
    enc = MAE_Encoder(HipViTMAEModel(shape), D, compute_dtype=torch.float16).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (n_img, 224, 224, 3), generator=g, dtype=torch.uint8).to(DEV)
    d_item = (torch.randn((n_img, D), generator=g) * 1e-2).to(DEV).half()

    def step():
        for p in enc.parameters():
            p.grad = None
        enc.encode(images).backward(d_item)

    for ratio in (0.75, 0.0):
        enc.image_net.config.mask_ratio = ratio
        T = shape.len_keep(ratio) + 1
        res = {}
        for v in (0, 2):
            knob(v)
            try:
                res[v] = alternate({"step": step}, iters if ratio > 0 else max(1, iters // 3), rounds)["step"]
            finally:
                knob(0)
        log(f"tower fwd + bwd, {n_img} images, mask ratio {ratio:4.2f} (T = {T:3d}), fp16:  attn_stream = 0 {fmt(res[0])}   "
            f"attn_stream = 2 {fmt(res[2])}   {n_img / statistics.median(res[0]) * 1e3:8.0f} | {n_img / statistics.median(res[2]) * 1e3:8.0f} images/s")


def front(n_img, iters, rounds, log):
    shape = MaeShape.named("mae_base")
    N, C, P = shape.num_patches, shape.hidden_size, shape.patch_size
    L = shape.len_keep()
    g = torch.Generator().manual_seed(2)
    images = torch.randint(0, 256, (n_img, 224, 224, 3), generator=g, dtype=torch.uint8).to(DEV)
    w = (torch.randn((C, 3 * P * P), generator=g) * 0.02).to(DEV).half()
    bias = torch.zeros(C, device=DEV)
    cls = torch.randn(C, generator=g).to(DEV)
    pos = torch.randn((N + 1, C), generator=g).to(DEV)
    pos16 = pos.half()

    def kept_only():
        keep = ops.mae_keep_ids(n_img, N, L, seed=7, device=DEV)
        e = ops.gemm_nt(ops.mae_patchify_keep(images, keep, P, torch.float16), w, bias=bias)
        return ops.mae_assemble_fwd(e, cls, pos, keep)

    def composed():
        ids = torch.argsort(torch.rand((n_img, N), device=DEV), dim=1)[:, :L]
        e = ops.gemm_nt(ops.swin_patchify_u8(images, P, torch.float16), w, bias=bias).view(n_img, N, C) + pos16[1:]
        e = torch.gather(e, 1, ids.unsqueeze(-1).expand(-1, -1, C))
        return torch.cat(((cls.half() + pos16[0]).expand(n_img, 1, C), e), dim=1)

    assert kept_only().shape[0] == composed().shape[0] * composed().shape[1]
    t = alternate({"kept": kept_only, "composed": composed}, iters * 4, rounds)
    log(f"front of the tower, {n_img} images, mask ratio 0.75, fp16:  kept patches only {fmt(t['kept'])}   full im2col + full GEMM + gather + cat "
        f"{fmt(t['composed'])}   composed / kept-only = {statistics.median(t['composed']) / statistics.median(t['kept']):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=704)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mae_bench.py measures on the device: no GPU here")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"# scripts/mae_bench.py on {torch.cuda.get_device_name(0)}: ViT-B/16 MAE tower, median (min .. max) per call over {a.rounds} windows")
    front(a.images, a.iters, a.rounds, log)
    tower(a.images, a.dim, a.iters, a.rounds, log)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
