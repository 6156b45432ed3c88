#!/usr/bin/env python
"""The ResNet item tower on the device, fp16 --

  * the implicit-GEMM convolution (``morec_conv2d_fwd``, ``csrc/conv.hip``) against im2col + ``gemm_nt`` (``morec_im2col_nhwc`` and the
    library's GEMM; the im2col time is reported on its own too) at the 3 x 3 stride-1 shapes of ResNet-50's four stages, ``--images`` images
    of 224 px: 56 x 56 x 64, 28 x 28 x 128, 14 x 14 x 256, 7 x 7 x 512; the data gradient (``morec_conv2d_bwd_data``) at the same shapes;
  * the BatchNorm pair (``morec_bn_stats`` + ``morec_bn_merge`` + ``morec_bn_apply_fwd`` with ReLU; ``morec_bn_bwd_reduce`` +
    ``morec_bn_bwd_apply``) against the torch composition (``F.batch_norm`` + ``relu`` and their autograd; torch's native kernels, the
    vendor library switched off) on the same [rows, C] matrix;
  * the tower: forward + backward of ``Resnet_Encoder`` over ResNet-50 from decoded uint8 images, training mode.

Timing: device events around windows of ``--iters`` calls after a warm-up of every variant, ``--rounds`` windows per variant, the variants
of a group alternating window by window; reported: median and min .. max per call.

    python scripts/resnet_bench.py [--out FILE] [--images 704]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.model.encoders import Resnet_Encoder  # noqa: E402
from idvs.morec_amd.model.resnet import HipResNet, ResNetShape  # noqa: E402

DEV = "cuda"


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters      # ms per call


def alternate(variants, iters, rounds, warm=2):
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


def convs(n_img, iters, rounds, log):
    gen = torch.Generator().manual_seed(3)
    for hw, C in ((56, 64), (28, 128), (14, 256), (7, 512)):
        x = (torch.randn((n_img * hw * hw, C), generator=gen) * 0.5).to(DEV).half()
        w = (torch.randn((C, 3, 3, C), generator=gen) * 0.05).to(DEV).half()
        wt = w.permute(3, 1, 2, 0).contiguous()
        dy = (torch.randn((n_img * hw * hw, C), generator=gen) * 0.5).to(DEV).half()
        w2 = w.view(C, -1)
        t = alternate({"conv": lambda: ops.conv2d_fwd(x, w, n_img, hw, hw, 1, 1),
                       "im2col": lambda: ops.im2col_nhwc(x, n_img, hw, hw, 3, 3, 1, 1),
                       "im2col_gemm": lambda: ops.gemm_nt(ops.im2col_nhwc(x, n_img, hw, hw, 3, 3, 1, 1), w2),
                       "bwd_data": lambda: ops.conv2d_bwd_data(dy, wt, n_img, hw, hw, 1, 1)}, iters, rounds)
        flop = 2.0 * n_img * hw * hw * C * 9 * C
        med = statistics.median(t["conv"])
        log(f"3 x 3 conv, {n_img} x {hw} x {hw} x {C} -> {C}, fp16:  conv kernel {fmt(t['conv'])} ({flop / med / 1e9:6.1f} TFLOP/s)   im2col + gemm_nt "
            f"{fmt(t['im2col_gemm'])} (im2col alone {fmt(t['im2col'])})   conv / (im2col + gemm) = "
            f"{med / statistics.median(t['im2col_gemm']):.3f}   data gradient {fmt(t['bwd_data'])}")
        del x, w, wt, dy


def batchnorm(n_img, iters, rounds, log):
    gen = torch.Generator().manual_seed(5)
    torch.backends.cudnn.enabled = False
    for hw, C in ((56, 256), (14, 1024)):
        rows = n_img * hw * hw
        x = (torch.randn((rows, C), generator=gen).abs_() + 0.5).to(DEV).half()
        dy = torch.randn((rows, C), generator=gen).to(DEV).half()
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        mean, rstd, _ = ops.bn_merge(ops.bn_stats(x), 1e-5)
        y = ops.bn_apply_fwd(x, mean, rstd, gamma, beta, relu=True)

        def ours_fwd():
            m, r, _ = ops.bn_merge(ops.bn_stats(x), 1e-5, rm, rv)
            return ops.bn_apply_fwd(x, m, r, gamma, beta, relu=True)

        def ours_bwd():
            return ops.bn_bwd_apply(dy, y, x, mean, rstd, gamma, ops.bn_bwd_reduce(dy, y, x, mean, rstd))

        xl, gl, bl = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

        def torch_fwd():
            with torch.no_grad():
                return F.relu(F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5))

        def torch_fwd_bwd():
            xl.grad = gl.grad = bl.grad = None
            F.relu(F.batch_norm(xl, rm, rv, gl, bl, True, 0.1, 1e-5)).backward(dy)

        t = alternate({"fwd": ours_fwd, "bwd": ours_bwd, "torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd}, iters, rounds)
        log(f"BatchNorm + ReLU over [{rows}, {C}], fp16:  forward (stats + merge + apply) {fmt(t['fwd'])}   backward (reduce + apply) "
            f"{fmt(t['bwd'])}   torch forward {fmt(t['torch_fwd'])}   torch forward + autograd backward {fmt(t['torch_fwd_bwd'])}   "
            f"forward ours / torch = {statistics.median(t['fwd']) / statistics.median(t['torch_fwd']):.3f}")
        del x, dy, y, xl


def tower(n_img, D, rounds, log):
    enc = Resnet_Encoder(HipResNet(ResNetShape.named("resnet50"), D), compute_dtype=torch.float16).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (n_img, 224, 224, 3), generator=g, dtype=torch.uint8).to(DEV)
    d_item = (torch.randn((n_img, D), generator=g) * 1e-2).to(DEV)

    def step():
        for p in enc.parameters():
            p.grad = None
        enc.encode(images).backward(d_item.to(torch.float16))

    def forward():
        with torch.no_grad():
            enc.encode(images)

    t = alternate({"step": step, "fwd": forward}, 1, rounds, warm=1)
    log(f"ResNet-50 tower, {n_img} images of 224 px, fp16, training mode:  forward + backward {fmt(t['step'])}   forward alone "
        f"{fmt(t['fwd'])}   {n_img / statistics.median(t['step']) * 1e3:8.0f} images/s   peak memory "
        f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--images", type=int, default=704)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_bench.py measures on the device: no GPU here")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:      # written line by line: a run that is cut short keeps what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    log(f"# scripts/resnet_bench.py on {torch.cuda.get_device_name(0)}: ResNet tower kernels, median (min .. max) per call over {a.rounds} windows")
    convs(a.images, a.iters, a.rounds, log)
    batchnorm(a.images, a.iters, a.rounds, log)
    tower(a.images, a.dim, a.rounds, log)


if __name__ == "__main__":
    main()
