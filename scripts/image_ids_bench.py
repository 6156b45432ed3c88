"""What ``--images_on_device`` (the image catalogue on the device, a batch as its item ids) changes at the bench shape: fp16, 224 px,
704 images per step (64 sequences x 11 slots) out of a 20 000-image synthetic catalogue.  Needs a GPU; fails without one.

    python scripts/image_ids_bench.py [--out profiles/image_ids.txt] [--rounds 5] [--skip swin,mae,resnet]

(a) the input side alone, per front kernel: host gather of the batch's images into a page-locked buffer + H2D + the front kernel's direct form, against
    H2D of the int32 ids + its indexed form (the same kernel reading the catalogue through the ids);
(b) a whole autograd step (forward + backward of the tower, AdamW left out) of the MAE-base and ResNet-50 towers, and the fused Swin-T
    step (``TrainStep``; the host side goes through ``DeviceImageFeed`` one batch ahead, as the driver does), with the batch as gathered
    pixels and as ids.  The "pixels" side is the baseline: it runs only kernels and Python paths that the flag leaves as they were;
(c) the one-off upload of the catalogue and the bytes it holds.
Each figure: the two sides alternate round by round in one process, every round ends in a device synchronise under a host clock; median
and range over the rounds are reported."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.data_utils.images import DeviceImageCatalogue, DeviceImageFeed  # noqa: E402

DEV = "cuda"
DT = torch.float16
R, N_ITEMS, B, S = 224, 20000, 64, 10
N_IMG = B * (S + 1)


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def ab(sides: dict, rounds, steps, warmup=2):
    """{name: fn(step index)} -> {name: [ms per step, one per round]}; the sides alternate within every round."""
    for fn in sides.values():
        timed(fn, warmup)
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(timed(fn, steps))
    return out


def fmt(v):
    return f"{statistics.median(v):9.3f} ms  (range {min(v):.3f} .. {max(v):.3f})"


def report(lines, title, res):
    lines.append(title)
    for k, v in res.items():
        lines.append(f"    {k:<28} {fmt(v)}")
    ks = list(res)
    if len(ks) == 2:
        lines.append(f"    {'median ' + ks[0] + ' / ' + ks[1]:<28} {statistics.median(res[ks[0]]) / statistics.median(res[ks[1]]):9.2f} x")
    print("\n".join(lines[-(len(res) + 2):]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/image_ids.txt")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--items", type=int, default=N_ITEMS)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_ids_bench.py measures on a GPU; none is visible")
    skip = set(a.skip.split(","))
    lines = [f"image_ids_bench: {torch.cuda.get_device_name(0)}, fp16, {R} px, {N_IMG} images per step, catalogue of {a.items} + 1 images, "
             f"{a.rounds} rounds x {a.steps} steps", ""]

    rng = np.random.default_rng(4321)
    host = rng.integers(0, 256, (a.items + 1, R, R, 3), dtype=np.uint8)
    batches = [rng.integers(1, a.items + 1, N_IMG) for _ in range(16)]
    stage = torch.empty((N_IMG, R, R, 3), dtype=torch.uint8).pin_memory()
    stage_np = stage.numpy()

    # (c)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cat = DeviceImageCatalogue(host, DEV)
    torch.cuda.synchronize()
    lines += [f"(c) catalogue upload: {time.perf_counter() - t0:.2f} s for {cat.nbytes / 2**30:.2f} GiB held on the device ({cat.n_chunks} chunks)", ""]
    print(lines[-2], flush=True)

    def gathered(k):
        """the host path: fancy-index gather into the page-locked buffer, one asynchronous H2D"""
        np.take(host, batches[k % 16], axis=0, out=stage_np)
        return stage.to(DEV, non_blocking=True)

    def as_ids(k):
        return cat.batch(batches[k % 16])

    def sides(px_fn, ids_fn):
        return {"gathered pixels": px_fn, "item ids": ids_fn}

    # (a)
    keep = ops.mae_keep_ids(N_IMG, 196, 49, seed=7, device=DEV)
    report(lines, "(a) input side, Swin / BEiT front (patch 4): gather + H2D + swin_patchify_u8  |  ids H2D + swin_patchify_u8(ids=)",
           ab(sides(lambda k: ops.swin_patchify_u8(gathered(k), 4, DT), lambda k: ops.swin_patchify_u8(cat.data, 4, DT, ids=as_ids(k).ids)),
              a.rounds, a.steps))
    report(lines, "(a) input side, MAE front (patch 16, 49 of 196 kept): gather + H2D + mae_patchify_keep  |  ids H2D + mae_patchify_keep(ids=)",
           ab(sides(lambda k: ops.mae_patchify_keep(gathered(k), keep, 16, DT),
                    lambda k: ops.mae_patchify_keep(cat.data, keep, 16, DT, ids=as_ids(k).ids)), a.rounds, a.steps))
    report(lines, "(a) input side, ResNet front: gather + H2D + pixels_to_nhwc  |  ids H2D + pixels_to_nhwc(ids=)",
           ab(sides(lambda k: ops.pixels_to_nhwc(gathered(k), DT), lambda k: ops.pixels_to_nhwc(cat.data, DT, ids=as_ids(k).ids)),
              a.rounds, a.steps))
    # the kernels alone, inputs resident: direct | indexed form of one kernel
    px0 = gathered(0)
    i0 = as_ids(0).ids
    report(lines, "    kernel alone, Swin front (pixels resident): direct | indexed",
           ab({"direct": lambda k: ops.swin_patchify_u8(px0, 4, DT), "indexed": lambda k: ops.swin_patchify_u8(cat.data, 4, DT, ids=i0)},
              a.rounds, 50))
    report(lines, "    kernel alone, MAE front: direct | indexed", ab({"direct": lambda k: ops.mae_patchify_keep(px0, keep, 16, DT),
                                                     "indexed": lambda k: ops.mae_patchify_keep(cat.data, keep, 16, DT, ids=i0)}, a.rounds, 50))
    report(lines, "    kernel alone, ResNet front: direct | indexed", ab({"direct": lambda k: ops.pixels_to_nhwc(px0, DT),
                                                        "indexed": lambda k: ops.pixels_to_nhwc(cat.data, DT, ids=i0)}, a.rounds, 50))
    del px0
    lines.append("")

    # (b) autograd towers
    def tower_step(enc):
        def step(x):
            enc.zero_grad(set_to_none=True)
            out = enc.encode(x)
            out.float().sum().backward()
        return step

    if "mae" not in skip:
        from idvs.morec_amd.mae_engine import MaeShape
        from idvs.morec_amd.model import MAE_Encoder
        from idvs.morec_amd.model.mae import HipViTMAEModel
        torch.manual_seed(1)
        enc = MAE_Encoder(HipViTMAEModel(MaeShape.named("mae_base")), 512, compute_dtype=DT).to(DEV).train()
        st = tower_step(enc)
        report(lines, "(b) MAE-base tower, autograd step (forward + backward), input side serial with the step",
               ab(sides(lambda k: st(gathered(k)), lambda k: st(as_ids(k))), a.rounds, a.steps))
        del enc, st
        torch.cuda.empty_cache()
    if "resnet" not in skip:
        from idvs.morec_amd.model.encoders import Resnet_Encoder
        from idvs.morec_amd.model.resnet import HipResNet, ResNetShape
        torch.manual_seed(1)
        enc = Resnet_Encoder(HipResNet(ResNetShape.named("resnet50"), 512), compute_dtype=DT).to(DEV).train()
        st = tower_step(enc)
        report(lines, "(b) ResNet-50 tower, autograd step (forward + backward), input side serial with the step",
               ab(sides(lambda k: st(gathered(k)), lambda k: st(as_ids(k))), a.rounds, max(2, a.steps // 2)))
        del enc, st
        torch.cuda.empty_cache()
    if "swin" not in skip:
        from idvs.morec_amd.model import Model
        from idvs.morec_amd.model.swin import HipSwinForImageClassification
        from idvs.morec_amd.swin_engine import SwinShape
        from idvs.morec_amd.train_step import TrainStep
        shape = SwinShape.named("swin_tiny")
        args = types.SimpleNamespace(max_seq_len=S, embedding_dim=2048, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                                     CV_model_load="swin_tiny", compute_dtype="fp16")
        pop = np.full(a.items + 1, 1.0 / a.items)
        pop[0] = 1.0
        torch.manual_seed(1)
        model = Model(args, a.items, True, HipSwinForImageClassification(shape, 2048), pop).to(DEV).train()
        ts = TrainStep(model, lr=1e-4, fine_tune_lr=5e-5, l2_weight=0.01, fine_tune_l2_weight=0.01)
        feed = DeviceImageFeed(DEV, R, shape.patch_size, ts.dtype)
        lm = torch.ones(B, S, device=DEV)
        ids_dev = [torch.from_numpy(b).to(DEV) for b in batches]
        stages = [torch.empty((N_IMG, R, R, 3), dtype=torch.uint8).pin_memory() for _ in range(3)]
        ahead = {}

        def submit(k):
            buf = stages[k % 3]
            np.take(host, batches[k % 16], axis=0, out=buf.numpy())
            return feed.submit(buf, None, None)

        def fused_pixels(k):      # the driver's loop: batch k + 1 is gathered and queued on the feed's stream before step k's launches
            slot = ahead.pop(k, None) or submit(k)
            ahead[k + 1] = submit(k + 1)
            ts.step(ids_dev[k % 16], feed.take(slot), lm)
            feed.release(slot)

        def fused_pixels_round(k):
            if k == 0:
                ahead.clear()
            fused_pixels(k)

        report(lines, "(b) fused Swin-T step (TrainStep, D = 2048): DeviceImageFeed one batch ahead  |  ImageIds",
               ab(sides(fused_pixels_round, lambda k: ts.step(ids_dev[k % 16], as_ids(k), lm)), a.rounds, a.steps))
        ts.close()
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"written to {a.out}")


if __name__ == "__main__":
    main()
