#!/usr/bin/env python
"""Capture golden vectors for the ResNet item tower from the imported reference.

Run once in the build container:   python tests/golden/make_golden_resnet.py

Imports the ``model`` packages of ``/root/reference/inbatch_sasrec_e2e_vision`` and ``/root/reference/bce_vision/main-end2end`` unmodified
(CPU) and wraps their ``Resnet_Encoder`` / ``Model`` around the plain-torch ResNet of ``tests/resnet_ref.py`` (torchvision is not
installed here; the reference's classes take the backbone as an object), with ``.fc`` replaced by ``Linear(num_fc_ftr, embedding_dim)``
as ``V/run.py:42-46`` does.  Weights, buffers and pixels come from ``utils/detgen`` (``resnet_ref.load_det``), so ``g32_resnet.npz`` holds
RESULTS only: for ``resnet_micro`` (BasicBlock) and ``resnet_micro_b`` (Bottleneck), at 6 images of 64 x 64 of which image 0 is the
all-zero image of a padding item,

  <net>.y / .y_eval                        training-mode and evaluation-mode (the initial running statistics) encoder output
  <net>.grad_keys / .grad64 / .grad_stats  every gradient of sum(y * R) (``keep_grads``: a committed file is capped at 1 MiB, so of a large
                                           tensor the fixture keeps 128 elements at detgen-drawn indices, the norm and the largest magnitude)
  <net>.running_keys / .running64 / ...    the running statistics after that one training forward
  <net>.inbatch.loss / .grad_keys ...      the in-batch ``Model`` (B = 2, S = 2: 6 images), training mode
  <net>.bce.loss / .grad_keys ...          the BCE ``Model`` (B = 1, S = 2: 3 positive / negative pairs), training mode

The values are the fp64 run's; next to each the fixture keeps the fp32 run's own error against it (``y`` beside ``y64``, ``grad_err``,
``running_err``): the yardstick of the fp32 reference's own rounding error.  The same errors of the reference run in bf16 and in fp16
(module and inputs cast as a whole, on the CPU) are kept as ``..._err_bf16`` / ``..._err_fp16``: the yardstick of 16-bit storage.  ``g32_resnet_keys.json`` holds the
``state_dict`` key list and the parameter order of the five real depths and the two test nets, written from ``tests/resnet_ref.py``; the
parameter counts are checked against torchvision's (62 / 110 / 161 / 314 / 467).
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resnet_ref  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal  # noqa: E402

torch.set_num_threads(8)


def ref_package(path):
    """The reference package ``model`` under ``path`` (two packages share the name: the cached modules are dropped first)."""
    for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
        del sys.modules[k]
    sys.path.insert(0, path)
    try:
        return importlib.import_module("model"), importlib.import_module("model.encoders")
    finally:
        sys.path.remove(path)


N_IMG, R0, D = 6, 64, 48
TORCHVISION_COUNTS = {"resnet18": 62, "resnet34": 110, "resnet50": 161, "resnet101": 314, "resnet152": 467}


def pixels():
    x = det_normal("g32.x", (N_IMG, 3, R0, R0), std=1.0)
    x[0] = 0.0      # the image of a padding item (V/data_utils/dataset.py: torch.zeros)
    return torch.from_numpy(x)


def backbone(name):
    net = resnet_ref.build(name)
    net.fc = torch.nn.Linear(net.fc.in_features, D)      # V/run.py:42-46
    return net


def grads_of(module):
    return {k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None}


LOW = (("bf16", torch.bfloat16), ("fp16", torch.float16))      # the reference's own 16-bit runs: module and inputs cast as a whole


def keep_grads(res, base, g32_, g64_, low=()):
    """Per gradient, in the order of ``<base>.grad_keys``: the fp64 values at ``resnet_ref.sample_idx`` (every element of a small tensor;
    concatenated in ``<base>.grad64``) and a row of ``<base>.grad_stats`` = the fp64 norm and largest magnitude of the whole tensor, then
    the reference's own error -- the largest |run - fp64| over the WHOLE tensor -- for its fp32, bf16 and fp16 runs."""
    keys, vals, stats = list(g64_), [], []
    for k in keys:
        flat = g64_[k].reshape(-1).numpy()
        vals.append(flat[resnet_ref.sample_idx(k, flat.size)])
        errs = [np.abs(g[k].reshape(-1).double().numpy() - flat).max() for g in [g32_] + [gl for _, gl in low]]
        stats.append([np.linalg.norm(flat), np.abs(flat).max()] + errs)
    res[f"{base}.grad_keys"] = np.array(keys)
    res[f"{base}.grad64"] = np.concatenate(vals)
    res[f"{base}.grad_stats"] = np.array(stats, dtype=np.float64)


def encoder_run(name, enc_cls, dtype):
    wrap = torch.nn.Module()
    wrap.cv_encoder = enc_cls(backbone(name))
    resnet_ref.load_det(wrap)
    wrap.to(dtype)
    x, Rm = pixels().to(dtype), torch.from_numpy(det_normal("g32.R", (N_IMG, D), std=1.0)).to(dtype)
    wrap.eval()
    with torch.no_grad():
        y_eval = wrap.cv_encoder(x)
    wrap.train()
    y = wrap.cv_encoder(x)
    (y * Rm).sum().backward()
    bufs = {k: b.detach().clone() for k, b in wrap.named_buffers() if b.dtype.is_floating_point}
    return y.detach(), y_eval, grads_of(wrap), bufs


def encoder_case(res, tag, name, enc_cls):
    y, y_eval, g, bufs = encoder_run(name, enc_cls, torch.float32)
    y64, y_eval64, g64_, bufs64 = encoder_run(name, enc_cls, torch.float64)
    res[f"{tag}.y"], res[f"{tag}.y64"], res[f"{tag}.y_eval"], res[f"{tag}.y_eval64"] = y.numpy(), y64.numpy(), y_eval.numpy(), y_eval64.numpy()
    low = [(t, encoder_run(name, enc_cls, dt)) for t, dt in LOW]
    keep_grads(res, tag, g, g64_, [(t, r[2]) for t, r in low])
    for t, r in low:
        res[f"{tag}.y_err_{t}"] = np.float64((r[0].double() - y64).abs().max())
        res[f"{tag}.y_eval_err_{t}"] = np.float64((r[1].double() - y_eval64).abs().max())
    keys = list(bufs64)
    res[f"{tag}.running_keys"] = np.array(keys)
    res[f"{tag}.running64"] = np.concatenate([bufs64[k].numpy() for k in keys])
    res[f"{tag}.running_stats"] = np.array([[float((r[k].double() - bufs64[k]).abs().max()) for r in [bufs] + [r[3] for _, r in low]]
                                            for k in keys], dtype=np.float64)
    return y, y64


def model_run(res, tag, name, kind, model_cls, dtype):
    S = 2
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load=name)
    x = pixels().to(dtype)
    item_num = 8
    if kind == "inbatch":
        ids = np.array([[0, 3, 5], [2, 7, 4]], dtype=np.int64)      # B = 2, S = 2; row 0 starts with a padding item: image 0, all zero
        log_mask = (ids[:, :-1] != 0).astype(np.float32)
        pop = np.abs(det_normal("g32.pop", (item_num + 1,), std=1.0)) + 0.05
        pop = (pop / pop.sum()).astype(np.float32)
        m = model_cls(args, item_num, True, backbone(name), pop.tolist())
        res[f"{tag}.inbatch.ids"], res[f"{tag}.inbatch.log_mask"], res[f"{tag}.inbatch.pop"] = ids, log_mask, pop
    else:
        log_mask = np.array([[0.0, 1.0]], dtype=np.float32)         # B = 1, S = 2: (positive, negative) x 3 slots; slot 0 is padding
        m = model_cls(args, item_num, True, backbone(name))
        res[f"{tag}.bce.log_mask"] = log_mask
    resnet_ref.load_det(m)
    if dtype in (torch.bfloat16, torch.float16):      # the reference's sequence model does not run in a 16-bit type on the CPU: the item
        m.cv_encoder.to(dtype)                         # tower alone is cast, its output handed on in fp32
        m.cv_encoder.register_forward_hook(lambda mod, inp, out: out.float())
        dtype = torch.float32
    else:
        m.to(dtype)
    m.train()
    if kind == "inbatch":
        loss = m(torch.from_numpy(ids).view(-1), x, torch.from_numpy(log_mask).to(dtype), "cpu")
    else:
        loss = m(x, torch.from_numpy(log_mask).to(dtype), "cpu")
    loss.backward()
    return float(loss.detach()), grads_of(m)


def model_case(res, tag, name, kind, model_cls):
    l32, g = model_run(res, tag, name, kind, model_cls, torch.float32)
    l64, g64_ = model_run(res, tag, name, kind, model_cls, torch.float64)
    res[f"{tag}.{kind}.loss"], res[f"{tag}.{kind}.loss64"] = np.float32(l32), np.float64(l64)
    low = [(t, model_run(res, tag, name, kind, model_cls, dt)) for t, dt in LOW]
    keep_grads(res, f"{tag}.{kind}", g, g64_, [(t, r[1]) for t, r in low])
    for t, r in low:
        res[f"{tag}.{kind}.loss_err_{t}"] = np.float64(abs(r[0] - l64))
    return l32, l64


def g32(out):
    ib_model, ib_enc = ref_package("/root/reference/inbatch_sasrec_e2e_vision")
    InbatchModel, RefResnetEncoder = ib_model.Model, ib_enc.Resnet_Encoder
    bce_model, _ = ref_package("/root/reference/bce_vision/main-end2end")
    BceModel = bce_model.Model
    res = {"cfg": np.array([N_IMG, R0, D])}
    for name in ("resnet_micro", "resnet_micro_b"):
        y, y64 = encoder_case(res, name, name, RefResnetEncoder)
        print("g32", name, "y norm", float(y.norm()), "fp32 vs fp64", float((y.double() - y64).abs().max()))
        for kind, cls in (("inbatch", InbatchModel), ("bce", BceModel)):
            print("g32", name, kind, "loss fp32 / fp64", *model_case(res, name, name, kind, cls))
    np.savez_compressed(os.path.join(out, "g32_resnet.npz"), **res)

    keys = {}
    for name in list(TORCHVISION_COUNTS) + ["resnet_micro", "resnet_micro_b"]:
        net = resnet_ref.build(name)
        keys[name] = dict(state_dict=[[k, list(v.shape)] for k, v in net.state_dict().items()],
                          named_parameters=[k for k, _ in net.named_parameters()])
        if name in TORCHVISION_COUNTS:
            assert len(keys[name]["named_parameters"]) == TORCHVISION_COUNTS[name], (name, len(keys[name]["named_parameters"]))
    with open(os.path.join(out, "g32_resnet_keys.json"), "w") as f:
        json.dump(keys, f)
    print("g32 keys", {k: len(v["named_parameters"]) for k, v in keys.items()})


if __name__ == "__main__":
    g32(HERE)
