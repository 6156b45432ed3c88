#!/usr/bin/env python
"""Capture golden vectors for the BEiT item tower from the imported reference.

Run once in the build container:   python tests/golden/make_golden_beit.py

Imports ``/root/reference/inbatch_sasrec_e2e_vision``'s ``model`` package unmodified (CPU, fp32) together with the installed HuggingFace
``BeitForImageClassification`` (``attn_implementation="eager"``; the third-party class the reference hands to its ``Vit_Encoder``, with
``.classifier`` replaced by ``Linear(hidden, embedding_dim)`` as ``V/run.py:47-54`` does), feeds deterministic synthetic pixels / weights
(``det_param`` into EVERY parameter: the layer scales and the relative-position tables included) and writes ``g28_beit.npz`` +
``g28_beit_keys.json`` next to this file: numeric OUTPUTS and inputs that cannot be regenerated only.  Nothing of the reference or of HF
is stored.

Every encoder case also stores the same module's fp64 run (``*.y64``, ``*.grad_norm64.*``, ``*.grad64.*``): the yardstick for the fp32
reference's own rounding error, from which a test may derive a bound where one of g11's does not hold.  ``rel_index.<g>`` is HF's
``BeitRelativePositionBias.generate_relative_position_index`` for g = 4, 7, 8, 14 (int16), for the CPU test of the host's index function.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/inbatch_sasrec_e2e_vision")

from idvs.morec_amd.utils.detgen import det_normal, det_param  # noqa: E402

from model import Model as RefModel  # noqa: E402  (reference package)
from model.encoders import Vit_Encoder as RefVitEncoder  # noqa: E402
from transformers import BeitConfig, BeitForImageClassification  # noqa: E402
from transformers.models.beit.modeling_beit import BeitRelativePositionBias  # noqa: E402

torch.set_num_threads(8)

MICRO = dict(patch_size=4, num_channels=3, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, use_relative_position_bias=True, use_mean_pooling=True,
             layer_scale_init_value=0.1, drop_path_rate=0.1)


def load_det(module, seed=12345):
    sd = module.state_dict()
    new = {k: torch.from_numpy(det_param(k, tuple(v.shape), seed=seed)) for k, v in sd.items() if v.dtype.is_floating_point}
    module.load_state_dict(new, strict=False)
    return module


def build_beit(image_size, D):
    cfg = BeitConfig(attn_implementation="eager", image_size=image_size, **MICRO)
    net = BeitForImageClassification(cfg)
    net.classifier = torch.nn.Linear(MICRO["hidden_size"], D)       # V/run.py:47-54
    return net


def run_case(wrap, enc, x, Rm, dtype):
    wrap.to(dtype)
    wrap.zero_grad()
    y = enc(x.to(dtype))
    (y * Rm.to(dtype)).sum().backward()
    named = dict(wrap.named_parameters())
    return y.detach(), {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}


def g28(out):
    res = {}
    N_IMG, D = 3, 48
    for g in (4, 7, 8, 14):
        idx = BeitRelativePositionBias.generate_relative_position_index((g, g))
        assert int(idx.max()) < 2 ** 15
        res[f"rel_index.{g}"] = idx.numpy().astype(np.int16)
    for tag, R0 in [("b17", 16), ("b50", 28), ("b65", 32)]:
        net = build_beit(R0, D)
        enc = RefVitEncoder(net)
        wrap = torch.nn.Module()
        wrap.cv_encoder = enc                       # keys get the reference's ``cv_encoder.`` prefix
        load_det(wrap)
        wrap.eval()
        x = torch.from_numpy(det_normal(f"g28{tag}.x", (N_IMG, 3, R0, R0), std=1.0))
        Rm = torch.from_numpy(det_normal(f"g28{tag}.R", (N_IMG, D), std=1.0))
        y, grads = run_case(wrap, enc, x, Rm, torch.float32)
        res[f"{tag}.cfg"] = np.array([R0, 4, MICRO["hidden_size"], MICRO["num_hidden_layers"], MICRO["num_attention_heads"],
                                      MICRO["intermediate_size"], N_IMG, D])
        res[f"{tag}.y"] = y.numpy()
        pre = "cv_encoder.image_net."
        L0 = pre + "beit.layers.0."
        full = [L0 + "relative_position_bias.relative_position_bias_table", L0 + "lambda_1", L0 + "attention.q_proj.bias",
                pre + "beit.embeddings.cls_token", pre + "beit.embeddings.patch_embeddings.projection.weight", pre + "classifier.weight"]
        for k, gr in grads.items():
            res[f"{tag}.grad_norm.{k}"] = np.float64(gr.double().norm().item())
        for k in full:
            res[f"{tag}.grad.{k}"] = grads[k].numpy().copy()
        y64, grads64 = run_case(wrap, enc, x, Rm, torch.float64)
        res[f"{tag}.y64"] = y64.numpy()
        for k, gr in grads64.items():
            res[f"{tag}.grad_norm64.{k}"] = np.float64(gr.norm().item())
        for k in full:
            res[f"{tag}.grad64.{k}"] = grads64[k].numpy().copy()
        print("g28", tag, "T", (R0 // 4) ** 2 + 1, "y norm", float(y.norm()), "fp32 vs fp64", float((y.double() - y64).abs().max()))

    # full vision Model.forward (V/model/model.py:35-73) with the micro BEiT tower, at the g11 ``full`` configuration
    from make_golden_vision import synth_batch
    S, D, item_num, B = 5, 48, 40, 3
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="beit_micro")
    pop = np.abs(det_normal("pop.g28", (item_num + 1,), std=1.0)) + 0.05
    pop = (pop / pop.sum()).astype(np.float32)
    net = build_beit(16, D)
    m = RefModel(args, item_num, True, net, pop.tolist())
    load_det(m)
    m.eval()
    ids, log_mask = synth_batch("g28f", B, S, item_num)
    images = det_normal("g28f.images", (item_num + 1, 3, 16, 16), std=1.0).astype(np.float32)
    images[0] = 0.0
    px = torch.from_numpy(images[ids.reshape(-1)])
    m.zero_grad()
    loss = m(torch.from_numpy(ids).view(-1), px, torch.from_numpy(log_mask), "cpu")
    loss.backward()
    res["full.cfg"] = np.array([S, D, item_num, B])
    res["full.ids"], res["full.log_mask"], res["full.pop"] = ids, log_mask, pop
    res["full.loss"] = np.float32(loss.item())
    for k, p in m.named_parameters():
        if p.grad is not None:
            res[f"full.grad_norm.{k}"] = np.float64(p.grad.double().norm().item())
    print("g28 full loss", loss.item())
    np.savez_compressed(os.path.join(out, "g28_beit.npz"), **res)

    # state_dict / named_parameters surface (V/run.py:58-60 freezes by parameter INDEX)
    keys = dict(state_dict=[[k, list(v.shape)] for k, v in m.state_dict().items()],
                named_parameters=[k for k, _ in m.named_parameters()],
                requires_grad={k: bool(p.requires_grad) for k, p in m.named_parameters()},
                image_net_named_parameters=[k for k, _ in net.named_parameters()],
                image_net_named_buffers=[k for k, _ in net.named_buffers()],
                encoder_named_parameters=[k for k, _ in m.cv_encoder.named_parameters()])
    with open(os.path.join(out, "g28_beit_keys.json"), "w") as f:
        json.dump(keys, f)
    print("g28 keys", len(keys["state_dict"]))


if __name__ == "__main__":
    g28(HERE)
