#!/usr/bin/env python
"""Capture golden vectors for the MAE (ViT) item tower from the imported reference.

Run once in the build container:   python tests/golden/make_golden_mae.py

Imports ``/root/reference/inbatch_sasrec_e2e_vision``'s ``model`` package unmodified (CPU, fp32) together with the installed HuggingFace
``ViTMAEModel`` (``attn_implementation="eager"``; the third-party class the reference hands to its ``MAE_Encoder``), feeds deterministic
synthetic pixels / weights (``det_param``) and a stored masking noise (a permutation / N per image: distinct values, so the kept set does
not depend on how a sort breaks ties) and writes ``g27_mae.npz`` + ``g27_mae_keys.json`` next to this file: numeric OUTPUTS and inputs that
cannot be regenerated only.

What this script adds around the reference (nothing of it is stored):
* the reference's ``MAE_Encoder`` hard-codes ``word_emb = 768``: its ``cv_proj`` is replaced by ``Linear(hidden, item_dim)`` after
  construction for the micro width;
* the reference calls ``image_net(item_content)`` and lets HF draw ``torch.rand`` noise: the network's ``forward`` is bound to pass the
  stored ``noise=``;
* the installed HF leaves ``position_embeddings`` at zero for a freshly constructed model (the patch projection is flagged initialised
  before ``ViTMAEEmbeddings.initialize_weights`` looks at it): the flag is cleared and HF's own ``initialize_weights`` is run, so the
  goldens use HF's sin-cos table (stored once per grid as ``pos.<grid>`` for the CPU test of the port).
Every case also stores the same module's fp64 run (``*.y64``, ``*.grad_norm64.*``, ``*.grad64.*``): the yardstick for the fp32 reference's
own rounding error, from which a test may derive a bound where one of g11's does not hold.
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

from idvs.morec_amd.utils.detgen import det_normal, det_param, det_uniform  # noqa: E402

from model import Model as RefModel  # noqa: E402  (reference package)
from model.encoders import MAE_Encoder as RefMaeEncoder  # noqa: E402
from transformers import ViTMAEConfig, ViTMAEModel  # noqa: E402

torch.set_num_threads(8)

MICRO = dict(patch_size=4, num_channels=3, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
POS = "embeddings.position_embeddings"


def det_noise(name, n_img, N):
    """fp32 [n_img, N]: per image a permutation of 0 .. N-1 (ranks of a deterministic uniform draw) divided by N."""
    u = det_uniform(name, (n_img, N), 0.0, 1.0).astype(np.float64) + np.arange(N)[None, :] * 1e-9
    perm = np.argsort(np.argsort(u, axis=1, kind="stable"), axis=1, kind="stable")
    return (perm.astype(np.float64) / N).astype(np.float32)


def load_det(module, seed=12345):
    """det_param into every floating-point entry except the (frozen) position table."""
    sd = module.state_dict()
    new = {k: torch.from_numpy(det_param(k, tuple(v.shape), seed=seed)) for k, v in sd.items()
           if v.dtype.is_floating_point and not k.endswith(POS)}
    module.load_state_dict(new, strict=False)
    return module


def build_mae(image_size, mask_ratio):
    cfg = ViTMAEConfig(attn_implementation="eager", image_size=image_size, mask_ratio=mask_ratio, **MICRO)
    net = ViTMAEModel(cfg)
    net.embeddings.patch_embeddings.projection._is_hf_initialized = False
    with torch.no_grad():
        net.embeddings.initialize_weights()          # HF's sin-cos table (the other values are overwritten by load_det)
    return net


def bind_noise(net, noise):
    plain = net.forward
    net.forward = lambda x: plain(x, noise=noise.to(x.dtype))
    return net


def build_encoder(image_size, mask_ratio, D):
    net = build_mae(image_size, mask_ratio)
    enc = RefMaeEncoder(net, D)
    enc.cv_proj = torch.nn.Linear(MICRO["hidden_size"], D)       # the reference's Linear(768, D) at the micro width
    return net, enc


def run_case(wrap, enc, x, Rm, dtype):
    wrap.to(dtype)
    wrap.zero_grad()
    y = enc(x.to(dtype))
    (y * Rm.to(dtype)).sum().backward()
    named = dict(wrap.named_parameters())
    return y.detach(), {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}


def g27(out):
    res = {}
    N_IMG, D = 3, 48
    for tag, R0, ratio in [("m17", 32, 0.75), ("m50", 56, 0.75), ("m65", 32, 0.0)]:
        n_patches = (R0 // 4) ** 2
        noise = det_noise(f"g27{tag}.noise", N_IMG, n_patches)
        net, enc = build_encoder(R0, ratio, D)
        bind_noise(net, torch.from_numpy(noise))
        wrap = torch.nn.Module()
        wrap.cv_encoder = enc                       # keys get the reference's ``cv_encoder.`` prefix
        load_det(wrap)
        wrap.eval()
        x = torch.from_numpy(det_normal(f"g27{tag}.x", (N_IMG, 3, R0, R0), std=1.0))
        Rm = torch.from_numpy(det_normal(f"g27{tag}.R", (N_IMG, D), std=1.0))
        len_keep = int(n_patches * (1 - ratio))
        keep = np.argsort(noise, axis=1, kind="stable")[:, :len_keep].astype(np.int32)
        y, grads = run_case(wrap, enc, x, Rm, torch.float32)
        res[f"{tag}.cfg"] = np.array([R0, 4, MICRO["hidden_size"], MICRO["num_hidden_layers"], MICRO["num_attention_heads"],
                                      MICRO["intermediate_size"], N_IMG, D])
        res[f"{tag}.mask_ratio"] = np.float64(ratio)
        res[f"{tag}.noise"], res[f"{tag}.keep"] = noise, keep
        res[f"{tag}.y"] = y.numpy()
        res[f"pos.{R0 // 4}"] = net.embeddings.position_embeddings.detach().float().numpy()[0]
        pre = "cv_encoder.image_net."
        full = [pre + "embeddings.cls_token", pre + "embeddings.patch_embeddings.projection.weight",
                pre + "embeddings.patch_embeddings.projection.bias", "cv_encoder.cv_proj.weight",
                pre + "layers.0.attention.k_proj.bias", pre + "layers.1.attention.q_proj.weight"]
        for k, g in grads.items():
            res[f"{tag}.grad_norm.{k}"] = np.float64(g.double().norm().item())
        for k in full:
            res[f"{tag}.grad.{k}"] = grads[k].numpy().copy()
        y64, grads64 = run_case(wrap, enc, x, Rm, torch.float64)
        res[f"{tag}.y64"] = y64.numpy()
        for k, g in grads64.items():
            res[f"{tag}.grad_norm64.{k}"] = np.float64(g.norm().item())
        for k in full:
            res[f"{tag}.grad64.{k}"] = grads64[k].numpy().copy()
        print("g27", tag, "T", len_keep + 1, "y norm", float(y.norm()), "fp32 vs fp64", float((y.double() - y64).abs().max()))

    # full vision Model.forward (V/model/model.py:35-73) with the micro MAE tower, at the g11 ``full`` configuration
    from make_golden_vision import synth_batch
    S, D, item_num, B = 5, 48, 40, 3
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="mae_micro")
    pop = np.abs(det_normal("pop.g27", (item_num + 1,), std=1.0)) + 0.05
    pop = (pop / pop.sum()).astype(np.float32)
    net = build_mae(32, 0.75)
    noise = det_noise("g27f.noise", B * (S + 1), 64)
    bind_noise(net, torch.from_numpy(noise))
    m = RefModel(args, item_num, True, net, pop.tolist())
    m.cv_encoder.cv_proj = torch.nn.Linear(MICRO["hidden_size"], D)
    load_det(m)
    m.eval()
    ids, log_mask = synth_batch("g27f", B, S, item_num)
    images = det_normal("g27f.images", (item_num + 1, 3, 32, 32), std=1.0).astype(np.float32)
    images[0] = 0.0
    px = torch.from_numpy(images[ids.reshape(-1)])
    m.zero_grad()
    loss = m(torch.from_numpy(ids).view(-1), px, torch.from_numpy(log_mask), "cpu")
    loss.backward()
    res["full.cfg"] = np.array([S, D, item_num, B])
    res["full.ids"], res["full.log_mask"], res["full.pop"], res["full.noise"] = ids, log_mask, pop, noise
    res["full.loss"] = np.float32(loss.item())
    for k, p in m.named_parameters():
        if p.grad is not None:
            res[f"full.grad_norm.{k}"] = np.float64(p.grad.double().norm().item())
    print("g27 full loss", loss.item())
    np.savez_compressed(os.path.join(out, "g27_mae.npz"), **res)

    # state_dict / named_parameters surface (V/run.py:58-60 freezes by parameter INDEX; the frozen position table counts)
    keys = dict(state_dict=[[k, list(v.shape)] for k, v in m.state_dict().items()],
                named_parameters=[k for k, _ in m.named_parameters()],
                requires_grad={k: bool(p.requires_grad) for k, p in m.named_parameters()},
                image_net_named_parameters=[k for k, _ in net.named_parameters()],
                encoder_named_parameters=[k for k, _ in m.cv_encoder.named_parameters()])
    with open(os.path.join(out, "g27_mae_keys.json"), "w") as f:
        json.dump(keys, f)
    print("g27 keys", len(keys["state_dict"]))


if __name__ == "__main__":
    g27(HERE)
