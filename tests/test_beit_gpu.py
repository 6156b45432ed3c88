"""-m gpu: the BEiT item tower on a real MI355X -- ``Vit_Encoder`` over the BEiT container / the vision ``Model`` against the golden vectors
captured from the imported reference over the installed HF ``BeitForImageClassification`` (``tests/golden/g28_beit.npz``), a training-mode
step against a torch restatement fed with the DropPath factors the kernels drew, relations that need no golden, and the driver in a child
process.  Bounds: those of ``tests/test_swin_gpu.py`` for the same quantities (``test_g11_vit_encoder_golden``,
``test_g11_vision_model_loss_golden``), as ``tests/test_mae_gpu.py`` applies them; g11 has one set for fp32 and one for every other type,
so fp16 runs under the 16-bit set."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import GOLDEN_DIR  # noqa: E402
from idvs.morec_amd import beit_engine, ops  # noqa: E402
from idvs.morec_amd.beit_engine import TABLE, BeitShape  # noqa: E402
from idvs.morec_amd.engine import DropCfg  # noqa: E402
from idvs.morec_amd.model import Model  # noqa: E402
from idvs.morec_amd.model.beit import HipBeitForImageClassification  # noqa: E402
from idvs.morec_amd.model.encoders import Vit_Encoder  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal, det_param  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
FULL = ["beit.layers.0." + TABLE, "beit.layers.0.lambda_1", "beit.layers.0.attention.q_proj.bias", "beit.embeddings.cls_token",
        "beit.embeddings.patch_embeddings.projection.weight", "classifier.weight"]


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def froerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def load_det(module, prefix=""):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            v.copy_(torch.from_numpy(det_param(prefix + k, tuple(v.shape))))
    return module


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN_DIR, "g28_beit.npz"))


def _shape(R0, **kw):
    return BeitShape(image_size=R0, patch_size=4, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, **kw)


def _case(G, tag, dt):
    R0, ps, C, layers, heads, inter, n_img, D = (int(v) for v in G[f"{tag}.cfg"])
    shape = BeitShape(image_size=R0, patch_size=ps, hidden_size=C, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter)
    enc = Vit_Encoder(HipBeitForImageClassification(shape, D), compute_dtype=DT[dt])
    load_det(enc, "cv_encoder.").to(DEV).eval()
    x = torch.from_numpy(det_normal(f"g28{tag}.x", (n_img, 3, R0, R0), std=1.0)).to(DEV)
    return shape, enc, x, n_img, D


# ------------------------------------------------------------------------------------------------ encoder / model vs goldens
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("tag", ["b17", "b50", "b65"])
def test_g28_beit_encoder_golden(G, tag, dt):
    """b17 (T = 17), b50 (T = 50) and b65 (T = 65: a second key tile holding one key) under ``test_g11_vit_encoder_golden``'s bounds."""
    shape, enc, x, n_img, D = _case(G, tag, dt)
    assert shape.num_patches + 1 == {"b17": 17, "b50": 50, "b65": 65}[tag]
    R = torch.from_numpy(det_normal(f"g28{tag}.R", (n_img, D), std=1.0)).to(DEV)
    y = enc(x)
    e_y = relerr(y.detach().cpu().numpy(), G[f"{tag}.y"])
    print(f"g28 {tag} {dt}: y relerr {e_y:.2e}")
    assert e_y < (1e-4 if dt == "fp32" else 5e-2), e_y
    (y * R).sum().backward()
    worst = 0.0
    named = dict(enc.named_parameters())
    for n, p in named.items():
        ref = float(G[f"{tag}.grad_norm.cv_encoder.{n}"])
        got = float(p.grad.double().norm())
        worst = max(worst, abs(got - ref) / (ref + 1e-12))
        assert abs(got - ref) <= (2e-3 if dt == "fp32" else 8e-2) * ref + (1e-6 if dt == "fp32" else 1e-3), (n, got, ref)
    for n in FULL:
        ref = G[f"{tag}.grad.cv_encoder.image_net.{n}"]
        assert np.abs(ref).max() > 1e-7, n
        e = froerr(named["image_net." + n].grad.cpu().numpy(), ref)
        print(f"g28 {tag} {dt}: {n} froerr {e:.2e}")
        assert e < (5e-4 if dt == "fp32" else 8e-2), (n, e)
    print(f"g28 {tag} {dt}: worst grad-norm err {worst:.2e}")


def _full_model(G, dt="fp32", tower="modal"):
    S, D, item_num, B = (int(v) for v in G["full.cfg"])
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="beit_micro", compute_dtype=dt, item_tower=tower)
    m = Model(args, item_num, True, HipBeitForImageClassification(BeitShape.named("beit_micro"), D), G["full.pop"].tolist())
    return load_det(m).to(DEV)


def _full_inputs(G):
    S, D, item_num, B = (int(v) for v in G["full.cfg"])
    ids, log_mask = G["full.ids"], G["full.log_mask"]
    images = det_normal("g28f.images", (item_num + 1, 3, 16, 16), std=1.0).astype(np.float32)
    images[0] = 0.0
    return (torch.from_numpy(ids).view(-1).to(DEV), torch.from_numpy(images[ids.reshape(-1)]).to(DEV), torch.from_numpy(log_mask).to(DEV))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_g28_beit_model_loss_golden(G, dt):
    """The reference ``Model`` over the micro BEiT tower at g11's ``full`` configuration, under ``test_g11_vision_model_loss_golden``'s bounds."""
    m = _full_model(G, dt).eval()
    loss = m(*_full_inputs(G), DEV)
    print(f"g28 full {dt}: loss {float(loss.detach()):.6f} (reference {float(G['full.loss']):.6f})")
    assert abs(float(loss.detach()) - float(G["full.loss"])) < (1e-3 if dt == "fp32" else 5e-2), (float(loss), float(G["full.loss"]))
    loss.backward()
    for n, p in m.named_parameters():
        ref = float(G[f"full.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert abs(got - ref) <= (3e-3 if dt == "fp32" else 1e-1) * ref + (1e-6 if dt == "fp32" else 1e-3), (n, got, ref)


# ------------------------------------------------------------------------------------------------ training mode
def beit_restated(p, shape, x, scales):
    """HF ``BeitForImageClassification`` + ``GELU`` in plain torch (the type of ``p`` / ``x``), with the DropPath factors given:
    ``scales[l] = (attention factor [n_img] or None, MLP factor or None)``."""
    net = "image_net.beit."
    n, C, heads, g = x.shape[0], shape.hidden_size, shape.num_attention_heads, shape.grid
    T, dh = g * g + 1, shape.hidden_size // shape.num_attention_heads
    e = F.conv2d(x, p[net + "embeddings.patch_embeddings.projection.weight"], p[net + "embeddings.patch_embeddings.projection.bias"],
                 stride=shape.patch_size).flatten(2).transpose(1, 2)
    h = torch.cat([p[net + "embeddings.cls_token"].expand(n, 1, C), e], 1)
    idx = ops.beit_relative_position_index(g).to(x.device).view(-1)
    for l in range(shape.num_hidden_layers):
        L = f"{net}layers.{l}."
        A = L + "attention."
        s1, s2 = (torch.ones(n, device=x.device, dtype=x.dtype) if s is None else s.to(x.dtype) for s in scales[l])
        xn = F.layer_norm(h, (C,), p[L + "layernorm_before.weight"], p[L + "layernorm_before.bias"], shape.layer_norm_eps)
        q = (xn @ p[A + "q_proj.weight"].t() + p[A + "q_proj.bias"]).view(n, T, heads, dh).transpose(1, 2)
        k = (xn @ p[A + "k_proj.weight"].t()).view(n, T, heads, dh).transpose(1, 2)
        v = (xn @ p[A + "v_proj.weight"].t() + p[A + "v_proj.bias"]).view(n, T, heads, dh).transpose(1, 2)
        bias = p[L + TABLE][idx].view(T, T, heads).permute(2, 0, 1)
        att = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5 + bias[None], -1)
        a = (att @ v).transpose(1, 2).reshape(n, T, C) @ p[A + "o_proj.weight"].t() + p[A + "o_proj.bias"]
        h = h + s1[:, None, None] * (p[L + "lambda_1"] * a)
        hn = F.layer_norm(h, (C,), p[L + "layernorm_after.weight"], p[L + "layernorm_after.bias"], shape.layer_norm_eps)
        f = F.gelu(hn @ p[L + "mlp.fc1.weight"].t() + p[L + "mlp.fc1.bias"]) @ p[L + "mlp.fc2.weight"].t() + p[L + "mlp.fc2.bias"]
        h = h + s2[:, None, None] * (p[L + "lambda_2"] * f)
    pooled = F.layer_norm(h[:, 1:].mean(1), (C,), p[net + "pooler.layernorm.weight"], p[net + "pooler.layernorm.bias"], shape.layer_norm_eps)
    return F.gelu(pooled @ p["image_net.classifier.weight"].t() + p["image_net.classifier.bias"]), pooled


def test_droppath_training_matches_restatement_with_exported_scales():
    """Training mode, fp32: the per-image DropPath factors the tower draws are re-created through ``ops.droppath_scale`` (site 2 l +
    sub-layer of the step's seed) and fed to the torch restatement (fp64), which must then reproduce output and gradients under
    ``test_g11_vit_encoder_golden``'s fp32 bounds."""
    shape = _shape(28, drop_path_rate=0.5)
    N, D = 6, 48
    enc = Vit_Encoder(HipBeitForImageClassification(shape, D), compute_dtype=torch.float32)
    load_det(enc, "cv_encoder.").to(DEV).train()
    x = torch.from_numpy(det_normal("g28dp.x", (N, 3, 28, 28))).to(DEV)
    R = torch.from_numpy(det_normal("g28dp.R", (N, D))).to(DEV)
    drop = DropCfg(0.0, 0.0, 0xABCDEF12345)
    y = enc.encode(x, drop)
    (y.float() * R).sum().backward()
    rates = shape.drop_path_rates()
    assert rates == [0.0, 0.5]
    scales = [(None, None) if r == 0 else tuple(ops.droppath_scale(N, r, drop.site(2 * l + k)) for k in range(2)) for l, r in enumerate(rates)]
    drawn = torch.stack(scales[1])
    assert bool((drawn == 0).any()) and bool((drawn == 2.0).any()) and not torch.equal(scales[1][0], scales[1][1])
    p = {n: t.detach().double().requires_grad_(True) for n, t in enc.named_parameters()}
    yr, _ = beit_restated(p, shape, x.double(), scales)
    e_y = relerr(y.detach().cpu().numpy(), yr.detach().cpu().numpy())
    print(f"droppath restatement: y relerr {e_y:.2e}")
    assert e_y < 1e-4
    (yr * R.double()).sum().backward()
    for n, t in enc.named_parameters():
        ref, got = float(p[n].grad.norm()), float(t.grad.double().norm())
        assert abs(got - ref) <= 2e-3 * ref + 1e-6, (n, got, ref)
    for n in FULL:
        assert froerr(dict(enc.named_parameters())["image_net." + n].grad.cpu().numpy(), p["image_net." + n].grad.cpu().numpy()) < 5e-4, n
    # evaluation mode draws nothing: the same call repeats bit for bit and differs from the training output
    enc.eval()
    with torch.no_grad():
        assert torch.equal(enc.encode(x, drop), enc.encode(x, drop)) and not torch.equal(enc.encode(x, drop), y)


def test_frozen_table_gets_no_gradient_and_changes_no_other(G):
    """``requires_grad = False`` on a relative-position table (``--freeze_paras_before`` reaches it by index) and on a layer scale: no
    gradient for them, every other gradient bit-equal (deterministic mode)."""
    def run(freeze):
        shape, enc, x, n_img, D = _case(G, "b65", "bf16")
        enc.train()
        named = dict(enc.named_parameters())
        for n in freeze:
            named[n].requires_grad = False
        R = torch.from_numpy(det_normal("g28b65.R", (n_img, D), std=1.0)).to(DEV)
        (enc(x) * R).sum().backward()
        torch.cuda.synchronize()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in named.items()}

    frozen = ["image_net.beit.layers.0." + TABLE, "image_net.beit.layers.1.lambda_2"]
    ops.set_deterministic(True)
    try:
        g0, g1 = run([]), run(frozen)
    finally:
        ops.set_deterministic(False)
    for n in g0:
        if n in frozen:
            assert g1[n] is None and g0[n] is not None and float(g0[n].abs().max()) > 0, n
        else:
            assert torch.equal(g0[n], g1[n]), n


def test_from_hf_matches_the_hf_model():
    """``from_hf`` of a micro HF model (its own initialisation, the tables and [CLS] made non-zero) against a direct call of that model."""
    from transformers import BeitConfig, BeitForImageClassification
    torch.manual_seed(5)
    cfg = BeitConfig(attn_implementation="eager", image_size=28, patch_size=4, num_channels=3, hidden_size=64, num_hidden_layers=2,
                     num_attention_heads=2, intermediate_size=256, use_relative_position_bias=True, use_mean_pooling=True)
    hf = BeitForImageClassification(cfg)
    hf.classifier = torch.nn.Linear(64, 48)
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if n.endswith("relative_position_bias_table") or n.endswith("cls_token"):
                p.normal_(std=0.2)
    hf.eval()
    x = torch.from_numpy(det_normal("g28hf.x", (3, 3, 28, 28)))
    with torch.no_grad():
        want = F.gelu(hf(x)[0])
    enc = Vit_Encoder(hf, compute_dtype=torch.float32).to(DEV).eval()
    assert enc.is_beit and [n for n, _ in enc.image_net.named_parameters()] == [n for n, _ in hf.named_parameters()]
    with torch.no_grad():
        got = enc(x.to(DEV))
    e = relerr(got.cpu().numpy(), want.numpy())
    print(f"from_hf: relerr {e:.2e}")
    assert e < 1e-4


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_features_only_is_the_pooler_output(G, dt):
    """``features_only`` / ``extract_item_features`` (what ``--save_features`` writes) return the pooler output: the restatement's pooled
    rows, and ``GELU(classifier(features))`` formed by torch in fp64 from them is the item vector."""
    from idvs.morec_amd.data_utils import extract_item_features
    shape, enc, x, n_img, D = _case(G, "b50", dt)
    p = dict(enc.named_parameters())
    with torch.no_grad():
        prep = beit_engine.beit_prepare(p, shape, DT[dt], "image_net.", features_only=True)
        feats, saved = beit_engine.beit_forward(p, prep, shape, x, DT[dt], False, "image_net.", features_only=True)
        y = enc(x)
        table = extract_item_features(enc, x.cpu(), 2, DEV)
        _, pooled = beit_restated({n: t.detach().double() for n, t in p.items()}, shape, x.double(), [(None, None)] * 2)
    assert saved is None and tuple(feats.shape) == (n_img, shape.hidden_size) and feats.dtype == DT[dt]
    assert table.dtype == torch.float32 and torch.equal(table, feats.float())
    assert relerr(feats.float().cpu().numpy(), pooled.cpu().numpy()) < (1e-4 if dt == "fp32" else 5e-2)
    w = enc.image_net.classifier.weight.detach().to(DT[dt]).double()
    want = F.gelu(feats.double() @ w.t() + enc.image_net.classifier.bias.detach().double())
    # fp32: the 64-term fp32 dot products and the kernel's erf (1.5e-7 absolute); bf16: one rounding of the output (2^-9 relative)
    assert relerr(y.cpu().numpy(), want.cpu().numpy()) < (1e-5 if dt == "fp32" else 2.0 ** -8)


def test_add_fusion_with_a_zero_id_table_is_the_plain_beit_model(G):
    """The fusion towers take the BEiT tower: ``modal_add`` with a zero id table is the plain modal model, bit for bit (deterministic
    mode; both models draw the same DropPath factors: the same seed and call counter)."""
    inputs = _full_inputs(G)
    ops.set_deterministic(True)
    try:
        outs = []
        for tower in ("modal", "modal_add"):
            torch.manual_seed(11)
            m = _full_model(G, "fp32", tower).train()
            if tower == "modal_add":
                with torch.no_grad():
                    m.id_embedding.weight.zero_()
            m.zero_grad()
            loss = m(*inputs, DEV)
            loss.backward()
            torch.cuda.synchronize()
            outs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    finally:
        ops.set_deterministic(False)
    (l0, g0), (l1, g1) = outs
    assert torch.equal(l0, l1), (float(l0), float(l1))
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ------------------------------------------------------------------------------------------------ driver
_DRIVER = r"""
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
run.main({inbatch!r})
print("=== BCE ===", file=sys.stderr, flush=True)
run.main({bce!r})
print("=== STAGE 1 ===", file=sys.stderr, flush=True)
run.main({stage1!r})
"""


def test_run_driver_beit_micro(tmp_path):
    """``run.py --item_tower modal --CV_model_load beit_micro --synthetic 48`` in a fresh child process: two short epochs with their
    validations and checkpoint under the in-batch loss, the same under ``--loss bce``, then stage 1 of ``--arch two_stage`` over the
    same tower with ``--save_features``."""
    feats = str(tmp_path / "features.npy")
    base = ["--item_tower", "modal", "--CV_model_load", "beit_micro", "--CV_resize", "16", "--synthetic", "48", "--synthetic_items", "60",
            "--embedding_dim", "64", "--batch_size", "16", "--max_seq_len", "5", "--lr", "1e-3", "--fine_tune_lr", "1e-4",
            "--freeze_paras_before", "0", "--compute_dtype", "bf16", "--collate_workers", "0", "--local_rank", "0"]
    inbatch = base + ["--epoch", "2", "--checkpoint_root", str(tmp_path / "a")]
    bce = base + ["--epoch", "2", "--loss", "bce", "--checkpoint_root", str(tmp_path / "b")]
    stage1 = base + ["--epoch", "1", "--arch", "two_stage", "--max_steps", "2", "--save_features", feats, "--checkpoint_root", str(tmp_path / "c")]
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, inbatch=inbatch, bce=bce, stage1=stage1)], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    in_log, rest = res.stderr.split("=== BCE ===")
    bce_log, stage_log = rest.split("=== STAGE 1 ===")
    for log in (in_log, bce_log):
        assert re.search(r"epoch 1: \d+ steps, mean loss [0-9.]+", log) and re.search(r"epoch 2: \d+ steps, mean loss [0-9.]+", log)
        assert "valid_methods   Hit10\tnDCG10" in log and re.search(r"valid_results   [0-9.]+\t[0-9.]+", log)
        saved = re.findall(r"Model saved to (\S+)", log)
        assert saved and "beit_micro" in saved[-1] and str(tmp_path) in saved[-1]
    assert "stage 1" in stage_log and os.path.exists(feats)
    table = np.load(feats)
    assert table.shape == (61, 64) and table.dtype == np.float32 and np.isfinite(table).all()
