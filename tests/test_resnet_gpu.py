"""-m gpu: the ResNet item tower on a real MI355X -- ``Resnet_Encoder`` and both ``Model`` classes over ``resnet_micro`` (BasicBlock) and
``resnet_micro_b`` (Bottleneck) against g32 (``tests/golden/g32_resnet.npz``: the reference's own classes around the plain-torch ResNet
of ``tests/resnet_ref.py``, 6 images of 64 x 64 with one all-zero padding image, training mode = batch statistics over all 6).

Bounds.  Every comparison is against the reference's fp64 run.
  fp32   item vectors, loss, running statistics and every backbone gradient: |ours - fp64| <= ``MULT`` = 4 x the reference's OWN
         |fp32 - fp64| stored in the fixture (largest over the tensor); four is the multiple ``tests/test_deberta_gpu.py``'s ``twin_bound``
         takes of the same quantity.  Gradients are compared at the elements the fixture keeps (``resnet_ref.sample_idx``: all of a small
         tensor, 128 of a large one) and by their norm (which moves by at most the error vector's norm).
  bf16 / fp16   item vectors and running statistics: 4 x the error of the reference itself run in that type (on the CPU); the loss:
         ``test_g31_bce_model_golden``'s 3e-2.  Backbone gradients: their relative error against the fp64 twin as MEASURED on an MI355X
         (``MEASURED16``: per case the median and the largest over the tensors), held to twice the recorded figure.  Six images through
         BatchNorm layers that see as few as 24 values per channel make 16-bit gradients noisy -- the reference's own bf16 gradients are
         off by up to 0.6 of a tensor's largest element -- so the fixed 16-bit bounds of the transformer towers do not apply, and a
         multiple of the reference's 16-bit error would pass a zero gradient.  The recorded medians are well below 1: a dropped or
         sign-flipped gradient of the matrix-core convolution, forward or data gradient, moves them to 1 and beyond.
The user encoder's gradients in the two ``Model`` cases are not the tower's: their norms are held to ``test_g31_deberta_micro_golden``'s
model-level bound, unchanged (fp32: 1e-3 relative + 1e-4; 16-bit: 1e-1 relative + 2e-2).

Measured (MI355X): see README "ResNet item tower".
"""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resnet_ref  # noqa: E402
from helpers import GOLDEN_DIR  # noqa: E402
from idvs.morec_amd import ops, resnet_engine  # noqa: E402
from idvs.morec_amd.model import BceModel, Model  # noqa: E402
from idvs.morec_amd.model.encoders import Resnet_Encoder  # noqa: E402
from idvs.morec_amd.model.resnet import HipResNet, ResNetShape  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
NETS = ["resnet_micro", "resnet_micro_b"]
MULT = 4.0


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN_DIR, "g32_resnet.npz"))


def pixels(G):
    n, R0, _ = (int(v) for v in G["cfg"])
    x = det_normal("g32.x", (n, 3, R0, R0), std=1.0)
    x[0] = 0.0
    return torch.from_numpy(x).to(DEV)


def encoder(name, dt, G):
    D = int(G["cfg"][2])
    wrap = torch.nn.Module()
    wrap.cv_encoder = Resnet_Encoder(HipResNet(ResNetShape.named(name), D), compute_dtype=DT[dt])
    resnet_ref.load_det(wrap)
    return wrap.to(DEV)


COL = {"fp32": 2, "bf16": 3, "fp16": 4}      # <base>.grad_stats: norm64, max64, then the reference's own error per number format

# 16-bit backbone gradients: per tensor, the relative error ||ours - fp64|| / ||fp64|| over the elements the fixture keeps; per case the
# MEDIAN and the LARGEST of these over the backbone's tensors, as measured on an MI355X against the fp64 twin.  The test holds both to
# TWICE the recorded figure (the kernels repeat their bits: the margin is for another compiler or torch build, not for noise).
MEASURED16 = {
    ('resnet_micro', 'bf16'): (0.2011, 0.2916),
    ('resnet_micro', 'fp16'): (0.0524, 0.0883),
    ('resnet_micro_b', 'bf16'): (0.2932, 0.4815),
    ('resnet_micro_b', 'fp16'): (0.1039, 0.1623),
    ('resnet_micro.inbatch', 'bf16'): (0.2028, 0.2937),
    ('resnet_micro.inbatch', 'fp16'): (0.0726, 0.1154),
    ('resnet_micro.bce', 'bf16'): (0.1956, 0.3040),
    ('resnet_micro.bce', 'fp16'): (0.0469, 0.0871),
    ('resnet_micro_b.inbatch', 'bf16'): (0.2992, 0.4105),
    ('resnet_micro_b.inbatch', 'fp16'): (0.1086, 0.1733),
    ('resnet_micro_b.bce', 'bf16'): (0.3024, 0.4692),
    ('resnet_micro_b.bce', 'fp16'): (0.0982, 0.1622),
}


def check_grads(G, base, named, dt, fails):
    """Every gradient the fixture holds under ``base`` (see the module docstring)."""
    keys, vals, stats = [str(k) for k in G[base + ".grad_keys"]], G[base + ".grad64"], G[base + ".grad_stats"]
    worst, at, rels = 0.0, 0, []
    for k, st in zip(keys, stats):
        got = named[k].grad
        assert got is not None and bool(torch.isfinite(got).all()), k
        flat = got.double().reshape(-1).cpu().numpy()
        idx = resnet_ref.sample_idx(k, flat.size)
        ref, at = vals[at:at + len(idx)], at + len(idx)
        gnorm, own = float(st[0]), float(st[COL[dt]])
        err, nerr = float(np.abs(flat[idx] - ref).max()), abs(float(np.linalg.norm(flat)) - gnorm)
        if not k.startswith("cv_encoder."):      # the user encoder: not the tower's
            bound, nbound = float("inf"), (1e-3 * gnorm + 1e-4 if dt == "fp32" else 1e-1 * gnorm + 2e-2)
            ok = nerr <= nbound
        elif dt == "fp32":
            bound, nbound = MULT * own, MULT * own * np.sqrt(flat.size)
            ok = err <= bound and nerr <= nbound
            worst = max(worst, err / bound if bound > 0 else float(err > 0))
        else:
            rels.append((float(np.linalg.norm(flat[idx] - ref) / (np.linalg.norm(ref) + 1e-300)), k))
            continue
        if not ok:
            fails.append((base, k, f"err {err:.3e} bound {bound:.3e} (reference's own {own:.3e}); norm err {nerr:.3e} bound {nbound:.3e}"))
    assert at == len(vals)
    if dt == "fp32":
        print(f"g32 {base} {dt}: {len(keys)} gradients, worst backbone err / bound {worst:.3f}")
        return
    med, (top, top_key) = float(np.median([r for r, _ in rels])), max(rels)
    print(f"g32 {base} {dt}: {len(rels)} backbone gradients, relative error median {med:.4f} largest {top:.4f} ({top_key})  MEASURED16 {(base, dt)!r}: ({med:.4f}, {top:.4f})")
    want = MEASURED16.get((base, dt))
    if want is None:
        fails.append((base, dt, "no recorded figure for this case"))
    elif not (med <= 2 * want[0] and top <= 2 * want[1]):
        fails.append((base, dt, f"relative error median {med:.4f} largest {top:.4f} ({top_key}); recorded {want}, bound twice that"))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", NETS)
def test_g32_encoder_golden(G, name, dt):
    """Training-mode output and every gradient, the running statistics after that one forward, then the evaluation-mode output."""
    n, R0, D = (int(v) for v in G["cfg"])
    wrap = encoder(name, dt, G)
    enc = wrap.cv_encoder
    x = pixels(G)
    f32 = dt == "fp32"
    fails = []

    def vec_check(what, got, key):
        ref = G[f"{name}.{key}64"]
        err = float(np.abs(got.detach().double().cpu().numpy() - ref).max())
        own = float(np.abs(G[f"{name}.{key}"].astype(np.float64) - ref).max()) if f32 else float(G[f"{name}.{key}_err_{dt}"])
        bound = MULT * own
        print(f"g32 {name} {dt} {what}: err {err:.3e} bound {bound:.3e} (reference's own {dt} error {own:.3e})")
        if not err <= bound:
            fails.append((name, what, err, bound))

    wrap.eval()
    with torch.no_grad():
        y_eval = enc(x)
        assert torch.equal(y_eval, enc(x))      # the bits repeat
    vec_check("y_eval", y_eval, "y_eval")
    wrap.train()
    y = enc(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, D)
    vec_check("y", y, "y")
    R = torch.from_numpy(det_normal("g32.R", (n, D), std=1.0)).to(DEV)
    (y * R).sum().backward()
    check_grads(G, name, dict(wrap.named_parameters()), dt, fails)
    worst, at = 0.0, 0
    bufs = dict(wrap.named_buffers())
    for k, st in zip((str(k) for k in G[name + ".running_keys"]), G[name + ".running_stats"]):
        b = bufs[k]
        ref, at = G[name + ".running64"][at:at + b.numel()], at + b.numel()
        err, bound = float(np.abs(b.double().cpu().numpy() - ref).max()), MULT * float(st[COL[dt] - 2])
        worst = max(worst, err / bound)
        if not err <= bound:
            fails.append((name, k, err, bound))
    assert all(int(b) == 1 for k, b in bufs.items() if k.endswith("num_batches_tracked"))
    print(f"g32 {name} {dt}: running statistics, worst err / bound {worst:.3f}")
    assert not fails, fails


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("kind", ["inbatch", "bce"])
@pytest.mark.parametrize("name", NETS)
def test_g32_model_golden(G, name, kind, dt):
    """The reference's in-batch ``Model`` (B = 2, S = 2) and BCE ``Model`` (B = 1, S = 2) over the tower, training mode: loss and every
    gradient, the user encoder's included."""
    D = int(G["cfg"][2])
    args = types.SimpleNamespace(max_seq_len=2, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2, CV_model_load=name,
                                 compute_dtype=dt, item_tower="modal")
    net = HipResNet(ResNetShape.named(name), D)
    x = pixels(G)
    if kind == "inbatch":
        m = resnet_ref.load_det(Model(args, 8, True, net, G[f"{name}.inbatch.pop"].tolist())).to(DEV).train()
        loss = m(torch.from_numpy(G[f"{name}.inbatch.ids"]).view(-1).to(DEV), x, torch.from_numpy(G[f"{name}.inbatch.log_mask"]).to(DEV), DEV)
    else:
        m = resnet_ref.load_det(BceModel(args, 8, True, net)).to(DEV).train()
        loss = m(x, torch.from_numpy(G[f"{name}.bce.log_mask"]).to(DEV), DEV)
    ref, own = float(G[f"{name}.{kind}.loss64"]), abs(float(G[f"{name}.{kind}.loss"]) - float(G[f"{name}.{kind}.loss64"]))
    err = abs(float(loss.detach()) - ref)
    # one number has no spread to take a multiple of (the reference's own fp16 loss of one case is off by 3e-6, of the next by 6e-3):
    # in 16 bits the loss is held to test_g31_bce_model_golden's bound, unchanged
    bound = MULT * own if dt == "fp32" else 3e-2 * max(1.0, abs(ref))
    print(f"g32 {name} {kind} {dt}: loss {float(loss.detach()):.7f} vs fp64 {ref:.7f}: err {err:.3e} bound {bound:.3e}")
    fails = [] if err <= bound else [(name, kind, "loss", err, bound)]
    loss.backward()
    check_grads(G, f"{name}.{kind}", dict(m.named_parameters()), dt, fails)
    assert not fails, fails


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_features_only_is_the_pooled_vector(G, dt):
    """``features_only`` / ``extract_item_features`` (what ``--save_features`` writes) return the globally pooled rows in front of ``fc``,
    evaluation mode: the plain-torch net's ``features`` in fp64, and ``GELU(fc(features))`` formed in fp64 from them is the item vector."""
    from idvs.morec_amd.data_utils import extract_item_features
    name = "resnet_micro_b"
    wrap = encoder(name, dt, G).eval()
    enc = wrap.cv_encoder
    x = pixels(G)
    p, bufs = dict(enc.named_parameters()), dict(enc.named_buffers())
    with torch.no_grad():
        prep = resnet_engine.resnet_prepare(p, enc.image_net.shape, DT[dt], "image_net.", need_grad=False, features_only=True)
        feats, saved = resnet_engine.resnet_forward(p, bufs, prep, enc.image_net.shape, x, DT[dt], False, "image_net.", features_only=True)
        y = enc(x)
        table = extract_item_features(enc, x.cpu(), 4, DEV)      # two chunks: the running statistics make the rows independent
    ref = resnet_ref.build(name, int(G["cfg"][2]))
    ref.load_state_dict({k: v.detach().cpu() for k, v in enc.image_net.state_dict().items()})
    ref = ref.double().eval()
    with torch.no_grad():
        want = ref.features(x.double().cpu())
    assert saved is None and tuple(feats.shape) == (x.shape[0], enc.image_net.shape.num_features) and feats.dtype == DT[dt]
    assert table.dtype == torch.float32 and torch.equal(table, feats.float())
    e = float((feats.double().cpu() - want).abs().max() / want.abs().max())
    print(f"features_only {dt}: relerr {e:.2e}")
    assert e < (1e-5 if dt == "fp32" else 5e-2)
    w = enc.image_net.fc.weight.detach().to(DT[dt]).double()
    item = torch.nn.functional.gelu(feats.double() @ w.t() + enc.image_net.fc.bias.detach().double())
    # fp32: 1024-term fp32 dot products and the kernel's erf (1.5e-7 absolute); bf16: one rounding of the output (2^-8 relative)
    assert float((y.double() - item).abs().max() / item.abs().max()) < (1e-5 if dt == "fp32" else 2.0 ** -7)


def test_frozen_prefix_gets_no_gradient_and_changes_no_other(G):
    """``--freeze_paras_before 5``: ``conv1``, ``bn1`` (gain and shift), ``layer1.0.conv1`` and ``layer1.0.bn1.weight`` frozen.  They get
    no gradient; every other gradient keeps its bits (deterministic mode): a frozen BatchNorm still normalises with batch statistics."""
    def run(k):
        wrap = encoder("resnet_micro", "bf16", G).train()
        for i, (_, prm) in enumerate(wrap.cv_encoder.image_net.named_parameters()):
            prm.requires_grad = i >= k
        R = torch.from_numpy(det_normal("g32.R", (6, int(G["cfg"][2])), std=1.0)).to(DEV)
        (wrap.cv_encoder(pixels(G)) * R).sum().backward()
        torch.cuda.synchronize()
        return {n: (None if prm.grad is None else prm.grad.clone()) for n, prm in wrap.named_parameters()}, dict(wrap.named_buffers())

    ops.set_deterministic(True)
    try:
        (g0, b0), (g1, b1) = run(0), run(5)
    finally:
        ops.set_deterministic(False)
    names = list(g0)
    assert names[3] == "cv_encoder.image_net.layer1.0.conv1.weight"
    for i, n in enumerate(names):
        if i < 5:
            assert g1[n] is None and g0[n] is not None and float(g0[n].abs().max()) > 0, n
        else:
            assert torch.equal(g0[n], g1[n]), n
    for n in b0:
        assert torch.equal(b0[n], b1[n]), n


# ------------------------------------------------------------------------------------------------ driver
_DRIVER = r"""
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
common = {common!r}
run.main(common)
print("=== TEST RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"])
print("=== BCE ===", file=sys.stderr, flush=True)
run.main({bce!r})
print("=== STAGE 1 ===", file=sys.stderr, flush=True)
run.main({stage1!r})
"""


def test_run_driver_resnet_micro(tmp_path):
    """``run.py --item_tower modal --CV_model_load resnet_micro --synthetic 48`` in a fresh child process: one short epoch with its
    validation (the catalogue pass in evaluation mode) and checkpoint, ``--mode test`` on it, two steps under ``--loss bce``, then stage 1
    of ``--arch two_stage`` with ``--save_features`` (``num_fc_ftr`` = 256 columns for the micro net)."""
    feats = str(tmp_path / "features.npy")
    base = ["--item_tower", "modal", "--CV_model_load", "resnet_micro", "--CV_resize", "32", "--synthetic", "48", "--synthetic_items", "60",
            "--epoch", "1", "--embedding_dim", "64", "--batch_size", "16", "--max_seq_len", "5", "--lr", "1e-3", "--fine_tune_lr", "1e-4",
            "--freeze_paras_before", "3", "--compute_dtype", "bf16", "--collate_workers", "0", "--local_rank", "0"]
    common = base + ["--checkpoint_root", str(tmp_path / "a")]
    bce = base + ["--loss", "bce", "--max_steps", "2", "--checkpoint_root", str(tmp_path / "b")]
    stage1 = base + ["--arch", "two_stage", "--max_steps", "2", "--save_features", feats, "--checkpoint_root", str(tmp_path / "c")]
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, common=common, bce=bce, stage1=stage1)], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    train_log, rest = res.stderr.split("=== TEST RUN ===")
    test_log, rest = rest.split("=== BCE ===")
    bce_log, stage_log = rest.split("=== STAGE 1 ===")
    assert re.search(r"epoch 1: \d+ steps, mean loss [0-9.]+", train_log)
    assert "valid_methods   Hit10\tnDCG10" in train_log and re.search(r"valid_results   [0-9.]+\t[0-9.]+", train_log)
    saved = re.findall(r"Model saved to (\S+)", train_log)
    assert saved and "resnet_micro" in saved[-1] and str(tmp_path) in saved[-1]
    assert "model loaded from" in test_log and re.search(r"test_results   [0-9.]+\t[0-9.]+", test_log)
    assert re.search(r"mean loss [0-9.]+", bce_log)
    assert "stage 1" in stage_log and os.path.exists(feats)
    table = np.load(feats)
    assert table.shape == (61, 256) and table.dtype == np.float32 and np.isfinite(table).all()
