"""-m gpu: the MAE (ViT) item tower on a real MI355X -- ``MAE_Encoder`` / the vision ``Model`` against the golden vectors captured from the
imported reference over the installed HF ``ViTMAEModel`` (``tests/golden/g27_mae.npz``: the kept patches are decided by a stored noise on
both sides), the generated-noise training step, relations that need no golden, and the driver in a child process.
Bounds: those of ``tests/test_swin_gpu.py`` for the same quantities (``test_g11_vit_encoder_golden``, ``test_g11_vision_model_loss_golden``)."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GOLDEN_DIR  # noqa: E402
from idvs.morec_amd import mae_engine, ops  # noqa: E402
from idvs.morec_amd.engine import DropCfg  # noqa: E402
from idvs.morec_amd.mae_engine import MaeShape  # noqa: E402
from idvs.morec_amd.model import MAE_Encoder, Model  # noqa: E402
from idvs.morec_amd.model.mae import HipViTMAEModel  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal, det_param  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
POS = "embeddings.position_embeddings"


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def froerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def load_det(module, prefix=""):
    """``det_param`` into every entry except the frozen position table (the container builds HF's sin-cos table itself)."""
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if not k.endswith(POS):
                v.copy_(torch.from_numpy(det_param(prefix + k, tuple(v.shape))))
    return module


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN_DIR, "g27_mae.npz"))


def _case(G, tag, dt, D=None):
    R0, ps, C, layers, heads, inter, n_img, D0 = (int(v) for v in G[f"{tag}.cfg"])
    shape = MaeShape(image_size=R0, patch_size=ps, hidden_size=C, num_hidden_layers=layers, num_attention_heads=heads,
                     intermediate_size=inter, mask_ratio=float(G[f"{tag}.mask_ratio"]))
    enc = MAE_Encoder(HipViTMAEModel(shape), D or D0, compute_dtype=DT[dt])
    load_det(enc, "cv_encoder.").to(DEV).eval()
    x = torch.from_numpy(det_normal(f"g27{tag}.x", (n_img, 3, R0, R0), std=1.0)).to(DEV)
    return shape, enc, x, n_img, D0


# ------------------------------------------------------------------------------------------------ encoder / model vs goldens
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["m17", "m50", "m65"])
def test_g27_mae_encoder_golden(G, tag, dt):
    """m17 (T = 17), m50 (T = 50: the production token count, N = 196 patches) and m65 (mask ratio 0, T = 65: one past the matrix-core
    attention kernels, every patch kept in shuffled order) under ``test_g11_vit_encoder_golden``'s bounds, its rule for the mathematically
    zero key-bias gradients included: what this side computes for them stays under 1e-6 (fp32) / 1e-2 (bf16).  g11 recognises such a
    gradient by the reference's value lying under 1e-7; here the reference's own rounding noise is max |.| = 1.4e-7 (m17), 5.6e-8 (m50),
    1.1e-7 (m65) in fp32 and still 4e-8 ... 6e-8 in its fp64 run (HF's eager softmax is fp32 whatever the model's type), so the key-bias
    gradient is recognised by its name and the reference's value is only required to be noise (under 1e-6)."""
    shape, enc, x, n_img, D = _case(G, tag, dt)
    noise = torch.from_numpy(G[f"{tag}.noise"]).to(DEV)
    assert torch.equal(enc.keep_ids(n_img, noise=noise).cpu(), torch.from_numpy(G[f"{tag}.keep"]))
    assert G[f"{tag}.keep"].shape[1] + 1 == {"m17": 17, "m50": 50, "m65": 65}[tag]
    R = torch.from_numpy(det_normal(f"g27{tag}.R", (n_img, D), std=1.0)).to(DEV)
    y = enc(x, noise=noise)
    e_y = relerr(y.detach().cpu().numpy(), G[f"{tag}.y"])
    print(f"g27 {tag} {dt}: y relerr {e_y:.2e}")
    assert e_y < (1e-4 if dt == "fp32" else 5e-2), e_y
    (y * R).sum().backward()
    worst = 0.0
    for n, p in enc.named_parameters():
        if n.endswith(POS):
            assert p.grad is None and not p.requires_grad
            continue
        ref = float(G[f"{tag}.grad_norm.cv_encoder.{n}"])
        got = float(p.grad.double().norm())
        worst = max(worst, abs(got - ref) / (ref + 1e-12)) if ref > 1e-6 else worst
        assert abs(got - ref) <= (2e-3 if dt == "fp32" else 8e-2) * ref + (1e-6 if dt == "fp32" else 1e-3), (n, got, ref)
    n_full = 0
    for k in G.files:
        if k.startswith(f"{tag}.grad."):
            n = k[len(f"{tag}.grad.cv_encoder."):]
            got = dict(enc.named_parameters())[n].grad.cpu().numpy()
            n_full += 1
            if n.endswith("k_proj.bias"):      # key-bias gradients are mathematically zero (softmax shift invariance)
                assert np.abs(G[k]).max() < 1e-6, (n, np.abs(G[k]).max())      # the reference's own value is rounding noise
                assert np.abs(got).max() < (1e-6 if dt == "fp32" else 1e-2), n
                continue
            e = froerr(got, G[k])
            print(f"g27 {tag} {dt}: {n} froerr {e:.2e}")
            assert e < (5e-4 if dt == "fp32" else 8e-2), (n, e)
    assert n_full == 6
    print(f"g27 {tag} {dt}: worst grad-norm err {worst:.2e}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_g27_mae_model_loss_golden(G, dt):
    """The reference ``Model`` over the micro MAE tower at g11's ``full`` configuration, under ``test_g11_vision_model_loss_golden``'s bounds."""
    S, D, item_num, B = (int(v) for v in G["full.cfg"])
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="mae_micro", compute_dtype=dt)
    m = Model(args, item_num, True, HipViTMAEModel(MaeShape.named("mae_micro")), G["full.pop"].tolist())
    load_det(m).to(DEV).eval()
    m.cv_encoder.noise = torch.from_numpy(G["full.noise"]).to(DEV)
    ids, log_mask = G["full.ids"], G["full.log_mask"]
    images = det_normal("g27f.images", (item_num + 1, 3, 32, 32), std=1.0).astype(np.float32)
    images[0] = 0.0
    px = torch.from_numpy(images[ids.reshape(-1)]).to(DEV)
    loss = m(torch.from_numpy(ids).view(-1).to(DEV), px, torch.from_numpy(log_mask).to(DEV), DEV)
    print(f"g27 full {dt}: loss {float(loss.detach()):.6f} (reference {float(G['full.loss']):.6f})")
    assert abs(float(loss.detach()) - float(G["full.loss"])) < (1e-3 if dt == "fp32" else 5e-2), (float(loss), float(G["full.loss"]))
    loss.backward()
    for n, p in m.named_parameters():
        if n.endswith(POS):
            assert p.grad is None
            continue
        ref = float(G[f"full.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert abs(got - ref) <= (3e-3 if dt == "fp32" else 1e-1) * ref + (1e-6 if dt == "fp32" else 1e-3), (n, got, ref)


# ------------------------------------------------------------------------------------------------ generated noise
def _full_inputs(G):
    S, D, item_num, B = (int(v) for v in G["full.cfg"])
    ids, log_mask = G["full.ids"], G["full.log_mask"]
    images = det_normal("g27f.images", (item_num + 1, 3, 32, 32), std=1.0).astype(np.float32)
    images[0] = 0.0
    return (torch.from_numpy(ids).view(-1).to(DEV), torch.from_numpy(images[ids.reshape(-1)]).to(DEV), torch.from_numpy(log_mask).to(DEV))


def _full_model(G, tower="modal", dt="fp32"):
    S, D, item_num, B = (int(v) for v in G["full.cfg"])
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 CV_model_load="mae_micro", compute_dtype=dt, item_tower=tower)
    m = Model(args, item_num, True, HipViTMAEModel(MaeShape.named("mae_micro")), G["full.pop"].tolist())
    return load_det(m).to(DEV)


def _step(m, inputs):
    m.zero_grad()
    loss = m(*inputs, DEV)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_generated_noise_training_step_is_a_function_of_the_seed(G):
    """Training mode without a noise argument, deterministic mode: the kept patches come from the step's dropout base seed, so the same
    seed gives the same loss and gradient bits, and another seed keeps other patches."""
    inputs = _full_inputs(G)
    n_img = inputs[1].shape[0]

    def run(seed):
        torch.manual_seed(seed)
        m = _full_model(G).train()
        out = _step(m, inputs)
        m._drop_calls = 0                      # the keep ids of the step that just ran: the same call counter, the same base seed
        keep = m.cv_encoder.keep_ids(n_img, m.dropout_cfgs()[0])
        return out + (keep,)

    ops.set_deterministic(True)
    try:
        (l0, g0, k0), (l1, g1, k1), (l2, _, k2) = run(7), run(7), run(8)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert set(g0) == set(g1) and "cv_encoder.image_net.embeddings.cls_token" in g0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert torch.equal(k0, k1) and not torch.equal(k0, k2)
    assert tuple(k0.shape) == (n_img, 16) and bool(torch.isfinite(l0)) and float(l0) != float(l2)


def test_eval_masking_repeats_and_follows_eval_mask_ratio(G):
    """Evaluation mode masks too (as the reference), from a fixed seed keyed by the row within the call: a pass repeats bit for bit;
    ``eval_mask_ratio = 0`` encodes from every patch."""
    _, enc, x, n_img, _ = _case(G, "m17", "bf16")
    with torch.no_grad():
        a, b = enc(x), enc(x)
        assert torch.equal(a, b)
        assert tuple(enc.keep_ids(n_img).shape) == (n_img, 16)
        assert torch.equal(enc.keep_ids(2)[0], enc.keep_ids(n_img)[0])     # row 0 of a call: the same mask whatever follows it
        enc.image_net.config.eval_mask_ratio = 0.0
        assert tuple(enc.keep_ids(n_img).shape) == (n_img, 64)
        c = enc(x)
        assert bool(torch.isfinite(c).all()) and not torch.equal(a, c)
        enc.train()
        assert tuple(enc.keep_ids(n_img).shape) == (n_img, 16)             # the training ratio is untouched


# ------------------------------------------------------------------------------------------------ relations that need no golden
def test_permuting_the_kept_set_leaves_the_tower_unchanged(G):
    """Mask ratio 0, fp32: with identity-ordered noise the tokens are the patches in raster order, with any other noise the same tokens
    in another order.  Attention is the only operator that mixes tokens, and without a mask it is symmetric in them: the [CLS] output can
    differ only by the order of its fp32 sums over the T = 65 keys (softmax denominator and P.V, each T terms: T . 2^-24 relative to the sum
    of magnitudes per sum), twice per layer over two layers, carried through LayerNorm / MLP Jacobians of order one -- bound
    32 . T . 2^-24 = 1.24e-4 of max |y| (2 layers x 2 sums x a factor 8 for the carry)."""
    shape, enc, x, n_img, _ = _case(G, "m65", "fp32")
    N = shape.num_patches
    ident = (torch.arange(N, dtype=torch.float64) / N).float().expand(n_img, N).contiguous().to(DEV)
    other = torch.from_numpy(G["m65.noise"]).to(DEV)
    assert torch.equal(enc.keep_ids(n_img, noise=ident).cpu(), torch.arange(N, dtype=torch.int32).expand(n_img, N))
    with torch.no_grad():
        y0, y1 = enc(x, noise=ident), enc(x, noise=other)
    e = relerr(y1.cpu().numpy(), y0.cpu().numpy())
    print(f"permuted kept set: relerr {e:.2e}")
    assert e <= 32 * 65 * 2.0 ** -24, e


def test_add_fusion_with_a_zero_id_table_is_the_plain_mae_model(G):
    """The a25 identity over the MAE tower: ``modal_add`` with a zero id table is the plain modal model, bit for bit (deterministic mode;
    both models draw the same masking noise: the same seed and call counter)."""
    inputs = _full_inputs(G)
    ops.set_deterministic(True)
    try:
        outs = []
        for tower in ("modal", "modal_add"):
            torch.manual_seed(11)
            m = _full_model(G, tower).train()
            if tower == "modal_add":
                with torch.no_grad():
                    m.id_embedding.weight.zero_()
                assert hasattr(m, "cv_encoder") and hasattr(m, "id_embedding")
            outs.append(_step(m, inputs))
    finally:
        ops.set_deterministic(False)
    (l0, g0), (l1, g1) = outs
    assert torch.equal(l0, l1), (float(l0), float(l1))
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_bce_model_step_over_the_mae_tower(G):
    """``BceModel`` (the ``bce_vision/main-end2end`` form: positives and one negative per slot, ``[B, S + 1, 2, 3, R, R]`` pixels) over the
    MAE tower, training mode, deterministic mode: the loss is finite, the gradient reaches the patch projection, the same seed repeats
    the loss and every gradient bit, and another seed (other kept patches) gives another loss."""
    from idvs.morec_amd.model import BceModel
    S, D, item_num, B = (int(v) for v in G["full.cfg"])
    ids, log_mask = G["full.ids"], G["full.log_mask"]
    images = det_normal("g27f.images", (item_num + 1, 3, 32, 32), std=1.0).astype(np.float32)
    images[0] = 0.0
    pairs = np.stack([ids, np.where(ids > 0, (ids + 7) % item_num + 1, 0)], axis=-1)                 # [B, S + 1, 2]
    px = torch.from_numpy(images[pairs.reshape(-1)]).view(B, S + 1, 2, 3, 32, 32).to(DEV)
    lm = torch.from_numpy(log_mask).to(DEV)

    def run(seed):
        torch.manual_seed(seed)
        args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                     CV_model_load="mae_micro", compute_dtype="fp32")
        m = load_det(BceModel(args, item_num, True, HipViTMAEModel(MaeShape.named("mae_micro")))).to(DEV).train()
        m.zero_grad()
        loss = m(px, lm, DEV)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    ops.set_deterministic(True)
    try:
        (l0, g0), (l1, g1), (l2, _) = run(3), run(3), run(4)
    finally:
        ops.set_deterministic(False)
    assert bool(torch.isfinite(l0)) and torch.equal(l0, l1) and float(l0) != float(l2)
    assert "cv_encoder.cv_proj.weight" in g0 and "cv_encoder.image_net.embeddings.cls_token" in g0
    assert float(g0["cv_encoder.image_net.embeddings.patch_embeddings.projection.weight"].abs().max()) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_features_only_is_the_input_of_cv_proj(G, dt):
    """``features_only`` returns the normalised [CLS] rows: ``GELU(cv_proj(features))`` formed by torch in fp64 from them is the item vector."""
    shape, enc, x, n_img, D = _case(G, "m50", dt)
    noise = torch.from_numpy(G["m50.noise"]).to(DEV)
    p = dict(enc.named_parameters())
    with torch.no_grad():
        prep = mae_engine.mae_prepare(p, shape, DT[dt], "", features_only=True)
        feats, saved = mae_engine.mae_forward(p, prep, shape, x, DT[dt], False, "", noise=noise, features_only=True)
        y = enc(x, noise=noise)
    assert saved is None and tuple(feats.shape) == (n_img, shape.hidden_size) and feats.dtype == DT[dt]
    w = enc.cv_proj.weight.detach().to(DT[dt]).double()
    want = torch.nn.functional.gelu(feats.double() @ w.t() + enc.cv_proj.bias.detach().double())
    # fp32: the 64-term fp32 dot products and the kernel's erf (1.5e-7 absolute); bf16: one rounding of the output (2^-9 relative)
    assert relerr(y.cpu().numpy(), want.cpu().numpy()) < (1e-5 if dt == "fp32" else 2.0 ** -8)


def test_extract_item_features_over_the_mae_tower(G):
    from idvs.morec_amd.data_utils import extract_item_features
    _, enc, x, n_img, _ = _case(G, "m17", "bf16")
    table = extract_item_features(enc, x.cpu(), 2, DEV)
    assert tuple(table.shape) == (n_img, 64) and table.dtype == torch.float32 and bool(torch.isfinite(table).all())
    assert torch.equal(table, extract_item_features(enc, x.cpu(), 2, DEV))


# ------------------------------------------------------------------------------------------------ driver
_DRIVER = r"""
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
common = {common!r}
run.main(common)
print("=== TEST RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"])
print("=== STAGE 1 ===", file=sys.stderr, flush=True)
run.main({stage1!r})
"""


def test_run_driver_mae_micro(tmp_path):
    """``run.py --item_tower modal --CV_model_load mae_micro --synthetic 48`` in a fresh child process: one short epoch with its
    validation and checkpoint (directory label = the vision rule: ``CV_model_load``), ``--mode test`` on it, then stage 1 of
    ``--arch two_stage`` over the same tower with ``--save_features``."""
    feats = str(tmp_path / "features.npy")
    base = ["--item_tower", "modal", "--CV_model_load", "mae_micro", "--CV_resize", "32", "--synthetic", "48", "--synthetic_items", "60",
            "--epoch", "1", "--embedding_dim", "64", "--batch_size", "16", "--max_seq_len", "5", "--lr", "1e-3", "--fine_tune_lr", "1e-4",
            "--freeze_paras_before", "0", "--compute_dtype", "bf16", "--collate_workers", "0", "--local_rank", "0"]
    common = base + ["--checkpoint_root", str(tmp_path / "a")]
    stage1 = base + ["--arch", "two_stage", "--max_steps", "2", "--save_features", feats, "--checkpoint_root", str(tmp_path / "b")]
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, common=common, stage1=stage1)], cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    train_log, rest = res.stderr.split("=== TEST RUN ===")
    test_log, stage_log = rest.split("=== STAGE 1 ===")
    assert re.search(r"epoch 1: \d+ steps, mean loss [0-9.]+", train_log)
    assert "valid_methods   Hit10\tnDCG10" in train_log and re.search(r"valid_results   [0-9.]+\t[0-9.]+", train_log)
    saved = re.findall(r"Model saved to (\S+)", train_log)
    assert saved and "mae_micro" in saved[-1] and str(tmp_path) in saved[-1]
    assert "model loaded from" in test_log and re.search(r"test_results   [0-9.]+\t[0-9.]+", test_log)
    assert "stage 1" in stage_log and os.path.exists(feats)
    table = np.load(feats)
    assert table.shape == (61, 64) and table.dtype == np.float32 and np.isfinite(table).all()
