"""-m gpu: the OPT text tower (causal pre-LN decoder, masked mean pooling) at model level.
  * g30 (``tests/golden/g30_opt.npz``: the installed HF ``OPTModel`` inside the reference's in-batch ``Model`` and its BCE ``Model``) under the
    bounds ``test_roberta_gpu.py`` takes from g5 for the same graph at the same size, with its ``twin_bound`` rule, in the padded and the
    packed layout; every encoder gradient is compared.  One gradient is exactly zero in exact arithmetic -- the key bias adds a per-row
    constant to the scores, which the softmax removes -- so the reference holds rounding noise there (its fp64 twin: below 1e-12 of the
    query bias's) and a relative error has no meaning: the tower's value must be exactly 0 instead.
  * the holes case against its stored encoder output and HF's position ids; padded against packed; dropout repeatability, and a pass
    with hidden dropout against an fp64 restatement under the library's masks; a frozen parameter prefix; ``from_hf`` of the installed
    micro ``OPTModel``; one short driver run per mode that reaches the tower."""
import json
import logging
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GOLDEN_DIR  # noqa: E402
from idvs.morec_amd import ops  # noqa: E402
from idvs.morec_amd.model import HipOPTModel, Model, OptShape, Text_Encoder_mean  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal, det_param  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
G = np.load(os.path.join(GOLDEN_DIR, "g30_opt.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g30_opt_keys.json")))
TE = "bert_encoder.text_encoders.title."
PE = TE + "bert_model.decoder.embed_positions.weight"
WE = TE + "bert_model.decoder.embed_tokens.weight"


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def make_args(**kw):
    d = dict(max_seq_len=20, embedding_dim=64, num_attention_heads=2, drop_rate=0.0, transformer_block=2, num_words_title=30,
             num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="opt_micro", word_embedding_dim=64,
             compute_dtype="fp32")
    d.update(kw)
    return types.SimpleNamespace(**d)


def load_det(module):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    return module


def twin_bound(bound, key, scale=1.0):
    """``test_roberta_gpu.twin_bound`` over g30: if the reference's own fp32 error against its fp64 run exceeds half the bound, the bound
    becomes four times that error.  ``scale`` turns an absolute error into the bound's units."""
    err = float(np.abs(np.asarray(G[key], np.float64) - G[key + ".64"]).max()) / scale
    return 4 * err if err > bound / 2 else bound


def set_layout(model, layout):
    model.bert_encoder.text_encoders["title"].unpad = layout == "packed"


def g30_model(dtype, cls=Model):
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    args = make_args(max_seq_len=S, embedding_dim=D, compute_dtype=dtype, num_words_title=T)
    bert = HipOPTModel(OptShape.named("opt_micro"))
    m = cls(args, item_num, True, bert, G["pop"]) if cls is Model else cls(args, item_num, True, bert)
    return load_det(m).to(DEV).eval()


def is_zero_in_exact_arithmetic(name):
    return name.endswith("self_attn.k_proj.bias")


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_g30_opt_micro_golden(dtype, layout):
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    m = g30_model(dtype)
    set_layout(m, layout)
    ids = torch.from_numpy(G["ids"]).to(DEV).view(-1)
    items = torch.from_numpy(G["content"][G["ids"].reshape(-1)]).to(DEV)
    lm = torch.from_numpy(G["log_mask"]).to(DEV)
    f32 = dtype == "fp32"
    vec = m.bert_encoder(items)
    assert vec.dtype == torch.float32 and np.isfinite(vec.detach().cpu().numpy()).all()
    vmax = float(np.abs(G["item_vecs"]).max())
    tol_vec = twin_bound(2e-5, "item_vecs", vmax) if f32 else 5e-2
    e_vec = relerr(vec.detach().cpu().numpy(), G["item_vecs"])      # every slot, the padding item's included: its vector is GELU(fc.bias)
    print(f"g30 {dtype} {layout}: item vec err {e_vec:.2e} (bound {tol_vec:.1e}; reference fp32 vs fp64 "
          f"{float(np.abs(G['item_vecs'] - G['item_vecs.64']).max()) / vmax:.2e})")
    assert e_vec < tol_vec
    R = torch.from_numpy(det_normal("g30.R", (B * (S + 1), D))).to(DEV)
    (vec * R).sum().backward()
    named = dict(m.named_parameters())
    gt = 3e-4 if f32 else 1e-1
    errs = {}
    for k in [k for k in G.files if k.startswith("enc_grad.") and not k.endswith(".64")]:
        name = k[len("enc_grad."):]
        got = named[name].grad
        assert got is not None and bool(torch.isfinite(got).all()), name
        if is_zero_in_exact_arithmetic(name):
            qb = np.abs(G["enc_grad." + name.replace("k_proj", "q_proj") + ".64"]).max()
            assert np.abs(G[k + ".64"]).max() < 1e-12 * qb      # the fp64 twin says so too
            assert float(got.abs().max()) == 0.0, name
            continue
        errs[name] = relerr(got.cpu().numpy(), G[k])
    print(f"g30 {dtype} {layout}: enc grad errs {({k[len(TE):]: f'{v:.1e}' for k, v in errs.items()})}")
    assert len(errs) == len(KEYS["parameters"]) + 2 - 2      # every encoder parameter and fc, minus the two key biases
    assert max(errs.values()) < gt, {k: v for k, v in errs.items() if v >= gt}
    assert float(named[PE].grad[:2].abs().max()) == 0.0      # row 1 = the masked tokens' row, row 0 is never read: no gradient
    assert float(named[PE].grad[2 + T:].abs().max()) == 0.0
    assert float(named[WE].grad[1].abs().max()) == 0.0       # padding_idx, whatever the mask says (item 7, in the batch, has an id 1 inside)
    for k in [k for k in G.files if k.startswith("enc_grad_norm.") and not k.endswith(".64")]:
        name = k[len("enc_grad_norm."):]
        got = named[name].grad.double().norm().item()
        assert abs(got - float(G[k])) <= (1e-3 if f32 else 1e-1) * float(G[k]) + (1e-4 if f32 else 2e-2), (name, got, float(G[k]))
    m.zero_grad()
    loss = m(ids, items, lm, DEV)
    print(f"g30 {dtype} {layout}: loss {loss.item():.6f} vs {float(G['loss']):.6f} (fp64 {float(G['loss.64']):.6f})")
    assert np.isfinite(loss.item())
    assert abs(loss.item() - float(G["loss"])) < (twin_bound(5e-5, "loss") if f32 else 3e-2)
    loss.backward()
    for k in [k for k in G.files if k.startswith("grad_norm.") and not k.endswith(".64")]:
        name = k[len("grad_norm."):]
        got = named[name].grad.double().norm().item()
        assert np.isfinite(got)
        assert abs(got - float(G[k])) <= (1e-3 if f32 else 1e-1) * float(G[k]) + (1e-4 if f32 else 2e-2), (name, got, float(G[k]))
    assert float(named[PE].grad[:2].abs().max()) == 0.0 and float(named[PE].grad[2 + T:].abs().max()) == 0.0


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_g30_bce_model_golden(dt, layout):
    from idvs.morec_amd.model.bce import BceModel
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    m = g30_model(dt, BceModel)
    set_layout(m, layout)
    x = torch.from_numpy(G["content"][G["bce.items"]]).view(-1, 2 * T).cuda()
    loss = m(x, torch.from_numpy(G["bce.log_mask"]).cuda(), "cuda")
    ref = float(G["bce.loss"])
    print(f"g30 bce {dt} {layout}: loss {float(loss.detach()):.6f} vs {ref:.6f} (fp64 {float(G['bce.loss.64']):.6f})")
    assert abs(float(loss.detach()) - ref) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(ref)), (float(loss.detach()), ref)
    loss.backward()
    for n, p in m.named_parameters():
        r = float(G[f"bce.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert np.isfinite(got)
        assert abs(got - r) <= (2e-3 if dt == "fp32" else 1e-1) * r + (1e-6 if dt == "fp32" else 2e-2), (n, got, r)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_padding_item_vector_is_gelu_of_the_bias(dtype):
    """A title whose mask is all zero pools to ``mean = 0``: its vector is ``GELU(fc.bias)``, in both layouts, whatever its ids."""
    T = int(G["cfg"][2])
    m = g30_model(dtype)
    te = m.bert_encoder.text_encoders["title"]
    rows = np.zeros((3, 2 * T), dtype=np.int64)
    rows[1, :T] = 1
    rows[2, :T] = np.arange(3, 3 + T)
    want = torch.nn.functional.gelu(te.fc.bias.detach().double()).cpu().numpy()
    # fp32: the kernels' erf is within 1.5e-7 of the exact one (csrc/common.hpp), |bias| < 1, plus the rounding of the result;
    # bf16: the bias sum and the result are each rounded to 8 bits
    tol = 1e-6 if dtype == "fp32" else 2.0 ** -7 * max(1.0, float(np.abs(want).max()))
    for layout in ("padded", "packed"):
        set_layout(m, layout)
        got = m.bert_encoder(torch.from_numpy(np.concatenate((rows, G["content"][5:7]))).to(DEV)).detach().cpu().numpy()
        assert np.isfinite(got).all()
        assert np.abs(got[:3] - want[None, :]).max() < tol
        assert (got[0] == got[1]).all() and (got[0] == got[2]).all()
        if dtype == "fp32":
            assert np.abs(got[0] - G["table_vecs"][0]).max() < 1e-6


def test_holes_case_and_position_ids():
    T = int(G["cfg"][2])
    n_pos = OptShape.named("opt_micro").num_positions
    for text, want in ((G["content"], G["position_ids"]), (G["holes.content"], G["holes.position_ids"])):
        mask32 = torch.from_numpy(text[:, T:]).to(torch.int32).contiguous().view(-1).to(DEV)
        pos_ids, _, _ = ops.mask_pos_ids(mask32, T, 2, n_pos)
        assert np.array_equal(pos_ids.cpu().numpy().reshape(-1, T), want)
    m = g30_model("fp32")
    hol = torch.from_numpy(G["holes.content"]).to(DEV)
    vmax = float(np.abs(G["holes.vecs"]).max())
    tol = twin_bound(2e-5, "holes.vecs", vmax)
    for layout in ("padded", "packed"):      # masks with holes keep the padded layout whatever is asked for
        set_layout(m, layout)
        got = m.bert_encoder(hol).detach().cpu().numpy()
        e = relerr(got, G["holes.vecs"])
        print(f"g30 holes {layout}: err {e:.2e} (bound {tol:.1e})")
        assert np.isfinite(got).all() and e < tol
    set_layout(m, "padded")
    a = m.bert_encoder(hol)
    set_layout(m, "packed")
    assert torch.equal(a, m.bert_encoder(hol))
    # the gradient of a masked-out row is exactly zero: a word row that only masked tokens name gets none
    m.zero_grad()
    text = G["holes.content"].copy()
    masked = text[:, T:] == 0
    text[:, :T][masked] = 79      # an id no kept token has
    text[:, :T][~masked] = np.minimum(text[:, :T][~masked], 78)
    set_layout(m, "padded")
    m.bert_encoder(torch.from_numpy(text).to(DEV)).square().sum().backward()
    named = dict(m.named_parameters())
    assert float(named[WE].grad[79].abs().max()) == 0.0 and float(named[WE].grad[2].abs().max()) > 0
    assert float(named[PE].grad[:2].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_padded_against_packed(dtype):
    m = g30_model(dtype)
    table = torch.from_numpy(G["content"]).to(DEV)
    set_layout(m, "padded")
    a = m.bert_encoder(table).detach().cpu().numpy()
    set_layout(m, "packed")
    b = m.bert_encoder(table).detach().cpu().numpy()
    e = relerr(b[1:], a[1:])
    print(f"padded vs packed {dtype}: {e:.2e}")
    assert e < (2e-5 if dtype == "fp32" else 5e-2)
    if dtype == "fp32":
        assert relerr(a, G["table_vecs"]) < twin_bound(2e-5, "table_vecs", float(np.abs(G["table_vecs"]).max()))


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_dropout_repeats_with_the_seed(layout):
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    ids = torch.from_numpy(G["ids"]).to(DEV).view(-1)
    items = torch.from_numpy(G["content"][G["ids"].reshape(-1)]).to(DEV)
    lm = torch.from_numpy(G["log_mask"]).to(DEV)
    saved = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        runs = []
        for seed in (11, 11, 12):
            torch.manual_seed(seed)
            args = make_args(max_seq_len=S, embedding_dim=D, compute_dtype="bf16", num_words_title=T, drop_rate=0.1)
            m = load_det(Model(args, item_num, True, HipOPTModel(OptShape.named("opt_micro"), dropout=0.1, attention_dropout=0.1), G["pop"]))
            m = m.to(DEV).train()
            set_layout(m, layout)
            loss = m(ids, items, lm, DEV)
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    finally:
        ops.set_deterministic(saved)
    (l0, g0), (l1, g1), (l2, g2) = runs
    assert bool(torch.isfinite(l0)) and all(bool(torch.isfinite(g).all()) for g in g0.values())
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert not torch.equal(l0, l2)
    m.eval()
    assert not torch.equal(m(ids, items, lm, DEV).detach(), l2)      # the masks did something


def _opt_fp64(p, shape, ids, mask, masks):
    """fp64 torch restatement of ``Text_Encoder_mean`` over OPT (names without prefix); ``masks[l] = (attention sub-layer, FFN)``: the
    scaled keep masks [N * T, H] of layer l's two hidden dropouts."""
    F = torch.nn.functional
    dec = "bert_model.decoder."
    N, T = ids.shape
    H, heads = shape.hidden_size, shape.num_attention_heads
    dh = H // heads
    pos = torch.cumsum(mask, 1) * mask - 1 + 2
    x = F.embedding(ids, p[dec + "embed_tokens.weight"], padding_idx=1) + p[dec + "embed_positions.weight"][pos]      # row 1: no gradient
    allowed = torch.tril(torch.ones(T, T, dtype=torch.bool, device=ids.device))[None, None] & (mask != 0)[:, None, None, :]
    add = torch.where(allowed, 0.0, torch.finfo(torch.float32).min).double()
    for l in range(shape.num_hidden_layers):
        L = dec + f"layers.{l}."
        h = F.layer_norm(x, (H,), p[L + "self_attn_layer_norm.weight"], p[L + "self_attn_layer_norm.bias"], 1e-5)
        q, k, v = (F.linear(h, p[L + f"self_attn.{n}.weight"], p[L + f"self_attn.{n}.bias"]).view(N, T, heads, dh).transpose(1, 2)
                   for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5 + add, -1) @ v
        o = F.linear(a.transpose(1, 2).reshape(N, T, H), p[L + "self_attn.out_proj.weight"], p[L + "self_attn.out_proj.bias"])
        x = x + o * masks[l][0].view(N, T, H)
        h = F.layer_norm(x, (H,), p[L + "final_layer_norm.weight"], p[L + "final_layer_norm.bias"], 1e-5)
        f = F.linear(torch.relu(F.linear(h, p[L + "fc1.weight"], p[L + "fc1.bias"])), p[L + "fc2.weight"], p[L + "fc2.bias"])
        x = x + f * masks[l][1].view(N, T, H)
    y = F.layer_norm(x, (H,), p[dec + "final_layer_norm.weight"], p[dec + "final_layer_norm.bias"], 1e-5)
    me = (mask != 0).double().unsqueeze(-1)
    mean = (y * me).sum(1) / me.sum(1).clamp(min=1e-9)
    return F.gelu(F.linear(mean, p["fc.weight"], p["fc.bias"]))


def test_hidden_dropout_against_fp64_with_the_same_masks():
    """Forward and every gradient of a training-mode pass (hidden dropout 0.25, padded layout, fp32) against the fp64 restatement under
    the masks the library reports (``ops.dropout_keep_mask`` at the sites ``opt_forward`` documents), under g5's fp32 bounds."""
    from idvs.morec_amd.engine import DropCfg
    T = int(G["cfg"][2])
    shape, p_drop = OptShape.named("opt_micro"), 0.25
    enc = load_det(Text_Encoder_mean(HipOPTModel(shape), 64, 64, torch.float32)).to(DEV).train()
    enc.unpad = False
    text = torch.from_numpy(G["content"][:12]).to(DEV)
    drop = DropCfg(p_drop, 0.0, 0x0123456789ABCDEF)
    R = torch.from_numpy(det_normal("g30.R", (12, 64))).to(DEV)
    out = enc.encode(text, drop)
    (out * R).sum().backward()
    inv_keep = 1.0 / (1.0 - int(p_drop * 65536) / 65536.0)
    n = 12 * T * shape.hidden_size
    masks = [tuple(ops.dropout_keep_mask(n, p_drop, drop.site(s + 3 * l)).double() * inv_keep for s in (2, 3))
             for l in range(shape.num_hidden_layers)]
    assert all(0.6 < float((mk > 0).double().mean()) < 0.9 for pair in masks for mk in pair)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in enc.named_parameters()}
    ref = _opt_fp64(p64, shape, text[:, :T], text[:, T:], masks)
    (ref * R.double()).sum().backward()
    errs = {"out": relerr(out.detach().cpu().numpy(), ref.detach().cpu().numpy())}
    for k, v in enc.named_parameters():
        if is_zero_in_exact_arithmetic(k):
            assert float(v.grad.abs().max()) == 0.0
            continue
        errs[k] = relerr(v.grad.cpu().numpy(), p64[k].grad.cpu().numpy())
    print("OPT tower with hidden dropout vs fp64:", {k: f"{v:.1e}" for k, v in errs.items()})
    assert errs["out"] < 2e-5 and max(errs.values()) < 3e-4, {k: v for k, v in errs.items() if v >= 3e-4}


@pytest.mark.parametrize("n_frozen", [2, 4, 20, 36])
def test_frozen_prefix_leaves_the_other_gradients_unchanged(n_frozen):
    """``--freeze_paras_before n``: the backward ends at the lowest trainable layer (2: the tables, 4: + the decoder-level LayerNorm,
    which sits above the layers; 20: + layer 0; 36: all of ``bert_model``), and what still trains gets the bits of the full pass."""
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    items = torch.from_numpy(G["content"][G["ids"].reshape(-1)]).to(DEV)
    R = torch.from_numpy(det_normal("g30.R", (B * (S + 1), D))).to(DEV)
    saved = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        grads = []
        for frozen in (0, n_frozen):
            m = g30_model("bf16")
            for i, (_, q) in enumerate(m.bert_encoder.text_encoders["title"].bert_model.named_parameters()):
                q.requires_grad = i >= frozen
            (m.bert_encoder(items) * R).sum().backward()
            torch.cuda.synchronize()
            grads.append({k: q.grad for k, q in m.bert_encoder.named_parameters()})
    finally:
        ops.set_deterministic(saved)
    full, part = grads
    names = list(full)
    assert all(part[k] is None for k in names[:n_frozen]) and all(part[k] is not None for k in names[n_frozen:])
    for k in names[n_frozen:]:
        assert torch.equal(part[k], full[k]), k


def test_from_hf_of_the_installed_micro_model():
    from transformers import OPTConfig, OPTModel
    torch.manual_seed(3)
    hf = OPTModel(OPTConfig(attn_implementation=KEYS["attn_implementation"], dropout=0.0, attention_dropout=0.0, **KEYS["config"])).eval()
    m = HipOPTModel.from_hf(hf)
    assert [[k, list(p.shape)] for k, p in m.named_parameters()] == [[k, list(s)] for k, s in KEYS["parameters"]]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in hf.named_parameters()]
    T = int(G["cfg"][2])
    text = torch.from_numpy(G["content"][1:])
    ids, mask = text[:, :T], text[:, T:]
    with torch.no_grad():
        hidden = hf(input_ids=ids, attention_mask=mask)[0]
        me = mask.unsqueeze(-1).float()
        want = ((hidden * me).sum(1) / me.sum(1).clamp(min=1e-9)).numpy()
    enc = Text_Encoder_mean(m, 64, 64, torch.float32).to(DEV).eval()
    for unpad in (False, True):
        enc.unpad = unpad
        got = enc.encode(text.to(DEV), features_only=True).float().cpu().numpy()
        e = relerr(got, want)
        print(f"from_hf forward (unpad={unpad}): {e:.2e}")
        assert got.shape == want.shape and e < 2e-5


# ------------------------------------------------------------------------------------------------------------------------------------
class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _main(argv):
    from idvs.morec_amd import run
    h = _Lines()
    run.Log.addHandler(h)
    run.Log.setLevel(logging.INFO)
    try:
        run.main(argv)
    finally:
        run.Log.removeHandler(h)
    return "\n".join(h.lines)


def _mean_loss(log):
    mt = re.search(r"epoch 1: \d+ steps, mean loss ([0-9.]+)", log)
    assert mt, log[-2000:]
    assert np.isfinite(float(mt.group(1)))
    return float(mt.group(1))


SMOKE = ["--synthetic", "48", "--synthetic_items", "60", "--bert_model_load", "opt_micro", "--freeze_paras_before", "0", "--batch_size", "16",
         "--embedding_dim", "64", "--max_seq_len", "6", "--lr", "1e-3", "--fine_tune_lr", "1e-4", "--local_rank", "0", "--epoch", "1",
         "--num_workers", "0"]


def test_driver_train_then_test(tmp_path):
    common = SMOKE + ["--item_tower", "modal", "--checkpoint_root", str(tmp_path)]
    log = _main(common + ["--max_steps", "3"])
    _mean_loss(log)
    assert "valid_results" in log
    assert re.search(r"test_results   [0-9.]+\t[0-9.]+", _main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"]))


def test_driver_bce_loss(tmp_path):
    _mean_loss(_main(SMOKE + ["--item_tower", "modal", "--loss", "bce", "--max_steps", "3", "--checkpoint_root", str(tmp_path)]))


def test_driver_fusion_tower(tmp_path):
    _mean_loss(_main(SMOKE + ["--item_tower", "modal_cat", "--loss", "bce", "--max_steps", "3", "--checkpoint_root", str(tmp_path)]))


def test_driver_two_stage_stage1_saves_the_pooled_mean(tmp_path):
    from idvs.morec_amd import run
    shape = OptShape.named("opt_micro")
    torch.manual_seed(21)
    tower = HipOPTModel(shape)
    (tmp_path / "opt_micro").mkdir()
    torch.save(tower.state_dict(), str(tmp_path / "opt_micro" / "pytorch_model.bin"))
    feats = str(tmp_path / "features.npy")
    log = _main(SMOKE + ["--arch", "two_stage", "--item_tower", "modal", "--save_features", feats, "--checkpoint_root", str(tmp_path),
                         "--pretrained_dir", str(tmp_path)])
    assert "stage 1" in log
    _mean_loss(log)
    table = np.load(feats)
    assert table.shape == (61, 64) and np.isfinite(table).all() and float(np.abs(table[1:]).max()) > 0
    assert float(np.abs(table[0]).max()) == 0.0      # the padding item pools to zero
    _, content, *_ = run.synthetic_dataset(48, 60, 6, 30, vocab=shape.vocab_size, opt=True)
    dt = table.dtype
    enc = Text_Encoder_mean(tower, 64, 64, torch.float16).to(DEV).eval()      # fp16: the driver's default --compute_dtype
    want = enc.encode(torch.from_numpy(content).to(DEV), features_only=True).float().cpu().numpy().astype(dt)
    assert np.array_equal(table, want)


@pytest.mark.parametrize("extra,word", [(["--fused_step"], "--fused_step"), (["--fused_step", "--graph"], "--fused_step"),
                                        (["--graph"], "--graph"), (["--arch", "dssm"], "--arch dssm")])
def test_driver_modes_that_exit_naming_opt(tmp_path, extra, word):
    with pytest.raises(SystemExit) as e:
        _main(SMOKE + ["--item_tower", "modal", "--max_steps", "1", "--checkpoint_root", str(tmp_path)] + extra)
    assert "OPT" in str(e.value) and word in str(e.value)
