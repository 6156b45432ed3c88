"""-m gpu: the DeBERTa text tower (disentangled attention) at model level.
  * g31 (``tests/golden/g31_deberta.npz``: the installed HF ``DebertaModel`` inside the reference's in-batch ``Model``, its BCE ``Model`` and
    its DSSM ``Model``) under the bounds ``test_roberta_gpu.py`` / ``test_opt_gpu.py`` take from g5 for the same graph at the same size, with
    their ``twin_bound`` rule unchanged: where the reference's own fp32 error against its fp64 run exceeds half the bound, the bound becomes
    four times that error.  (The kernels scale the score sum once, HF divides q and PQ before the products: sqrt(3 dh) is no power of two,
    so the two orders differ in the last bit, which is what the rule absorbs.)  Item vectors -- the padding item's included: every score of
    an all-masked title is replaced by the fill value, a uniform average --, loss and every encoder gradient are compared.
  * ``rel_embeddings.grad`` outside rows P-T+1 .. P+T-1 is exactly zero; a frozen parameter prefix changes no trainable gradient's bits and
    no dPK / dPQ is formed where nothing needs it; ``from_hf`` of the installed micro model; one short driver run per mode."""
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
from idvs.morec_amd.model import DebertaShape, HipDebertaModel, Model, Text_Encoder  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal, det_param  # noqa: E402

DEV = "cuda"
G = np.load(os.path.join(GOLDEN_DIR, "g31_deberta.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g31_deberta_keys.json")))
TE = "bert_encoder.text_encoders.title."
REL = TE + "bert_model.encoder.rel_embeddings.weight"
DTYPES = ["fp32", "bf16", "fp16"]


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def make_args(**kw):
    d = dict(max_seq_len=20, embedding_dim=64, num_attention_heads=2, drop_rate=0.0, transformer_block=2, num_words_title=30,
             num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="deberta_micro", word_embedding_dim=64,
             compute_dtype="fp32", item_tower="modal", num_workers=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def load_det(module):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    return module


def twin_err(key, scale=1.0):
    """The reference's own fp32 error against its fp64 run, in units of ``scale``."""
    if key.startswith("enc_grad."):
        d = G["enc_grad_twin_minus_fp32." + key[len("enc_grad."):]]
    else:
        d = np.asarray(G[key], np.float64) - G[key + ".64"]
    return float(np.abs(d).max()) / scale


def twin_bound(bound, key, scale=1.0):
    """``test_opt_gpu.twin_bound`` over g31: if the reference's own fp32 error against its fp64 run exceeds half the bound, the bound
    becomes four times that error.  ``scale`` turns an absolute error into the bound's units."""
    err = twin_err(key, scale)
    return 4 * err if err > bound / 2 else bound


def tower():
    return HipDebertaModel(DebertaShape.named("deberta_micro"), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def g31_model(dtype, cls=Model):
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    args = make_args(max_seq_len=S, embedding_dim=D, compute_dtype=dtype, num_words_title=T)
    m = cls(args, item_num, True, tower(), G["pop"]) if cls is Model else cls(args, item_num, True, tower())
    return load_det(m).to(DEV).eval()


@pytest.mark.parametrize("dtype", DTYPES)
def test_g31_deberta_micro_golden(dtype):
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    m = g31_model(dtype)
    ids = torch.from_numpy(G["ids"]).to(DEV).view(-1)
    items = torch.from_numpy(G["content"][G["ids"].reshape(-1)]).to(DEV)
    lm = torch.from_numpy(G["log_mask"]).to(DEV)
    f32 = dtype == "fp32"
    vec = m.bert_encoder(items)
    assert vec.dtype == torch.float32 and np.isfinite(vec.detach().cpu().numpy()).all()
    vmax = float(np.abs(G["item_vecs"]).max())
    tol_vec = twin_bound(2e-5, "item_vecs", vmax) if f32 else 5e-2
    e_vec = relerr(vec.detach().cpu().numpy(), G["item_vecs"])      # every slot, the padding item's (the left padding of the batch) included
    print(f"g31 {dtype}: item vec err {e_vec:.2e} (bound {tol_vec:.1e}; reference fp32 vs fp64 {twin_err('item_vecs', vmax):.2e})")
    assert e_vec < tol_vec
    R = torch.from_numpy(det_normal("g31.R", (B * (S + 1), D))).to(DEV)
    (vec * R).sum().backward()
    named = dict(m.named_parameters())
    errs, bounds = {}, {}
    for k in [k for k in G.files if k.startswith("enc_grad.")]:
        name = k[len("enc_grad."):]
        got = named[name].grad
        assert got is not None and bool(torch.isfinite(got).all()), name
        errs[name] = relerr(got.cpu().numpy(), G[k])
        bounds[name] = twin_bound(3e-4, k, float(np.abs(G[k]).max())) if f32 else 1e-1
    print(f"g31 {dtype}: enc grad err / bound " + str({k[len(TE):]: f"{v:.1e}/{bounds[k]:.1e}" for k, v in errs.items()}))
    assert len(errs) == len(KEYS["parameters"]) + 2      # every encoder parameter and fc
    assert all(errs[k] < bounds[k] for k in errs), {k: (v, bounds[k]) for k, v in errs.items() if v >= bounds[k]}
    P = DebertaShape.named("deberta_micro").rel_positions
    g_rel = named[REL].grad
    assert float(g_rel[:P - T + 1].abs().max()) == 0.0 and float(g_rel[P + T:].abs().max()) == 0.0      # d = 0 never occurs
    assert float(g_rel[P - T + 1:P + T].abs().max(1).values.min()) > 0
    for k in [k for k in G.files if k.startswith("enc_grad_norm.") and not k.endswith(".64")]:
        name = k[len("enc_grad_norm."):]
        got = named[name].grad.double().norm().item()
        assert abs(got - float(G[k])) <= (1e-3 if f32 else 1e-1) * float(G[k]) + (1e-4 if f32 else 2e-2), (name, got, float(G[k]))
    m.zero_grad()
    loss = m(ids, items, lm, DEV)
    tol_loss = twin_bound(5e-5, "loss") if f32 else 3e-2
    print(f"g31 {dtype}: loss {loss.item():.6f} vs {float(G['loss']):.6f} (fp64 {float(G['loss.64']):.6f}; bound {tol_loss:.1e})")
    assert np.isfinite(loss.item())
    assert abs(loss.item() - float(G["loss"])) < tol_loss
    loss.backward()
    for k in [k for k in G.files if k.startswith("grad_norm.") and not k.endswith(".64")]:
        name = k[len("grad_norm."):]
        got = named[name].grad.double().norm().item()
        assert np.isfinite(got)
        assert abs(got - float(G[k])) <= (1e-3 if f32 else 1e-1) * float(G[k]) + (1e-4 if f32 else 2e-2), (name, got, float(G[k]))


@pytest.mark.parametrize("dt", DTYPES)
def test_g31_bce_model_golden(dt):
    from idvs.morec_amd.model.bce import BceModel
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    m = g31_model(dt, BceModel)
    x = torch.from_numpy(G["content"][G["bce.items"]]).view(-1, 2 * T).cuda()
    loss = m(x, torch.from_numpy(G["bce.log_mask"]).cuda(), "cuda")
    ref = float(G["bce.loss"])
    print(f"g31 bce {dt}: loss {float(loss.detach()):.6f} vs {ref:.6f} (fp64 {float(G['bce.loss.64']):.6f})")
    assert abs(float(loss.detach()) - ref) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(ref)), (float(loss.detach()), ref)
    loss.backward()
    for n, p in m.named_parameters():
        r = float(G[f"bce.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert np.isfinite(got)
        assert abs(got - r) <= (2e-3 if dt == "fp32" else 1e-1) * r + (1e-6 if dt == "fp32" else 2e-2), (n, got, r)


@pytest.mark.parametrize("dt", DTYPES)
def test_g31_dssm_model_golden(dt):
    """The reference's own home for this tower: loss and per-parameter gradient norms under ``test_dssm_gpu``'s bounds for g24."""
    from idvs.morec_amd.model import DssmModel
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    user_num, _, neg, dnn = (int(v) for v in G["dssm.cfg"])
    args = make_args(embedding_dim=D, compute_dtype=dt, num_words_title=T, dnn_layers=dnn, neg_num=neg)
    m = load_det(DssmModel(args, user_num, item_num, True, tower()))
    with torch.no_grad():
        m.user_embedding.weight.mul_(float(G["dssm.table_scale"]))
    m = m.to(DEV).eval()
    x = torch.from_numpy(G["content"][G["dssm.sample_items"]]).to(DEV)
    loss = m(torch.from_numpy(G["dssm.input_user"]).to(DEV), x, torch.from_numpy(G["dssm.bce_label"]).to(DEV))
    ref = float(G["dssm.loss"])
    print(f"g31 dssm {dt}: loss {float(loss.detach()):.6f} vs {ref:.6f} (fp64 {float(G['dssm.loss.64']):.6f})")
    assert abs(float(loss.detach()) - ref) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(ref)), (float(loss.detach()), ref)
    loss.backward()
    rel, floor = (2e-3, 1e-6) if dt == "fp32" else (1e-1, 2e-2)
    for n, p in m.named_parameters():
        r = float(G[f"dssm.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert np.isfinite(got) and abs(got - r) <= rel * r + floor, (n, got, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_item_and_table_against_the_golden(dtype):
    """The whole content table, row 0 -- the all-masked padding item -- included, and the case with holes in the masks."""
    m = g31_model(dtype)
    f32 = dtype == "fp32"
    for text, key in ((G["content"], "table_vecs"), (G["holes.content"], "holes.vecs")):
        got = m.bert_encoder(torch.from_numpy(text).to(DEV)).detach().cpu().numpy()
        vmax = float(np.abs(G[key]).max())
        tol = twin_bound(2e-5, key, vmax) if f32 else 5e-2
        e = relerr(got, G[key])
        print(f"g31 {dtype} {key}: err {e:.2e} (bound {tol:.1e}; reference fp32 vs fp64 {twin_err(key, vmax):.2e})")
        assert np.isfinite(got).all() and e < tol
        if key == "table_vecs":
            e0 = float(np.abs(got[0] - G[key][0]).max()) / vmax
            print(f"g31 {dtype} padding item: err {e0:.2e}")
            assert e0 < tol and float(np.abs(G[key][0]).max()) > 0


def _enc_grads(frozen=0, freeze_names=()):
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    items = torch.from_numpy(G["content"][G["ids"].reshape(-1)]).to(DEV)
    R = torch.from_numpy(det_normal("g31.R", (B * (S + 1), D))).to(DEV)
    m = g31_model("bf16")
    for i, (n, q) in enumerate(m.bert_encoder.text_encoders["title"].bert_model.named_parameters()):
        q.requires_grad = i >= frozen and n not in freeze_names
    calls = []
    real = ops.disent_attn_bwd

    def spy(*a, **kw):
        calls.append(bool(kw.get("need_dpos", True)))
        return real(*a, **kw)
    ops.disent_attn_bwd = spy
    try:
        (m.bert_encoder(items) * R).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.disent_attn_bwd = real
    return {k: q.grad for k, q in m.bert_encoder.named_parameters()}, calls


@pytest.mark.parametrize("frozen", [3, 19])
def test_frozen_prefix_gives_the_same_trainable_gradients(frozen):
    """``--freeze_paras_before`` 3 (the embedding stage) and 19 (+ layer 0): the trainable gradients keep their bits.  ``rel_embeddings`` is
    registered last, so it trains in both cases and every layer still forms dPK / dPQ for it."""
    saved = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        (full, c_full), (part, c_part) = _enc_grads(0), _enc_grads(frozen)
    finally:
        ops.set_deterministic(saved)
    names = list(full)
    assert all(part[k] is None for k in names[:frozen]) and all(part[k] is not None for k in names[frozen:])
    for k in names[frozen:]:
        assert torch.equal(part[k], full[k]), k
    assert c_full == [True, True] and c_part == [True, True]


def test_no_position_gradient_work_where_nothing_needs_it():
    """``rel_embeddings`` and layer 0's ``pos_*`` frozen by hand: layer 0 forms no dPK / dPQ; with layer 1's frozen too and layer 0 below
    the lowest trainable parameter, the backward never reaches layer 0 at all."""
    L0 = "encoder.layer.0.attention.self."
    L1 = "encoder.layer.1.attention.self."
    pos = ("pos_proj.weight", "pos_q_proj.weight", "pos_q_proj.bias")
    saved = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        full, _ = _enc_grads(0)
        part, calls = _enc_grads(0, ("encoder.rel_embeddings.weight",) + tuple(L0 + k for k in pos))
        assert calls == [True, False]      # layer 1 first (the backward walks down)
        for k, g in part.items():
            if g is not None:
                assert torch.equal(g, full[k]), k
        part, calls = _enc_grads(19, ("encoder.rel_embeddings.weight",) + tuple(L1 + k for k in pos))
        assert calls == [False]
        k = "text_encoders.title.bert_model.encoder.layer.1.output.dense.weight"
        assert part[k] is not None and torch.equal(part[k], full[k])
    finally:
        ops.set_deterministic(saved)


def test_from_hf_round_trip_of_the_installed_micro_model():
    from transformers import DebertaConfig, DebertaModel
    torch.manual_seed(3)
    hf = DebertaModel(DebertaConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **KEYS["config"])).eval()
    with torch.no_grad():
        for n, q in hf.named_parameters():      # (q_bias / v_bias start as zeros)
            if n.endswith("_bias"):
                q.normal_(std=0.3)
    m = HipDebertaModel.from_hf(hf)
    assert [[k, list(p.shape)] for k, p in m.named_parameters()] == [[k, list(s)] for k, s in KEYS["parameters"]]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in hf.named_parameters()]
    sd, sd_hf = m.state_dict(), hf.state_dict()
    assert list(sd) == [k for k in sd_hf if not k.endswith("position_ids")]
    assert all(torch.equal(sd[k], sd_hf[k]) for k in sd)      # in_proj.weight keeps HF's interleaved layout
    T = int(G["cfg"][2])
    text = torch.from_numpy(G["content"])
    with torch.no_grad():
        want = hf(input_ids=text[:, :T], attention_mask=text[:, T:])[0][:, 0].numpy()
    enc = Text_Encoder(m, 64, 64, torch.float32).to(DEV).eval()
    got = enc.encode(text.to(DEV), features_only=True).float().cpu().numpy()
    e = relerr(got, want)
    print(f"from_hf forward: {e:.2e}")
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


SMOKE = ["--synthetic", "48", "--synthetic_items", "60", "--bert_model_load", "deberta_micro", "--freeze_paras_before", "0", "--batch_size", "16",
         "--embedding_dim", "64", "--max_seq_len", "6", "--lr", "1e-3", "--fine_tune_lr", "1e-4", "--local_rank", "0", "--epoch", "1",
         "--num_workers", "0", "--item_tower", "modal", "--max_steps", "3"]


def test_driver_inbatch_three_steps_then_test(tmp_path):
    common = SMOKE + ["--loss", "inbatch", "--checkpoint_root", str(tmp_path)]
    log = _main(common)
    _mean_loss(log)
    assert "valid_results" in log
    assert re.search(r"test_results   [0-9.]+\t[0-9.]+", _main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"]))


def test_driver_dssm_three_steps(tmp_path):
    _mean_loss(_main(SMOKE + ["--arch", "dssm", "--dnn_layers", "2", "--neg_num", "4", "--checkpoint_root", str(tmp_path)]))


def test_driver_bce_fusion_tower(tmp_path):
    argv = SMOKE[:SMOKE.index("--item_tower")] + ["--item_tower", "modal_cat", "--max_steps", "3", "--loss", "bce", "--checkpoint_root", str(tmp_path)]
    _mean_loss(_main(argv))


def test_driver_two_stage_stage1_saves_the_cls_rows(tmp_path):
    from idvs.morec_amd import run
    shape = DebertaShape.named("deberta_micro")
    torch.manual_seed(21)
    bert = HipDebertaModel(shape)
    (tmp_path / "deberta_micro").mkdir()
    torch.save(bert.state_dict(), str(tmp_path / "deberta_micro" / "pytorch_model.bin"))
    feats = str(tmp_path / "features.npy")
    argv = [a for a in SMOKE if a not in ("--max_steps", "3")]
    log = _main(argv + ["--arch", "two_stage", "--save_features", feats, "--checkpoint_root", str(tmp_path), "--pretrained_dir", str(tmp_path)])
    assert "stage 1" in log
    _mean_loss(log)
    table = np.load(feats)
    assert table.shape == (61, 64) and np.isfinite(table).all() and float(np.abs(table[1:]).max()) > 0
    _, content, *_ = run.synthetic_dataset(48, 60, 6, 30, vocab=shape.vocab_size, deberta=True)
    enc = Text_Encoder(bert, 64, 64, torch.float16).to(DEV).eval()      # fp16: the driver's default --compute_dtype
    want = enc.encode(torch.from_numpy(content).to(DEV), features_only=True).float().cpu().numpy().astype(table.dtype)
    assert np.array_equal(table, want)
