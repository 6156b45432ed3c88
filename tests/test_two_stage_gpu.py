"""-m gpu: two-stage training on frozen item features (``--arch two_stage``) on the device -- ``TwoStageModel`` against the golden captured
from the reference's ``bce_text/main-2stage(SASRec)`` package (g25: loss, gradient norms, the full ``fc.fc.weight`` gradient, stage-1
features, the item table, eval ranks and metrics) in both input forms (gathered float features; ids + device feature table), dropout
through ``FeatProjFn`` + ``MlpFn``, and the driver end to end in child processes."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import two_stage_ref as ref
from helpers import GOLDEN_DIR
from idvs.morec_amd.utils.detgen import det_normal, det_param

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = np.load(os.path.join(GOLDEN_DIR, "g25_two_stage.npz"))
G14 = np.load(os.path.join(GOLDEN_DIR, "g14_bce.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g25_two_stage_keys.json")))
S, D, ITEM_NUM, B, W = (int(v) for v in G25["cfg"])
CASES = ("mlp_0", "mlp_2")


def _args(case, dt, drop_rate=0.0):
    return types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=drop_rate, transformer_block=2,
                                 dnn_layer=int(G25[f"{case}.dnn_layer"]), word_embedding_dim=W, compute_dtype=dt, num_workers=0)


def _table(case):
    return torch.from_numpy(det_normal("g25.table", (ITEM_NUM + 1, W), std=1.0).astype(np.float32) * np.float32(G25[f"{case}.table_scale"]))


def _model(case, dt, drop_rate=0.0):
    from idvs.morec_amd.model import TwoStageModel
    m = TwoStageModel(_args(case, dt, drop_rate), ITEM_NUM)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    return m.to(DEV)


@pytest.mark.parametrize("form", ["floats", "ids"])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_two_stage_model_golden(case, dt, form):
    """Loss and per-parameter gradient norms under the per-dtype tolerances of ``test_dssm_gpu.py::test_dssm_model_golden`` (fp32: loss 1e-4,
    norms 2e-3 r + 1e-6; 16-bit: loss 3e-2, norms 1e-1 r + 2e-2), and the full ``fc.fc.weight`` gradient to the same relative size in the
    Frobenius norm.  For scale: the fp64 restatement fed the 16-bit-rounded weights and table (nothing else rounded) sits at a loss
    distance of 1.4e-3 / 2.3e-3 (bf16, mlp_0 / mlp_2) and 2.5e-5 / 2.2e-6 (fp16) from the golden, at most 0.036 of the norm bound, and
    1.3e-2 / 6.9e-3 (bf16), 8.6e-4 / 3.0e-3 (fp16) in the ``fc.fc.weight`` gradient: four times those distances stays inside these
    bounds, so they are not widened.  ``ids``: the table itself receives no gradient."""
    m = _model(case, dt).eval()
    table, ids = _table(case), torch.from_numpy(G25["ids"])
    lm = torch.from_numpy(G25["log_mask"]).to(DEV)
    if form == "ids":
        m.set_feature_table(table.to(DEV))
        x = ids.to(DEV)
    else:
        x = table[ids].view(-1, W).to(DEV)          # the reference's batch: [B * (L + 1) * 2, W] fp32
    loss = m(x, lm, DEV)
    want = float(G25[f"{case}.loss"])
    print(f"g25 {case} {dt} {form}: loss {float(loss.detach()):.6f} (reference {want:.6f})")
    loss.backward()
    rel, floor = (2e-3, 1e-6) if dt == "fp32" else (1e-1, 2e-2)
    worst = max(abs(float(p.grad.double().norm()) - float(G25[f"{case}.grad_norm.{n}"])) / (rel * float(G25[f"{case}.grad_norm.{n}"]) + floor)
                for n, p in m.named_parameters())
    gw = torch.from_numpy(G25[f"{case}.grad.fc.fc.weight"]).double()
    err_w = float((m.fc.fc.weight.grad.double().cpu() - gw).norm() / gw.norm())
    print(f"g25 {case} {dt} {form}: largest gradient-norm error as a share of its bound {worst:.3f}; fc.fc.weight gradient rel {err_w:.2e}")
    assert abs(float(loss.detach()) - want) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(want)), (float(loss.detach()), want)
    assert [n for n, _ in m.named_parameters()] == [k for k, _ in KEYS[case]]
    for n, p in m.named_parameters():
        r = float(G25[f"{case}.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert p.grad.dtype == torch.float32 and abs(got - r) <= rel * r + floor, (n, got, r)
    assert err_w <= rel, err_w
    if form == "ids":
        assert not m.feature_table.requires_grad and m.feature_table.grad is None and "feature_table" not in m.state_dict()


def test_featproj_fn_returns_no_gradient_for_the_table():
    """Even a table that asks for one: the features are frozen, the backward runs no input-gradient product."""
    from idvs.morec_amd import functional as F_
    table = _table("mlp_0").to(DEV).to(torch.bfloat16).requires_grad_(True)
    w = torch.from_numpy(det_param("fc.fc.weight", (D, W))).to(DEV).requires_grad_(True)
    b = torch.zeros(D, device=DEV, requires_grad=True)
    out = F_.FeatProjFn.apply(torch.from_numpy(G25["ids"]).to(DEV), table, torch.bfloat16, w, b)
    out.float().sum().backward()
    assert table.grad is None and w.grad is not None and b.grad is not None and float(w.grad.abs().max()) > 0


def test_stage_one_features_golden():
    """``extract_item_features`` over g14's token rows (bert-micro, ``det_param("bert_encoder." + key)``) against the reference's
    ``get_item_word_embs``: rel < 1e-5 in fp32.  Row 0 is the all-[PAD] item: left out, as in the g17 / g23 / g24 table tests."""
    from idvs.morec_amd.data_utils import extract_item_features
    from idvs.morec_amd.model import Bert_Encoder, BertShape, HipBertModel
    args = types.SimpleNamespace(embedding_dim=D, num_words_title=30, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="bert_micro", word_embedding_dim=64, compute_dtype="fp32")
    enc = Bert_Encoder(args, HipBertModel(BertShape.named("micro")))
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            v.copy_(torch.from_numpy(det_param("bert_encoder." + k, tuple(v.shape))))
    enc = enc.to(DEV).train()      # the extraction itself switches to eval mode
    feats = extract_item_features(enc, G14["content"], 16)          # 51 rows in chunks of 16
    assert not enc.training and tuple(feats.shape) == (ITEM_NUM + 1, 64) and feats.dtype == torch.float32 and not feats.requires_grad
    want = torch.from_numpy(G25["features"]).double()
    err = float((feats.double().cpu()[1:] - want[1:]).abs().max() / want[1:].abs().max())
    print(f"g25 stage-1 features: rel err {err:.2e}")
    assert err < 1e-5


def test_stage_one_vision_features_are_the_classifier_input():
    """``extract_item_features`` over a ``Vit_Encoder`` (Swin micro, fp32) returns the pooled features in front of the classifier:
    ``GELU(classifier(features))`` in fp64 reproduces the tower's own item vectors to 1e-5, in chunks that do not divide the catalogue."""
    from idvs.morec_amd.data_utils import extract_item_features
    from idvs.morec_amd.model.encoders import Vit_Encoder
    from idvs.morec_amd.model.swin import HipSwinForImageClassification
    from idvs.morec_amd.swin_engine import SwinShape
    shape = SwinShape.named("swin_micro")
    enc = Vit_Encoder(HipSwinForImageClassification(shape, D), compute_dtype=torch.float32)
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            v.copy_(torch.from_numpy(det_param("cv_encoder." + k, tuple(v.shape))))
    enc = enc.to(DEV)
    px = torch.from_numpy(det_normal("two_stage.images", (7, 3, shape.image_size, shape.image_size)).astype(np.float32))
    feats = extract_item_features(enc, px, 3)
    assert feats.dtype == torch.float32 and feats.shape[0] == 7 and feats.shape[1] == enc.image_net.classifier.weight.shape[1]
    with torch.no_grad():
        want = enc(px.to(DEV)).double().cpu()
    w, b = enc.image_net.classifier.weight.detach().double().cpu(), enc.image_net.classifier.bias.detach().double().cpu()
    got = ref.gelu(feats.double().cpu() @ w.t() + b)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"vision stage-1 features -> classifier: rel err {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("case", CASES)
def test_two_stage_eval_golden(case):
    """``get_item_embeddings_two_stage`` to rel < 1e-5 of the golden item table (fp32), then the golden ranks exactly and the golden HR@10 /
    nDCG@10 through the unchanged ``eval_model``; the generic ``get_item_embeddings`` hands a two-stage model to the same function."""
    from idvs.morec_amd.data_utils import eval_model, get_item_embeddings, get_item_embeddings_two_stage
    from idvs.morec_amd.data_utils.metrics import eval_ranks
    m = _model(case, "fp32")
    table = _table(case)
    itab = get_item_embeddings_two_stage(m, table, 16)          # 51 rows in chunks of 16
    assert tuple(itab.shape) == (ITEM_NUM + 1, D) and itab.dtype == torch.float32 and not m.training
    want = torch.from_numpy(G25[f"{case}.item_table"]).double()
    err = float((itab.double().cpu() - want).abs().max() / want.abs().max())
    print(f"g25 {case} item table: rel err {err:.2e}")
    assert err < 1e-5
    assert torch.equal(get_item_embeddings(m, table, 16, m.args, True, DEV), itab)
    seqs = {u: [int(i) for i in row if i >= 0] for u, row in enumerate(G25[f"{case}.eval_seqs"])}
    history = {u: torch.LongTensor(s[:-1]) for u, s in seqs.items()}
    ranks = eval_ranks(m, history, seqs, itab, list(seqs), m.args, DEV).cpu()
    assert ranks.tolist() == G25[f"{case}.eval_ranks"].tolist()
    p = ref.double_params(m.state_dict(), requires_grad=False)
    assert ranks.tolist() == ref.eval_ranks(p, itab.cpu(), list(seqs.values()), S, 2).tolist()

    class _Log:
        lines = []

        def info(self, s):
            self.lines.append(s)

    hit = eval_model(m, history, seqs, itab, 7, m.args, ITEM_NUM, _Log(), "valid", DEV)
    assert abs(hit - float(G25[f"{case}.hit10"])) < 1e-6
    got = [float(x) for x in _Log.lines[1].split("valid_results")[1].split()]
    assert abs(got[0] - 100 * float(G25[f"{case}.hit10"])) < 1e-3 and abs(got[1] - 100 * float(G25[f"{case}.ndcg10"])) < 1e-3


def test_mlp_layers_dropout_masks_match_between_forward_and_backward():
    """``MLP_Layers.encode_ids`` (``FeatProjFn`` + ``MlpFn``) with ``drop_rate = 0.5`` against the fp64 restatement under the masks the
    library reports (``ops.dropout_keep_mask``), the way ``test_mlp_fn_autograd_against_fp64_with_the_same_masks`` does it: output and
    every weight / bias gradient to rel < 1e-5 (fp32) -- a backward that drew other masks than the forward would miss by O(1).  R = 37."""
    from idvs.morec_amd import ops
    from idvs.morec_amd.engine import DropCfg
    from idvs.morec_amd.model import MLP_Layers
    R, p_drop = 37, 0.5
    drop = DropCfg(p_drop, 0.0, 0x0123456789ABCDEF)
    mlp = MLP_Layers(W, D, [D, D, D], p_drop, compute_dtype=torch.float32)
    with torch.no_grad():
        for k, v in mlp.state_dict().items():
            v.copy_(torch.from_numpy(det_normal("two_stage.mlp." + k, tuple(v.shape), std=0.2)))
    mlp = mlp.to(DEV)
    table = torch.from_numpy(det_normal("two_stage.mlp.table", (ITEM_NUM + 1, W), std=1.0)).to(DEV)
    ids = torch.from_numpy(np.arange(R) * 7 % (ITEM_NUM + 1)).to(DEV)
    dout = torch.from_numpy(det_normal("two_stage.mlp.dout", (R, D), std=1.0)).to(DEV)
    out = mlp.encode_ids(ids, table, drop)
    out.backward(dout)
    inv_keep = 1.0 / (1.0 - int(p_drop * 65536) / 65536.0)
    masks = [ops.dropout_keep_mask(R * D, p_drop, drop.site(l)).view(R, D).double().cpu() * inv_keep for l in range(2)]
    assert all(0.3 < float((mk > 0).double().mean()) < 0.7 for mk in masks) and not torch.equal(masks[0], masks[1])
    p64 = ref.double_params({"fc." + k: v for k, v in mlp.state_dict().items()})
    want = ref.mlp_layers(table.double().cpu()[ids.cpu()], p64, mask=masks)
    want.backward(dout.double().cpu())
    rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())
    errs = {"out": rel(out.detach(), want.detach())}
    errs.update({k: rel(v.grad, p64["fc." + k].grad) for k, v in mlp.named_parameters()})
    print("MLP_Layers with dropout vs fp64:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs
    # the float form draws the same masks: the same bits
    mlp.zero_grad()
    out2 = mlp.encode(table[ids], drop)
    assert torch.equal(out2, out)


def test_two_stage_model_dropout_streams():
    """Training mode, ``drop_rate = 0.5``: the same seed and call count give the same loss, another seed another, ``.eval()`` is the
    ``drop_rate = 0`` model.  (``morec_bce_fwd`` sums the loss with fp32 atomics: "the same" is to 1e-5 relative, the reordering bound
    ``test_fusion_gpu.py`` uses for it.)"""
    case = "mlp_2"
    m = _model(case, "bf16", drop_rate=0.5).train()
    m.set_feature_table(_table(case).to(DEV))
    x, lm = torch.from_numpy(G25["ids"]).to(DEV), torch.from_numpy(G25["log_mask"]).to(DEV)

    def step(seed):
        torch.manual_seed(seed)
        m._drop_calls = 0
        m.zero_grad()
        loss = m(x, lm, DEV)
        loss.backward()
        return float(loss.detach())

    l1, l2, l3 = step(5), step(5), step(6)
    plain = _model(case, "bf16").train()
    plain.set_feature_table(_table(case).to(DEV))
    l0 = float(plain(x, lm, DEV).detach())
    same = lambda a, b: abs(a - b) <= 1e-5 * abs(b)
    assert same(l1, l2) and not same(l3, l1) and not same(l1, l0), (l1, l2, l3, l0)
    assert same(float(m.eval()(x, lm, DEV).detach()), l0)


_DRIVER = r"""
import os
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
common = {common!r}
run.main(common)
print("=== TEST RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"])
for extra in {extras!r}:
    print("=== EXTRA RUN ===", file=sys.stderr, flush=True)
    run.main(common + extra)
"""


def _drive(common, tmp_path, extras=()):
    from idvs.morec_amd.parameters import parse_args
    from idvs.morec_amd.run import two_stage_model_dir
    model_dir = two_stage_model_dir(parse_args(common))
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, common=common, extras=list(extras))], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    train_log, test_log = res.stderr.split("=== TEST RUN ===")
    test_log, *extra_logs = test_log.split("=== EXTRA RUN ===")
    assert len(extra_logs) == len(extras)
    assert re.search(r"epoch 1: \d+ steps, mean loss [0-9.]+", train_log)
    assert "valid_methods   Hit10\tnDCG10" in train_log and re.search(r"valid_results   [0-9.]+\t[0-9.]+", train_log)
    saved = re.findall(r"Model saved to (\S+)", train_log)
    assert saved and all(os.path.dirname(s) == model_dir for s in saved) and os.path.basename(saved[-1]) == "epoch-1.pt"
    assert os.path.basename(model_dir).startswith("cpt_modal_bert_tiny_mlp_2_bs_") and str(tmp_path) in model_dir
    ckpt = torch.load(saved[-1], map_location="cpu", weights_only=False)
    assert {"model_state_dict", "optimizer", "rng_state", "cuda_rng_state"} <= set(ckpt)
    keys = list(ckpt["model_state_dict"])
    assert keys[:6] == [k for k, _ in KEYS["mlp_2"]][:6] and tuple(ckpt["model_state_dict"]["fc.fc.weight"].shape) == (64, 128)
    assert "model loaded from" in test_log and re.search(r"test_results   [0-9.]+\t[0-9.]+", test_log)
    return train_log, test_log, extra_logs


def test_run_driver_two_stage(tmp_path):
    """``run.py --arch two_stage --synthetic 64 --epoch 1`` in a fresh child process: stage 1 (BERT-tiny over 200 synthetic items), one
    epoch, the validation, a checkpoint under the reference's label, then ``--mode test`` on it; the table it wrote with
    ``--save_features`` then drives the same run through ``--features_npy`` in a second child process (no tower is built there), followed
    there by ``--mode test --cold_seqs`` and ``--mode recommend`` on its checkpoint."""
    feats = str(tmp_path / "features.npy")
    common = ["--arch", "two_stage", "--item_tower", "modal", "--bert_model_load", "bert_tiny", "--synthetic", "64", "--synthetic_items", "200",
              "--epoch", "1", "--embedding_dim", "64", "--dnn_layer", "2", "--batch_size", "16", "--lr", "1e-3", "--local_rank", "0",
              "--checkpoint_root", str(tmp_path / "a")]
    train_log, _, _ = _drive(common + ["--save_features", feats], tmp_path)
    assert "stage 1" in train_log and os.path.exists(feats)
    table = np.load(feats)
    assert table.shape == (201, 128) and table.dtype == np.float32 and np.isfinite(table).all()
    common[-1] = str(tmp_path / "b")
    cold, rec = str(tmp_path / "cold.tsv"), str(tmp_path / "top5.tsv")
    ckpt = ["--load_ckpt_name", "epoch-1.pt"]
    train_log, _, (cold_log, rec_log) = _drive(common + ["--features_npy", feats], tmp_path, extras=[
        ["--mode", "test", "--cold_seqs", cold] + ckpt, ["--mode", "recommend", "--topk", "5", "--recommend_out", rec] + ckpt])
    assert "stage 1" not in train_log
    # the cold-start users and the recommendation lists go through the unchanged catalogue paths (the catalogue is fc over the table)
    assert os.path.exists(cold) and "cold-start / new-item eval" in cold_log and re.search(r"test_results   [0-9.]+\t[0-9.]+", cold_log)
    lines = open(rec).read().splitlines()
    assert len(lines) == 64 and "recommend: top-5 lists of 64 users" in rec_log
    for line in lines:
        user, items = line.split("\t")
        pairs = [x.split(":") for x in items.split(" ")]
        assert len(pairs) == 5 and all(re.fullmatch(r"N\d+", n) and 1 <= int(n[1:]) <= 200 for n, _ in pairs)
        assert [float(v) for _, v in pairs] == sorted((float(v) for _, v in pairs), reverse=True)
