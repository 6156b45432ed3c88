"""-m gpu: the DSSM two-tower model (``--arch dssm``) on the device -- ``DssmModel`` against the golden captured from the reference's
``bce_text/main-end2end(DSSM)`` package (g24: loss, gradient norms, full table gradients, both tables, eval ranks and metrics), dropout
through ``functional.MlpFn``, and the driver end to end in a child process."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dssm_ref
from helpers import GOLDEN_DIR
from idvs.morec_amd.utils.detgen import det_normal, det_param

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G24 = np.load(os.path.join(GOLDEN_DIR, "g24_dssm.npz"))
G14 = np.load(os.path.join(GOLDEN_DIR, "g14_bce.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g24_dssm_keys.json")))
USER_NUM, ITEM_NUM, D, B = (int(v) for v in G24["cfg"])
CASES = ("id_0_1", "id_2_4", "modal_2_4")


def _args(case, dt, drop_rate=0.0, **kw):
    d = dict(embedding_dim=D, dnn_layers=int(G24[f"{case}.dnn_layers"]), neg_num=int(G24[f"{case}.neg_num"]), drop_rate=drop_rate,
             num_words_title=30, num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="bert_micro",
             word_embedding_dim=64, compute_dtype=dt, item_tower="modal" if case.startswith("modal") else "id", num_workers=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _model(case, dt, drop_rate=0.0):
    from idvs.morec_amd.model import BertShape, DssmModel, HipBertModel
    modal = case.startswith("modal")
    m = DssmModel(_args(case, dt, drop_rate), USER_NUM, ITEM_NUM, modal, HipBertModel(BertShape.named("micro")) if modal else None)
    scale = float(G24[f"{case}.table_scale"])
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
        m.user_embedding.weight.mul_(scale)
        if not modal:
            m.id_embedding.weight.mul_(scale)
    return m.to(DEV)


def _inputs(case):
    items = G24[f"{case}.sample_items"]
    x = torch.from_numpy(G14["content"][items]) if case.startswith("modal") else torch.from_numpy(items)
    return torch.from_numpy(G24[f"{case}.input_user"]).to(DEV), x.to(DEV), torch.from_numpy(G24[f"{case}.bce_label"]).to(DEV)


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_dssm_model_golden(case, dt):
    """Loss and per-parameter gradient norms with the bounds ``test_fusion_gpu.py`` uses for g23; fp32 also both table gradients element by
    element (rtol 1e-4 / atol 1e-7)."""
    m = _model(case, dt).eval()
    loss = m(*_inputs(case))
    ref = float(G24[f"{case}.loss"])
    print(f"g24 {case} {dt}: loss {float(loss.detach()):.6f} (reference {ref:.6f})")
    loss.backward()
    rel, floor = (2e-3, 1e-6) if dt == "fp32" else (1e-1, 2e-2)
    worst = max(abs(float(p.grad.double().norm()) - float(G24[f"{case}.grad_norm.{n}"])) / (rel * float(G24[f"{case}.grad_norm.{n}"]) + floor)
                for n, p in m.named_parameters() if "pooler" not in n)
    print(f"g24 {case} {dt}: largest gradient-norm error as a share of its bound {worst:.3f}")
    assert abs(float(loss.detach()) - ref) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(ref)), (float(loss.detach()), ref)
    for n, p in m.named_parameters():
        if "pooler" in n:
            continue
        r = float(G24[f"{case}.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert abs(got - r) <= rel * r + floor, (n, got, r)
    tables = ["user_embedding"] + ([] if case.startswith("modal") else ["id_embedding"])
    for t in tables:
        g = getattr(m, t).weight.grad
        assert g.dtype == torch.float32 and float(g[0].abs().max()) == 0.0      # padding_idx = 0
        if dt == "fp32":
            np.testing.assert_allclose(g.cpu().numpy(), G24[f"{case}.grad.{t}.weight"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("case", CASES)
def test_dssm_eval_golden(case):
    """Both tables to rel < 1e-5, the golden ranks exactly and the golden HR@10 / nDCG@10 (fp32); the checker agrees on the same tables.
    (Row 0 of the TEXT tower's table is the padding item, a title of [PAD] tokens only with every key masked: the library's attention and
    the reference's differ on such a row, no evaluation reads it -- ``morec_eval_rank`` starts at item 1 -- and the g17 / g23 table tests
    leave it out the same way.)"""
    from idvs.morec_amd.data_utils import dssm as dd
    m = _model(case, "fp32")
    modal = case.startswith("modal")
    content = G14["content"] if modal else np.arange(ITEM_NUM + 1)
    utab = dd.get_user_embeddings(m, USER_NUM, 8, m.args, DEV)          # 21 rows in chunks of 8
    itab = dd.get_item_embeddings(m, content, 16, m.args, modal, DEV)
    assert tuple(utab.shape) == (USER_NUM + 1, D) and tuple(itab.shape) == (ITEM_NUM + 1, D) and utab.dtype == itab.dtype == torch.float32
    for got, name in ((utab, "user_table"), (itab, "item_table")):
        ref = torch.from_numpy(G24[f"{case}.{name}"]).double()
        lo = 1 if (modal and name == "item_table") else 0      # row 0 of the text table is the all-[PAD] item: left out, as in the g17 / g23 tests
        err = float((got.double().cpu()[lo:] - ref[lo:]).abs().max() / ref[lo:].abs().max())
        print(f"g24 {case} {name}: rel err {err:.2e}")
        assert err < 1e-5
    pairs, hist = G24[f"{case}.eval_pairs"], G24[f"{case}.eval_hist"]
    history = {int(u): torch.from_numpy(h[h >= 0]) for (u, _), h in zip(pairs, hist)}
    ranks = dd.eval_ranks(history, pairs, utab, itab, 7, DEV).cpu()      # 20 pairs in chunks of 7
    assert ranks.tolist() == G24[f"{case}.eval_ranks"].tolist()
    assert ranks.tolist() == dssm_ref.eval_ranks(utab.cpu(), itab.cpu(), torch.from_numpy(pairs), torch.from_numpy(hist)).tolist()

    class _Log:
        lines = []

        def info(self, s):
            self.lines.append(s)

    hit = dd.eval_model(m, history, pairs, utab, itab, 7, m.args, ITEM_NUM, _Log(), "valid", DEV)
    assert abs(hit - float(G24[f"{case}.hit10"])) < 1e-6
    assert _Log.lines[0] == "valid_methods   Hit10\tnDCG10"
    got = [float(x) for x in _Log.lines[1].split("valid_results")[1].split()]
    assert abs(got[0] - 100 * float(G24[f"{case}.hit10"])) < 1e-3 and abs(got[1] - 100 * float(G24[f"{case}.ndcg10"])) < 1e-3


def _step(m, case, seed):
    torch.manual_seed(seed)
    m._drop_calls = 0
    m.zero_grad()
    loss = m(*_inputs(case))
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_dssm_dropout_streams():
    """Training mode, ``drop_rate = 0.5``, two layers: the same seed and call count give the same bits (loss and every gradient; the
    deterministic mode is on, since the bias and table gradients otherwise end in fp32 atomics), another seed another loss, and
    ``.eval()`` is the ``drop_rate = 0`` model."""
    from idvs.morec_amd import ops
    case = "id_2_4"
    m = _model(case, "fp32", drop_rate=0.5).train()
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        l1, g1 = _step(m, case, 5)
        l2, g2 = _step(m, case, 5)
        l3, _ = _step(m, case, 6)
    finally:
        ops.set_deterministic(was)
    assert torch.equal(l1, l2) and g1.keys() == g2.keys() and all(torch.equal(g1[n], g2[n]) for n in g1)
    assert float(l3) != float(l1)
    plain = float(_model(case, "fp32", drop_rate=0.0).train()(*_inputs(case)).detach())
    assert float(l1) != plain                                             # the masks did something
    assert float(m.eval()(*_inputs(case)).detach()) == plain


def test_mlp_fn_autograd_against_fp64_with_the_same_masks():
    """``functional.MlpFn`` with dropout against an fp64 torch MLP under the masks the library reports (``ops.dropout_keep_mask``): output,
    input gradient and every weight / bias gradient to rel < 1e-5 (fp32).  R = 37 rows: not a multiple of any tile."""
    from idvs.morec_amd import functional as F_, ops
    from idvs.morec_amd.engine import DropCfg
    R, p_drop = 37, 0.5
    drop = DropCfg(p_drop, 0.0, 0x0123456789ABCDEF)
    x = torch.from_numpy(det_normal("dssm.mlp.x", (R, D), std=1.0)).to(DEV).requires_grad_(True)
    params = []
    for l in range(2):
        params += [torch.from_numpy(det_normal(f"dssm.mlp.w{l}", (D, D), std=0.2)).to(DEV).requires_grad_(True),
                   torch.from_numpy(det_normal(f"dssm.mlp.b{l}", (D,), std=0.2)).to(DEV).requires_grad_(True)]
    dout = torch.from_numpy(det_normal("dssm.mlp.dout", (R, D), std=1.0)).to(DEV)
    out = F_.MlpFn.apply(x, (torch.float32, drop), *params)
    out.backward(dout)
    thresh = int(p_drop * 65536)
    inv_keep = 1.0 / (1.0 - thresh / 65536.0)
    masks = [ops.dropout_keep_mask(R * D, p_drop, drop.site(l)).view(R, D).double() * inv_keep for l in range(2)]
    assert all(0.3 < float((mk > 0).double().mean()) < 0.7 for mk in masks) and not torch.equal(masks[0], masks[1])
    x64 = x.detach().double().requires_grad_(True)
    p64 = [t.detach().double().requires_grad_(True) for t in params]
    sd = {"MLP.mlp_layers.1.weight": p64[0], "MLP.mlp_layers.1.bias": p64[1], "MLP.mlp_layers.4.weight": p64[2], "MLP.mlp_layers.4.bias": p64[3]}
    ref = dssm_ref.mlp(x64, sd, "", mask=masks)
    ref.backward(dout.double())
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    errs = {"out": rel(out.detach(), ref.detach()), "dx": rel(x.grad, x64.grad)}
    errs.update({f"dparam{i}": rel(params[i].grad, p64[i].grad) for i in range(4)})
    print("MlpFn vs fp64:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs
    assert bool((x.grad[masks[0] == 0] == 0).all())      # a dropped input element receives no gradient


_DRIVER = r"""
import os
import sys
sys.path.insert(0, {root!r})
from idvs.morec_amd import run
common = {common!r}
run.main(common)
print("=== TEST RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "test", "--load_ckpt_name", sorted(os.listdir({model_dir!r}))[-1]])
"""


def test_run_driver_dssm(tmp_path):
    """``run.py --arch dssm`` in a fresh child process: 30 steps on synthetic pairs, then ``--mode test`` on the checkpoint it wrote.
    (``--lr 1e-2``: at the default 1e-5 thirty steps move nothing measurable; ``--logging_num 1000``: a loss line per step;
    ``--checkpoint_root``: the test's own directory.)"""
    from idvs.morec_amd.parameters import parse_args
    from idvs.morec_amd.run import dssm_model_dir
    common = ["--arch", "dssm", "--item_tower", "id", "--dnn_layers", "2", "--neg_num", "4", "--synthetic", "300", "--synthetic_items", "200",
              "--max_steps", "30", "--compute_dtype", "fp32", "--lr", "1e-2", "--logging_num", "1000", "--local_rank", "0",
              "--checkpoint_root", str(tmp_path)]
    model_dir = dssm_model_dir(parse_args(common))
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, common=common, model_dir=model_dir)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    train_log, test_log = res.stderr.split("=== TEST RUN ===")
    losses = [float(x) for x in re.findall(r"batch loss ([0-9.]+),", train_log)]
    assert len(losses) == 30
    print("dssm driver: first ten", np.mean(losses[:10]), "last ten", np.mean(losses[-10:]))
    assert np.mean(losses[-10:]) < np.mean(losses[:10])
    for split in ("valid", "test"):
        assert f"{split}_methods   Hit10\tnDCG10" in train_log and re.search(split + r"_results   [0-9.]+\t[0-9.]+", train_log)
    saved = re.findall(r"Model saved to (\S+)", train_log)      # whatever label the run's validations gave it: the last file written
    assert saved and os.path.dirname(saved[-1]) == model_dir and re.fullmatch(r"epoch-1-\d+\.pt", os.path.basename(saved[-1]))
    path = saved[-1]
    assert os.path.exists(path) and "dnn_2" in path and sorted(os.listdir(model_dir))[-1] == os.path.basename(path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert {"model_state_dict", "optimizer", "rng_state", "cuda_rng_state"} <= set(ckpt)
    assert list(ckpt["model_state_dict"]) == [k for k, _ in KEYS["id_2_4"]]
    assert tuple(ckpt["model_state_dict"]["user_embedding.weight"].shape) == (301, 256)
    hit_train = re.findall(r"test_results   ([0-9.]+)\t", train_log)
    hit_test = re.findall(r"test_results   ([0-9.]+)\t", test_log)
    assert len(hit_train) == 1 and hit_test == hit_train
