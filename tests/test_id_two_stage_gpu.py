"""-m gpu: two-stage ID (+) modality fusion (``--arch id_two_stage``) on the device -- ``IdTwoStageModel`` against the golden captured from
the reference's ``bce_text/id_plus_mo-2stage`` package (g26: loss, gradient norms, the full ``turn_dim.fc.weight`` and
``id_embedding.weight`` gradients, the catalogue, eval ranks and metrics) in fp32 and both input forms; the 16-bit modes against the fp32
run; the fused and the composed item tower (``MOREC_FEATFUSE`` 2 / 1) bit for bit under dropout; the frozen table; the catalogue; and the
driver end to end in a child process.  Bounds: ``tests/test_two_stage_gpu.py``'s, for the same quantities against g25."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import id_two_stage_ref as ref
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G26 = np.load(os.path.join(GOLDEN_DIR, "g26_id_two_stage.npz"))
KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g26_id_two_stage_keys.json")))
S, D, ITEM_NUM, B, W = (int(v) for v in G26["cfg"])
CASES = ref.CASES
FULL = ("turn_dim.fc.weight", "id_embedding.weight")
_FP32 = {}


def _args(case, dt, drop_rate=0.0):
    kind, mo, dnn = case.split("_")
    return types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=drop_rate, transformer_block=2,
                                 dnn_layers=int(dnn), mo_dnn_layers=int(mo), word_embedding_dim=W, item_tower="modal_" + kind,
                                 compute_dtype=dt, num_workers=0)


def _table(case):
    return torch.from_numpy(ref.feature_table(ITEM_NUM, W, float(G26[f"{case}.table_scale"])))


def _model(case, dt, drop_rate=0.0):
    from idvs.morec_amd.model import IdTwoStageModel
    m = IdTwoStageModel(_args(case, dt, drop_rate), ITEM_NUM, True, None)
    state = ref.golden_state(KEYS[case], float(G26[f"{case}.table_scale"]), float(G26[f"{case}.mlp_scale"]))
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.from_numpy(state[k]))
    return m.to(DEV)


def _run(case, dt, form, m=None):
    """One eval-mode forward + backward: (loss, {name: fp32 gradient on the CPU}, model)."""
    m = _model(case, dt).eval() if m is None else m
    table, ids = _table(case), torch.from_numpy(G26["ids"])
    lm = torch.from_numpy(G26["log_mask"]).to(DEV)
    flat = ids.reshape(-1).to(DEV)
    if form == "ids":
        m.set_feature_table(table.to(DEV))
        loss = m(flat, None, lm, DEV)
    else:
        loss = m(flat, table[ids].view(-1, W).to(DEV), lm, DEV)      # the reference's batch: ids and [B * (L + 1) * 2, W] fp32
    loss.backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in m.parameters())
    return float(loss.detach()), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}, m


def _fp32_run(case):
    """The fp32 id-form run of a case: computed once, shared, never written."""
    if case not in _FP32:
        _FP32[case] = _run(case, "fp32", "ids")[:2]
    return _FP32[case]


@pytest.mark.parametrize("form", ["floats", "ids"])
@pytest.mark.parametrize("case", CASES)
def test_id_two_stage_model_golden_fp32(case, form):
    """fp32 against g26: loss to 1e-4, per-parameter gradient norms to 2e-3 r + 1e-6, the full ``turn_dim.fc.weight`` and
    ``id_embedding.weight`` gradients to 2e-3 in the Frobenius norm (``test_two_stage_model_golden``'s fp32 bounds)."""
    loss, grads, m = _run(case, "fp32", "floats") if form == "floats" else _fp32_run(case) + (None,)
    want = float(G26[f"{case}.loss"])
    rel, floor = 2e-3, 1e-6
    worst = max(abs(float(g.double().norm()) - float(G26[f"{case}.grad_norm.{n}"])) / (rel * float(G26[f"{case}.grad_norm.{n}"]) + floor)
                for n, g in grads.items())
    errs = {n: float((grads[n].double() - torch.from_numpy(G26[f"{case}.grad.{n}"]).double()).norm()
                     / torch.from_numpy(G26[f"{case}.grad.{n}"]).double().norm()) for n in FULL}
    print(f"g26 {case} fp32 {form}: loss {loss:.6f} (reference {want:.6f}); largest gradient-norm error as a share of its bound {worst:.3f}; "
          f"full gradients rel {errs}")
    assert abs(loss - want) < 1e-4 * max(1.0, abs(want)), (loss, want)
    assert list(grads) == [k for k, _ in KEYS[case]]
    for n, g in grads.items():
        r = float(G26[f"{case}.grad_norm.{n}"])
        assert abs(float(g.double().norm()) - r) <= rel * r + floor, (n, float(g.double().norm()), r)
    assert max(errs.values()) <= rel, errs
    assert float(grads["id_embedding.weight"][0].abs().max()) == 0.0      # padding_idx


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES)
def test_id_two_stage_model_16bit_against_fp32(case, dt):
    """bf16 / fp16 (ids form: ``FeatFuseFn`` where ``mo_dnn_layers == 0``) against the fp32 run of the same model, under
    ``test_two_stage_model_golden``'s 16-bit bounds: loss 3e-2, gradient norms 1e-1 r + 2e-2, the full gradients 1e-1 in the Frobenius
    norm.  The gathered-float form gives the same loss within the loss bound."""
    want, gref = _fp32_run(case)
    loss, grads, m = _run(case, dt, "ids")
    rel, floor = 1e-1, 2e-2
    worst = max(abs(float(grads[n].double().norm()) - float(gref[n].double().norm())) / (rel * float(gref[n].double().norm()) + floor) for n in gref)
    errs = {n: float((grads[n].double() - gref[n].double()).norm() / gref[n].double().norm()) for n in FULL}
    m.zero_grad()
    loss_f = _run(case, dt, "floats", m)[0]
    print(f"g26 {case} {dt}: loss {loss:.6f} (fp32 {want:.6f}, float form {loss_f:.6f}); largest gradient-norm error as a share of its bound "
          f"{worst:.3f}; full gradients rel {errs}")
    assert abs(loss - want) < 3e-2 * max(1.0, abs(want)), (loss, want)
    for n in gref:
        r, got = float(gref[n].double().norm()), float(grads[n].double().norm())
        assert abs(got - r) <= rel * r + floor, (n, got, r)
    assert max(errs.values()) <= rel, errs
    assert abs(loss_f - loss) < 3e-2 * max(1.0, abs(loss)), (loss_f, loss)
    assert float(grads["id_embedding.weight"][0].abs().max()) == 0.0


@pytest.mark.parametrize("case", CASES)
def test_id_and_float_forms_give_the_same_loss_fp32(case):
    """fp32: both forms run gather + GEMM over the same rows; the loss agrees to the reordering bound of ``morec_bce_fwd``'s atomic sum
    (1e-5 relative, ``test_two_stage_model_dropout_streams``)."""
    a = _fp32_run(case)[0]
    b = _run(case, "fp32", "floats")[0]
    assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (a, b)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ["add_0_0", "add_0_2", "cat_0_0", "cat_0_2"])
def test_fused_and_composed_towers_give_the_same_bits(case, dt):
    """Path independence: in the deterministic mode, ``MOREC_FEATFUSE`` 1 (featproj + fuse_add_fwd / fuse_cat_fwd) and 2
    (``morec_featfuse_fwd``) give ``torch.equal`` loss and every parameter gradient, training mode, dropout 0.1."""
    from idvs.morec_amd import ops
    m = _model(case, dt, drop_rate=0.1).train()
    m.set_feature_table(_table(case).to(DEV))
    flat, lm = torch.from_numpy(G26["ids"]).reshape(-1).to(DEV), torch.from_numpy(G26["log_mask"]).to(DEV)
    R = flat.numel()

    def step(knob):
        ops.set_featfuse(knob)
        assert ops.featfuse_supported(R, W, D, m.compute_dtype) == (knob == 2)
        torch.manual_seed(11)
        m._drop_calls = 0
        m.zero_grad()
        loss = m(flat, None, lm, DEV)
        loss.backward()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    ops.set_deterministic(True)
    try:
        l1, g1 = step(1)
        l2, g2 = step(2)
        l2b, g2b = step(2)
    finally:
        ops.set_deterministic(False)
        ops.set_featfuse(0)
    assert torch.equal(l2, l2b) and all(torch.equal(g2[n], g2b[n]) for n in g2), "the deterministic mode does not repeat itself"
    assert torch.equal(l1, l2), (float(l1), float(l2))
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    plain = _model(case, dt).train()      # the dropout is really on: drop_rate 0 gives another loss
    plain.set_feature_table(_table(case).to(DEV))
    assert abs(float(plain(flat, None, lm, DEV).detach()) - float(l1)) > 1e-4 * abs(float(l1))


@pytest.mark.parametrize("kind", ["add", "cat"])
def test_the_feature_table_is_frozen(kind):
    """The feature table receives no gradient -- even one that asks for it -- and is not in ``state_dict``; the pad row of the id table
    receives none either."""
    from idvs.morec_amd import functional as F_
    from idvs.morec_amd.engine import NO_DROP
    case = f"{kind}_0_0"
    m = _model(case, "bf16")
    m.set_feature_table(_table(case).to(DEV))
    assert "feature_table" not in m.state_dict() and not any("feature_table" in n for n, _ in m.named_buffers())
    assert not m.feature_table.requires_grad and m.feature_table.dtype == torch.bfloat16
    table = m.feature_table.clone().requires_grad_(True)
    ids = torch.from_numpy(G26["ids"]).reshape(-1).to(DEV)
    assert bool((ids == 0).any())
    out = F_.FeatFuseFn.apply(ids, table, m.id_embedding.weight, (kind, torch.bfloat16, NO_DROP, 0), m.turn_dim.fc.weight, m.turn_dim.fc.bias,
                              *m.fc._params())
    out.float().sum().backward()
    assert table.grad is None and m.turn_dim.fc.weight.grad is not None and float(m.turn_dim.fc.weight.grad.abs().max()) > 0
    g = m.id_embedding.weight.grad
    assert g is not None and float(g[0].abs().max()) == 0.0 and float(g[1:].abs().max()) > 0


@pytest.mark.parametrize("case", CASES)
def test_id_two_stage_catalogue_and_eval_golden(case):
    """``get_item_embeddings_id_two_stage`` (fp32) to rel < 1e-5 of the golden catalogue, equal to the training path's vectors in eval mode,
    then the golden ranks exactly and HR@10 / nDCG@10 through the unchanged ``eval_model``; the generic ``get_item_embeddings`` hands the
    model to the same function."""
    from idvs.morec_amd.data_utils import eval_model, get_item_embeddings, get_item_embeddings_id_two_stage
    from idvs.morec_amd.data_utils.metrics import eval_ranks
    m = _model(case, "fp32")
    table = _table(case)
    itab = get_item_embeddings_id_two_stage(m, table, 16)          # 51 rows in chunks of 16
    assert tuple(itab.shape) == (ITEM_NUM + 1, D) and itab.dtype == torch.float32 and not m.training and m.feature_table is None
    want = torch.from_numpy(G26[f"{case}.item_table"]).double()
    err = float((itab.double().cpu() - want).abs().max() / want.abs().max())
    print(f"g26 {case} catalogue: rel err {err:.2e}")
    assert err < 1e-5
    m.set_feature_table(table.to(DEV))
    assert torch.equal(get_item_embeddings(m, m.feature_table, 16, m.args, True, DEV), itab)
    with torch.no_grad():      # the training path over the same ids, in one piece
        E = m.encode_items(torch.arange(ITEM_NUM + 1, device=DEV)).float()
    assert float((E - itab).abs().max()) <= 1e-6 * float(itab.abs().max())
    seqs = {u: [int(i) for i in row if i >= 0] for u, row in enumerate(G26[f"{case}.eval_seqs"])}
    history = {u: torch.LongTensor(s[:-1]) for u, s in seqs.items()}
    ranks = eval_ranks(m, history, seqs, itab, list(seqs), m.args, DEV).cpu()
    assert ranks.tolist() == G26[f"{case}.eval_ranks"].tolist()

    class _Log:
        lines = []

        def info(self, s):
            self.lines.append(s)

    hit = eval_model(m, history, seqs, itab, 7, m.args, ITEM_NUM, _Log(), "valid", DEV)
    assert abs(hit - float(G26[f"{case}.hit10"])) < 1e-6
    got = [float(x) for x in _Log.lines[1].split("valid_results")[1].split()]
    assert abs(got[0] - 100 * float(G26[f"{case}.hit10"])) < 1e-3 and abs(got[1] - 100 * float(G26[f"{case}.ndcg10"])) < 1e-3


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ["add_0_0", "cat_0_0", "cat_2_2"])
def test_catalogue_equals_the_training_path_16bit(case, dt):
    """16-bit, eval mode: the chunked catalogue and the training path's ``encode_items`` over all ids are the same rows (every kernel of
    the tower writes a row from that row's inputs alone)."""
    from idvs.morec_amd.data_utils import get_item_embeddings_id_two_stage
    m = _model(case, dt).eval()
    m.set_feature_table(_table(case).to(DEV))
    itab = get_item_embeddings_id_two_stage(m, m.feature_table, 16)
    with torch.no_grad():
        E = m.encode_items(torch.arange(ITEM_NUM + 1, device=DEV)).float()
    assert m.feature_table is not None and torch.equal(E, itab)


def test_dropout_streams_and_counter():
    """Training mode, ``drop_rate = 0.5``: the same seed and call count give the same loss, another seed another; ``.eval()`` is the
    ``drop_rate = 0`` model; the call counter advances once per training forward (it goes into the checkpoint as ``morec_drop_calls``)."""
    case = "cat_2_2"
    m = _model(case, "bf16", drop_rate=0.5).train()
    m.set_feature_table(_table(case).to(DEV))
    flat, lm = torch.from_numpy(G26["ids"]).reshape(-1).to(DEV), torch.from_numpy(G26["log_mask"]).to(DEV)

    def step(seed):
        torch.manual_seed(seed)
        m._drop_calls = 0
        m.zero_grad()
        loss = m(flat, None, lm, DEV)
        loss.backward()
        assert m._drop_calls == 1
        return float(loss.detach())

    l1, l2, l3 = step(5), step(5), step(6)
    d = m.dropout_cfgs()
    assert m._drop_calls == 2 and len({c.seed for c in d}) == 4 and all(c.p_hidden == 0.5 for c in d)
    plain = _model(case, "bf16").train()
    plain.set_feature_table(_table(case).to(DEV))
    l0 = float(plain(flat, None, lm, DEV).detach())
    same = lambda a, b: abs(a - b) <= 1e-5 * abs(b)
    assert same(l1, l2) and not same(l3, l1) and not same(l1, l0), (l1, l2, l3, l0)
    assert same(float(m.eval()(flat, None, lm, DEV).detach()), l0)


_DRIVER = r"""
import os
import sys
sys.path.insert(0, {root!r})
import torch
from idvs.morec_amd import run
common = {common!r}
run.main(common)
print("=== TEST RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "test", "--load_ckpt_name", "epoch-1.pt"])
print("=== RECOMMEND RUN ===", file=sys.stderr, flush=True)
run.main(common + ["--mode", "recommend", "--topk", "5", "--recommend_out", {rec!r}, "--load_ckpt_name", "epoch-1.pt"])
# the checkpoint, loaded into a fresh model, on the validation split again
from idvs.morec_amd.data_utils import load_feature_table
from idvs.morec_amd.model import IdTwoStageModel
from idvs.morec_amd.model.encoders import resolve_dtype
from idvs.morec_amd.parameters import parse_args
args = parse_args(common)
model_dir = run.id_two_stage_model_dir(args)
del args.CV_model_load
item_num, _, _, users_valid, _, hist_valid, _, _, _ = run.load_dataset(args, False, False)
table = load_feature_table(args.features_npy, item_num, resolve_dtype(args), 0)
model = IdTwoStageModel(args, item_num, True, num_fc_ftr=int(table.shape[1])).to(0)
model.set_feature_table(table)
run.load_model(model, run.get_checkpoint(model_dir, "epoch-1.pt"))
hit = run.run_eval(model, model.feature_table, hist_valid, users_valid, 512, item_num, True, args, "valid", 0)
print("REVALID %.7f" % (hit * 100), file=sys.stderr, flush=True)
"""


@pytest.mark.parametrize("tower,mo,dnn", [("modal_add", 0, 0), ("modal_cat", 2, 2)])
def test_run_driver_id_two_stage(tmp_path, tower, mo, dnn):
    """``run.py --arch id_two_stage --synthetic 64 --epoch 1 --features_npy ...`` in a fresh child process: one epoch, the validation, a
    checkpoint under the reference's label with the reference's keys and the dropout counter; ``--mode test`` on it; ``--mode recommend``
    writes 5 unseen items per user; the checkpoint loaded into a fresh model reproduces the validation metric of the training run."""
    from idvs.morec_amd.parameters import parse_args
    from idvs.morec_amd.run import id_two_stage_model_dir
    from idvs.morec_amd.utils.detgen import det_normal
    feats, rec = str(tmp_path / "features.npy"), str(tmp_path / "top5.tsv")
    np.save(feats, det_normal("id_two_stage.driver.table", (201, 128), std=1.0).astype(np.float32))
    common = ["--arch", "id_two_stage", "--item_tower", tower, "--bert_model_load", "bert_tiny", "--synthetic", "64", "--synthetic_items", "200",
              "--epoch", "1", "--embedding_dim", "64", "--mo_dnn_layers", str(mo), "--dnn_layers", str(dnn), "--batch_size", "16", "--lr", "1e-3",
              "--local_rank", "0", "--features_npy", feats, "--checkpoint_root", str(tmp_path / "ck")]
    model_dir = id_two_stage_model_dir(parse_args(common))
    res = subprocess.run([sys.executable, "-c", _DRIVER.format(root=ROOT, common=common, rec=rec)], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    train_log, rest = res.stderr.split("=== TEST RUN ===")
    test_log, rest = rest.split("=== RECOMMEND RUN ===")
    assert "stage 1" not in train_log and "id-two-stage:" in train_log
    assert re.search(r"epoch 1: \d+ steps, mean loss [0-9.]+", train_log)
    valid = re.findall(r"valid_results   ([0-9.]+)\t([0-9.]+)", train_log)
    assert "valid_methods   Hit10\tnDCG10" in train_log and len(valid) == 1
    saved = re.findall(r"Model saved to (.+epoch-\d+\.pt)", train_log)
    assert saved and all(os.path.dirname(s) == model_dir for s in saved) and os.path.basename(saved[-1]) == "epoch-1.pt"
    assert os.path.basename(model_dir) == f"cpt_{tower}-bert_tiny-MOdnn_{mo}-dnn_{dnn}_ed_64_bs_16_lr_0.001"
    assert os.path.basename(os.path.dirname(model_dir)) == f"checkpoint_behaviors_l5_tr_v.tsv _bert_tiny_MOdnn_{mo}" and str(tmp_path) in model_dir
    ckpt = torch.load(saved[-1], map_location="cpu", weights_only=False)
    assert {"model_state_dict", "optimizer", "rng_state", "cuda_rng_state", "morec_drop_calls"} <= set(ckpt)
    assert int(ckpt["morec_drop_calls"]) == int(re.search(r"epoch 1: (\d+) steps", train_log).group(1))
    keys = list(ckpt["model_state_dict"])
    want = [k for k, _ in KEYS[f"{tower[6:]}_{mo}_{dnn}"]]
    assert keys == want and tuple(ckpt["model_state_dict"]["turn_dim.fc.weight"].shape) == (64, 128)
    assert tuple(ckpt["model_state_dict"]["id_embedding.weight"].shape) == (201, 64)
    assert "model loaded from" in test_log and re.search(r"test_results   [0-9.]+\t[0-9.]+", test_log)
    # save -> load reproduces the validation metric
    revalid = re.search(r"REVALID ([0-9.]+)", rest)
    again = re.findall(r"valid_results   ([0-9.]+)\t([0-9.]+)", rest)
    assert revalid and len(again) == 1
    assert abs(float(revalid.group(1)) - float(valid[0][0])) < 1e-4 and again[0] == valid[0], (valid, again, revalid.group(1))
    # the recommendation lists: 5 catalogue items per user, none of them in the user's sequence, best first
    lines = open(rec).read().splitlines()
    assert len(lines) == 64 and "recommend: top-5 lists of 64 users" in rest
    from idvs.morec_amd.run import load_dataset
    a = parse_args(common)
    del a.CV_model_load
    users_test = load_dataset(a, False, False)[4]
    seen = {str(u): set(int(i) for i in seq) for u, seq in users_test.items()}
    assert len(seen) == 64
    for line in lines:
        user, items = line.split("\t")
        pairs = [x.split(":") for x in items.split(" ")]
        assert len(pairs) == 5 and all(re.fullmatch(r"N\d+", n) and 1 <= int(n[1:]) <= 200 for n, _ in pairs)
        assert len({n for n, _ in pairs}) == 5 and not ({int(n[1:]) for n, _ in pairs} & seen[user]), line
        assert [float(v) for _, v in pairs] == sorted((float(v) for _, v in pairs), reverse=True)
