"""-m gpu: the RoBERTa text tower (position ids counted from the pad token) at model level.
  * g29 (``tests/golden/g29_roberta.npz``: the installed HF ``RobertaModel`` inside the reference's in-batch ``Model`` and its BCE
    ``Model``) under the bounds ``test_model_gpu.py::test_g5_g8_bert_micro_golden`` sets for the same graph at the same size, and the BCE
    loss under ``test_bce.py::test_bce_model_golden``'s;
  * the relation to the BERT tower: on right-padded titles whose real tokens avoid the ids 0 and 1, the BERT tower with the position
    table shifted by two rows computes the same thing;
  * the fused step against the autograd ``Model`` (``test_train_step_gpu.py::test_train_step_matches_autograd_model``'s body and bounds),
    and a captured step replayed against eager steps (``test_graph_step_gpu.py``'s comparison and its text-tower floor);
  * one short driver run per mode that reaches the tower."""
import logging
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
from idvs.morec_amd.model import BertShape, HipBertModel, Model  # noqa: E402
from idvs.morec_amd.utils.detgen import det_normal, det_param  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
G = np.load(os.path.join(GOLDEN_DIR, "g29_roberta.npz"))


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def make_args(**kw):
    d = dict(max_seq_len=20, embedding_dim=64, num_attention_heads=2, drop_rate=0.0, transformer_block=2, num_words_title=30,
             num_words_abstract=50, num_words_body=50, news_attributes=["title"], bert_model_load="roberta_micro", word_embedding_dim=64,
             compute_dtype="fp32")
    d.update(kw)
    return types.SimpleNamespace(**d)


def load_det(module):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    return module


def twin_bound(bound, key, scale=1.0):
    """A bound of g5's that g29 might not admit: if the reference's own fp32 error against its fp64 run (g29's ``*.64`` twins) exceeds
    half the bound, the bound becomes four times that error (it does not for any quantity stored in g29: item vectors 5e-7, loss 8e-7).  ``scale`` turns an absolute error into the bound's units."""
    err = float(np.abs(np.asarray(G[key], np.float64) - G[key + ".64"]).max()) / scale
    return 4 * err if err > bound / 2 else bound


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_g29_roberta_micro_golden(dtype):
    from idvs.morec_amd import engine as _engine
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    shape = BertShape.named("roberta_micro")
    args = make_args(max_seq_len=S, embedding_dim=D, word_embedding_dim=shape.hidden_size, compute_dtype=dtype, num_words_title=T)
    m = load_det(Model(args, item_num, True, HipBertModel(shape), G["pop"])).to(DEV).eval()
    ids = torch.from_numpy(G["ids"]).to(DEV).view(-1)
    items = torch.from_numpy(G["content"][G["ids"].reshape(-1)]).to(DEV)
    lm = torch.from_numpy(G["log_mask"]).to(DEV)
    f32 = dtype == "fp32"
    saved_unpad, _engine.UNPAD_DEFAULT = _engine.UNPAD_DEFAULT, False      # padded layout for the every-slot cotangent (see g5's test)
    try:
        vec = m.bert_encoder(items)
        assert vec.dtype == torch.float32 and np.isfinite(vec.detach().cpu().numpy()).all()
        real = G["ids"].reshape(-1) != 0
        vmax = float(np.abs(G["item_vecs"][real]).max())
        tol_vec = twin_bound(2e-5, "item_vecs", vmax) if f32 else 5e-2
        e_vec = relerr(vec.detach().cpu().numpy()[real], G["item_vecs"][real])
        print(f"g29 {dtype}: item vec err {e_vec:.2e} (bound {tol_vec:.1e})")
        assert e_vec < tol_vec
        R = torch.from_numpy(det_normal("g29.R", (B * (S + 1), D))).to(DEV)
        (vec * R).sum().backward()
        named = dict(m.named_parameters())
        gt = 3e-4 if f32 else 1e-1
        errs = {k: relerr(named[k[len("enc_grad."):]].grad.cpu().numpy(), G[k]) for k in G.files
                if k.startswith("enc_grad.") and not k.endswith(".64")}
        print(f"g29 {dtype}: enc grad errs {errs}")
        assert max(errs.values()) < gt, errs
        pe = "bert_encoder.text_encoders.title.bert_model.embeddings.position_embeddings.weight"
        assert float(named[pe].grad[:2].abs().max()) == 0.0      # row 1 = padding_idx, row 0 is never read
        assert float(named[pe].grad[2 + T:].abs().max()) == 0.0
        for k in [k for k in G.files if k.startswith("enc_grad_norm.") and not k.endswith(".64")]:
            name = k[len("enc_grad_norm."):]
            if "pooler" in name:
                continue
            got = named[name].grad.double().norm().item()
            assert abs(got - float(G[k])) <= (1e-3 if f32 else 1e-1) * float(G[k]) + (1e-4 if f32 else 2e-2), (name, got, float(G[k]))
    finally:
        _engine.UNPAD_DEFAULT = saved_unpad
    # the unpadded layout keeps a title's tokens up to the end of its mask: the position ids still come from the padded ids
    vec_u = m.bert_encoder(items)
    assert relerr(vec_u.detach().cpu().numpy()[real], G["item_vecs"][real]) < tol_vec
    m.zero_grad()
    loss = m(ids, items, lm, DEV)
    print(f"g29 {dtype}: loss {loss.item():.6f} vs {float(G['loss']):.6f} (fp64 {float(G['loss.64']):.6f})")
    assert abs(loss.item() - float(G["loss"])) < (twin_bound(5e-5, "loss") if f32 else 3e-2)
    loss.backward()
    for k in [k for k in G.files if k.startswith("grad_norm.") and not k.endswith(".64")]:
        name = k[len("grad_norm."):]
        if "pooler" in name:
            continue
        got = named[name].grad.double().norm().item()
        assert abs(got - float(G[k])) <= (1e-3 if f32 else 1e-1) * float(G[k]) + (1e-4 if f32 else 2e-2), (name, got, float(G[k]))
    if not f32:
        return
    pool = [k for k in named if "pooler" in k]
    before = {k: p.detach().clone() for k, p in named.items()}
    opt = torch.optim.AdamW([{"params": [p for k, p in named.items() if "bert_model" in k and k not in pool], "lr": 5e-5, "weight_decay": 0.01},
                             {"params": [p for k, p in named.items() if "bert_model" not in k], "lr": 1e-4, "weight_decay": 0.01}])
    opt.step()
    for k in [k for k in G.files if k.startswith("step_delta.")]:
        name = k[len("step_delta."):]
        big = (named[name].grad.abs() > 1e-5).cpu().numpy()
        delta = (named[name].detach() - before[name]).cpu().numpy()
        assert np.abs(delta - G[k])[big].max() < 5e-7, name
    opt.zero_grad()
    loss2 = m(ids, items, lm, DEV)
    assert abs(loss2.item() - float(G["loss_after_step"])) < 1e-4


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_g29_bce_model_golden(dt):
    from idvs.morec_amd.model.bce import BceModel
    S, D, T, item_num, B = (int(v) for v in G["cfg"])
    m = BceModel(make_args(max_seq_len=S, embedding_dim=D, compute_dtype=dt, num_words_title=T), item_num, True,
                 HipBertModel(BertShape.named("roberta_micro")))
    m = load_det(m).cuda().eval()
    x = torch.from_numpy(G["content"][G["bce.items"]]).view(-1, 2 * T).cuda()
    loss = m(x, torch.from_numpy(G["bce.log_mask"]).cuda(), "cuda")
    ref = float(G["bce.loss"])
    print(f"g29 bce {dt}: loss {float(loss.detach()):.6f} vs {ref:.6f} (fp64 {float(G['bce.loss.64']):.6f})")
    assert abs(float(loss.detach()) - ref) < (1e-4 if dt == "fp32" else 3e-2) * max(1.0, abs(ref)), (float(loss.detach()), ref)
    loss.backward()
    for n, p in m.named_parameters():
        if "pooler" in n:
            continue
        r = float(G[f"bce.grad_norm.{n}"])
        got = float(p.grad.double().norm())
        assert abs(got - r) <= (2e-3 if dt == "fp32" else 1e-1) * r + (1e-6 if dt == "fp32" else 2e-2), (n, got, r)


def _relation_models(S, D, T, item_num, pop):
    rs = BertShape.named("roberta_micro")
    bs = BertShape(vocab_size=512, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                   max_position_embeddings=64, type_vocab_size=1, layer_norm_eps=1e-5)
    args = make_args(max_seq_len=S, embedding_dim=D, num_words_title=T)
    mr = load_det(Model(args, item_num, True, HipBertModel(rs), pop))
    mb = Model(make_args(max_seq_len=S, embedding_dim=D, num_words_title=T, bert_model_load="bert_micro"), item_num, True, HipBertModel(bs), pop)
    pe = "bert_encoder.text_encoders.title.bert_model.embeddings.position_embeddings.weight"
    sd = {k: v.clone() for k, v in mr.state_dict().items()}
    sd[pe] = sd[pe][2:66].clone()      # position t of the BERT tower = row t + 2 of the RoBERTa table
    mb.load_state_dict(sd)
    return mr.to(DEV).eval(), mb.to(DEV).eval(), pe


def test_relation_to_the_bert_tower():
    S, D, T, item_num, B = 6, 64, 30, 40, 5
    rng = np.random.default_rng(5)
    pop = rng.random(item_num + 1) + 0.05
    pop[1:] /= pop[1:].sum()
    pop[0] = 1.0
    cr = np.ones((item_num + 1, 2 * T), dtype=np.int64)      # RoBERTa titles: padded with id 1 ...
    cr[:, T:] = 0
    cb = np.zeros((item_num + 1, 2 * T), dtype=np.int64)     # ... the BERT tower's with id 0; the real tokens avoid both
    for i in range(1, item_num + 1):
        L = T if i == 3 else int(rng.integers(3, T + 1))
        toks = rng.integers(2, 512, L)
        cr[i, :L], cb[i, :L] = toks, toks
        cr[i, T:T + L], cb[i, T:T + L] = 1, 1
    cr[0, :T] = 0                                            # the padding item as get_doc_input_bert leaves it
    ids = np.zeros((B, S + 1), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(rng.integers(2, S + 2))
        ids[b, S + 1 - L:] = rng.integers(1, item_num + 1, L)
        lm[b, S + 1 - L:] = 1
    mr, mb, pe = _relation_models(S, D, T, item_num, pop)
    tdev = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    real = torch.from_numpy(ids.reshape(-1) != 0).to(DEV)
    vr, vb = mr.bert_encoder(tdev(cr[ids.reshape(-1)])), mb.bert_encoder(tdev(cb[ids.reshape(-1)]))
    assert torch.equal(vr[real], vb[real])      # pad rows never reach a real row: the same arithmetic on the same numbers
    grads = []
    for m, c in ((mr, cr), (mb, cb)):
        m.zero_grad(set_to_none=True)
        loss = m(tdev(ids).view(-1), tdev(c[ids.reshape(-1)]), tdev(lm), DEV)
        loss.backward()
        grads.append((loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    (lr_, gr), (lb_, gb) = grads
    assert lr_ == lb_
    we = "bert_encoder.text_encoders.title.bert_model.embeddings.word_embeddings.weight"
    for k, g in gb.items():
        a = gr[k]
        if k == pe:
            assert float(a[:2].abs().max()) == 0.0 and float(a[2 + T:].abs().max()) == 0.0
            a, g = a[2:2 + T], g[:T]
        elif k == we:       # each tower skips its own pad row and sees no token of the other's
            a, g = a[2:], g[2:]
        scale = g.abs().max().item() + 1e-12
        if scale < 1e-7:
            continue
        assert (a - g).abs().max().item() / scale < 1e-4, k


def _setup_roberta(dtype, seed=0, S=10, D=128, B=9, item_num=200):
    """``test_train_step_gpu._setup`` on a RoBERTa tower: 66 positions, one token type, eps 1e-5, titles padded with id 1."""
    T = 30
    shape = BertShape(vocab_size=1500, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                      max_position_embeddings=66, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, position_rule="pad_relative")
    args = make_args(max_seq_len=S, embedding_dim=D, num_words_title=T, bert_model_load="roberta_x", word_embedding_dim=128, compute_dtype=dtype)
    rng = np.random.default_rng(seed)
    pop = rng.random(item_num + 1) + 0.05
    pop[1:] /= pop[1:].sum()
    pop[0] = 1.0
    model = load_det(Model(args, item_num, True, HipBertModel(shape), pop))
    content = np.zeros((item_num + 1, 2 * T), dtype=np.int64)
    for i in range(1, item_num + 1):
        L = int(rng.integers(3, T + 1))
        content[i, :T] = 1
        content[i, :L] = rng.integers(1, 1500, L)      # (an id 1 inside a title now and then: a pad token for the rule)
        content[i, T:T + L] = 1
    ids = np.zeros((B, S + 1), dtype=np.int64)
    lm = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        L = int(rng.integers(2, S + 2))
        ids[b, S + 1 - L:] = rng.integers(1, item_num + 1, L)
        lm[b, S + 1 - L:] = 1
    return model.to(DEV).eval(), ids, content[ids.reshape(-1)], lm


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_step_matches_autograd_model_roberta(dtype):
    from idvs.morec_amd.train_step import TrainStep
    model, ids, items, lm = _setup_roberta(dtype)
    tdev = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    loss = model(tdev(ids).view(-1), tdev(items), tdev(lm), DEV)
    loss.backward()
    ref = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    pe = "bert_encoder.text_encoders.title.bert_model.embeddings.position_embeddings.weight"
    assert float(ref[pe][2:32].abs().max()) > 0 and float(ref[pe][:2].abs().max()) == 0.0
    model.zero_grad(set_to_none=True)
    ts = TrainStep(model, lr=1e-4, fine_tune_lr=5e-5, l2_weight=0.01, fine_tune_l2_weight=0.01)
    loss2 = ts.forward_backward(tdev(ids).view(-1), tdev(items), tdev(lm))
    assert abs(loss.item() - loss2.item()) < 1e-6 * max(1, abs(loss.item())) + (0 if dtype == "fp32" else 1e-3)
    for k, g in ref.items():
        got = ts.g[k]
        scale = g.abs().max().item() + 1e-12
        if scale < 1e-7:
            continue
        assert (got - g).abs().max().item() / scale < (1e-4 if dtype == "fp32" else 2e-2), k


# ``tests/test_graph_step_gpu.py``: FLOOR["text"] = (max |d loss|, relative parameter distance), measured there for a text tower in fp16 at
# lr 3e-3 over 8 steps and added to 10 x the eager run-to-run noise; the same recipe over 4 steps of a smaller tower moves no further.
FLOOR_TEXT = (1.5e-2, 3e-2)


@pytest.mark.parametrize("layout", ["padded", "bucketed"])
def test_graph_replays_equal_eager_steps_roberta(layout):
    """Call 0 runs eagerly, call 1 captures and replays, calls 2 and 3 replay: against four eager steps."""
    from idvs.morec_amd import engine
    from idvs.morec_amd.train_step import TrainStep
    B, S, T, D, item_num, steps = 16, 6, 30, 64, 300, 4
    rng = np.random.default_rng(9)
    content = np.zeros((item_num + 1, 2 * T), dtype=np.int64)
    for i in range(1, item_num + 1):
        L = int(rng.integers(3, T + 1))
        content[i, :T] = 1
        content[i, :L] = rng.integers(1, 512, L)
        content[i, 0], content[i, L - 1] = 0, 2
        content[i, T:T + L] = 1
    ids_all = rng.integers(1, item_num + 1, (steps, B, S + 1))
    pop = np.bincount(ids_all.reshape(-1), minlength=item_num + 1).astype(np.float64) + 1.0
    pop /= pop[1:].sum()
    pop[0] = 1.0
    shape = BertShape.named("roberta_micro")
    from idvs.morec_amd import ops
    saved, saved_det = engine.UNPAD_DEFAULT, ops.DETERMINISTIC
    res = {}
    try:
        engine.UNPAD_DEFAULT = layout != "padded"
        ops.set_deterministic(False)      # (the deterministic mode cannot size its scratch inside a capture: tests/test_train_step_clip_gpu.py)
        for mode in ("eager", "eager2", "graph"):
            args = make_args(max_seq_len=S, embedding_dim=D, num_words_title=T, compute_dtype="fp16")
            torch.manual_seed(7)
            m = Model(args, item_num, True, HipBertModel(shape, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), pop).to(DEV).train()
            ts = TrainStep(m, lr=3e-3, fine_tune_lr=3e-3, l2_weight=0.01, fine_tune_l2_weight=0.01, pool_negatives=False, loss_scale=1024.0,
                           graph=(mode == "graph"))
            losses = []
            for i in range(steps):
                rows = content[ids_all[i].reshape(-1)]
                pack = None
                if layout == "bucketed":
                    hp = engine.token_packing_host(rows[:, T:], rows[:, :T], pad_to=128 if mode == "graph" else 0)
                    pack = tuple(t.to(DEV) for t in hp)
                fn = ts.step_graphed if mode == "graph" else ts.step
                losses.append(float(fn(torch.from_numpy(ids_all[i]).to(DEV).view(-1), torch.from_numpy(rows).to(DEV),
                                       torch.ones(B, S, device=DEV), token_packing=pack)))
            if mode == "graph":
                n_graphs = len([v for v in ts._graphs.values() if v != "seen"])
                assert 1 <= n_graphs <= 3 and ts.sp.host().step == steps
            torch.cuda.synchronize()
            res[mode] = (losses, [g["arena"].data.clone() for g in ts.groups])
            ts.close()
    finally:
        engine.UNPAD_DEFAULT = saved
        ops.set_deterministic(saved_det)

    def dist(a, b):
        dl = max(abs(x - y) for x, y in zip(a[0], b[0]))
        dp = max(float((x.double() - y.double()).norm() / y.double().norm()) for x, y in zip(a[1], b[1]))
        return dl, dp
    noise, d = dist(res["eager"], res["eager2"]), dist(res["graph"], res["eager"])
    print(f"roberta fp16 {layout}: graph vs eager over {steps} steps: max |d loss| {d[0]:.2e} (eager run-to-run {noise[0]:.2e}), "
          f"parameter distance {d[1]:.2e} ({noise[1]:.2e})")
    assert all(np.isfinite(res["graph"][0]))
    assert d[0] <= 10 * noise[0] + FLOOR_TEXT[0] and d[1] <= 10 * noise[1] + FLOOR_TEXT[1]


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
    m = re.search(r"epoch 1: \d+ steps, mean loss ([0-9.]+)", log)
    assert m, log[-2000:]
    assert np.isfinite(float(m.group(1)))
    return float(m.group(1))


SMOKE = ["--synthetic", "48", "--synthetic_items", "60", "--bert_model_load", "roberta_micro", "--freeze_paras_before", "0", "--batch_size", "16",
         "--embedding_dim", "64", "--max_seq_len", "6", "--lr", "1e-3", "--fine_tune_lr", "1e-4", "--local_rank", "0", "--epoch", "1",
         "--num_workers", "0"]      # (collate inline: forking twelve loader workers out of the suite's process takes seconds per run)


def test_driver_train_test_recommend_cold_new(tmp_path):
    common = SMOKE + ["--item_tower", "modal", "--checkpoint_root", str(tmp_path)]
    log = _main(common + ["--max_steps", "3"])
    _mean_loss(log)
    assert "valid_results" in log
    ckpt = ["--load_ckpt_name", "epoch-1.pt"]
    assert re.search(r"test_results   [0-9.]+\t[0-9.]+", _main(common + ["--mode", "test"] + ckpt))
    rec = str(tmp_path / "top5.tsv")
    _main(common + ["--mode", "recommend", "--topk", "5", "--recommend_out", rec] + ckpt)
    assert len(open(rec).read().splitlines()) == 48
    log = _main(common + ["--mode", "test", "--cold_seqs", str(tmp_path / "cold.tsv"), "--new_seqs", str(tmp_path / "new.tsv")] + ckpt)
    for tag in ("cold_results", "new_results"):
        assert tag in log, log[-1500:]


@pytest.mark.parametrize("tower", ["modal_add", "modal_cat"])
def test_driver_fusion_towers(tmp_path, tower):
    _mean_loss(_main(SMOKE + ["--item_tower", tower, "--loss", "bce", "--max_steps", "3", "--checkpoint_root", str(tmp_path)]))


def test_driver_bce_loss(tmp_path):
    _mean_loss(_main(SMOKE + ["--item_tower", "modal", "--loss", "bce", "--max_steps", "3", "--checkpoint_root", str(tmp_path)]))


def test_driver_dssm(tmp_path):
    log = _main(SMOKE + ["--arch", "dssm", "--item_tower", "modal", "--neg_num", "2", "--max_steps", "4", "--logging_num", "1000",
                         "--checkpoint_root", str(tmp_path)])
    losses = [float(x) for x in re.findall(r"batch loss ([0-9.]+),", log)]
    assert len(losses) == 4 and np.isfinite(losses).all(), log[-1500:]
    assert re.search(r"test_results   [0-9.]+\t[0-9.]+", log)


@pytest.mark.parametrize("arch,tower", [("two_stage", "modal"), ("id_two_stage", "modal_add")])
def test_driver_two_stage_stage1(tmp_path, arch, tower):
    feats = str(tmp_path / "features.npy")
    log = _main(SMOKE + ["--arch", arch, "--item_tower", tower, "--save_features", feats, "--checkpoint_root", str(tmp_path)])
    assert "stage 1" in log
    _mean_loss(log)
    table = np.load(feats)
    assert table.shape == (61, 64) and np.isfinite(table).all() and float(np.abs(table[1:]).max()) > 0


def test_driver_fused_step_graph(tmp_path):
    """``--fused_step --graph`` in a child process (a stepper's captured graphs live as long as its process).  The child runs the driver's
    default summation mode whatever this process holds: ``import bench`` (other test modules do) puts ``MOREC_DETERMINISTIC=1`` into the
    environment, and the deterministic mode cannot size its partial-row scratch inside a capture -- for any tower (the graph tests of
    ``test_graph_step_gpu.py`` / ``test_train_step_clip_gpu.py`` run with the mode off for the same reason; ``test_bench_launch.py``
    cleans its child's environment the same way)."""
    argv = SMOKE + ["--item_tower", "modal", "--fused_step", "--graph", "--compute_dtype", "bf16", "--max_steps", "6",
                    "--checkpoint_root", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k != "MOREC_DETERMINISTIC"}
    res = subprocess.run([sys.executable, "-m", "idvs.morec_amd.run"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=240, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    _mean_loss(res.stderr)
