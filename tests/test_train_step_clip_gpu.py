"""-m gpu: ``TrainStep(max_grad_norm=, lr_schedule=)`` -- global-norm clipping and the LR schedule inside the fused step, on the smallest
configurations of ``tests/test_train_step_gpu.py`` / ``tests/test_graph_step_gpu.py`` (ID tower, micro text tower), deterministic mode."""
import types

import numpy as np
import pytest
import torch

from idvs.morec_amd import ops
from idvs.morec_amd.lr_schedule import LrSchedule

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(lr=1e-3, fine_tune_lr=1e-4, l2_weight=0.01, fine_tune_l2_weight=0.02, pool_negatives=False)


@pytest.fixture(autouse=True)
def _deterministic():
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(False)


def _restated(t, kind, warmup, total, min_ratio=0.0):
    import math
    if t < warmup:
        return t / warmup
    if kind == "constant":
        return 1.0
    q = min(1.0, (t - warmup) / max(1, total - warmup))
    if kind == "linear":
        return min_ratio + (1.0 - min_ratio) * (1.0 - q)
    return min_ratio + (1.0 - min_ratio) * (1.0 + math.cos(math.pi * q)) / 2.0


def _data(use_modal, steps, seed=0, S=6, T=30, B=5, item_num=40, vocab=512):
    rng = np.random.default_rng(seed)
    pop = rng.random(item_num + 1) + 0.05
    pop[1:] /= pop[1:].sum()
    pop[0] = 1.0
    content = np.zeros((item_num + 1, 2 * T), dtype=np.int64)
    for i in range(1, item_num + 1):
        L = int(rng.integers(3, T + 1))
        content[i, :L] = rng.integers(1, vocab, L)
        content[i, T:T + L] = 1
    batches = []
    for _ in range(steps):
        ids = np.zeros((B, S + 1), dtype=np.int64)
        lm = np.zeros((B, S), dtype=np.float32)
        for b in range(B):
            L = int(rng.integers(2, S + 2))
            ids[b, S + 1 - L:] = rng.integers(1, item_num + 1, L)
            lm[b, S + 1 - L:] = 1
        items = content[ids.reshape(-1)] if use_modal else ids.reshape(-1)
        batches.append(tuple(torch.from_numpy(a).to(DEV) for a in (ids.reshape(-1), items, lm)))
    return pop, batches


def _model(dtype, use_modal, pop, S=6, D=64, T=30, item_num=40):
    """The micro text tower / the ID tower of ``__graft_entry__.smoke`` with deterministic parameters, dropout off."""
    from idvs.morec_amd.model import BertShape, HipBertModel, Model
    from idvs.morec_amd.utils.detgen import det_param
    shape = BertShape.named("micro")
    args = types.SimpleNamespace(max_seq_len=S, embedding_dim=D, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                                 num_words_title=T, num_words_abstract=50, num_words_body=50, news_attributes=["title"],
                                 bert_model_load="bert_micro", word_embedding_dim=shape.hidden_size, compute_dtype=dtype)
    model = Model(args, item_num, use_modal, HipBertModel(shape) if use_modal else None, pop)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(det_param(k, tuple(v.shape))))
    model.eval()
    return model.to(DEV)


def _run(ts, batches):
    losses = [ts.step(*b).clone() for b in batches]
    ts.flush()
    torch.cuda.synchronize()
    return losses


def test_inactive_clip_and_constant_schedule_change_no_bit_in_fp16():
    from idvs.morec_amd.train_step import TrainStep
    pop, batches = _data(True, 3)
    out = []
    for kw in ({}, dict(max_grad_norm=1e9, lr_schedule=LrSchedule("constant"))):
        ts = TrainStep(_model("fp16", True, pop), loss_scale=1024.0, **KW, **kw)
        per_step = []
        for b in batches:
            loss = ts.step(*b).clone()
            ts.flush()
            per_step.append((loss, [g["arena"].data.clone() for g in ts.groups]))
        assert ts.applied_steps() == 3
        out.append(per_step)
    assert out[1] and ts.step_stats()[1:] == (1.0, 1.0) and 0.0 < ts.step_stats()[0] < 1e9
    for (l0, p0), (l1, p1) in zip(*out):
        assert torch.equal(l0, l1)
        for a, b in zip(p0, p1):
            assert torch.equal(a, b)


def test_active_clip_matches_the_autograd_path_with_torch_clip_and_adamw():
    """fp32, one step, threshold at a quarter of the measured norm.  AdamW's first step is ``lr g / (|g| + eps)``: with the default eps it is
    ``+- lr`` whatever the clip coefficient (and amplifies rounding noise of near-zero gradients to a full ``lr``), so the comparison runs
    at eps = 1e-3, inside the range of the gradients, where a missing or per-group clip moves the parameters.  Tolerance: the relative
    1e-4 of ``test_train_step_matches_autograd_model`` for fp32, applied to the parameters, the first moments (0.1 x the clipped gradient)
    and the norm."""
    from idvs.morec_amd.train_step import TrainStep
    pop, batches = _data(True, 1)
    eps = 1e-3
    ref = _model("fp32", True, pop)
    loss = ref(*batches[0], DEV)
    loss.backward()
    named = [(n, p) for n, p in ref.named_parameters() if p.grad is not None and ".pooler." not in n]
    tower = [p for n, p in named if "bert_model" in n]
    rest = [p for n, p in named if "bert_model" not in n]
    norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad.double()) for _, p in named])))
    max_norm = norm / 4.0
    before = {n: p.detach().clone() for n, p in named}
    got_norm = torch.nn.utils.clip_grad_norm_([p for _, p in named], max_norm)
    assert abs(float(got_norm) - norm) / norm < 1e-5
    opt = torch.optim.AdamW([{"params": tower, "lr": KW["fine_tune_lr"], "weight_decay": KW["fine_tune_l2_weight"]},
                             {"params": rest, "lr": KW["lr"], "weight_decay": KW["l2_weight"]}], eps=eps)
    opt.step()
    res = {}
    for clip in (True, False):
        m = _model("fp32", True, pop)
        ts = TrainStep(m, eps=eps, **KW, max_grad_norm=max_norm if clip else 0.0)
        ts.step(*batches[0])
        ts.flush()
        torch.cuda.synchronize()
        res[clip] = (dict(m.named_parameters()), ts)
    ts = res[True][1]
    gn, coef, mult = ts.step_stats()
    print(f"autograd norm {norm:.8g}, fused {gn:.8g}; clip coefficient {coef:.6f}")
    assert abs(gn - norm) / norm < 1e-4 and abs(coef - 0.25) < 1e-4 and mult == 1.0
    worst_p = worst_m = moved = 0.0
    for n, p in named:
        upd = (p.detach() - before[n]).abs().max().item()
        if p.grad.abs().max().item() < 1e-7:      # key biases: the true gradient is zero, what is left is rounding noise
            continue
        a = ts._arena_of(n)["arena"]
        d = (res[True][0][n].detach() - p.detach()).abs().max().item() / (p.detach().abs().max().item() + 1e-12)
        st = opt.state[p]["exp_avg"]
        dm = (a.view(a.exp_avg, n) - st).abs().max().item() / (st.abs().max().item() + 1e-12)
        worst_p, worst_m = max(worst_p, d), max(worst_m, dm)
        assert d < 1e-4 and dm < 1e-4, (n, d, dm)
        # the unclipped step is somewhere else: by a good part of this parameter's own update
        moved = max(moved, (res[False][0][n].detach() - p.detach()).abs().max().item() / (upd + 1e-30))
    print(f"worst relative parameter distance {worst_p:.2e}, first moment {worst_m:.2e}; unclipped step off by {moved:.2f} of an update")
    assert moved > 0.5
    # the gradient arenas' padding is zero (the norm pass reads it)
    for grp in ts.groups:
        a = grp["arena"]
        pad = torch.ones(a.numel, dtype=torch.bool, device=DEV)
        for o, cnt, _ in a.offsets.values():
            pad[o:o + cnt] = False
        assert float(a.grad[pad].abs().sum()) == 0.0 if bool(pad.any()) else True


def test_schedule_multiplier_follows_the_formula_step_by_step():
    from idvs.morec_amd.train_step import TrainStep
    pop, batches = _data(False, 6)
    ts = TrainStep(_model("bf16", False, pop), **KW, lr_schedule=dict(kind="linear", warmup_steps=3, total_steps=6))
    first = [g["arena"].data.clone() for g in ts.groups]
    for t, b in enumerate(batches):
        ts.step(*b)
        gn, coef, mult = ts.step_stats()
        assert mult == np.float32(_restated(t, "linear", 3, 6)) and coef == 1.0 and gn > 0.0, t
        if t == 0:      # multiplier 0: the first step moves the moments and nothing else
            assert all(torch.equal(g["arena"].data, f) for g, f in zip(ts.groups, first))
            assert all(float(g["arena"].exp_avg.abs().max()) > 0.0 for g in ts.groups)
    assert ts.applied_steps() == 6
    assert not any(torch.equal(g["arena"].data, f) for g, f in zip(ts.groups, first))


def test_a_skipped_step_does_not_advance_the_schedule():
    """fp16 with an absurd initial loss scale, as ``test_loss_scaler_skips_overflowing_steps_whole_and_backs_off`` provokes its skips: the
    steps overflow by themselves until the scale fits."""
    from idvs.morec_amd.train_step import TrainStep
    pop, batches = _data(True, 1)
    ts = TrainStep(_model("fp16", True, pop), loss_scale=2.0 ** 40, **KW, max_grad_norm=1.0,
                   lr_schedule=LrSchedule("linear", 3, 6))
    seen_skip = seen_apply = 0
    for i in range(60):
        ts.step(*batches[0])
        h = ts.sp.host()
        assert h.step + h.skipped == i + 1
        if h.apply == 0:
            seen_skip += 1
            assert ts.step_stats()[2] == np.float32(_restated(h.step, "linear", 3, 6))          # the next applied step's, unchanged by the skip
        else:
            seen_apply += 1
            assert ts.step_stats()[2] == np.float32(_restated(h.step - 1, "linear", 3, 6))
        if seen_apply == 4:
            break
    assert seen_skip >= 1 and seen_apply == 4 and ts.applied_steps() == 4
    assert ts.step_stats()[2] == np.float32(_restated(3, "linear", 3, 6)) == 1.0


def test_bf16_gets_a_block_and_every_arena_is_stepped_once_after_the_verdict(monkeypatch):
    from idvs.morec_amd.train_step import TrainStep
    pop, batches = _data(True, 2)
    ts = TrainStep(_model("bf16", True, pop), **KW, max_grad_norm=1.0)
    assert ts.sp is not None and not ts.sp.dynamic and not ts._decide_first
    assert float(ts.sp.loss_scale_dev.item()) == 1.0
    events = []
    real_sp, real_plain, real_ex = ops.adamw_sp_, ops.adamw_, ts.sp.decide_ex_
    monkeypatch.setattr(ops, "adamw_sp_", lambda p, *a, **k: (events.append(("adamw_sp", p.data_ptr(), p.numel())), real_sp(p, *a, **k))[1])
    monkeypatch.setattr(ops, "adamw_", lambda p, *a, **k: (events.append(("adamw", p.data_ptr(), p.numel())), real_plain(p, *a, **k))[1])
    monkeypatch.setattr(ts.sp, "decide_ex_", lambda *a, **k: (events.append(("decide",)), real_ex(*a, **k))[1])
    for i, b in enumerate(batches):
        del events[:]
        ts.step(*b)
        ts.flush()
        assert events[0] == ("decide",) and not any(e[0] == "adamw" for e in events)
        covered = {}
        for e in events[1:]:
            assert e[0] == "adamw_sp"
            for g in ts.groups:
                a = g["arena"].data
                if a.data_ptr() <= e[1] < a.data_ptr() + 4 * a.numel():
                    covered[a.data_ptr()] = covered.get(a.data_ptr(), 0) + e[2]
        assert covered == {g["arena"].data.data_ptr(): g["arena"].numel for g in ts.groups}      # each element once
        assert ts.applied_steps() == i + 1


# ``tests/test_graph_step_gpu.py``: FLOOR["id"] = (max |d loss|, relative parameter distance) added to 10 x the eager run-to-run noise
FLOOR_ID = (2e-3, 4e-3)


def test_graph_replays_advance_the_schedule_and_equal_eager_steps():
    from idvs.morec_amd.train_step import TrainStep
    # as tests/test_graph_step_gpu.py runs its comparisons: the deterministic mode sizes its scratch by allocating inside the first steps,
    # which a capture cannot do -- hence the eager run-to-run noise and the floor instead of equality
    ops.set_deterministic(False)
    pop, batches = _data(False, 6, B=16, item_num=300)
    sched = LrSchedule("linear", 4, 8)
    res = {}
    for mode in ("eager", "eager2", "graph"):
        ts = TrainStep(_model("bf16", False, pop, item_num=300), **KW, graph=(mode == "graph"), max_grad_norm=0.5, lr_schedule=sched)
        assert ts.graph == (mode == "graph")
        losses, mults = [], []
        for b in batches:
            losses.append(float(ts.step_graphed(*b)))
            mults.append(ts.step_stats()[2])
        assert ts.applied_steps() == 6
        if mode == "graph":      # call 0 ran eagerly, call 1 captured and replayed, calls 2 .. 5 replayed: one graph
            assert len([v for v in ts._graphs.values() if v != "seen"]) == 1
        torch.cuda.synchronize()
        res[mode] = (losses, [g["arena"].data.clone() for g in ts.groups], mults)
        ts.close()

    def dist(a, b):
        dl = max(abs(x - y) for x, y in zip(a[0], b[0]))
        dp = max(float((x.double() - y.double()).norm() / y.double().norm()) for x, y in zip(a[1], b[1]))
        return dl, dp
    noise, d = dist(res["eager"], res["eager2"]), dist(res["graph"], res["eager"])
    print(f"graph vs eager with clip + schedule: max |d loss| {d[0]:.2e} (eager run-to-run {noise[0]:.2e}), parameter distance {d[1]:.2e} ({noise[1]:.2e})")
    assert d[0] <= 10 * noise[0] + FLOOR_ID[0] and d[1] <= 10 * noise[1] + FLOOR_ID[1]
    want = [float(np.float32(_restated(t, "linear", 4, 8))) for t in range(6)]
    assert res["graph"][2] == want == res["eager"][2]
    assert len(set(res["graph"][2][1:])) >= 4          # the multiplier differs between replays: nothing of it is frozen in the graph


def test_resume_mid_warmup_repeats_the_uninterrupted_step():
    from idvs.morec_amd.train_step import TrainStep
    pop, batches = _data(True, 3)
    kw = dict(loss_scale=1024.0, max_grad_norm=0.5, lr_schedule=LrSchedule("cosine", 5, 10, 0.1), **KW)
    full = TrainStep(_model("fp16", True, pop), **kw)
    losses = _run(full, batches)
    part_model = _model("fp16", True, pop)
    part = TrainStep(part_model, **kw)
    _run(part, batches[:2])
    saved = ({k: v.detach().clone() for k, v in part_model.state_dict().items()}, part.optimizer_state_dict(), part.scaler_state_dict())
    fresh_model = _model("fp16", True, pop)
    fresh = TrainStep(fresh_model, **kw)
    fresh.load_state_dict(saved[0])
    fresh.load_optimizer_state_dict(saved[1])
    fresh.load_scaler_state_dict(saved[2])
    assert fresh.applied_steps() == 2
    loss3 = _run(fresh, batches[2:])[0]
    assert torch.equal(loss3, losses[2])
    assert fresh.step_stats() == full.step_stats() and fresh.step_stats()[2] == np.float32(_restated(2, "cosine", 5, 10, float(np.float32(0.1))))
    for a, b in zip(fresh.groups, full.groups):
        assert torch.equal(a["arena"].data, b["arena"].data) and torch.equal(a["arena"].exp_avg_sq, b["arena"].exp_avg_sq)
        assert torch.equal(a["arena"].shadow, b["arena"].shadow)
