"""CPU: the pieces the three training drivers of run.py share -- resume (one read of the file), ``save_model(name=...)``, the autograd
step, the early-stop record and the epoch's negatives generator -- each against the literal code it replaced."""
import os
import types

import numpy as np
import pytest
import torch

from idvs.morec_amd.data_utils.utils import save_model
from idvs.morec_amd.lr_schedule import AutogradStepControl, LrSchedule
from idvs.morec_amd.run import EarlyStop, autograd_step, epoch_neg_rng, resume_checkpoint

KEYS = {"model_state_dict", "optimizer", "rng_state", "cuda_rng_state", "scaler_state"}


def _net():
    return torch.nn.Sequential(torch.nn.Linear(4, 5), torch.nn.Linear(5, 3))


def test_resume_reads_the_file_once_and_restores_everything(tmp_path, monkeypatch):
    torch.manual_seed(11)
    net = _net()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    net(torch.randn(6, 4)).square().mean().backward()
    opt.step()
    rng = torch.get_rng_state()
    first, second = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(first)
    save_model(4, net, second, opt, rng, None, None, None, extra={"morec_drop_calls": 7})
    want = {k: v.clone() for k, v in net.state_dict().items()}
    torch.manual_seed(999)      # scramble the generator and the weights
    with torch.no_grad():
        for p in net.parameters():
            p.normal_()
    net._drop_calls = 0
    calls, real_load = [], torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: (calls.append(a[0]), real_load(*a, **k))[1])
    args = types.SimpleNamespace(load_ckpt_name="epoch-4.pt")
    ckpt, start_epoch = resume_checkpoint(net, [first, second], args)
    assert calls == [os.path.join(second, "epoch-4.pt")]
    assert start_epoch == 4 and net._drop_calls == 7
    assert torch.equal(torch.get_rng_state(), rng)
    for k, v in net.state_dict().items():
        assert torch.equal(v, want[k]), k
    assert set(ckpt) == KEYS | {"morec_drop_calls"}
    exp_avg = [s["exp_avg"] for s in opt.state_dict()["state"].values()]
    assert all(torch.equal(a, b["exp_avg"]) for a, b in zip(exp_avg, ckpt["optimizer"]["state"].values())) and len(exp_avg) == 4
    # no flag: nothing is read, nothing changes
    assert resume_checkpoint(net, [first], types.SimpleNamespace(load_ckpt_name="None")) == (None, 0) and len(calls) == 1


def test_resume_names_where_it_looked(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = types.SimpleNamespace(load_ckpt_name="epoch-9.pt")
    with pytest.raises(SystemExit) as e:
        resume_checkpoint(_net(), [a], args)
    assert str(e.value) == f"--load_ckpt_name epoch-9.pt: not found under {a}"
    with pytest.raises(SystemExit) as e:
        resume_checkpoint(_net(), [a, b], args)
    assert str(e.value) == f"--load_ckpt_name epoch-9.pt: not found under any of {[a, b]}"


def test_save_model_file_name_keys_and_unwrap(tmp_path):
    net = _net()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    ddp_like = types.SimpleNamespace(module=net)
    d = str(tmp_path)
    p1 = save_model(3, ddp_like, d, opt, torch.get_rng_state(), None, None, None, extra={"morec_drop_calls": 2})
    p2 = save_model(3, ddp_like, d, opt, torch.get_rng_state(), None, None, None, extra={"morec_drop_calls": 2}, name="epoch-3-5.pt")
    assert (p1, p2) == (os.path.join(d, "epoch-3.pt"), os.path.join(d, "epoch-3-5.pt")) and os.path.exists(p1) and os.path.exists(p2)
    for p in (p1, p2):
        ck = torch.load(p, map_location="cpu", weights_only=False)
        assert set(ck) == KEYS | {"morec_drop_calls"} and ck["morec_drop_calls"] == 2 and ck["scaler_state"] == {}
        assert list(ck["model_state_dict"]) == list(net.state_dict())      # the unwrapped module's keys: no "module." prefix
        assert all(torch.equal(v, net.state_dict()[k]) for k, v in ck["model_state_dict"].items())
        assert ck["optimizer"]["param_groups"] == opt.state_dict()["param_groups"]


def _three_steps(through_helper, control):
    torch.manual_seed(5)
    lin = torch.nn.Linear(4, 3)
    opt = torch.optim.AdamW(lin.parameters(), lr=1e-2)
    ctl = AutogradStepControl(opt, None, **control)
    scaler, losses = None, []
    for _ in range(3):
        x = torch.randn(8, 4)
        forward = lambda inp: lin(inp).square().mean()
        if through_helper:
            loss = autograd_step(forward, opt, scaler, ctl, x)
            assert not loss.requires_grad and loss.grad_fn is None
        else:      # the sequence the drivers spelled out before
            opt.zero_grad()
            loss = forward(x)
            (scaler.scale(loss) if scaler is not None else loss).backward()
            ctl.step()
            loss = loss.detach()
        losses.append(loss.clone())
    return lin, opt, losses


@pytest.mark.parametrize("control", [{}, {"max_grad_norm": 0.5, "lr_schedule": LrSchedule("linear", 2, 6, 0.1)}], ids=["plain", "clip+warmup"])
def test_autograd_step_is_the_sequence_it_replaced(control):
    lin_a, opt_a, loss_a = _three_steps(True, control)
    lin_b, opt_b, loss_b = _three_steps(False, control)
    for pa, pb in zip(lin_a.parameters(), lin_b.parameters()):
        assert torch.equal(pa, pb)
    for sa, sb in zip(opt_a.state.values(), opt_b.state.values()):
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert all(torch.equal(a, b) for a, b in zip(loss_a, loss_b))
    assert [g["lr"] for g in opt_a.param_groups] == [g["lr"] for g in opt_b.param_groups]
    # the returned value is the forward's: recompute the first loss from the same seed and input
    torch.manual_seed(5)
    lin = torch.nn.Linear(4, 3)
    assert torch.equal(loss_a[0], lin(torch.randn(8, 4)).square().mean().detach())


def _literal_early_stop(seq, gap, is_early_stop, epochs):
    """The block the drivers carried (``train()`` before the record), state after every element."""
    best, max_epoch, early_stop_count, early_stop_epoch = 0.0, 0, 0, epochs
    out = []
    for now_epoch, hit10 in enumerate(seq, 1):
        need_break = False
        if hit10 > best:
            best, max_epoch, early_stop_count = hit10, now_epoch, 0
        else:
            early_stop_count += 1
            if early_stop_count > gap:
                need_break = is_early_stop
                early_stop_epoch = now_epoch
        out.append((best, max_epoch, early_stop_count, early_stop_epoch, need_break))
    return out


RISING = [0.01 * k for k in range(1, 9)]
SEQS = {"rising": RISING, "flat": [0.3] * 14, "zero": [0.0] * 13, "rise_after_count": [0.2, 0.1, 0.1, 0.1, 0.25, 0.2, 0.2] + [0.1] * 12,
        "ties": [0.1, 0.1, 0.2, 0.2, 0.2, 0.3] + [0.3] * 12, "late_rise": [0.5] + [0.4] * 11 + [0.6] + [0.6] * 8}


@pytest.mark.parametrize("enabled", [True, False])
@pytest.mark.parametrize("gap", [6, 10])
@pytest.mark.parametrize("name", sorted(SEQS))
def test_early_stop_record_matches_the_block_it_replaced(name, gap, enabled):
    seq = SEQS[name]
    want = _literal_early_stop(seq, gap, enabled, epochs=50)
    stop = EarlyStop(gap, enabled, 50)
    for now_epoch, (hit10, w) in enumerate(zip(seq, want), 1):
        improved = stop.update(hit10, now_epoch)
        assert (stop.best, stop.max_epoch, stop.early_stop_count, stop.early_stop_epoch, stop.need_break) == w, (name, now_epoch)
        assert improved == (w[1] == now_epoch)
    if name == "flat":      # the counter has to EXCEED the gap: validations 2 .. gap + 1 do not stop the run, validation gap + 2 does
        assert [w[4] for w in want[:gap + 1]] == [False] * (gap + 1) and want[gap + 1][4] == enabled and want[gap + 1][2] == gap + 1


def test_epoch_neg_rng_is_seed_rank_epoch():
    torch.manual_seed(12345)
    draws = {}
    for rank in (0, 1):
        for epoch in (1, 2):
            got = epoch_neg_rng(rank, epoch).integers(0, 1 << 40, 16)
            want = np.random.default_rng([torch.initial_seed() % (1 << 63), rank, epoch]).integers(0, 1 << 40, 16)
            assert np.array_equal(got, want)
            draws[rank, epoch] = tuple(got)
    assert len(set(draws.values())) == 4
