"""CPU: global-norm gradient clipping and the LR schedule -- the command line, the C-ABI's argument checks (nothing is launched), the
layout of the step block, the host form of the schedule formula and the glue of the autograd paths."""
import ctypes as C
import math

import pytest
import torch

from idvs.morec_amd import _lib
from idvs.morec_amd.lr_schedule import AutogradStepControl, LrSchedule, lr_multiplier, schedule_from_args


def test_flags_default_off_and_reach_both_paths():
    from idvs.morec_amd.parameters import parse_args
    from idvs.morec_amd.run import autograd_step_control, clip_schedule_kwargs
    a = parse_args([])
    assert a.max_grad_norm == 0.0 and a.lr_schedule == "constant" and a.warmup_steps == 0 and a.min_lr_ratio == 0.0
    assert clip_schedule_kwargs(a, 100) == {"max_grad_norm": 0.0, "lr_schedule": None}
    a = parse_args(["--max_grad_norm", "1.5", "--lr_schedule", "cosine", "--warmup_steps", "7", "--min_lr_ratio", "0.1"])
    kw = clip_schedule_kwargs(a, 120)
    assert kw == {"max_grad_norm": 1.5, "lr_schedule": LrSchedule("cosine", 7, 120, 0.1)}
    # the keyword names are TrainStep's
    import inspect
    from idvs.morec_amd.train_step import TrainStep
    sig = inspect.signature(TrainStep.__init__).parameters
    assert sig["max_grad_norm"].default == 0.0 and sig["lr_schedule"].default is None
    # warmup alone is a schedule (constant after it)
    assert schedule_from_args(parse_args(["--warmup_steps", "3"]), 10) == LrSchedule("constant", 3, 10, 0.0)
    with pytest.raises(SystemExit):
        parse_args(["--lr_schedule", "step"])
    # autograd paths: the helper carries the same values
    lin = torch.nn.Linear(2, 1)
    opt = torch.optim.AdamW(lin.parameters(), lr=1e-2)
    ctl = autograd_step_control(a, opt, None, 120)
    assert ctl.max_grad_norm == 1.5 and ctl.schedule == LrSchedule("cosine", 7, 120, 0.1) and ctl.scheduler is not None
    off = autograd_step_control(parse_args([]), torch.optim.AdamW(lin.parameters(), lr=1e-2), None, 120)
    assert off.max_grad_norm == 0.0 and off.scheduler is None


def test_step_block_layout_is_unchanged():
    S = _lib.StepParams
    assert C.sizeof(S) == 64
    want = {"step": 0, "found_inf": 4, "growth_tracker": 8, "skipped": 12, "loss_scale": 16, "inv_scale": 20, "bc1": 24, "bc2": 28,
            "apply": 32, "drop_seed": 40, "drop_seed_mixed": 48}
    for name, off in want.items():
        assert getattr(S, name).offset == off, name
    # the three words that used to be padding
    assert (S.ctl_flags.offset, S.clip_coef.offset, S.lr_mult.offset) == (36, 56, 60)
    assert C.sizeof(_lib.LrSchedule) == 16


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    h = _lib.lib()
    ok = C.c_void_p(4096)      # never dereferenced: every call below is refused on its arguments
    # morec_grad_norm_check(grad, n, sp, partials, slot, n_slots, stream)
    assert h.morec_grad_norm_check(None, 8, ok, ok, 0, 16, None) == -1
    assert h.morec_grad_norm_check(ok, 8, None, ok, 0, 16, None) == -1
    assert h.morec_grad_norm_check(ok, 8, ok, None, 0, 16, None) == -1
    assert h.morec_grad_norm_check(ok, 6, ok, ok, 0, 16, None) == -2            # n % 4
    assert h.morec_grad_norm_check(C.c_void_p(4100), 8, ok, ok, 0, 16, None) == -2      # grad off 16 bytes
    assert h.morec_grad_norm_check(ok, 8, ok, ok, 16, 16, None) == -1           # the partials would run past the buffer
    assert h.morec_grad_norm_check(ok, 4096 * 4, ok, ok, 1, 16, None) == -1     # 16 blocks into 15 slots
    assert h.morec_grad_norm_check(ok, 0, ok, ok, 0, 0, None) == 0              # empty arena: nothing to do
    # slots are a function of n alone: one per 1024 elements, capped
    nb = h.morec_grad_norm_blocks
    assert (nb(0), nb(4), nb(1024), nb(1028), nb(2048 * 1024), nb(2048 * 1024 + 4), nb(1 << 30)) == (0, 1, 1, 2, 2048, 2048, 2048)
    # morec_step_decide_ex(sp, b1, b2, growth, backoff, interval, dynamic, partials, n_partials, max_norm, sched, grad_norm_out, stream)
    base = (0.9, 0.999, 2.0, 0.5, 2000, 1)
    assert h.morec_step_decide_ex(None, *base, ok, 4, 1.0, None, None, None) == -1
    assert h.morec_step_decide_ex(ok, 0.9, 0.999, 2.0, 0.5, 0, 1, ok, 4, 1.0, None, None, None) == -1       # as morec_step_decide: interval < 1
    assert h.morec_step_decide_ex(ok, 0.9, 0.999, 0.5, 0.5, 2000, 1, ok, 4, 1.0, None, None, None) == -1    # growth < 1
    assert h.morec_step_decide_ex(ok, *base, None, 4, 0.0, None, None, None) == -1       # partials announced, none given
    assert h.morec_step_decide_ex(ok, *base, None, 0, 1.0, None, None, None) == -1       # clipping without a norm
    assert h.morec_step_decide_ex(ok, *base, ok, 0, 1.0, None, None, None) == -1
    assert h.morec_step_decide_ex(ok, *base, ok, 4, float("nan"), None, None, None) == -1
    assert h.morec_step_decide_ex(ok, *base, C.c_void_p(4098), 4, 1.0, None, None, None) == -2
    assert h.morec_step_decide_ex(ok, *base, ok, 4, 1.0, None, C.c_void_p(4098), None) == -2
    for bad in (_lib.LrSchedule(3, 0, 10, 0.0), _lib.LrSchedule(-1, 0, 10, 0.0), _lib.LrSchedule(1, -1, 10, 0.0),
                _lib.LrSchedule(1, 0, 10, 1.5), _lib.LrSchedule(1, 0, 10, -0.1), _lib.LrSchedule(2, 11, 10, 0.0)):
        assert h.morec_step_decide_ex(ok, *base, ok, 4, 1.0, C.byref(bad), None, None) == -1


def _restated(t, kind, warmup, total, min_ratio):
    """The formula of ``include/morec_hip.h`` (at ``morec_lr_schedule``), written out again."""
    if t < warmup:
        return t / warmup
    if kind == "constant":
        return 1.0
    q = (t - warmup) / max(1, total - warmup)
    q = 1.0 if q > 1.0 else q
    if kind == "linear":
        return min_ratio + (1.0 - min_ratio) * (1.0 - q)
    return min_ratio + (1.0 - min_ratio) * (1.0 + math.cos(math.pi * q)) / 2.0


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
@pytest.mark.parametrize("warmup", [0, 3])
@pytest.mark.parametrize("min_ratio", [0.0, 0.1])
def test_schedule_function_against_the_restated_formula(kind, warmup, min_ratio):
    total = 11
    steps = sorted({0, 1, max(0, warmup - 1), warmup, warmup + 1, total - 1, total, total + 5})
    s = LrSchedule(kind, warmup, total, min_ratio)
    for t in steps:
        want = _restated(t, kind, warmup, total, min_ratio)
        assert s.multiplier(t) == pytest.approx(want, rel=0, abs=1e-15), (t, kind)
        assert lr_multiplier(t, kind, warmup, total, min_ratio) == s.multiplier(t)
    # the landmarks, spelled out
    if warmup:
        assert s.multiplier(0) == 0.0 and s.multiplier(1) == 1 / 3 and s.multiplier(warmup) == 1.0
    else:
        assert s.multiplier(0) == 1.0
    if kind == "constant":
        assert s.multiplier(total + 5) == 1.0
    else:
        assert s.multiplier(total) == pytest.approx(min_ratio, abs=1e-15) and s.multiplier(total + 5) == s.multiplier(total)
        assert s.multiplier(total - 1) > s.multiplier(total)


def test_schedule_refuses_what_the_kernel_refuses():
    for bad in (dict(kind="step"), dict(kind="linear", warmup_steps=-1, total_steps=5), dict(kind="linear", min_ratio=1.5, total_steps=5),
                dict(kind="cosine", warmup_steps=6, total_steps=5)):
        with pytest.raises(ValueError):
            LrSchedule(**bad)
    assert LrSchedule.coerce(dict(kind="linear", warmup_steps=2, total_steps=5)) == LrSchedule("linear", 2, 5, 0.0)
    c = LrSchedule("cosine", 2, 9, 0.25).c_struct()
    assert (c.kind, c.warmup_steps, c.total_steps, c.min_ratio) == (_lib.LR_COSINE, 2, 9, 0.25)


def test_autograd_glue_equals_a_hand_written_clip_and_adamw_loop():
    """Two-parameter ``nn.Linear`` on the CPU, 4 steps: ``AutogradStepControl`` (clip + ``LambdaLR``) against ``clip_grad_norm_`` +
    ``AdamW`` with the learning rate of each step set by hand from the restated formula."""
    torch.manual_seed(0)
    x, y = torch.randn(16, 1, dtype=torch.float64), torch.randn(16, 1, dtype=torch.float64)
    sched = LrSchedule("linear", 2, 4, 0.1)
    max_norm, lr, wd = 0.05, 1e-2, 0.1

    def model():
        torch.manual_seed(1)
        return torch.nn.Linear(1, 1).double()      # weight + bias: the norm runs over two tensors

    a = model()
    opt_a = torch.optim.AdamW(a.parameters(), lr=lr, weight_decay=wd)
    ctl = AutogradStepControl(opt_a, None, max_grad_norm=max_norm, lr_schedule=sched)
    b = model()
    opt_b = torch.optim.AdamW(b.parameters(), lr=lr, weight_decay=wd)
    clipped = 0
    for t in range(4):
        assert ctl.lr_mult() == _restated(t, "linear", 2, 4, 0.1)
        opt_a.zero_grad()
        ((a(x) - y) ** 2).mean().backward()
        ctl.step()
        opt_b.zero_grad()
        ((b(x) - y) ** 2).mean().backward()
        norm = torch.nn.utils.clip_grad_norm_(list(b.parameters()), max_norm)
        clipped += int(float(norm) > max_norm)
        for g in opt_b.param_groups:
            g["lr"] = lr * _restated(t, "linear", 2, 4, 0.1)
        opt_b.step()
        assert float(ctl.last_norm) == float(norm)
        assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias), t
    assert clipped == 4      # the clip was active at every step
    # a resumed optimizer puts the schedule where it stood
    c = model()
    opt_c = torch.optim.AdamW(c.parameters(), lr=lr, weight_decay=wd)
    ctl_c = AutogradStepControl(opt_c, None, max_grad_norm=max_norm, lr_schedule=sched)
    opt_c.load_state_dict(opt_a.state_dict())
    ctl_c.resume_from_optimizer()
    assert ctl_c.scheduler.last_epoch == 4 and ctl_c.lr_mult() == ctl.lr_mult()
    assert opt_c.param_groups[0]["lr"] == pytest.approx(lr * _restated(4, "linear", 2, 4, 0.1))
    # off: the step is the optimizer's own
    d = model()
    opt_d = torch.optim.AdamW(d.parameters(), lr=lr, weight_decay=wd)
    off = AutogradStepControl(opt_d, None)
    e = model()
    opt_e = torch.optim.AdamW(e.parameters(), lr=lr, weight_decay=wd)
    for m, stepper in ((d, off.step), (e, opt_e.step)):
        ((m(x) - y) ** 2).mean().backward()
        stepper()
    assert torch.equal(d.weight, e.weight)


def test_autograd_glue_does_not_advance_the_schedule_over_a_step_the_scaler_skipped():
    lin = torch.nn.Linear(1, 1)
    opt = torch.optim.AdamW(lin.parameters(), lr=1e-2)
    scaler = torch.amp.GradScaler("cpu", init_scale=4.0)
    ctl = AutogradStepControl(opt, scaler, max_grad_norm=1.0, lr_schedule=LrSchedule("linear", 2, 4))
    x = torch.ones(2, 1)
    seen = []
    for it in range(4):
        opt.zero_grad()
        scaler.scale(lin(x).sum()).backward()
        if it == 1:
            lin.weight.grad[0, 0] = float("inf")
        before = lin.weight.detach().clone()
        ctl.step()
        seen.append((ctl.scheduler.last_epoch, ctl.lr_mult(), scaler.get_scale()))
        assert torch.equal(before, lin.weight.detach()) == (it in (0, 1))      # step 0 runs at multiplier 0, step 1 is skipped
    assert seen == [(1, 0.5, 4.0), (1, 0.5, 2.0), (2, 1.0, 2.0), (3, 0.5, 2.0)]
