"""-m gpu: ``morec_grad_norm_check`` + ``morec_step_decide_ex`` + ``morec_adamw_sp`` -- global-norm gradient clipping and the LR schedule
decided on the device.  Kernel level: the norm against fp64, bit-reproducibility, the overflow protocol, the clip coefficient, the zero-words
rule of the step block, and five steps over two arenas against ``torch.optim.AdamW`` + ``clip_grad_norm_`` + ``LambdaLR`` in fp64.

Geometry of the norm pass (``csrc/optim.hip``): blocks = min(ceil(n / 1024), 2048) of 256 threads, one float4 per thread and trip, so a
thread makes k = ceil(n / 4 / (256 blocks)) trips.  Additions on the longest fp32 chain into one partial: 2 inside a float4
((x^2 + y^2) + (z^2 + w^2)), k into the thread's accumulator, 6 in the wavefront's butterfly, 3 over the block's four wavefronts: c = k + 11.
The partials are folded in double.  All terms are non-negative, so recursive summation is off by at most (c + 1) 2^-24 relative on the total
(the + 1: the rounding of each square); the norm is its square root (half the relative error) rounded to fp32 once more (2^-24)."""
import numpy as np
import pytest
import torch

from idvs.morec_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL_GRID = 2048 * 256 * 4      # elements one trip of the whole grid covers


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def rnd(n, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + n)
    return (torch.randn(n, generator=g) * scale).to(DEV)


def _chain(n):
    blocks = min((n // 4 + 255) // 256, 2048)
    k = -(-(n // 4) // (256 * blocks))
    return k + 11


def _block(scale=1.0, slots=8192, **kw):
    sp = ops.StepParams(DEV, init_scale=scale, **kw)
    sp.reserve_partials(slots)
    return sp


# n = 4: one float4; 252: less than a block; 1024: exactly one block; FULL_GRID + 4: the grid-stride loop wraps once (k = 2);
# 4096 * 3 + 8: not a multiple of the block's span of 1024
@pytest.mark.parametrize("n", [4, 252, 1024, FULL_GRID + 4, 4096 * 3 + 8])
@pytest.mark.parametrize("scale", [1.0, 65536.0])
def test_grad_norm_against_fp64(n, scale):
    c = _chain(n)
    assert c == (13 if n > FULL_GRID else 12)
    bound = (c + 1) * 2.0 ** -24
    assert 2 * bound <= 1e-5
    g = rnd(n, scale=1e-2, seed=1)
    ref = float(np.linalg.norm(g.cpu().numpy().astype(np.float64)))
    sp = _block(scale)
    slots = sp.norm_slots(n)
    assert slots == min((n // 4 + 255) // 256, 2048)
    sp.norm_check_(g * scale, 0)          # (a power of two: the scaled gradients are exact, and so is the kernel's unscaling)
    sp.decide_ex_(0.9, 0.999, slots, 1.0)
    got = sp.grad_norm()
    err = abs(got - ref) / ref
    print(f"n {n} scale {scale:g}: norm {got:.9g} vs fp64 {ref:.9g}, relative error {err:.2e} (bound x 2: {2 * bound:.2e}, c = {c})")
    assert err <= 2 * bound
    h = sp.host()
    assert h.apply == 1 and h.step == 1 and h.found_inf == 0 and h.ctl_flags == _lib.SP_CLIP
    # the partials themselves: their fp64 sum is the total
    tot = float(sp.partials[:slots].double().sum())
    assert abs(tot - ref * ref) / (ref * ref) <= bound


def test_norm_is_bit_reproducible_and_independent_of_other_slots():
    nA, nB = 4096 * 5 + 8, FULL_GRID + 4096 + 4
    gA, gB = rnd(nA, 1e-2, 1), rnd(nB, 1e-2, 2)
    runs = []
    for first_a in (False, False, True):
        sp = _block(1.0)
        sA, sB = sp.norm_slots(nA), sp.norm_slots(nB)
        if first_a:                       # arena A into the slots in front, B behind them
            sp.norm_check_(gA, 0)
            sp.norm_check_(gB, sA)
            pB = sp.partials[sA:sA + sB].clone()
            sp2 = _block(1.0)             # ... and the norm of B alone, from where A left it
            sp2.partials[:sB].copy_(pB)
            sp2.decide_ex_(0.9, 0.999, sB, 1.0)
            runs.append((pB, sp2.partials[-1:].clone()))
        else:
            sp.norm_check_(gB, 0)
            pB = sp.partials[:sB].clone()
            sp.decide_ex_(0.9, 0.999, sB, 1.0)
            runs.append((pB, sp.partials[-1:].clone()))
    for pB, nrm in runs[1:]:
        assert torch.equal(pB.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(nrm.view(torch.int32), runs[0][1].view(torch.int32))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_overflow_protocol_through_the_new_entry_points(bad, where):
    n = 4096 * 2 + 8
    p, g = rnd(n), rnd(n, 1e-2, 1)
    m, v = rnd(n, 1e-3, 2), rnd(n, 1e-3, 3).abs()
    shadow = p.to(torch.bfloat16)
    sp = _block(1024.0, growth_interval=2)
    slots = sp.norm_slots(n)
    gs = g * 1024.0
    sp.norm_check_(gs, 0)
    sp.decide_ex_(0.9, 0.999, slots, 1.0, None)
    ops.adamw_sp_(p, gs, m, v, shadow, 1e-3, 0.9, 0.999, 1e-8, 0.01, sp)
    h = sp.host()
    assert h.apply == 1 and h.step == 1 and h.loss_scale == 1024.0
    snap = [t.clone() for t in (p, m, v, shadow)]
    gs = gs.clone()
    gs[{"first": 0, "middle": n // 2 + 1, "last": n - 1}[where]] = bad
    sp.norm_check_(gs, 0)
    sp.decide_ex_(0.9, 0.999, slots, 1.0, None)
    ops.adamw_sp_(p, gs, m, v, shadow, 1e-3, 0.9, 0.999, 1e-8, 0.01, sp)
    h = sp.host()
    assert h.apply == 0 and h.skipped == 1 and h.step == 1 and h.found_inf == 0
    assert h.loss_scale == 512.0 and float(sp.loss_scale_dev.item()) == 512.0
    for t, s in zip((p, m, v, shadow), snap):
        assert torch.equal(t, s)


def _two_updates(max_norm_of, n=4096 * 3 + 8):
    """The same AdamW launch after plain ``decide_`` and after ``decide_ex_`` with ``max_norm = max_norm_of(norm)``."""
    g = rnd(n, 1e-2, 1)
    norm = float(np.linalg.norm(g.cpu().numpy().astype(np.float64)))
    out = []
    for ex in (False, True):
        p, m, v = rnd(n), rnd(n, 1e-3, 2), rnd(n, 1e-3, 3).abs()
        shadow = torch.empty(n, device=DEV, dtype=torch.float16)
        sp = _block(256.0)
        gs = g * 256.0
        if ex:
            sp.norm_check_(gs, 0)
            sp.decide_ex_(0.9, 0.999, sp.norm_slots(n), max_norm_of(norm))
        else:
            sp.check_finite_(gs)
            sp.decide_(0.9, 0.999)
        ops.adamw_sp_(p, gs, m, v, shadow, 1e-3, 0.9, 0.999, 1e-8, 0.01, sp)
        out.append((p, m, v, shadow, sp))
    return norm, out


def test_clip_coefficient_inactive_active_and_off():
    # norm / threshold = 0.5: the coefficient is exactly 1 and the update is the plain one, bit for bit
    norm, (plain, ex) = _two_updates(lambda nrm: 2.0 * nrm)
    h = ex[4].host()
    assert h.ctl_flags == _lib.SP_CLIP and h.clip_coef == 1.0 and ex[4].clip_coef() == 1.0
    for a, b in zip(plain[:4], ex[:4]):
        assert torch.equal(a, b)
    # norm / threshold = 4
    norm, (plain, ex) = _two_updates(lambda nrm: nrm / 4.0)
    want = (norm / 4.0) / (norm + 1e-6)
    got = ex[4].clip_coef()
    assert abs(got - want) / want <= 1e-6, (got, want)
    assert abs(ex[4].grad_norm() - norm) / norm <= 2 * (_chain(4096 * 3 + 8) + 1) * 2.0 ** -24
    assert not torch.equal(plain[0], ex[0])
    assert rel(ex[1] - 0.9 * rnd(4096 * 3 + 8, 1e-3, 2), (plain[1] - 0.9 * rnd(4096 * 3 + 8, 1e-3, 2)) * want) < 1e-4      # (1 - b1) g, clipped
    # max_norm = 0: off -- flags clear, bit-equal to plain, the norm is still reported
    norm, (plain, ex) = _two_updates(lambda nrm: 0.0)
    h = ex[4].host()
    assert h.ctl_flags == 0 and ex[4].clip_coef() == 1.0 and ex[4].lr_mult() == 1.0
    for a, b in zip(plain[:4], ex[:4]):
        assert torch.equal(a, b)
    assert abs(ex[4].grad_norm() - norm) / norm <= 1e-5


def test_zero_words_block_drives_adamw_sp_like_host_scalars():
    """``morec_step_params_init`` + ``morec_step_decide`` (the three formerly spare words zero) + ``morec_adamw_sp`` == ``morec_adamw`` with the
    same step and scale as host scalars, bit for bit."""
    n = 4096 * 3 + 8
    g = rnd(n, 1e-2, 1) * 512.0
    res = []
    for block in (True, False):
        p, m, v = rnd(n), rnd(n, 1e-3, 2), rnd(n, 1e-3, 3).abs()
        shadow = torch.empty(n, device=DEV, dtype=torch.bfloat16)
        if block:
            sp = ops.StepParams(DEV, init_scale=512.0, step=2)
            h = sp.host()
            assert (h.ctl_flags, h.clip_coef, h.lr_mult) == (0, 0.0, 0.0)
            sp.check_finite_(g)
            sp.decide_(0.9, 0.999)
            h = sp.host()
            assert (h.ctl_flags, h.clip_coef, h.lr_mult, h.step) == (0, 0.0, 0.0, 3)
            ops.adamw_sp_(p, g, m, v, shadow, 1e-4, 0.9, 0.999, 1e-8, 0.01, sp)
        else:
            ops.adamw_(p, g, m, v, shadow, 1e-4, 0.9, 0.999, 1e-8, 0.01, 3, grad_scale=1.0 / 512.0)
        res.append((p, m, v, shadow))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_decide_ex_after_a_block_was_driven_plain_and_back():
    """Flags do not outlive the decision that set them: ``decide_`` after ``decide_ex_`` clears them (a stale coefficient is never applied)."""
    n = 1024
    g = rnd(n, 1e-2, 1)
    sp = _block(1.0)
    sp.norm_check_(g, 0)
    sp.decide_ex_(0.9, 0.999, 1, 1e-3, ops_schedule("linear", 2, 5, 0.0))
    h = sp.host()
    assert h.ctl_flags == (_lib.SP_CLIP | _lib.SP_LR_MULT) and h.lr_mult == 0.0 and 0.0 < h.clip_coef < 1.0
    sp.check_finite_(g)
    sp.decide_(0.9, 0.999)
    h = sp.host()
    assert h.ctl_flags == 0 and h.step == 2 and sp.clip_coef() == 1.0 and sp.lr_mult() == 1.0


def ops_schedule(kind, warmup, total, min_ratio):
    from idvs.morec_amd.lr_schedule import LrSchedule
    return LrSchedule(kind, warmup, total, min_ratio)


def _restated(t, kind, warmup, total, min_ratio):
    import math
    if t < warmup:
        return t / warmup
    if kind == "constant":
        return 1.0
    q = min(1.0, (t - warmup) / max(1, total - warmup))
    if kind == "linear":
        return min_ratio + (1.0 - min_ratio) * (1.0 - q)
    return min_ratio + (1.0 - min_ratio) * (1.0 + math.cos(math.pi * q)) / 2.0


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_device_schedule_equals_the_formula(kind):
    """The multiplier the kernel stores, at every applied-step count from 0 to total + 2 (warmup 3, total 7, floor 0.1); a skipped step
    (non-finite norm) does not advance it."""
    sched = ops_schedule(kind, 3, 7, 0.1)
    r = float(np.float32(0.1))      # morec_lr_schedule.min_ratio is a float: the kernel evaluates the formula (in double) with THAT value
    g = rnd(1024, 1e-2, 1)
    bad = g.clone()
    bad[5] = float("inf")
    sp = _block(1.0, dynamic=False)
    t = 0
    for it in range(11):
        skip = it in (2, 6)
        sp.norm_check_(bad if skip else g, 0)
        sp.decide_ex_(0.9, 0.999, 1, 0.0, sched)
        h = sp.host()
        assert h.ctl_flags == _lib.SP_LR_MULT and h.apply == (0 if skip else 1) and h.step == t + (0 if skip else 1)
        assert h.lr_mult == np.float32(_restated(t, kind, 3, 7, r)), (it, t)
        t = h.step
    assert t == 9 and sp.host().skipped == 2


def test_five_steps_two_arenas_against_torch_adamw_clip_and_lambda_lr():
    """Two arenas with their own lr / weight decay, ONE norm over both (their norms differ by 10 x, the threshold sits at a quarter of the
    joint norm: clipping per arena would leave the small arena unclipped), linear schedule with warmup 2 and total 5.  Bounds: those of
    ``test_adamw_step_block_is_the_grad_scaler_protocol`` for this kernel."""
    from torch.optim.lr_scheduler import LambdaLR
    nA, nB = 4096 * 2 + 8, 4096 + 24
    hyp = [(1e-3, 0.01), (3e-4, 0.1)]
    # parameters N(0, 0.25^2): all below 2 in magnitude, so the ten fp32 roundings of a parameter over the five steps (decay, subtraction; half an
    # ulp = 6e-8 each) stay below the 1e-6 bound even if they all pointed the same way -- the bound then measures the update, not the storage
    P = [rnd(nA, 0.25, 10), rnd(nB, 0.25, 11)]
    assert max(float(x.abs().max()) for x in P) < 2.0
    G = [[rnd(nA, 1e-2, 20 + t), rnd(nB, 1e-3 * (nA / nB) ** 0.5, 40 + t)] for t in range(5)]
    nrm = [float(np.linalg.norm(x.cpu().numpy().astype(np.float64))) for x in G[0]]
    assert 9.0 < nrm[0] / nrm[1] < 11.0
    max_norm = float(np.hypot(*nrm)) / 4.0
    sched = ops_schedule("linear", 2, 5, 0.0)
    # reference: fp64 on the CPU
    ref = [torch.nn.Parameter(x.cpu().double().clone()) for x in P]
    opt = torch.optim.AdamW([{"params": [r], "lr": lr, "weight_decay": wd} for r, (lr, wd) in zip(ref, hyp)], betas=(0.9, 0.999), eps=1e-8)
    lam = LambdaLR(opt, lr_lambda=lambda t: _restated(t, "linear", 2, 5, 0.0))
    # device
    scale = 1024.0
    sp = _block(scale)
    M = [torch.zeros_like(x) for x in P]
    V = [torch.zeros_like(x) for x in P]
    SH = [torch.empty(x.numel(), device=DEV, dtype=torch.bfloat16) for x in P]
    slots = [0, sp.norm_slots(nA)]
    n_part = slots[1] + sp.norm_slots(nB)
    for t in range(5):
        for r, g in zip(ref, G[t]):
            r.grad = g.cpu().double().clone()
        total = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt.step()
        lam.step()
        gs = [g * scale for g in G[t]]
        for g, s in zip(gs, slots):
            sp.norm_check_(g, s)
        sp.decide_ex_(0.9, 0.999, n_part, max_norm, sched)
        for p, g, m, v, sh, (lr, wd) in zip(P, gs, M, V, SH, hyp):
            ops.adamw_sp_(p, g, m, v, sh, lr, 0.9, 0.999, 1e-8, wd, sp)
        h = sp.host()
        assert h.apply == 1 and h.step == t + 1
        assert h.lr_mult == np.float32(_restated(t, "linear", 2, 5, 0.0))
        assert abs(sp.grad_norm() - float(total)) / float(total) <= 1e-5
        assert abs(h.clip_coef - max_norm / (float(total) + 1e-6)) / h.clip_coef <= 1e-5 and 0.2 < h.clip_coef < 0.3
        for i, (p, m, v, sh) in enumerate(zip(P, M, V, SH)):
            st = opt.state[ref[i]]
            assert (p.cpu().double() - ref[i].detach()).abs().max() < 1e-6, (t, i)
            assert rel(m.cpu(), st["exp_avg"]) < 1e-5 and rel(v.cpu(), st["exp_avg_sq"]) < 5e-5, (t, i)
            assert torch.equal(sh, p.to(torch.bfloat16))
    assert not torch.equal(P[0], rnd(nA, 0.25, 10))
