"""GPU: ``morec_dssm_bce_fwd`` / ``morec_dssm_bce_bwd`` (csrc/dssm.hip) against fp64 autograd of ``sum softplus(s) - y s``.

Inputs are four-bit grid values (``test_scoring_edges_gpu.grid``): exact in fp32, bf16 and fp16, and their fp32 dot products are exact in
any order, so the scores are compared bit for bit and everything behind them sees the same numbers in all three storage types.

Shapes (B, n1): (1, 2) one user; (5, 2) the default neg_num = 1; (6, 1) no negatives; (3, 6) neither B nor R = B n1 fills a block of four
waves; (2, 131) more items per user than lanes, than two passes of a 64-wide item loop, and than the 16 waves a user's rows are spread
over in the backward -- the backward cuts each user's rows into 8 segments of 17 rows (the last: 12) and folds the segments' dU;
(1, 300), beyond the issue's list: 18 segments, the last one with 11 rows for 16 waves.  D: 4 (fp32) / 8 the smallest row, 260 a ragged second pass of a 256-element loop (and, in 16 bits, a row pitch off
16 bytes: the 8-byte access path), 512 the real width."""
import functools

import pytest
import torch

from idvs.morec_amd import ops
from test_kernels_gpu import t16
from test_scoring_edges_gpu import DTS, assert_grid_exact, grid

DEV = "cuda"
gpu = pytest.mark.gpu
SHAPES = [(1, 2), (5, 2), (6, 1), (3, 6), (2, 131), (1, 300)]
WIDTHS = [8, 260, 512]
EPS32 = 2.0 ** -23            # one ulp of an fp32 value in [1, 2)
# |c| below this is below half the smallest fp32 subnormal (2^-150) with room for g <= 1/2 and one ulp of expf: the kernel's c is exactly 0
C_UNDERFLOW = 2.0 ** -160


@functools.lru_cache(maxsize=None)
def case(B, n1, D, mult, soft):
    """Inputs and the fp64 reference, computed once per case and shared (nothing below modifies them)."""
    R = B * n1
    U, E = grid((B, D), 12, mult), grid((R, D), 13, mult)      # seeds: the x8 case saturates positives and negatives on both sides
    assert_grid_exact(U, E)
    hard = torch.zeros(B, n1)
    hard[:, 0] = 1.0
    if soft:
        y = torch.rand((B, n1), generator=torch.Generator().manual_seed(B * 1000 + n1)).to(torch.float32)
        if mult > 1:      # c = 0 needs sigmoid(s) == y exactly: only a saturated score with the label at its limit gives that
            s = (U[:, None, :].double() * E.view(B, n1, D).double()).sum(-1)
            at_limit = (s > 0).to(torch.float32)                  # even rows: c = 0; odd rows: the opposite label, c = +-g
            even = (torch.arange(R).view(B, n1) % 2 == 0)
            y = torch.where(s.abs() > 115, torch.where(even, at_limit, 1 - at_limit), y)
    else:
        y = hard
    y = y.reshape(-1).contiguous()
    g = 1.0 / R
    Ud, Ed = U.double().requires_grad_(True), E.double().requires_grad_(True)
    s = (Ud[:, None, :] * Ed.view(B, n1, D)).sum(-1).reshape(-1)
    terms = -torch.nn.functional.logsigmoid(-s) - y.double() * s          # softplus(s) - y s
    (g * terms.sum()).backward()
    sd, yd = s.detach(), y.double()      # sigmoid(s) - y without fp64 absorbing a tiny tail into 1: (1 - y) - sigmoid(-s) where s >= 0
    c = g * torch.where(sd >= 0, (1 - yd) - torch.sigmoid(-sd), torch.sigmoid(sd) - yd)
    return dict(U=U, E=E, y=y, g=g, s=s.detach(), terms=terms.detach(), dU=Ud.grad, dE=Ed.grad, c=c)


def run(B, n1, D, dtype, mult, soft, prefill=float("nan")):
    """Both kernels on caller-provided outputs filled with ``prefill``."""
    c = case(B, n1, D, mult, soft)
    R = B * n1
    U, E = c["U"].to(DEV).to(dtype).contiguous(), c["E"].to(DEV).to(dtype).contiguous()
    labels = c["y"].to(DEV) if soft else None                                  # None: the library's own [1, 0, ..., 0]
    out_f = tuple(torch.full((n,), prefill, device=DEV, dtype=torch.float32) for n in (R, R, 1))
    scores, terms, loss_sum = ops.dssm_bce_fwd(U, E, labels, B, n1, out=out_f)
    assert scores is out_f[0] and terms is out_f[1] and loss_sum is out_f[2]
    out_b = (torch.full_like(U, prefill), torch.full_like(E, prefill))
    dU, dE = ops.dssm_bce_bwd(U, E, labels, scores, torch.tensor([c["g"]], device=DEV), B, n1, out=out_b)
    assert dU is out_b[0] and dE is out_b[1]
    torch.cuda.synchronize()
    return scores, terms, loss_sum, dU, dE


def check(B, n1, D, dt, mult=1.0, soft=False):
    dtype = DTS[dt]
    c = case(B, n1, D, mult, soft)
    scores, terms, loss_sum, dU, dE = run(B, n1, D, dtype, mult, soft)
    for t in (scores, terms, loss_sum, dU, dE):      # NaN pre-fill: every element was written, and with something finite
        assert bool(torch.isfinite(t.float()).all())
    assert torch.equal(scores.double().cpu(), c["s"])
    t_err = (terms.double().cpu() - c["terms"]).abs()
    t_cap = 2 * EPS32 * c["terms"].abs().clamp(min=1.0)
    print(f"dssm ({B}, {n1}, {D}) {dt} x{mult:g} soft={soft}: term err / bound {float((t_err / t_cap).max()):.3f}")
    assert bool((t_err <= t_cap).all())
    err, cap = abs(float(loss_sum.double().cpu()) - float(c["terms"].sum())), 2.0 ** -20 * float(c["terms"].abs().sum())
    print(f"    loss err / bound {err / (cap + 1e-300):.3f}")
    assert err <= cap
    dUc, dEc = dU.double().cpu(), dE.double().cpu()
    tol = t16(dtype, 1e-5, 1e-2)
    e_u, e_e = float((dUc - c["dU"]).norm() / c["dU"].norm()), float((dEc - c["dE"]).norm() / c["dE"].norm())
    print(f"    dU {e_u:.2e} dE {e_e:.2e} (bound {tol:g})")
    assert e_u < tol and e_e < tol
    zero = c["c"].abs() < C_UNDERFLOW
    assert bool((dEc[zero] == 0).all())
    return c, dUc, dEc, zero


@gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B,n1", SHAPES)
def test_dssm_bce_vs_fp64(B, n1, D, soft, dt):
    check(B, n1, 4 if (D == 8 and dt == "fp32") else D, dt, soft=soft)


@gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_dssm_bce_saturated_scores(soft, dt):
    """|score| > 100 on both sides: exp overflows in the literal formulas.  Everything stays finite (``check``), rows whose coefficient
    underflows give exact zeros, and a row at the other limit gives -+g x vector."""
    B, n1, D = 5, 2, 512
    c, dUc, dEc, zero = check(B, n1, D, dt, mult=8.0, soft=soft)
    assert float(c["s"].max()) > 100 and float(c["s"].min()) < -100
    assert int(zero.sum()) >= 1                                   # the case does contain rows with c = 0
    y = c["y"].double()
    full = ((c["s"] > 100) & (y == 0)) | ((c["s"] < -100) & (y == 1))      # sigmoid - y = +-1 to 2^-144
    assert int(full.sum()) >= 1
    sign = torch.where(y == 0, 1.0, -1.0).double()
    want = (c["g"] * sign)[:, None] * c["U"].double().repeat_interleave(n1, 0)
    tol = t16(DTS[dt], 1e-6, 1e-2)
    assert float((dEc[full] - want[full]).norm() / want[full].norm()) < tol
    for b in range(B):                                             # a user all of whose rows have c = 0 gets an exactly zero gradient
        if bool(zero.view(B, n1)[b].all()):
            assert bool((dUc[b] == 0).all())


@gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("B,n1,D", [(3, 6, 260), (2, 131, 512), (6, 1, 8)])
def test_dssm_bce_outputs_written_exactly_once(B, n1, D, dt):
    """Whatever the caller's buffers held (NaN, a large number), the results are the same bits: nothing is accumulated into them."""
    a = run(B, n1, D, DTS[dt], 1.0, True, prefill=float("nan"))
    b = run(B, n1, D, DTS[dt], 1.0, True, prefill=3.0e38 if dt != "fp16" else 6.0e4)
    for x, y in zip(a, b):
        assert not bool(torch.isnan(x.float()).any())
        assert torch.equal(x, y)
    U, E = case(B, n1, D, 1.0, True)["U"].to(DEV).to(DTS[dt]), case(B, n1, D, 1.0, True)["E"].to(DEV).to(DTS[dt])
    own = ops.dssm_bce_fwd(U, E, case(B, n1, D, 1.0, True)["y"].to(DEV), B, n1)            # the allocating form
    for x, y in zip(a[:3], own):
        assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("B,n1,D", [(5, 2, 512), (2, 131, 260)])
def test_dssm_bce_is_reproducible_in_both_modes(B, n1, D, dt):
    was = ops.DETERMINISTIC
    try:
        outs = []
        for on in (False, True):
            ops.set_deterministic(on)
            outs.append(run(B, n1, D, DTS[dt], 1.0, True))
            outs.append(run(B, n1, D, DTS[dt], 1.0, True))
    finally:
        ops.set_deterministic(was)
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert torch.equal(x, y)
