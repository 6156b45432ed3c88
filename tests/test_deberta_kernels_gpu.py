"""``morec_disent_attn_fwd`` / ``_bwd`` (csrc/deberta.hip) against ``deberta_ref`` in fp64 on operands rounded to the storage type.

Shapes: the edges of the 16-row MFMA blocks, of the 32-slot k-steps and of the Toeplitz index d = i - j + T (T = 1, 2, 17, 31, 32, 33, 63,
64), both paths (gen: dh 16 and 48, every storage type; mfma16: dh 32, 64, 128 in bf16 / fp16), 2 heads, n_seq = 3 and 11 (11: the sequence
sum of dPK / dPQ runs over uneven chunks of 2, a short chunk of 1 and two empty ones).  The five mask kinds of ``test_opt_kernels_gpu`` cycle
over the rows, starting at a kind that moves with T.

Bounds: the project's own for the same quantities (``test_kernels_gpu``): rel(ctx) < tol(dt), rel(dqkv) < t16(dt, 1e-4, 3e-2).  dPK and dPQ
are fp32 sums that are never rounded to the storage type, so they are held to the dqkv bound at both n_seq (the argument of the BEiT test for
``d_pos_bias``).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from idvs.morec_amd import _lib, ops  # noqa: E402
from deberta_ref import disent_attn_ref  # noqa: E402
from test_kernels_gpu import rel, rnd, t16, tol  # noqa: E402
from test_opt_kernels_gpu import make_mask  # noqa: E402

DEV = "cuda"
NAMES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
HEADS = 2
TS = [1, 2, 17, 31, 32, 33, 63, 64]


def inputs(dt, T, dh, n_seq):
    H = HEADS * dh
    qkv = rnd(n_seq * T, 3 * H, dt=dt, scale=0.7, seed=T)
    pk = rnd(2 * T, H, dt=dt, scale=0.7, seed=T + 1)
    pq = rnd(2 * T, H, dt=dt, scale=0.7, seed=T + 2)
    dctx = rnd(n_seq * T, H, dt=dt, seed=9)
    keep = make_mask(n_seq, T, seed=T).to(DEV).float()
    return qkv, keep, pk, pq, dctx


def drop_factors(desc, p, seed, n_seq, T):
    """What the kernels keep of P, as the library reports it: the descriptor's element index at TP = 64."""
    tp = ops.DISENT_DROP_TP
    m = ops.dropout_keep_mask(n_seq * HEADS * tp * tp, p, seed).view(n_seq, HEADS, tp, tp)[:, :, :T, :T]
    return m.double() / (1.0 - int(p * 65536) / 65536.0)


def run_case(dt, T, dh, n_seq, p_drop=0.0):
    H = HEADS * dh
    qkv, keep, pk, pq, dctx = inputs(dt, T, dh, n_seq)
    scale = 1.0 / math.sqrt(3 * dh)
    seed = 0x5EED + T
    desc = ops.attn_desc(n_seq, T, HEADS, dh, False, scale, ops.FLT_MIN_MASK, dt, p_drop=p_drop, seed=seed)
    ctx = ops.disent_attn_fwd(desc, qkv, keep, pk, pq)
    qd, kd, pd = (x.double().requires_grad_(True) for x in (qkv, pk, pq))
    fac = drop_factors(desc, p_drop, seed, n_seq, T) if p_drop else None
    ref = disent_attn_ref(qd, keep, kd, pd, HEADS, scale, p_keep=fac)
    (ref * dctx.double()).sum().backward()
    dbias = torch.full((3 * H,), 0.25, device=DEV)
    dqkv, dpk, dpq = ops.disent_attn_bwd(desc, qkv, keep, pk, pq, dctx, dbias=dbias)
    e = {"ctx": rel(ctx, ref), "dqkv": rel(dqkv, qd.grad), "dPK": rel(dpk, kd.grad), "dPQ": rel(dpq, pd.grad)}
    print(f"disent {dt} T={T} dh={dh} n_seq={n_seq} p={p_drop}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["ctx"] < tol(dt)
    assert e["dqkv"] < t16(dt, 1e-4, 3e-2)
    if T > 1:      # (T = 1: d = 1 only, softmax over one key: every score gradient is an exact zero, in the reference too)
        assert e["dPK"] < t16(dt, 1e-4, 3e-2) and e["dPQ"] < t16(dt, 1e-4, 3e-2)
    else:
        assert float(dpk.abs().max()) == 0.0 and float(dpq.abs().max()) == 0.0 and float(kd.grad.abs().max()) == 0.0
    # d = 0 never occurs
    assert float(dpk[0].abs().max()) == 0.0 and float(dpq[0].abs().max()) == 0.0
    # the fused q|k|v bias gradient: += the column sums of dqkv
    want = 0.25 + dqkv.double().sum(0)
    assert (dbias.double() - want).abs().max().item() <= t16(dt, 1e-5, 3e-3) * max(1.0, want.abs().max().item())
    if not p_drop:
        # a masked query row attends to all T keys alike: the plain mean of the T value rows
        v = qkv[:, 2 * H:].double().view(n_seq, T, H)
        mean_v = v.mean(1, keepdim=True).expand(n_seq, T, H).reshape(n_seq * T, H)
        rows = (keep == 0).view(-1)
        if bool(rows.any()):
            assert rel(ctx[rows], mean_v[rows]) < tol(dt)
    return desc, (qkv, keep, pk, pq, dctx), (ctx, dqkv, dpk, dpq)


def exact_properties(desc, ins, outs):
    """Two calls give the same bits whatever the outputs and the workspace held before (NaN here), in either summation mode; with dPK / dPQ
    NULL dqkv has the same bits."""
    qkv, keep, pk, pq, dctx = ins
    ctx, dqkv, dpk, dpq = outs
    was = ops.DETERMINISTIC
    try:
        for mode in (True, False):
            ops.set_deterministic(mode)
            n_ws = int(_lib.lib().morec_disent_attn_ws_bytes(ops.C.byref(desc))) // 4
            ws = torch.full((n_ws,), float("nan"), device=DEV)
            dqkv2 = torch.full_like(qkv, float("nan"))
            dpk2, dpq2 = torch.full_like(dpk, float("nan")), torch.full_like(dpq, float("nan"))
            ops.check(_lib.lib().morec_disent_attn_bwd(ops.C.byref(desc), ops._p(qkv), ops._p(keep), ops._p(pk), ops._p(pq), ops._p(dctx),
                                                       ops._p(dqkv2), None, ops._p(dpk2), ops._p(dpq2), ops._p(ws), n_ws * 4, ops._stream()),
                      "morec_disent_attn_bwd")
            assert torch.equal(dqkv2, dqkv) and torch.equal(dpk2, dpk) and torch.equal(dpq2, dpq)
            assert torch.equal(ops.disent_attn_fwd(desc, qkv, keep, pk, pq), ctx)
            dqkv3, n1, n2 = ops.disent_attn_bwd(desc, qkv, keep, pk, pq, dctx, need_dpos=False)
            assert n1 is None and n2 is None and torch.equal(dqkv3, dqkv)
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("n_seq", [3, 11])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dh", [16, 48])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_disent_gen(dt, dh, T, n_seq):
    """The fp32-arithmetic path: fp32 storage, and head widths that are no multiple of 32 in every storage type."""
    run_case(NAMES[dt], T, dh, n_seq)


@pytest.mark.parametrize("n_seq", [3, 11])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dh", [32, 64, 128])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_disent_mfma16(dt, dh, T, n_seq):
    """Every product on v_mfma_f32_16x16x32: one, two and four k-steps over the head width."""
    run_case(NAMES[dt], T, dh, n_seq)


@pytest.mark.parametrize("T", [17, 33, 64])
@pytest.mark.parametrize("dt,dh", [("fp32", 16), ("bf16", 48), ("bf16", 64), ("fp16", 32)])
def test_disent_exact_properties(dt, dh, T):
    desc, ins, outs = run_case(NAMES[dt], T, dh, 11)
    exact_properties(desc, ins, outs)


@pytest.mark.parametrize("T", [17, 32, 50, 64])
@pytest.mark.parametrize("dt,dh", [("fp32", 16), ("fp16", 48), ("bf16", 64), ("fp16", 128)])
def test_disent_dropout_on_p(dt, dh, T):
    """p_drop = 0.1: the mask the library reports (``ops.dropout_keep_mask`` with the descriptor's indexing) fed to the reference, under the
    same bounds; forward and backward draw the same mask, and two calls the same bits."""
    desc, ins, outs = run_case(NAMES[dt], T, dh, 3, p_drop=0.1)
    exact_properties(desc, ins, outs)
