"""-m gpu: the kernel sequence of synchronised BatchNorm (csrc/resnet.hip) in ONE process: the rows of
``tests/test_resnet_kernels_gpu.py``'s cases are cut into the shards that ranks would hold, every shard runs what its rank would run, and the
all-gather is replaced by ``torch.stack`` of the shards' results -- stats -> the shard's own slabs merged -> [W, 3, C] -> ``morec_bn_merge``
in rank order (with the running statistics) -> apply; backward: the shard's sums -> [W, 2, C] -> ``morec_bn_bwd_fold`` -> ``morec_bn_bwd_apply_n``
with the folded sums and the merged count row.

Yardstick and bound are that file's, unchanged: mean-100 input, torch's native fp32 ``batch_norm`` and its fp64 twin over the WHOLE batch
(cuDNN off), error <= ``RATIO`` = 4 x torch-fp32's own error against fp64, per quantity: y, running_mean, running_var, the concatenated
dx, and d gamma / d beta summed over the shards (they stay local sums; DDP's average times W is this sum).  Shards: 63 + 63, 1 + 125 (a
one-row rank), 1024 + 1027 (a full slab against a slab and a 3-row tail), 700 + 3 + 1348 (three ranks); C in {32, 48}; residual and ReLU
varied independently.  The ratios are printed; the largest measured for the unsharded path was 2.3.

Largest measured ratio over every sharded case and quantity (MI355X): 2.70 (dbeta at 700 + 3 + 1348, C = 32, residual and ReLU); next
2.52 (dbeta, same shards, neither) and 2.25 (dgamma at 1024 + 1027, C = 32).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from idvs.morec_amd import ops  # noqa: E402
from test_resnet_kernels_gpu import EPS, bn_case, ratio_check  # noqa: E402

SHARDS = [(63, 63), (1, 125), (1024, 1027), (700, 3, 1348)]


def cut(t, shards):
    return [s.contiguous() for s in torch.split(t, list(shards))] if t is not None else [None] * len(shards)


def sync_forward(xs, gamma, beta, ress, relu, rm, rv):
    """-> (ys, mean, rstd, count): what W ranks compute, the gather a ``torch.stack``."""
    local = torch.stack([ops.bn_merged(ops.bn_stats(x)) for x in xs])      # [W, 3, C], rank-major
    mean, rstd, merged = ops.bn_merge(local, EPS, rm, rv, 0.1, need_merged=True)
    ys = [ops.bn_apply_fwd(x, mean, rstd, gamma, beta, res=r, relu=relu) for x, r in zip(xs, ress)]
    return ys, mean, rstd, merged[0]


def sync_backward(dys, yrs, xs, mean, rstd, gamma, count, need_dz=False):
    """-> (dxs, dzs, the shards' local sums, the folded sums)."""
    local = [ops.bn_bwd_reduce(dy, yr, x, mean, rstd) for dy, yr, x in zip(dys, yrs, xs)]
    sums = ops.bn_bwd_fold(torch.stack(local))
    outs = [ops.bn_bwd_apply(dy, yr, x, mean, rstd, gamma, sums, need_dz=need_dz, count=count) for dy, yr, x in zip(dys, yrs, xs)]
    return [o[0] for o in outs], [o[1] for o in outs], local, sums


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("C", [32, 48])
@pytest.mark.parametrize("shards", SHARDS, ids=lambda s: "+".join(map(str, s)))
def test_sharded_batchnorm_is_the_whole_batch_fp32(shards, C, with_res, relu):
    rows = sum(shards)
    inp, r64, r32 = bn_case(rows, C, with_res, relu)
    gamma, beta = inp["gamma"], inp["beta"]
    xs, dys, ress = cut(inp["x"], shards), cut(inp["dy"], shards), cut(inp["res"], shards)
    rm, rv = inp["rm0"].clone(), inp["rv0"].clone()
    ys, mean, rstd, count = sync_forward(xs, gamma, beta, ress, relu, rm, rv)
    assert bool((count == float(rows)).all())
    tag = f"syncbn {'+'.join(map(str, shards))} C {C} {'res' if with_res else 'nores'} {'relu' if relu else 'linear'}"
    ratio_check(tag + " y", torch.cat(ys), r64["y"], r32["y"])
    ratio_check(tag + " running_mean", rm, r64["rm"], r32["rm"])
    ratio_check(tag + " running_var", rv, r64["rv"], r32["rv"])
    yrs = ys if relu else [None] * len(xs)
    dxs, dzs, local, sums = sync_backward(dys, yrs, xs, mean, rstd, gamma, count, need_dz=with_res)
    ratio_check(tag + " dx", torch.cat(dxs), r64["dx"], r32["dx"])
    dgb = torch.stack(local).sum(0)      # d gamma, d beta: the sum over ranks of the LOCAL sums
    ratio_check(tag + " dgamma", dgb[1], r64["dgamma"], r32["dgamma"])
    ratio_check(tag + " dbeta", dgb[0], r64["dbeta"], r32["dbeta"])
    if with_res:
        assert torch.equal(torch.cat(dzs).double(), r64["dres"]), "the residual gradient is dy under the ReLU mask, exactly"
    # the bits repeat
    rm2, rv2 = inp["rm0"].clone(), inp["rv0"].clone()
    ys2, mean2, rstd2, count2 = sync_forward(xs, gamma, beta, ress, relu, rm2, rv2)
    dxs2, _, _, sums2 = sync_backward(dys, yrs, xs, mean, rstd, gamma, count, need_dz=with_res)
    assert all(torch.equal(a, b) for a, b in zip(ys + dxs + [mean, rstd, count, rm, rv, sums], ys2 + dxs2 + [mean2, rstd2, count2, rm2, rv2, sums2]))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_sharded_batchnorm_16bit(dt):
    """``test_batchnorm_16bit``'s case and bound (one rounding of the output, 2^-8 / 2^-11 relative, + 1e-5 for the fp32 statistics of a
    mean-100 input; dx alike + 1e-4), the rows cut 700 + 3 + 1348."""
    shards, C = (700, 3, 1348), 48
    inp, _, _ = bn_case(sum(shards), C, True, True)
    rt = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    x, res, dy = inp["x"].to(dt), inp["res"].to(dt), inp["dy"].to(dt)
    x64 = x.double().requires_grad_(True)
    pre = F.batch_norm(x64, None, None, inp["gamma"].double(), inp["beta"].double(), True, 0.1, EPS) + res.double()
    xs, ress = cut(x, shards), cut(res, shards)
    ys, mean, rstd, count = sync_forward(xs, inp["gamma"], inp["beta"], ress, True, None, None)
    y, y64 = torch.cat(ys), F.relu(pre)
    assert bool(((y.double() - y64).abs() <= rt * y64.abs() + 1e-5).all())
    far = pre.detach().abs() > 0.05      # elements whose ReLU mask bit cannot depend on the output's rounding
    (y64 * far).backward(dy.double())
    dyf = torch.where(far, dy, torch.zeros_like(dy))
    dxs, _, _, sums = sync_backward(cut(dyf, shards), ys, xs, mean, rstd, inp["gamma"], count)
    dx = torch.cat(dxs)
    assert bool(((dx.double() - x64.grad).abs() <= rt * x64.grad.abs() + 1e-4).all())
    assert sums.shape == (2, C) and bool(torch.isfinite(sums).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("rows", [126, 2051])
def test_old_apply_entry_is_the_new_one_with_its_own_count(rows, dt):
    """``morec_bn_bwd_apply`` divides by its own row count on the host; ``morec_bn_bwd_apply_n`` handed that count in device memory (the
    merged count row of the plain path) writes the same bits: 1 / rows is one correctly rounded division either way."""
    inp, _, _ = bn_case(rows, 48, True, True)
    x, res, dy = inp["x"].to(dt), inp["res"].to(dt), inp["dy"].to(dt)
    mean, rstd, merged = ops.bn_merge(ops.bn_stats(x), EPS, need_merged=True)
    y = ops.bn_apply_fwd(x, mean, rstd, inp["gamma"], inp["beta"], res=res, relu=True)
    sums = ops.bn_bwd_reduce(dy, y, x, mean, rstd)
    assert torch.equal(sums, ops.bn_bwd_fold(sums.unsqueeze(0).contiguous()))      # one rank: the fold adds to zero, exactly
    old = ops.bn_bwd_apply(dy, y, x, mean, rstd, inp["gamma"], sums, need_dz=True)
    new = ops.bn_bwd_apply(dy, y, x, mean, rstd, inp["gamma"], sums, need_dz=True, count=merged[0].contiguous())
    assert float(merged[0, 0]) == rows
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    assert float(old[0].float().abs().max()) > 0


def test_fold_adds_in_index_order():
    """Against a host loop in the same order: bit-equal (fp32 additions, no fma to contract); against fp64 within one rounding per addition."""
    parts = torch.randn((5, 2, 48), generator=torch.Generator().manual_seed(2)).mul(1e3).cuda()
    got = ops.bn_bwd_fold(parts)
    want = torch.zeros((2, 48))
    for i in range(5):
        want = want + parts[i].cpu()
    assert torch.equal(got.cpu(), want) and torch.equal(got, ops.bn_bwd_fold(parts))
    assert bool(((got.double() - parts.double().sum(0)).abs() <= 5 * 2.0 ** -24 * parts.double().abs().sum(0)).all())
