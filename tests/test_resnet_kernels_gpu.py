"""-m gpu: the ResNet tower's kernels that are not convolutions (csrc/resnet.hip): BatchNorm2d forward / backward over [rows, C], its
running-statistics update, the 3 x 3 stride-2 max pool with torch's tie rule, the global average pool and the pixel layout change.

BatchNorm: the input has mean 100 and standard deviation 1 per channel -- the case in which ``E[x^2] - mean^2`` loses every digit in fp32.
Bound: the fp32 error against an fp64 evaluation may be at most ``RATIO`` = 4 x the error of torch's own fp32 ``batch_norm`` (the native
device kernels) against the same fp64 values on the same inputs, per quantity (output, dx, dgamma, dbeta, the residual gradient; the
largest |error| over the tensor).  Both chains are fp32 with different summation orders, which is what the factor leaves room for; a wrong
formula is orders of magnitude out.  Residual add and ReLU vary independently.  Where a ReLU follows, the residual (or, without one, the channel's shift) is nudged so that no pre-activation lies within 1e-3 of zero: a
mask bit decided differently in fp32 and fp64 would move a whole gradient element, in torch's chain as in this one, and say nothing about
either.  rows in {126, 2 slab + 3} (one short slab; two full slabs and a 3-row tail through the Chan merge), C in {32, 48} (48: the
second half of a 16-vector channel group is empty in fp32, a ragged group in 16-bit).

Largest measured ratio over every case and quantity (MI355X): 2.3 (dbeta at rows = 126, C = 48, residual and ReLU).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from idvs.morec_amd import ops, resnet_engine  # noqa: E402

DEV = "cuda"
RATIO = 4.0
EPS = 1e-5
SLAB = ops.bn_slab_rows()
ROWS = [126, 2 * SLAB + 3]


@functools.lru_cache(maxsize=None)
def bn_case(rows, C, with_res, relu):
    """Inputs (fp32, device) and the fp64 / torch-fp32 results of ``relu?(batch_norm(x) (+ res))`` and its backward."""
    g = torch.Generator().manual_seed(rows * 131 + C + int(with_res) + 2 * int(relu))
    x = (100.0 + torch.randn((rows, C), generator=g)).to(DEV)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    dy = torch.randn((rows, C), generator=g).to(DEV)
    res = torch.randn((rows, C), generator=g).to(DEV) if with_res else None
    rm0, rv0 = (0.1 * torch.randn(C, generator=g)).to(DEV), (1.0 + 0.3 * torch.rand(C, generator=g)).to(DEV)
    if relu:      # keep every pre-activation 1e-3 away from zero (see the module docstring): nudge the residual, or the shift
        z = F.batch_norm(x.double(), None, None, gamma.double(), beta.double(), True, 0.1, EPS) + (res.double() if with_res else 0.0)
        if with_res:
            res = torch.where(z.abs() < 1e-3, res + 0.01 * torch.where(z >= 0, 1.0, -1.0).float(), res)
        else:      # per channel: move beta until no element of the channel is near zero
            for _ in range(50):
                near = (z.abs() < 1e-3).any(0)
                if not bool(near.any()):
                    break
                beta = beta + 0.0137 * near.float()
                z = z + 0.0137 * near.double()
            assert not bool((z.abs() < 1e-3).any())

    def run(dt):
        xx, gg, bb = (t.to(dt).detach().requires_grad_(True) for t in (x, gamma, beta))
        rr = res.to(dt).detach().requires_grad_(True) if with_res else None
        rm, rv = rm0.to(dt).clone(), rv0.to(dt).clone()
        with torch.backends.cudnn.flags(enabled=False):      # torch's native kernels
            y = F.batch_norm(xx, rm, rv, gg, bb, True, 0.1, EPS)
            if with_res:
                y = y + rr
            if relu:
                y = F.relu(y)
            y.backward(dy.to(dt))
        return dict(y=y.detach(), dx=xx.grad, dgamma=gg.grad, dbeta=bb.grad, dres=rr.grad if with_res else None, rm=rm, rv=rv)

    return dict(x=x, gamma=gamma, beta=beta, dy=dy, res=res, rm0=rm0, rv0=rv0), run(torch.float64), run(torch.float32)


def ratio_check(what, got, ref64, torch32):
    e_got = float((got.double() - ref64).abs().max())
    e_torch = float((torch32.double() - ref64).abs().max())
    print(f"{what}: |err| {e_got:.3e}, torch fp32 {e_torch:.3e}, ratio {e_got / max(e_torch, 1e-300):.2f}")
    assert e_got <= RATIO * e_torch, (what, e_got, e_torch)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("C", [32, 48])
@pytest.mark.parametrize("rows", ROWS)
def test_batchnorm_fwd_bwd_fp32(rows, C, with_res, relu):
    inp, r64, r32 = bn_case(rows, C, with_res, relu)
    x, gamma, beta = inp["x"], inp["gamma"], inp["beta"]
    rm, rv = inp["rm0"].clone(), inp["rv0"].clone()
    part = ops.bn_stats(x)
    assert tuple(part.shape) == ((rows + SLAB - 1) // SLAB, 3, C)
    mean, rstd, _ = ops.bn_merge(part, EPS, rm, rv, 0.1)
    y = ops.bn_apply_fwd(x, mean, rstd, gamma, beta, res=inp["res"], relu=relu)
    tag = f"bn rows {rows} C {C} {'res' if with_res else 'nores'} {'relu' if relu else 'linear'}"
    ratio_check(tag + " y", y, r64["y"], r32["y"])
    # the running statistics: torch's rule (momentum 0.1, unbiased variance)
    ratio_check(tag + " running_mean", rm, r64["rm"], r32["rm"])
    ratio_check(tag + " running_var", rv, r64["rv"], r32["rv"])
    yr = y if relu else None
    sums = ops.bn_bwd_reduce(inp["dy"], yr, x, mean, rstd)
    dx, dz = ops.bn_bwd_apply(inp["dy"], yr, x, mean, rstd, gamma, sums, need_dz=with_res)
    ratio_check(tag + " dx", dx, r64["dx"], r32["dx"])
    ratio_check(tag + " dgamma", sums[1], r64["dgamma"], r32["dgamma"])
    ratio_check(tag + " dbeta", sums[0], r64["dbeta"], r32["dbeta"])
    if with_res:
        assert torch.equal(dz.double(), r64["dres"]), "the residual gradient is dy under the ReLU mask, exactly"
    # bits repeat
    assert torch.equal(part, ops.bn_stats(x)) and torch.equal(sums, ops.bn_bwd_reduce(inp["dy"], yr, x, mean, rstd))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_batchnorm_16bit(dt):
    """16-bit storage: the statistics of the ROUNDED input in fp32, the output rounded once.  Against fp64 on the rounded operands:
    |y - ref| <= 2^-8 (bf16) / 2^-11 (fp16) relative (one rounding) + 1e-5 (the fp32 statistics of a mean-100 input, as measured by
    the fp32 test's yardstick); dx alike with the rounding of its own magnitude."""
    rows, C = 2 * SLAB + 3, 48
    inp, _, _ = bn_case(rows, C, True, True)
    rt = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    x, res, dy = inp["x"].to(dt), inp["res"].to(dt), inp["dy"].to(dt)
    x64 = x.double().requires_grad_(True)
    pre = F.batch_norm(x64, None, None, inp["gamma"].double(), inp["beta"].double(), True, 0.1, EPS) + res.double()
    mean, rstd, _ = ops.bn_merge(ops.bn_stats(x), EPS)
    y = ops.bn_apply_fwd(x, mean, rstd, inp["gamma"], inp["beta"], res=res, relu=True)
    y64 = F.relu(pre)
    assert bool(((y.double() - y64).abs() <= rt * y64.abs() + 1e-5).all())
    far = pre.detach().abs() > 0.05      # elements whose ReLU mask bit cannot depend on the output's rounding
    (y64 * far).backward(dy.double())
    sums = ops.bn_bwd_reduce(dy, y, x, mean, rstd)
    dyf = torch.where(far, dy, torch.zeros_like(dy))
    sums_f = ops.bn_bwd_reduce(dyf, y, x, mean, rstd)
    dx, _ = ops.bn_bwd_apply(dyf, y, x, mean, rstd, inp["gamma"], sums_f)
    assert bool(((dx.double() - x64.grad).abs() <= rt * x64.grad.abs() + 1e-4).all())
    assert sums.shape == (2, C) and bool(torch.isfinite(sums).all())


def test_merge_on_device_is_the_host_merge():
    """``merge_bn_partials``: the device kernel and the host loop run the same fp32 operations in the same order."""
    x = (100.0 + torch.randn((3 * SLAB + 77, 32), generator=torch.Generator().manual_seed(5))).to(DEV)
    part = ops.bn_stats(x)
    dev, host = resnet_engine.merge_bn_partials(part), resnet_engine.merge_bn_partials(part.cpu())
    assert dev.shape == (3, 32) and float(dev[0, 0]) == x.shape[0]
    assert bool(((dev.cpu() - host).abs() <= 2.0 ** -20 * host.abs()).all())      # three merges whose fma contraction may differ: a few ulps, no more
    # against fp64.  A slab sum is 64 additions per row lane and 16 across the lanes, each rounding a partial sum of at most
    # 1024 x 100 to fp32: |mean error| <= 80 x 2^-24 x 100; the centred squares sum to ~1024 per slab: 80 x 2^-24 x 1100 / 1024 per unit
    # of variance, plus the square of the mean's error
    ref = x.double()
    assert bool(((host[1].double() - ref.mean(0).cpu()).abs() <= 80 * 2.0 ** -24 * 100).all())
    assert bool(((host[2].double() / x.shape[0] - ref.var(0, unbiased=False).cpu()).abs() < 1e-5).all())


def test_evaluation_mode_applies_running_statistics():
    inp, _, _ = bn_case(126, 32, False, False)
    rstd = ops.bn_rstd(inp["rv0"], EPS)
    y = ops.bn_apply_fwd(inp["x"], inp["rm0"], rstd, inp["gamma"], inp["beta"])
    want = F.batch_norm(inp["x"].double(), inp["rm0"].double(), inp["rv0"].double(), inp["gamma"].double(), inp["beta"].double(), False, 0.1, EPS)
    assert bool(((y.double() - want).abs() <= 2.0 ** -21 * want.abs() + 1e-6).all())
    dx, _ = ops.bn_bwd_apply(inp["dy"], None, inp["x"], inp["rm0"], rstd, inp["gamma"], None)      # constants: dx = gamma rstd dy
    want_dx = inp["dy"].double() * inp["gamma"].double() * rstd.double()
    assert bool(((dx.double() - want_dx).abs() <= 2.0 ** -22 * want_dx.abs()).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [32, 48])
def test_maxpool_exact_on_tie_heavy_integers(C, dt):
    """Post-ReLU data: mostly zeros, small integers.  Output, selected taps' gradient: EXACTLY torch's (first tap in scan order among
    equals; ``tests/test_resnet_cpu.py`` shows that this is torch's rule)."""
    N, H, W = 2, 9, 7
    g = torch.Generator().manual_seed(C)
    x = torch.randint(0, 3, (N, H, W, C), generator=g).float() * (torch.rand((N, H, W, C), generator=g) < 0.4)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt = F.max_pool2d(xt, 3, 2, 1)
    dy = torch.randint(-2, 3, tuple(yt.shape), generator=g).float()
    yt.backward(dy)
    y, idx = ops.maxpool3x3s2_fwd(x.reshape(-1, C).to(DEV).to(dt), N, H, W)
    assert torch.equal(y.float().cpu(), yt.detach().permute(0, 2, 3, 1).reshape(-1, C)) and int(idx.max()) <= 8
    dx = ops.maxpool3x3s2_bwd(dy.permute(0, 2, 3, 1).reshape(-1, C).to(DEV).to(dt), idx, N, H, W)
    assert torch.equal(dx.float().cpu(), xt.grad.permute(0, 2, 3, 1).reshape(-1, C))


@pytest.mark.parametrize("tokens", [4, 49])
def test_global_average_pool_is_the_fp32_mean(tokens):
    """The tower reuses ``morec_swin_pool_fwd`` / ``_bwd``: the fp32 sum over an image's rows in row order, times 1 / tokens, one rounding.
    Against the fp64 mean: at most ``tokens`` roundings of the running sum, 2^-24 relative to the largest partial sum each."""
    n, C = 3, 48
    x = torch.randn((n * tokens, C), generator=torch.Generator().manual_seed(tokens)).to(DEV)
    y = ops.swin_pool_fwd(x, n, tokens)
    want = x.double().view(n, tokens, C).mean(1)
    lim = (tokens + 1) * 2.0 ** -24 * float(x.abs().view(n, tokens, C).sum(1).max()) / tokens
    assert bool(((y.double() - want).abs() <= lim).all())
    d = torch.randn((n, C), generator=torch.Generator().manual_seed(1)).to(DEV)
    dx = ops.swin_pool_bwd(d, n, tokens)
    want_dx = (d.double() / tokens)[:, None, :].expand(n, tokens, C).reshape(-1, C)
    assert bool(((dx.double() - want_dx).abs() <= 2.0 ** -23 * want_dx.abs()).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_pixels_to_nhwc_bit_equal(dt):
    g = torch.Generator().manual_seed(9)
    n, Hh, Ww = 2, 9, 7
    px = torch.randn((n, 3, Hh, Ww), generator=g)
    assert torch.equal(ops.pixels_to_nhwc(px.to(DEV), dt).cpu(), px.permute(0, 2, 3, 1).reshape(-1, 3).to(dt))
    u8 = torch.randint(0, 256, (n, Hh, Ww, 3), generator=g, dtype=torch.uint8)
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)      # every byte value
    host = ((u8.float() / 255.0) - 0.5) / 0.5
    assert torch.equal(ops.pixels_to_nhwc(u8.to(DEV), dt).cpu(), host.reshape(-1, 3).to(dt))
