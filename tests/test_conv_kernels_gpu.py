"""-m gpu: the convolution kernels of the ResNet tower (csrc/conv.hip: ``morec_conv2d_fwd``, ``morec_conv2d_bwd_data``,
``morec_im2col_nhwc`` + the weight-gradient GEMM as ``resnet_engine.conv_wgrad`` composes them) against the exact product.

Every output is compared element by element with torch's fp64 convolution of the SAME rounded operands under the bound form of
``tests/test_gemm2w_gpu.py`` (16-bit outputs) / ``tests/test_gemm_tn_gpu.py`` (fp32 outputs), unchanged:

    forward, data gradient:  |out - ref| <= rtol |ref| + 1e-4 sigma,  rtol = 2^-8 (bf16) | 2^-11 (fp16) | 0 (fp32),  sigma = 0.25 sqrt(K)
    weight gradient (fp32):  |out - ref| <= 1e-4 sigma,               sigma = 0.25 sqrt(rows)

with operands ~ N(0, 0.5), K the full reduction length KH KW C (border outputs sum fewer terms: the bound is not widened for them) and
rows = N Ho Wo.  A dropped tap, a tap read from the wrong pixel or a tile edge row left out is an error of order sigma / sqrt(taps).

Shapes: the smallest at which the kernels can still go wrong.  N = 2 images of H x W = 9 x 7 (odd and unequal; 126 rows is no multiple of
the 64-row tile, so the last tile has rows of BOTH kinds and the row -> (n, h, w) decode crosses an image); Cin in {32, 64} (one and
two k-steps per tap: a K step of the main loop inside one tap and across two) and Cout = 48 (a column edge: the second 32-column half of
a wave holds 16 live columns); 3 x 3 stride 1 pad 1, 3 x 3 stride 2 pad 1, 1 x 1 stride 2; 7 x 7 stride 2 pad 3 with Cin = 3, the generic
path.  The data gradient reduces over Cout = 48, which is no multiple of 32: in 16-bit storage it runs the generic kernel; with the
operands swapped (``test_bwd_data_mfma``: Cout in {32, 64} reduced, Cin = 48 written) it runs the gather form on the matrix cores.
The weight gradient runs with one image per chunk: two chunks accumulate into one buffer.  Every call is made twice: ``torch.equal``.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from idvs.morec_amd import _lib, ops, resnet_engine  # noqa: E402

DEV = "cuda"
SCALE = 0.5
N, H, W = 2, 9, 7
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
# (k, stride, pad, Cin, Cout)
GEOMS = [(3, 1, 1, 32, 48), (3, 1, 1, 64, 48), (3, 2, 1, 32, 48), (3, 2, 1, 64, 48), (1, 2, 0, 32, 48), (1, 2, 0, 64, 48), (7, 2, 3, 3, 48)]
GID = [f"k{k}s{s}p{p}-c{ci}x{co}" for k, s, p, ci, co in GEOMS]


@functools.lru_cache(maxsize=None)
def case(geom, dt):
    """Operands (rounded to ``dt``, on the device, in the kernels' layouts) and the fp64 references, made once and shared."""
    k, s, p, Cin, Cout = geom
    g = torch.Generator().manual_seed(1000 * k + 100 * s + Cin + Cout)
    Ho, Wo = ops.conv_out_size(H, k, s, p), ops.conv_out_size(W, k, s, p)
    x = (torch.randn((N, H, W, Cin), generator=g) * SCALE).to(DT[dt])
    w = (torch.randn((Cout, k, k, Cin), generator=g) * SCALE).to(DT[dt])
    dy = (torch.randn((N, Ho, Wo, Cout), generator=g) * SCALE).to(DT[dt])
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.double().permute(0, 3, 1, 2).requires_grad_(True)
    y64 = F.conv2d(x64, w64, stride=s, padding=p)
    y64.backward(dy.double().permute(0, 3, 1, 2))
    ref = dict(y=y64.detach().permute(0, 2, 3, 1).reshape(-1, Cout), dx=x64.grad.permute(0, 2, 3, 1).reshape(-1, Cin),
               dw=w64.grad.permute(0, 2, 3, 1).contiguous())
    dev = dict(x=x.reshape(-1, Cin).to(DEV), w=w.to(DEV), wt=w.permute(3, 1, 2, 0).contiguous().to(DEV), dy=dy.reshape(-1, Cout).to(DEV))
    return dev, ref, (Ho, Wo)


def check(what, out, ref, rtol, sigma):
    out, ref = out.double().cpu(), ref.double()
    assert out.shape == ref.shape and bool(torch.isfinite(out).all()), what
    err = (out - ref).abs()
    bound = rtol * ref.abs() + 1e-4 * sigma
    print(f"{what}: max |err| {float(err.max()):.4g}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("geom", GEOMS, ids=GID)
def test_fwd(geom, dt):
    k, s, p, Cin, Cout = geom
    dev, ref, _ = case(geom, dt)
    assert ops.conv2d_uses_mfma(Cin, DT[dt]) == (dt != "fp32" and Cin % 32 == 0)
    y = ops.conv2d_fwd(dev["x"], dev["w"], N, H, W, s, p)
    check(f"fwd {geom} {dt}", y, ref["y"], RTOL[DT[dt]], SCALE * SCALE * math.sqrt(k * k * Cin))
    assert torch.equal(y, ops.conv2d_fwd(dev["x"], dev["w"], N, H, W, s, p))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("geom", GEOMS[:-1], ids=GID[:-1])
def test_bwd_data(geom, dt):
    """The data gradient of every geometry but the stem's (its input, the pixels, takes no gradient; three channels are no 16-byte row,
    which the entry point refuses: ``test_stem_data_gradient_is_refused``)."""
    k, s, p, Cin, Cout = geom
    dev, ref, _ = case(geom, dt)
    dx = ops.conv2d_bwd_data(dev["dy"], dev["wt"], N, H, W, s, p)
    check(f"bwd_data {geom} {dt}", dx, ref["dx"], RTOL[DT[dt]], SCALE * SCALE * math.sqrt(k * k * Cout))
    assert torch.equal(dx, ops.conv2d_bwd_data(dev["dy"], dev["wt"], N, H, W, s, p))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", [(3, 1, 1, 48, 32), (3, 2, 1, 48, 64), (1, 2, 0, 48, 32)], ids=["k3s1", "k3s2", "k1s2"])
def test_bwd_data_mfma(geom, dt):
    """The gather form on the matrix cores: the reduced channel count (Cout) is a multiple of 32, the written one (Cin = 48) a column edge."""
    k, s, p, Cin, Cout = geom
    dev, ref, _ = case(geom, dt)
    assert ops.conv2d_uses_mfma(Cout, DT[dt])
    dx = ops.conv2d_bwd_data(dev["dy"], dev["wt"], N, H, W, s, p)
    check(f"bwd_data mfma {geom} {dt}", dx, ref["dx"], RTOL[DT[dt]], SCALE * SCALE * math.sqrt(k * k * Cout))
    assert torch.equal(dx, ops.conv2d_bwd_data(dev["dy"], dev["wt"], N, H, W, s, p))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("geom", GEOMS, ids=GID)
def test_wgrad_two_chunks(geom, dt):
    k, s, p, Cin, Cout = geom
    dev, ref, (Ho, Wo) = case(geom, dt)
    dw = resnet_engine.conv_wgrad(dev["dy"], dev["x"], (N, H, W), k, s, p, chunk_images=1)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (Cout, k, k, Cin)
    check(f"wgrad {geom} {dt}", dw, ref["dw"], 0.0, SCALE * SCALE * math.sqrt(N * Ho * Wo))
    assert torch.equal(dw, resnet_engine.conv_wgrad(dev["dy"], dev["x"], (N, H, W), k, s, p, chunk_images=1))


@pytest.mark.parametrize("dt", list(DT))
def test_im2col_rows_and_pad_columns(dt):
    """A row range of the stem's im2col (element-wise path, pitch padded from 147 to a whole vector) and of a 3 x 3 layer (16-byte
    copies) against ``F.unfold`` of the same values: bit-equal, zeros outside the image and in the pad columns."""
    for k, s, p, Cin in ((7, 2, 3, 3), (3, 2, 1, 32)):
        dev, _, (Ho, Wo) = case((k, s, p, Cin, 48), dt)
        x = dev["x"]
        r0, r1 = 3, N * Ho * Wo - 2
        col = ops.im2col_nhwc(x, N, H, W, k, k, s, p, r0, r1)
        K = k * k * Cin
        assert col.shape[0] == r1 - r0 and col.shape[1] >= K and (col.shape[1] * col.element_size()) % 16 == 0
        un = F.unfold(x.float().view(N, H, W, Cin).permute(0, 3, 1, 2), k, padding=p, stride=s)      # [N, Cin k k, Ho Wo], (c, kh, kw) order
        want = un.view(N, Cin, k * k, Ho * Wo).permute(0, 3, 2, 1).reshape(N * Ho * Wo, K)[r0:r1]
        assert torch.equal(col[:, :K].float(), want) and not bool(col[:, K:].any())


def test_stem_data_gradient_is_refused():
    x = torch.zeros((N * 5 * 4, 48), device=DEV, dtype=torch.bfloat16)
    wt = torch.zeros((3, 7, 7, 48), device=DEV, dtype=torch.bfloat16)
    with pytest.raises(_lib.MorecError):
        ops.conv2d_bwd_data(x, wt, N, H, W, 2, 3)


def test_wgrad_keeps_off_the_weight_gradient_streams_workspace():
    """``conv_wgrad`` runs on the current stream while ``engine.linear_wgrad_`` runs on the weight-gradient stream: the slab partials of
    its split launches go to a workspace of its own, never to ``ops._TN_WS``, which a launch on the other stream may be using.
    8 images of 12 x 12 = 1152 rows: the smallest round size at which the token range is split (``_splitk``: 1024 rows and up)."""
    from idvs.morec_amd.engine import _splitk
    n, hw, Cin, Cout = 8, 12, 64, 48
    assert _splitk(Cout, 9 * Cin, n * hw * hw) > 1      # the workspace is in play at this size
    g = torch.Generator().manual_seed(77)
    x = (torch.randn((n, hw, hw, Cin), generator=g) * SCALE).to(torch.bfloat16)
    dy = (torch.randn((n, hw, hw, Cout), generator=g) * SCALE).to(torch.bfloat16)
    w64 = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w64, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    shared = ops._scratch(ops._TN_WS, torch.device(DEV, torch.cuda.current_device()), 1, 20 * 1024 * 1024)
    shared.fill_(float("nan"))
    dw = resnet_engine.conv_wgrad(dy.reshape(-1, Cout).to(DEV), x.reshape(-1, Cin).to(DEV), (n, hw, hw), 3, 1, 1)
    check("wgrad own workspace", dw, w64.grad.permute(0, 2, 3, 1), 0.0, SCALE * SCALE * math.sqrt(n * hw * hw))
    assert bool(torch.isnan(shared).all()) and resnet_engine._CONV_TN_WS
