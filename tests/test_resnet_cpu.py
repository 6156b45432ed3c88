"""CPU: the host side of the ResNet item tower -- containers and models construct, torchvision's key order, ``--freeze_paras_before``
indices, the driver's argument checks, ``merge_bn_partials`` against fp64, and torch's max-pool tie rule (the rule the kernel implements)."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ref
from helpers import GOLDEN_DIR
from idvs.morec_amd import _lib, resnet_engine
from idvs.morec_amd.model import BceModel, Model
from idvs.morec_amd.model.encoders import Resnet_Encoder
from idvs.morec_amd.model.resnet import HipResNet, ResNetShape
from idvs.morec_amd.parameters import check_resnet_args, is_resnet_run, parse_args

KEYS = json.load(open(os.path.join(GOLDEN_DIR, "g32_resnet_keys.json")))


def _args(**kw):
    base = dict(max_seq_len=5, embedding_dim=48, num_attention_heads=2, drop_rate=0.0, transformer_block=2, CV_model_load="resnet_micro",
                compute_dtype="fp32")
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("name", ["resnet_micro", "resnet_micro_b"])
def test_both_models_construct_over_the_tower(name):
    """Fails before the tower existed: both ``Model`` classes raised ``NotImplementedError`` for a name with 'resnet'."""
    net = HipResNet(ResNetShape.named(name), 48)
    m = Model(_args(CV_model_load=name), 40, True, net, [1.0] * 41)
    assert isinstance(m.cv_encoder, Resnet_Encoder) and m.cv_encoder.image_net is net
    b = BceModel(_args(CV_model_load=name), 40, True, HipResNet(ResNetShape.named(name), 48))
    assert isinstance(b.cv_encoder, Resnet_Encoder)
    want = ["cv_encoder.image_net." + k for k, _ in KEYS[name]["state_dict"]]
    assert [k for k in m.state_dict() if k.startswith("cv_encoder.")][:-2] == want[:-2]      # fc was built with 48 outputs
    # a plain-torch module with torchvision's keys is adopted: weights, buffers, parameter order and requires_grad flags
    ref = resnet_ref.load_det(resnet_ref.build(name, 48))
    for i, (_, p) in enumerate(ref.named_parameters()):
        p.requires_grad = i >= 5
    enc = Resnet_Encoder(ref, compute_dtype=torch.float32)
    assert isinstance(enc.image_net, HipResNet) and enc.image_net.shape == ResNetShape.named(name)
    for (k1, v1), (k2, v2) in zip(enc.image_net.state_dict().items(), ref.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    assert [p.requires_grad for p in enc.image_net.parameters()] == [p.requires_grad for p in ref.parameters()]


def test_image_net_none_still_raises():
    for cls, extra in ((Model, ([1.0] * 41,)), (BceModel, ())):
        with pytest.raises(NotImplementedError, match="ResNet tower"):
            cls(_args(CV_model_load="resnet50"), 40, True, None, *extra)
    with pytest.raises(NotImplementedError):
        HipResNet.from_torch(torch.nn.Linear(3, 3))


@pytest.mark.parametrize("name,count", [("resnet18", 62), ("resnet34", 110), ("resnet50", 161), ("resnet-50", 161), ("resnet101", 314),
                                        ("resnet152", 467)])
def test_key_order_is_torchvisions(name, count):
    """``state_dict`` keys, shapes and ``named_parameters`` order against the list written from ``tests/resnet_ref.py``, whose counts were
    checked against torchvision's known ones when the fixture was made."""
    with torch.device("meta"):
        net = HipResNet(ResNetShape.named(name))
    want = KEYS[name.replace("-", "")]
    assert len(want["named_parameters"]) == count
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want["state_dict"]
    assert [k for k, _ in net.named_parameters()] == want["named_parameters"]
    assert net.shape.num_features == (512 if net.shape.block == "basic" else 2048)
    assert [n for n, *_ in resnet_engine.conv_names(net.shape, "")] == [k for k in want["named_parameters"] if k.endswith("weight") and
                                                                         ("conv" in k or "downsample.0" in k)]


def test_unknown_name_and_v15_stride():
    with pytest.raises(ValueError, match="resnet18"):
        ResNetShape.named("resnet77")
    for wide in ("wide_resnet50_2", "resnext50_32x4d"):
        with pytest.raises(ValueError, match="not built"):
            ResNetShape.named(wide)
    ref = resnet_ref.build("resnet_micro", 8)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.05
    assert (HipResNet.from_torch(ref).shape.eps, HipResNet.from_torch(ref).layer3[0].bn2.momentum) == (1e-3, 0.05)      # adopted, not defaulted
    net = HipResNet(ResNetShape.named("resnet_micro_b"))
    blk = net.layer2[0]
    assert blk.conv1.stride == (1, 1) and blk.conv2.stride == (2, 2) and blk.downsample[0].stride == (2, 2)      # v1.5
    assert float(blk.bn3.weight.detach().min()) == 1.0      # zero_init_residual is off


def test_freeze_paras_before_counts_torchvisions_order():
    """``V/run.py:58-60``: ``index < freeze_paras_before`` over ``named_parameters`` of the image network."""
    net = HipResNet(ResNetShape.named("resnet50"))
    names = [n for n, _ in net.named_parameters()]
    assert names[:3] == ["conv1.weight", "bn1.weight", "bn1.bias"] and names[3] == "layer1.0.conv1.weight"
    assert names[12:15] == ["layer1.0.downsample.0.weight", "layer1.0.downsample.1.weight", "layer1.0.downsample.1.bias"]
    assert names.index("layer2.0.conv1.weight") == 33 and names.index("layer4.0.conv1.weight") == 129 and names[-2:] == ["fc.weight", "fc.bias"]


def test_argument_checks_name_the_tower(monkeypatch):
    base = ["--item_tower", "modal", "--CV_model_load", "resnet-50"]
    assert is_resnet_run(parse_args(base)) and check_resnet_args(parse_args(base)) is True
    assert check_resnet_args(parse_args(["--item_tower", "modal", "--CV_model_load", "swin_tiny"])) is False
    assert check_resnet_args(parse_args(["--item_tower", "id", "--CV_model_load", "resnet50"])) is False
    for extra, word in ((["--fused_step"], "--fused_step"), (["--graph"], "--graph"), (["--arch", "dssm"], "--arch dssm")):
        with pytest.raises(SystemExit, match="ResNet item tower") as e:
            check_resnet_args(parse_args(base + extra))
        assert word in str(e.value)
    for tower in ("modal_add", "modal_cat"):
        with pytest.raises(SystemExit, match="ResNet item tower.*fusion"):
            check_resnet_args(parse_args(["--item_tower", tower, "--CV_model_load", "resnet50"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="ResNet item tower.*SyncBatchNorm"):
        check_resnet_args(parse_args(base))


def test_new_exports_have_signatures():
    for n in ("morec_conv2d_fwd", "morec_conv2d_bwd_data", "morec_im2col_nhwc", "morec_bn_stats", "morec_bn_merge", "morec_bn_apply_fwd",
              "morec_bn_bwd_reduce", "morec_bn_bwd_apply", "morec_maxpool3x3s2_fwd", "morec_maxpool3x3s2_bwd", "morec_pixels_to_nhwc"):
        assert n in _lib.EXPORTS and hasattr(_lib.lib(), n)
    assert _lib.lib().morec_bn_slab_rows() > 0
    # the entry points judge their arguments before any launch: no device is needed for a refusal
    assert _lib.lib().morec_conv2d_fwd(None, None, None, 1, 8, 8, 32, 32, 5, 5, 1, 1, _lib.BF16, None) == -3      # 5 x 5: unsupported
    assert _lib.lib().morec_conv2d_fwd(None, None, None, 1, 8, 8, 32, 32, 3, 3, 3, 1, _lib.BF16, None) == -3      # stride 3
    assert _lib.lib().morec_conv2d_fwd(None, None, None, 1, 8, 8, 32, 32, 3, 3, 1, 3, _lib.BF16, None) == -3      # pad >= K
    assert _lib.lib().morec_conv2d_fwd(None, None, None, 1, 8, 8, 32, 32, 3, 3, 1, 1, _lib.BF16, None) == -1      # null pointers
    assert _lib.lib().morec_conv2d_uses_mfma(64, _lib.F16) == 1 and _lib.lib().morec_conv2d_uses_mfma(3, _lib.F16) == 0
    assert _lib.lib().morec_conv2d_uses_mfma(64, _lib.F32) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_merge_bn_partials_against_fp64(dtype):
    """Mean 100, standard deviation 1: slabs of unequal length merged in slab order.  fp32 partials built the kernel's way (slab mean,
    then centred squares) merge to the fp64 statistics within a few fp32 roundings of the MEAN's magnitude; ``E[x^2] - mean^2`` in fp32
    is shown to lose the variance outright on the same data."""
    g = torch.Generator().manual_seed(3)
    x = 100.0 + torch.randn((2500, 16), generator=g, dtype=torch.float64)
    slabs = [x[:1024], x[1024:2048], x[2048:]]
    part = torch.stack([torch.stack([torch.full((16,), float(s.shape[0]), dtype=dtype), s.to(dtype).mean(0),
                                     ((s.to(dtype) - s.to(dtype).mean(0)) ** 2).sum(0)]) for s in slabs])
    n, mean, m2 = resnet_engine.merge_bn_partials(part)
    assert n.dtype == dtype and float(n[0]) == 2500.0
    tol = 1e-12 if dtype == torch.float64 else 4 * 2.0 ** -24 * 100.0      # roundings of a value near 100
    assert float((mean.double() - x.mean(0)).abs().max()) <= tol
    assert float((m2.double() / 2500 - x.var(0, unbiased=False)).abs().max()) <= (1e-12 if dtype == torch.float64 else 1e-4)
    if dtype == torch.float32:
        x32 = x.float()
        naive = (x32 * x32).mean(0) - x32.mean(0) ** 2
        assert float((naive.double() - x.var(0, unbiased=False)).abs().max()) > 1e-3
    one = resnet_engine.merge_bn_partials(part[:1])
    assert torch.equal(one, part[0])


def test_torch_maxpool_sends_the_gradient_to_the_first_tap_in_scan_order():
    """On the reference: ``F.max_pool2d(3, 2, 1)`` over integer-valued, zero-heavy (post-ReLU-like) data routes each window's gradient
    to the FIRST position in (kh, kw) scan order among the window's equal maxima, padding excluded."""
    g = torch.Generator().manual_seed(11)
    x = (torch.randint(0, 3, (2, 4, 9, 7), generator=g).float() * (torch.rand((2, 4, 9, 7), generator=g) < 0.4)).requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    dy = torch.randint(1, 4, tuple(y.shape), generator=g).float()
    y.backward(dy)
    want = torch.zeros_like(x)
    xd = x.detach()
    ties = 0
    for n in range(2):
        for c in range(4):
            for ho in range(y.shape[2]):
                for wo in range(y.shape[3]):
                    taps = [(2 * ho - 1 + kh, 2 * wo - 1 + kw) for kh in range(3) for kw in range(3)
                            if 0 <= 2 * ho - 1 + kh < 9 and 0 <= 2 * wo - 1 + kw < 7]
                    vals = [float(xd[n, c, h, w]) for h, w in taps]
                    ties += vals.count(max(vals)) > 1
                    h, w = taps[int(np.argmax(vals))]      # argmax returns the first of equal values
                    want[n, c, h, w] += dy[n, c, ho, wo]
    assert ties > 50 and torch.equal(x.grad, want)
