"""``HipResNet``: parameter container with torchvision ``ResNet``'s module tree, ``state_dict`` keys and parameter order (the reference's
default vision encoder: ``--CV_model_load resnet-50``, ``Resnet_Encoder`` in ``V/model/encoders.py:34-41``, selected by ``'resnet' in
CV_model_load``, ``V/model/model.py:24-25``; ``V/run.py:38-46`` builds ``torchvision.models.resnet*``, loads ``<pretrained>/<name>`` with
``load_state_dict`` and replaces ``.fc`` by a Xavier-initialised ``Linear(num_fc_ftr, embedding_dim)``).  Forward arithmetic is in
``libmorec_hip.so`` (``functional.TowerFn`` over ``resnet_engine.TOWER``); this class only owns the weights and the BatchNorm buffers,
so that a torchvision checkpoint loads key for key and ``--freeze_paras_before`` counts parameters as it does in the reference.

torchvision's v1.5 layout: the stride of a Bottleneck sits on ``conv2``; ``zero_init_residual`` is off."""
from dataclasses import dataclass

import torch
import torch.nn as nn


@dataclass
class ResNetShape:
    block: str = "bottleneck"               # "basic" | "bottleneck"
    layers: tuple = (3, 4, 6, 3)
    widths: tuple = (64, 128, 256, 512)     # planes of layer1 .. layer4; the stem has widths[0] channels
    num_channels: int = 3
    eps: float = 1e-5
    momentum: float = 0.1

    @staticmethod
    def named(name: str) -> "ResNetShape":
        """``resnet18 | 34 | 50 | 101 | 152`` (a '-' as in ``resnet-50`` is accepted) and the two test nets ``resnet_micro`` (BasicBlock)
        and ``resnet_micro_b`` (Bottleneck): [1, 1, 1, 1] blocks of widths 32 / 64 / 128 / 256."""
        key = str(name).lower().replace("-", "").replace("_", "")
        if "wide" in key or "resnext" in key:
            raise ValueError(f"unknown CV_model_load {name!r}: the wide and grouped variants of ResNet are not built")
        micro = (32, 64, 128, 256)
        table = [("resnetmicrob", ResNetShape("bottleneck", (1, 1, 1, 1), micro)), ("resnetmicro", ResNetShape("basic", (1, 1, 1, 1), micro)),
                 ("resnet18", ResNetShape("basic", (2, 2, 2, 2))), ("resnet34", ResNetShape("basic", (3, 4, 6, 3))),
                 ("resnet50", ResNetShape("bottleneck", (3, 4, 6, 3))), ("resnet101", ResNetShape("bottleneck", (3, 4, 23, 3))),
                 ("resnet152", ResNetShape("bottleneck", (3, 8, 36, 3)))]
        for k, shape in table:
            if k in key:
                return shape
        raise ValueError(f"unknown CV_model_load {name!r}: the ResNet tower knows resnet18 | 34 | 50 | 101 | 152 (and resnet_micro, "
                         "resnet_micro_b)")

    @property
    def expansion(self) -> int:
        return 4 if self.block == "bottleneck" else 1

    @property
    def num_features(self) -> int:
        """``num_fc_ftr``: the width of the pooled vector in front of ``fc`` (512 or 2048 for the real nets)."""
        return self.widths[3] * self.expansion

    def blocks(self):
        """[(name, inplanes, planes, stride, has_downsample)] in forward order."""
        out, inplanes = [], self.widths[0]
        for li, (n, planes) in enumerate(zip(self.layers, self.widths)):
            for b in range(n):
                stride = 2 if (b == 0 and li > 0) else 1
                down = stride != 1 or inplanes != planes * self.expansion
                out.append((f"layer{li + 1}.{b}", inplanes, planes, stride, down))
                inplanes = planes * self.expansion
        return out


def _conv(cin, cout, k, stride=1, pad=0):
    return nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=pad, bias=False)


class _Block(nn.Module):
    """torchvision ``BasicBlock`` / ``Bottleneck``: the sub-module names in their registration order."""

    def __init__(self, s: ResNetShape, inplanes, planes, stride, down):
        super().__init__()
        out = planes * s.expansion
        if s.block == "basic":
            self.conv1, self.bn1 = _conv(inplanes, planes, 3, stride, 1), nn.BatchNorm2d(planes, s.eps, s.momentum)
            self.conv2, self.bn2 = _conv(planes, planes, 3, 1, 1), nn.BatchNorm2d(planes, s.eps, s.momentum)
        else:
            self.conv1, self.bn1 = _conv(inplanes, planes, 1), nn.BatchNorm2d(planes, s.eps, s.momentum)
            self.conv2, self.bn2 = _conv(planes, planes, 3, stride, 1), nn.BatchNorm2d(planes, s.eps, s.momentum)
            self.conv3, self.bn3 = _conv(planes, out, 1), nn.BatchNorm2d(out, s.eps, s.momentum)
        if down:
            self.downsample = nn.Sequential(_conv(inplanes, out, 1, stride), nn.BatchNorm2d(out, s.eps, s.momentum))


class HipResNet(nn.Module):
    def __init__(self, shape: ResNetShape, num_classes: int = 1000):
        super().__init__()
        self.shape = shape
        w0 = shape.widths[0]
        self.conv1 = _conv(shape.num_channels, w0, 7, 2, 3)
        self.bn1 = nn.BatchNorm2d(w0, shape.eps, shape.momentum)
        blocks = shape.blocks()
        at = 0
        for li, n in enumerate(shape.layers):
            setattr(self, f"layer{li + 1}", nn.Sequential(*[_Block(shape, *b[1:]) for b in blocks[at:at + n]]))
            at += n
        self.fc = nn.Linear(shape.num_features, num_classes)      # V/run.py:42-46 replaces it by Linear(num_fc_ftr, embedding_dim)
        for m in self.modules():       # torchvision ResNet.__init__
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        raise NotImplementedError("HipResNet only holds the weights: run it through Resnet_Encoder (resnet_engine)")

    @staticmethod
    def shape_of(module) -> ResNetShape:
        """The shape of any module with torchvision's ResNet keys, read from its ``state_dict``."""
        sd = module.state_dict()
        if "conv1.weight" not in sd or "layer1.0.conv1.weight" not in sd or not hasattr(module, "fc"):
            raise NotImplementedError(f"ResNet tower: from_torch adopts a module with torchvision's ResNet keys, got {type(module).__name__}")
        bottleneck = "layer1.0.conv3.weight" in sd
        layers, widths = [], []
        for li in range(1, 5):
            n = 0
            while f"layer{li}.{n}.conv1.weight" in sd:
                n += 1
            layers.append(n)
            widths.append(sd[f"layer{li}.0.conv1.weight"].shape[0])
        bn = getattr(module, "bn1", None)      # eps / momentum of the adopted module's BatchNorm layers (one value for the net, as torchvision builds it)
        eps, momentum = float(getattr(bn, "eps", 1e-5)), getattr(bn, "momentum", 0.1)
        if momentum is None:
            raise NotImplementedError("ResNet tower: BatchNorm momentum=None (cumulative average) is not built")
        return ResNetShape("bottleneck" if bottleneck else "basic", tuple(layers), tuple(widths), num_channels=sd["conv1.weight"].shape[1],
                           eps=eps, momentum=float(momentum))

    @staticmethod
    def from_torch(module) -> "HipResNet":
        """Adopt any module with those keys (a torchvision ``ResNet``, its ``fc`` as it stands): weights and buffers copied, the
        ``requires_grad`` flags kept, the parameter ORDER checked (``V/run.py`` freezes parameters by index)."""
        shape = HipResNet.shape_of(module)
        m = HipResNet(shape, num_classes=module.fc.out_features)
        m.load_state_dict(module.state_dict())
        theirs = list(module.named_parameters())
        mine = list(m.named_parameters())
        assert [n for n, _ in mine] == [n for n, _ in theirs], "parameter order differs from torchvision's"
        for (_, p1), (_, p2) in zip(mine, theirs):
            p1.requires_grad = p2.requires_grad
        return m
