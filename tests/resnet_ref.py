"""A plain-torch ResNet that restates torchvision's module tree (``torchvision.models.resnet``: ``conv1``, ``bn1``, ``relu``, ``maxpool``,
``layer{1..4}`` of ``BasicBlock`` / ``Bottleneck`` with ``downsample.{0,1}``, ``avgpool``, ``fc``), with the same key names and registration
order, built from ``nn.Conv2d``, ``BatchNorm2d``, ``MaxPool2d`` and ``AdaptiveAvgPool2d`` only.  torchvision is not installed where the
goldens are made; the reference's ``Resnet_Encoder`` / ``Model`` take the backbone as an object, so this module stands in for it.
v1.5 (the stride on ``conv2`` of a Bottleneck), ``zero_init_residual`` off.  Not a test file."""
import torch
import torch.nn as nn


def conv3x3(i, o, stride=1):
    return nn.Conv2d(i, o, kernel_size=3, stride=stride, padding=1, bias=False)


def conv1x1(i, o, stride=1):
    return nn.Conv2d(i, o, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv1x1(inplanes, planes)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = conv3x3(planes, planes, stride)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = conv1x1(planes, planes * self.expansion)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, block, layers, widths=(64, 128, 256, 512), num_classes=1000):
        super().__init__()
        self.inplanes = widths[0]
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, widths[0], layers[0])
        self.layer2 = self._make_layer(block, widths[1], layers[1], stride=2)
        self.layer3 = self._make_layer(block, widths[2], layers[2], stride=2)
        self.layer4 = self._make_layer(block, widths[3], layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(widths[3] * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride), nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def features(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return torch.flatten(self.avgpool(x), 1)

    def forward(self, x):
        return self.fc(self.features(x))


MICRO = (32, 64, 128, 256)
NETS = {
    "resnet18": (BasicBlock, (2, 2, 2, 2)), "resnet34": (BasicBlock, (3, 4, 6, 3)), "resnet50": (Bottleneck, (3, 4, 6, 3)),
    "resnet101": (Bottleneck, (3, 4, 23, 3)), "resnet152": (Bottleneck, (3, 8, 36, 3)),
    "resnet_micro": (BasicBlock, (1, 1, 1, 1), MICRO), "resnet_micro_b": (Bottleneck, (1, 1, 1, 1), MICRO),
}


def build(name, num_classes=1000):
    return ResNet(*NETS[name], num_classes=num_classes)


def det_value(key, shape):
    """The deterministic value of a ``state_dict`` key (``utils/detgen``): BatchNorm gains 1 +- 0.1, running means ~ N(0, 0.1^2),
    running variances in [0.7, 1.3), everything else ``det_param``.  None: leave the entry (``num_batches_tracked``)."""
    import numpy as np
    from idvs.morec_amd.utils.detgen import det_normal, det_param, det_uniform
    if key.endswith("num_batches_tracked"):
        return None
    if key.endswith("running_mean"):
        return det_normal(key, shape, std=0.1)
    if key.endswith("running_var"):
        return (1.0 + 0.3 * det_uniform(key, shape)).astype(np.float32)
    if key.endswith(".weight") and len(shape) == 1:
        return (1.0 + 0.1 * det_uniform(key, shape)).astype(np.float32)
    return det_param(key, shape)


def load_det(module, prefix=""):
    with torch.no_grad():
        for k, v in module.state_dict().items():
            val = det_value(prefix + k, tuple(v.shape))
            if val is not None:
                v.copy_(torch.from_numpy(val))
    return module


N_SAMPLE = 128


def sample_idx(key, numel):
    """The flat indices of the elements of gradient ``key`` that the g32 fixture keeps (all of them up to ``N_SAMPLE``)."""
    import numpy as np
    from idvs.morec_amd.utils.detgen import det_randint
    return np.arange(numel) if numel <= N_SAMPLE else det_randint("g32.idx." + key, (N_SAMPLE,), 0, numel)
