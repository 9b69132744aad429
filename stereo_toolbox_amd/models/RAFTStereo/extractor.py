"""The residual block of the RAFT-family feature and context encoders with its instance norms on csrc/instnorm.hip.

`ResidualBlock` is a drop-in for the class the reference defines in RAFTStereo/extractor.py:6-60 and, with the same class text
(up to the spelling of `super()` and blank lines), in the extractors of DEFOMStereo, IGEVStereo, MonSter, StereoAnywhere,
SelectiveIGEV and SelectiveRAFT: same constructor, forward, module tree and state-dict keys (`conv1 / conv2 . weight / bias`,
`downsample.0 . weight / bias`, the norms' own keys for 'group' and 'batch'), so their checkpoints load.  One class object
serves those packages.  FoundationStereo's block adds a 'layer' norm and is not this class.  The encoders themselves
(BasicEncoder, MultiBasicEncoder, BottleneckBlock) are not built.
"""
import torch.nn as nn

from ... import ops


def _norm(norm_fn, planes):
    if norm_fn == "group":
        return nn.GroupNorm(num_groups=planes // 8, num_channels=planes)
    if norm_fn == "batch":
        return nn.BatchNorm2d(planes)
    if norm_fn == "instance":
        return nn.InstanceNorm2d(planes)
    if norm_fn == "none":
        return nn.Sequential()
    return None                                                          # (the reference builds no norm for an unknown name)


class ResidualBlock(nn.Module):
    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        projected = not (stride == 1 and in_planes == planes)
        if _norm(norm_fn, planes) is not None:
            self.norm1 = _norm(norm_fn, planes)
            self.norm2 = _norm(norm_fn, planes)
            if projected:
                self.norm3 = _norm(norm_fn, planes)
        self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3) if projected else None
        self.fused = norm_fn == "instance"

    def forward(self, x):
        if not self.fused:
            y = self.relu(self.norm1(self.conv1(x)))
            y = self.relu(self.norm2(self.conv2(y)))
            if self.downsample is not None:
                x = self.downsample(x)
            return self.relu(x + y)
        # norm1 + relu in one pass; norm2 + relu + add + relu in one pass with the shortcut as `skip`; norm3 without activation
        y = ops.instance_norm(self.conv1(x), "relu", eps=self.norm1.eps)
        if self.downsample is not None:
            x = ops.instance_norm(self.downsample[0](x), "none", eps=self.norm3.eps)
        return ops.instance_norm(self.conv2(y), "relu", eps=self.norm2.eps, skip=x)
