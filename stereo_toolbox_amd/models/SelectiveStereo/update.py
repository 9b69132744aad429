"""What SelectiveStereo adds to the iterative families, on csrc/selgru.hip and csrc/csa.hip.

Drop-ins for the classes the reference defines with the same text in SelectiveStereo/SelectiveRAFT/update.py and
SelectiveStereo/SelectiveIGEV/update.py: `RaftConvGRU` (:15-30; the SelectiveIGEV copy adds `dilation`, served at 1),
`SelectiveConvGRU` (:61-71), `ChannelAttentionEnhancement` (:106-121) and `SpatialAttentionExtractor` (:123-135) -- same
constructors, forward signatures and state-dict keys, so their checkpoints load.  One class object serves both sub-packages.  `contextual_spatial_attention` is the two list comprehensions of
SelectiveIGEV/igev_stereo.py:225-226 on the fused op.  The rest of the update block (motion encoders, heads, pool2x / interp,
BasicSelectiveMultiUpdateBlock, RaftSepConvGRU) is not built.
"""
import torch.nn as nn

from ... import ops


class RaftConvGRU(nn.Module):
    def __init__(self, hidden_dim=128, input_dim=256, kernel_size=3, dilation=1):
        super().__init__()
        if dilation != 1:
            raise ops.StxError(f"RaftConvGRU: dilation {dilation}; the gfx950 cells serve dilation 1 only")
        if kernel_size not in (1, 3):
            raise ops.StxError(f"RaftConvGRU: kernel_size {kernel_size}; the gfx950 cells serve 1x1 and 3x3")
        # nn.Conv2d holds the parameters (keys, shapes and default initialisation of the reference); it is never called
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)

    def weights(self):
        return (self.convz.weight, self.convz.bias, self.convr.weight, self.convr.bias, self.convq.weight, self.convq.bias)

    def forward(self, h, *x_list):
        return ops.raft_convgru(h, x_list, *self.weights())


class SelectiveConvGRU(nn.Module):
    def __init__(self, hidden_dim=128, input_dim=256, small_kernel_size=1, large_kernel_size=3):
        super().__init__()
        if 1 not in (small_kernel_size, large_kernel_size):
            raise ops.StxError(f"SelectiveConvGRU: kernel sizes {small_kernel_size} and {large_kernel_size}; one cell must be 1x1 "
                               "(its kernel forms the blend)")
        self.small_gru = RaftConvGRU(hidden_dim, input_dim, small_kernel_size)
        self.large_gru = RaftConvGRU(hidden_dim, input_dim, large_kernel_size)

    def forward(self, att, h, *x):
        return ops.selective_convgru(att, h, x, self.small_gru.weights(), self.large_gru.weights())


class ChannelAttentionEnhancement(nn.Module):
    def __init__(self, in_planes, ratio=16):
        super().__init__()
        # (the reference ignores `ratio` too: the hidden width is in_planes // 16)
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.max_pool = nn.AdaptiveMaxPool2d(1)
        self.fc = nn.Sequential(nn.Conv2d(in_planes, in_planes // 16, 1, bias=False),
                                nn.ReLU(),
                                nn.Conv2d(in_planes // 16, in_planes, 1, bias=False))
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return ops.csa_gate(x, self.fc[0].weight, self.fc[2].weight)


class SpatialAttentionExtractor(nn.Module):
    def __init__(self, kernel_size=7):
        super().__init__()
        self.samconv = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        return ops.csa_spatial(x, self.samconv.weight)


def contextual_spatial_attention(cam, sam, x_list):
    """`inp_list = [cam(x) * x for x in x_list]; att = [sam(x) for x in inp_list]` (reference SelectiveIGEV/igev_stereo.py:225-226)
    with one fused call per map; returns (inp_list, att_list)."""
    pairs = [ops.csa(x, cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight) for x in x_list]
    return [p[0] for p in pairs], [p[1] for p in pairs]
