"""The cost-volume entry of the IGEV family (IGEV-Stereo, and with the same call MonSter, MonSter/submodule.py:151-171;
FoundationStereo's volume is a DIFFERENT function -- per-group cosine similarity -- and lives in models/FoundationStereo) on the HIP
kernels -- drop-in functions of reference models/IGEVStereo/submodule.py plus the two lines of
`IGEVStereo.forward` that sit on the hot path (igev_stereo.py:206 and :211-212).  The 3-D regularisation between them
(`corr_stem`, `corr_feature_att`, `cost_agg` = hourglass(8), `classifier`) is in aggregation.py, the geometry-encoding lookup
of the GRU iterations (`Combined_Geo_Encoding_Volume`) in geometry.py, and `context_upsample` (submodule.py:243-255, the convex 4x upsampling of igev_stereo.py:164,254) below; the
rest of those models (feature backbones, GRU updates) is outside the scope of this package.

    gwc_volume = build_gwc_volume(match_left, match_right, max_disp // 4, 8)      # 96 channels -> 8 groups of 12
    prob       = F.softmax(classifier(volume).squeeze(1), dim=1)
    init_disp  = disparity_regression(prob, max_disp // 4)                        # [B,1,H/4,W/4]

The volume runs on the MFMA builder with K = 12 channels per group (three v_mfma_f32_16x16x4_f32 steps per tile), its
backward on the generic gather kernel; softmax + regression on the estimator kernels.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..GwcNet.submodule import build_gwc_volume, groupwise_correlation  # noqa: F401  (same arithmetic, submodule.py:153-171)


def disparity_regression(x, maxdisp):
    """reference IGEVStereo/submodule.py:221-225: sum_d d * x[b,d,h,w], keepdim -> [B,1,H,W]."""
    return ops.softargmax(x, maxdisp, keepdim=True)


def init_gwc_volume(match_left, match_right, max_disp, num_groups=8):
    """igev_stereo.py:206 -> [B, 8, max_disp/4, H/4, W/4]."""
    return build_gwc_volume(match_left, match_right, max_disp // 4, num_groups)


class _SoftmaxDFn(torch.autograd.Function):
    """softmax over the disparity axis of a dense [B,D,H,W] cost on the HIP kernel, with its (elementwise) backward."""

    @staticmethod
    def forward(ctx, x):
        y = ops.softmax_over_d(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return y * (g - (g * y).sum(1, keepdim=True))


def init_disparity(cost, max_disp):
    """igev_stereo.py:211-212: cost [B,1,D',H',W'] (classifier output) -> init_disp [B,1,H',W'] at 1/4 resolution."""
    c = cost.squeeze(1).contiguous()
    prob = _SoftmaxDFn.apply(c) if (torch.is_grad_enabled() and c.requires_grad) else ops.softmax_over_d(c)
    return disparity_regression(prob, max_disp // 4)


def context_upsample(disp_low, up_weights):
    """reference IGEVStereo/submodule.py:243-255: disp_low [B,1,h,w], up_weights [B,9,4h,4w] -> [B,4h,4w], every output pixel
    the up_weights-weighted sum of the 3x3 low-resolution neighbourhood of its cell (zero padding); one fused kernel forward,
    two backward (stx_context_upsample_fwd / _bwd), no unfolded or nearest-upsampled temporary."""
    return ops.context_upsample(disp_low, up_weights)


def upsample_disp_from_logits(disp, spx_logits):
    """The two lines `spx_pred = F.softmax(spx_pred, 1)`, `context_upsample(disp * 4., spx_pred)` of igev_stereo.py:158-166 (and of
    MonSter, FoundationStereo, Selective-IGEV) in one kernel that takes the LOGITS of the `spx` head: disp [B,1,h,w], spx_logits
    [B,9,4h,4w] -> [B,4h,4w].  The full-resolution soft-max pass and its saved output are gone; the backward re-forms it."""
    return ops.softmax_context_upsample(disp, spx_logits, 4.0)


# --------------------------------------------------------------------------------------- convolution + instance norm blocks
_CONVS = {(False, False): nn.Conv2d, (False, True): nn.ConvTranspose2d, (True, False): nn.Conv3d, (True, True): nn.ConvTranspose3d}


class BasicConv_IN(nn.Module):
    """Drop-in for the reference's BasicConv_IN (IGEVStereo/submodule.py:82-108; the same class text in FoundationStereo, MonSter,
    SelectiveIGEV and SelectiveRAFT): bias-free conv or transposed conv in 2-D or 3-D (`**kwargs` go to it), instance norm when
    `IN`, LeakyReLU(0.01) when `relu`.  Children `conv` and `IN` as in the reference (`IN` has neither parameters nor buffers and
    is not called when the fused kernel runs); the state dict is `conv.weight`.  The convolution is stock; norm + activation are
    one pass of ops.instance_norm, whose backward keeps the conv output alone."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, IN=True, relu=True, **kwargs):
        super().__init__()
        self.relu = relu
        self.use_in = IN
        self.conv = _CONVS[bool(is_3d), bool(deconv)](in_channels, out_channels, bias=False, **kwargs)
        self.IN = (nn.InstanceNorm3d if is_3d else nn.InstanceNorm2d)(out_channels)

    def forward(self, x):
        x = self.conv(x)
        if self.use_in:
            return ops.instance_norm(x, "lrelu" if self.relu else "none", eps=self.IN.eps)
        return F.leaky_relu(x) if self.relu else x


class Conv2x_IN(nn.Module):
    """Drop-in for the reference's Conv2x_IN (IGEVStereo/submodule.py:111-150; the same class text in MonSter, SelectiveIGEV and
    SelectiveRAFT -- FoundationStereo's differs: a ResnetBasicBlock as conv2 and a bilinear resize): conv1 halves (or, as a
    transposed conv, doubles) the resolution, the result is resized to `rem` by nearest neighbour when the shapes differ,
    concatenated with `rem` (or added to it), and goes through conv2.  Both are BasicConv_IN blocks."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, concat=True, keep_concat=True, IN=True, relu=True,
                 keep_dispc=False):
        super().__init__()
        self.concat = concat
        self.is_3d = is_3d
        if deconv and is_3d and keep_dispc:
            geom = dict(kernel_size=(1, 4, 4), stride=(1, 2, 2), padding=(0, 1, 1))
        else:
            geom = dict(kernel_size=((4, 4, 4) if is_3d else 4) if deconv else 3, stride=2, padding=1)
        self.conv1 = BasicConv_IN(in_channels, out_channels, deconv, is_3d, IN=True, relu=True, **geom)
        cin, cout = (2 * out_channels, out_channels * (2 if keep_concat else 1)) if concat else (out_channels, out_channels)
        self.conv2 = BasicConv_IN(cin, cout, False, is_3d, IN, relu, kernel_size=3, stride=1, padding=1)

    def forward(self, x, rem):
        x = self.conv1(x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="nearest")
        x = torch.cat((x, rem), 1) if self.concat else x + rem
        return self.conv2(x)
