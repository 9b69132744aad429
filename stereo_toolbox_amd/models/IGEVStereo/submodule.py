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
