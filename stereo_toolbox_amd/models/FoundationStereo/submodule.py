"""FoundationStereo's initial cost volume on the HIP kernels -- drop-in functions of reference
models/FoundationStereo/submodule.py:388-427 and the four lines of `FoundationStereo.forward` that build the combined volume
(foundation_stereo.py:243-248).  NOT the same arithmetic as the IGEV / MonSter volume (VERDICT r5 "Missing" 2):

  * `groupwise_correlation` is a per-group COSINE similarity: both maps are L2-normalised over each group's channels at every
    pixel (`F.normalize(fea.float(), dim=2)`, eps 1e-12) and the products are SUMMED, not averaged; the reference computes it
    outside autocast in fp32 (:394-395) -- so does this (ops.fp32_region);
  * `build_concat_volume` leaves the LEFT half unmasked (:418-424, like ACVNet's), the right half is the shifted copy.

The norm of a pixel does not depend on the disparity, so the normalised volume is the plain group-wise correlation volume of the
two normalised maps: one HBM-bound pre-pass per map (csrc/group_normalize.hip), then the MFMA builder (20 / 28 channels per
group for the 160 / 224-channel maps of the vitb / vitl backbones, 16 for vits).

Behind the volume, `Conv3dNormActReduced` -- the "axial-planar convolution" that makes up twelve layers of the reference's
`hourglass` (foundation_stereo.py:46-124) -- runs on csrc/conv3d_axial.hip.  NOT built: the disparity transformer
(`CostVolumeDisparityAttention`, flash attention), the composed `hourglass` / `corr_stem` / `classifier` (the classifier's
7x7x7 convolution is another unsupported shape), the GRU update block and the DepthAnything backbone.  `corr_stem` etc. take
the dense NDHWC volume of `init_comb_volume` through aggregation.conv_block like the IGEV aggregation does.
"""
import torch.nn as nn

from ... import ops
from ...aggregation import axial_conv_block


def groupwise_correlation(fea1, fea2, num_groups):
    """reference FoundationStereo/submodule.py:388-397 -> [B, G, H, W]: sum_c normalize(fea1)[g,c] * normalize(fea2)[g,c]."""
    B, C, H, W = fea1.shape
    assert C % num_groups == 0, f"C:{C}, num_groups:{num_groups}"
    cost = ops.cost_volume(fea1, fea2, None, None, 1, num_groups, normalize=True)          # [B,1,H,W,G]
    cost = cost.reshape(B, H, W, num_groups).permute(0, 3, 1, 2)
    assert cost.shape == (B, num_groups, H, W)
    return cost


def build_gwc_volume(refimg_fea, targetimg_fea, maxdisp, num_groups, stride=1):
    """reference :399-413 -> [B, G, D, H, W] (zero where w < d); `stride` is accepted and unused, as in the reference."""
    B, C, H, W = refimg_fea.shape
    assert C % num_groups == 0, f"C:{C}, num_groups:{num_groups}"
    return ops.to_ncdhw(ops.cost_volume(refimg_fea, targetimg_fea, None, None, maxdisp, num_groups, normalize=True))


def build_concat_volume(refimg_fea, targetimg_fea, maxdisp):
    """reference :416-427 -> [B, 2C, D, H, W]: left half = the left map at every disparity (NOT masked), right half shifted."""
    return ops.to_ncdhw(ops.cost_volume(None, None, refimg_fea, targetimg_fea, maxdisp, 0, mask_left=False))


def disparity_regression(x, maxdisp):
    """reference FoundationStereo/submodule.py `disparity_regression`: sum_d d * x[b,d,h,w], keepdim -> [B,1,H,W]."""
    return ops.softargmax(x, maxdisp, keepdim=True)


def init_comb_volume(features_left, features_right, left_tmp, right_tmp, max_disp, cv_group=8):
    """foundation_stereo.py:243-248 in one pass: cat(build_gwc_volume(features[0]), build_concat_volume(proj_cmb(features[0])))
    written straight into the dense channels-last volume [B, max_disp/4, H/4, W/4, cv_group + 2 * 12] that `corr_stem` reads
    (`ops.to_ncdhw` gives the reference's [B, C, D, H, W] view)."""
    return ops.cost_volume(features_left, features_right, left_tmp, right_tmp, max_disp // 4, cv_group, mask_left=False,
                           normalize=True)


class Conv3dNormActReduced(nn.Module):
    """reference FoundationStereo/submodule.py:89-114: Conv3d (1,k,k) + norm + ReLU, then Conv3d (kernel_disp,1,1) + norm + ReLU,
    both convolutions with a bias -- same signature, same state-dict keys (`conv1.0.weight`, `conv1.0.bias`, `conv1.1.*`,
    `conv2.0.*`, `conv2.1.*`), shapes and order.  The nn modules are parameter containers; the arithmetic runs on the
    axial-planar MFMA kernels (aggregation.axial_conv_block), in fp32 also under autocast.

    Served: kernel_size 3, kernel_disp odd up to 17, stride 1, norm = BatchNorm3d (SyncBatchNorm after conversion).  Anything else
    raises StxError at construction; there is no CPU fallback.

    The gradient of `conv*.0.bias` under a train-mode BatchNorm is analytically zero (the batch mean removes the bias); the
    block returns exact zeros for it, where the reference's autograd leaves rounding noise (1e-14 in fp64).  With eval-mode
    BatchNorm and gradients enabled it is the channel sum of the raw output's gradient."""

    def __init__(self, C_in, C_out, hidden=None, kernel_size=3, kernel_disp=None, stride=1, norm=nn.BatchNorm3d):
        super().__init__()
        if kernel_disp is None:
            kernel_disp = kernel_size
        if hidden is None:
            hidden = C_out
        if stride != 1:
            raise ops.StxError(f"Conv3dNormActReduced: stride {stride} is not served (stride 1 only)")
        if kernel_size != 3:
            raise ops.StxError(f"Conv3dNormActReduced: kernel_size {kernel_size} is not served (3 only)")
        if kernel_disp % 2 != 1 or not 3 <= kernel_disp <= ops.AXIAL_MAX_TAPS:
            raise ops.StxError(f"Conv3dNormActReduced: kernel_disp {kernel_disp} is not served (odd, 3..{ops.AXIAL_MAX_TAPS})")
        if not (isinstance(norm, type) and issubclass(norm, nn.modules.batchnorm._BatchNorm)):
            raise ops.StxError(f"Conv3dNormActReduced: norm {getattr(norm, '__name__', norm)} is not a BatchNorm")
        if max(C_in, hidden, C_out) > ops.AXIAL_MAX_CHANNELS:
            raise ops.StxError(f"Conv3dNormActReduced: more than {ops.AXIAL_MAX_CHANNELS} channels are not served")
        self.conv1 = nn.Sequential(
            nn.Conv3d(C_in, hidden, kernel_size=(1, kernel_size, kernel_size), padding=(0, kernel_size // 2, kernel_size // 2),
                      stride=(1, stride, stride)),
            norm(hidden),
            nn.ReLU(),
        )
        self.conv2 = nn.Sequential(
            nn.Conv3d(hidden, C_out, kernel_size=(kernel_disp, 1, 1), padding=(kernel_disp // 2, 0, 0), stride=(stride, 1, 1)),
            norm(C_out),
            nn.ReLU(),
        )

    def run(self, x):
        """x: dense [B, D, H, W, C] on a ROCm device -> dense [B, D, H, W, C_out]."""
        x = axial_conv_block(x, self.conv1[0], self.conv1[1])
        return axial_conv_block(x, self.conv2[0], self.conv2[1])

    @ops.fp32_region
    def forward(self, x):
        """x: logical [B, C, D, H, W] (any strides; a view of a dense NDHWC tensor costs no copy) -> logical [B, C_out, D, H, W]."""
        if x.dim() != 5:
            raise ops.StxError(f"Conv3dNormActReduced: expected [B, C, D, H, W], got shape {tuple(x.shape)}")
        return ops.to_ncdhw(self.run(ops.to_ndhwc(x)))
