"""The volume-sized helpers of StereoAnywhere (reference models/StereoAnywhere/utils/utils.py:112-170, 216-238) on the kernels of
csrc/allpairs.hip: disparity and confidence regressed from the all-pairs volume [B, 1, H, W2, W3] in both directions, and the
truncation mask.  Same signatures, shapes ([B, 1, H, W]) and dtypes as the reference.  Each `estimate_*` asks the fused op for its
own output only (the other direction is not run); a model that wants the set -- stereoanywhere.py:285-331 calls all four on one
volume, two to three times per forward -- calls `estimate_all`, which reads the volume once per direction.  All are differentiated
with respect to the volume (one backward launch for whatever was asked).  W2 and W3 must lie in 2..512.

The mono-stereo alignment stage (utils/utils.py:48-54, 172-198, 240-269, 345-384, 412-422; stereoanywhere.py:167-235) runs on the
kernels of csrc/mono_align.hip: `generate_masks`, `masked_volume`, `softlrc`, `weighted_lsq`, `handcrafted_mirror_detector`, and
`align_mono`, which composes stereoanywhere.py:218-235 from them without a host synchronisation."""
import collections

import torch

from ... import ops


def estimate_all(corr_volume):
    """corr_volume [B, 1, H, W2, W3] -> (disp_left [B,1,H,W2], conf_left [B,1,H,W2], disp_right [B,1,H,W3], conf_right [B,1,H,W3])"""
    return ops.allpairs_estimates(corr_volume, ops.ALLPAIRS_ALL)


def _crop(x, vol_pad):
    return x[:, :, :, vol_pad[0]:x.shape[3] - vol_pad[1]]


def estimate_left_disparity(corr_volume, vol_pad=[0, 0]):
    """w2 - sum_w3 softmax_w3(volume) w3, cropped by vol_pad along W (utils.py:112-131)."""
    return _crop(ops.allpairs_estimates(corr_volume, ops.ALLPAIRS_DISP_LEFT)[0], vol_pad)


def estimate_right_disparity(corr_volume, vol_pad=[0, 0]):
    """sum_w2 softmax_w2(volume) w2 - w3, cropped by vol_pad along W (utils.py:133-152)."""
    return _crop(ops.allpairs_estimates(corr_volume, ops.ALLPAIRS_DISP_RIGHT)[2], vol_pad)


def estimate_left_confidence(corr_volume, logsumexp_eps=1e-3):
    """1 - entropy of softmax_w3 / log2(W3) with the reference's log2(p + 1e-6) (utils.py:154-161); `logsumexp_eps` is unused
    there too."""
    return ops.allpairs_estimates(corr_volume, ops.ALLPAIRS_CONF_LEFT)[1]


def estimate_right_confidence(corr_volume, logsumexp_eps=1e-3):
    """The same along W2, normalised by log2(W2) (utils.py:163-170)."""
    return ops.allpairs_estimates(corr_volume, ops.ALLPAIRS_CONF_RIGHT)[3]


def truncate_corr_volume_v2(disp_left, conf_left, conf_th=0.5, attenuation_gain=0.1):
    """[B, 1, H, W] x 2 -> the mask volume [B, 1, H, W, W] (utils.py:216-238); conf_th=None uses conf_left as it is."""
    return ops.truncate_mask(disp_left, conf_left, conf_th, attenuation_gain)


def convex_upflow(flow, mask, n_downsample=2, use_scale_factor=True):
    """reference StereoAnywhere/utils/utils.py:97-110 on the fused kernel of csrc/convex_upsample.hip: flow [N,D,H,W], mask
    [N,9*4^n,H,W] (logits) -> [N,D,2^n H,2^n W]."""
    return ops.convex_upsample(flow, mask, n_downsample=n_downsample, use_scale_factor=use_scale_factor)


def generate_masks(mde, N=16):
    """mde [B, 1, H, W] -> one-hot fp16 masks [B, N, H, W] (utils.py:48-54): channel i where i/N <= mde < (i+1)/N, the thresholds
    rounded to fp32 as the reference's comparison does."""
    return ops.generate_masks(mde, N)


def masked_volume(volume, mde_left, mde_right, n_masks):
    """volume [B, 1, H, W2, W3] -> [B, N, H, W2, W3] = volume * generate_masks(mde_left).unsqueeze(4) *
    generate_masks(mde_right).unsqueeze(3) (stereoanywhere.py:180,193) in one pass.  The maps are at the volume's resolution: for
    vol_downsample > 0 the reference nearest-interpolates the masks, which equals the masks of the strided maps
    (mde[:, :, ::2**k, ::2**k]) -- the caller strides.  A non-finite volume entry under a zero mask gives 0 (NaN in the reference)."""
    return ops.masked_volume(volume, mde_left, mde_right, n_masks)


def softlrc(disp2, disp3, lrc_th=1.0):
    """Soft left-right consistency of both views (utils.py:189-198), each [B, 1, H, W] in (0, 1); lrc_th <= 20."""
    return ops.softlrc(disp2, disp3, lrc_th)


def weighted_lsq(mde, disp, conf, min_quantile=0.2, max_quantile=0.9):
    """(scale, shift), each [B, 1, 1, 1] (utils.py:345-384), without the reference's loop over the batch, boolean indexing, sorts
    and lstsq call: see ops.weighted_lsq (a singular system gives scale 0 and the weighted mean as shift)."""
    return ops.weighted_lsq(mde, disp, conf, min_quantile, max_quantile)


def handcrafted_mirror_detector(stereo_disp, mono_disp, stereo_conf, mono_conf, conf_th=0.5, step_gain=20):
    """(MONO >> STEREO and both confident) or (mono confident and stereo not), as a soft step (utils.py:255-269)."""
    return ops.mirror_detector(stereo_disp, mono_disp, stereo_conf, mono_conf, conf_th, step_gain)


def fuzzy_and(x, y):
    return x * y


def fuzzy_or(x, y):
    return x + y - x * y


def fuzzy_not(x):
    return 1 - x


def apply_scale_shift(mde, scales, shifts, masks=None):
    """sum over the N masks of (scales * mde + shifts) * masks (utils.py:412-422); masks=None: one channel of ones."""
    scaled = scales * mde + shifts
    return torch.sum(scaled if masks is None else scaled * masks, dim=1, keepdim=True)


MonoAlignment = collections.namedtuple("MonoAlignment", [
    "softlrc_mono2", "softlrc_mono3",      # softlrc of the coarse mono-volume disparities
    "conf2", "conf3",                      # fuzzy_and(learned confidence, softlrc)
    "scale", "shift",                      # weighted_lsq on the concatenated pairs, [B, 1, 1, 1]
    "scaled_mde2", "scaled_mde3",          # scale * mde + shift
    "softlrc_scaled_mde2",                 # softlrc of the scaled maps (left)
    "mirror_conf2",                        # handcrafted_mirror_detector
    "truncate_mask"])                      # truncate_corr_volume_v2(scaled_mde2, mirror_conf2, conf_th=None), detached


def align_mono(mde2, mde3, dispmono2, dispmono3, lconf2, lconf3, lrc_th=1.0, mirror_conf_th=0.98, mirror_attenuation=0.9):
    """stereoanywhere.py:218-235 on the maps at volume resolution, all [B, 1, H, W]: the monocular depth maps, the disparities
    regressed from the mono volume and their learned confidences -> MonoAlignment.  Runs without a host synchronisation."""
    lrc2, lrc3 = softlrc(dispmono2, dispmono3, lrc_th=lrc_th)
    conf2, conf3 = fuzzy_and(lconf2, lrc2), fuzzy_and(lconf3, lrc3)
    scale, shift = weighted_lsq(torch.cat([mde2, mde3], 1), torch.cat([dispmono2, dispmono3], 1), torch.cat([conf2, conf3], 1))
    scaled2 = torch.sum(scale * mde2 + shift, dim=1, keepdim=True)
    scaled3 = torch.sum(scale * mde3 + shift, dim=1, keepdim=True)
    lrc_scaled2, _ = softlrc(scaled2, scaled3, lrc_th=lrc_th)
    mirror2 = handcrafted_mirror_detector(dispmono2, scaled2, conf2, lrc_scaled2, conf_th=mirror_conf_th)
    mask = truncate_corr_volume_v2(scaled2, mirror2, conf_th=None, attenuation_gain=mirror_attenuation).detach()
    return MonoAlignment(lrc2, lrc3, conf2, conf3, scale, shift, scaled2, scaled3, lrc_scaled2, mirror2, mask)
