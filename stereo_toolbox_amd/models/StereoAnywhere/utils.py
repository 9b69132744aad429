"""The volume-sized helpers of StereoAnywhere (reference models/StereoAnywhere/utils/utils.py:112-170, 216-238) on the kernels of
csrc/allpairs.hip: disparity and confidence regressed from the all-pairs volume [B, 1, H, W2, W3] in both directions, and the
truncation mask.  Same signatures, shapes ([B, 1, H, W]) and dtypes as the reference.  Each `estimate_*` asks the fused op for its
own output only (the other direction is not run); a model that wants the set -- stereoanywhere.py:285-331 calls all four on one
volume, two to three times per forward -- calls `estimate_all`, which reads the volume once per direction.  All are differentiated
with respect to the volume (one backward launch for whatever was asked).  W2 and W3 must lie in 2..512."""
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
