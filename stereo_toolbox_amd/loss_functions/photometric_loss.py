"""reference loss_functions/photometric_loss.py on csrc/selfsup_loss.hip (stereo_toolbox_amd.ops)."""
from .. import ops

__all__ = ["warp_right_to_left", "ssim", "photometric_loss"]


def warp_right_to_left(right_image, disp):
    """right_image [B, C, H, W], disp [B, 1, H, W] -> (warped_right, valid_mask), both [B, C, H, W]; reference :5-37.  The gradient
    goes to disp; valid_mask carries none."""
    return ops.photo_warp(right_image, disp)


def ssim(x, y, window_size=7, pad_mode='reflect'):
    """SSIM distance clamp((1 - SSIM) / 2, 0, 1), [B, C, H, W]; reference :40-77.  Odd windows 3 .. 11, reflect padding only."""
    return ops.ssim_distance(x, y, window_size, pad_mode)


def photometric_loss(left_image, right_image, disp=None, ssim_weight=0.85, enable_mask=True):
    """[B, 1, H, W]; reference :80-104, one kernel launch.  disp=None with enable_mask=True, where the reference dies on an
    unbound valid_mask, raises StxError."""
    return ops.photometric_loss(left_image, right_image, disp, ssim_weight, enable_mask)
