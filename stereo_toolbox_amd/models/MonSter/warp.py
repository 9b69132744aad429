"""Reference models/MonSter/warp.py on csrc/monster.hip."""
from ... import ops


def disp_warp(img, disp, padding_mode='border'):
    """Warping by disparity (reference warp.py:53-79), one launch instead of two grid_sample passes.
    Args:
        img: [B, C, H, W]
        disp: [B, 1, H, W]
        padding_mode: 'zeros' or 'border'
    Returns:
        warped_img: [B, C, H, W]
        valid_mask: [B, C, H, W] (a broadcast view; 1 everywhere under 'border')
    """
    return ops.monster_disp_warp(img, disp, padding_mode)
