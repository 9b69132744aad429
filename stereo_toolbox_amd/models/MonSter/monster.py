"""The mono / stereo mutual refinement of reference models/MonSter/monster.py:456-494 on csrc/monster.hip.

`compute_scale_shift` keeps the reference's contract (two Python floats, so it synchronises); the forward loop should call
`align_mono_disp` and `mutual_flaws` instead, which stay on the device.  The update blocks, the motion encoders, REMP's
convolutions, Feat_transfer*, DepthAnything and a whole `Monster` module are not built here.
"""
from ... import ops


def compute_scale_shift(monocular_depth, gt_depth, mask=None):
    """reference monster.py:31-66: (scale, shift) as Python floats of the least-squares fit gt ~ scale mono + shift over `mask`
    (default: gt > 0, mono > 1e-2, mono above its value of rank int(0.2 n)).  One image, any shape: (H, W), (N, H, W), ..."""
    mono, gt = monocular_depth.reshape(1, -1), gt_depth.reshape(1, -1)
    ss = ops.monster_scale_shift(mono, gt, None if mask is None else mask.reshape(1, -1))
    scale, shift = ss[0].tolist()
    return scale, shift


def align_mono_disp(disp_mono_4x, disp):
    """monster.py:463-467 without the loop over the batch and its two `.item()` per sample: disp_mono_4x [B, 1, H, W] fitted to
    disp [B, 1, H, W] per image and returned as scale_b * disp_mono_4x[b] + shift_b (a new tensor; the gradient goes to
    disp_mono_4x with the fit held constant, as in the reference)."""
    return ops.monster_align(disp_mono_4x, disp)


def mutual_flaws(features_left0, features_right0, disp, disp_mono_4x):
    """monster.py:469-473 -> (flaw_stereo, flaw_mono): disp_warp(features_right0, d)[0] - features_left0 for d = disp and
    d = disp_mono_4x from one launch; features_left0 is read once."""
    return ops.monster_flaws(features_left0, features_right0, disp, disp_mono_4x)


def refinement_flaws(left_img, right_img, disp_mono, disp_stereo):
    """REMP's front (refinement.py:403-407) -> (flaw_mono, flaw_stereo) at full resolution."""
    return ops.monster_flaws(left_img, right_img, disp_mono, disp_stereo)
