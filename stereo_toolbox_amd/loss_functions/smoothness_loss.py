"""reference loss_functions/smoothness_loss.py on csrc/selfsup_loss.hip (stereo_toolbox_amd.ops)."""
from .. import ops

__all__ = ["smoothness_loss"]


def smoothness_loss(disp, img, warn=True):
    """Edge-aware smoothness of the mean-normalised disparity, a 0-d tensor; reference :5-44.  warn=True keeps the reference's
    `img.max() > 1.0` warning (a device-to-host sync, the max itself costs no extra pass); warn=False never syncs."""
    return ops.smoothness_loss(disp, img, warn)
