"""reference loss_functions/auto_mask.py on csrc/selfsup_loss.hip (stereo_toolbox_amd.ops)."""
from .. import ops

__all__ = ["auto_mask"]


def auto_mask(left_image, right_image, disp, denorm=False):
    """bool [B, 1, H, W]: the reprojection error is below the identity error; reference :7-17, one kernel launch, no gradient."""
    return ops.auto_mask(left_image, right_image, disp, denorm)
