"""Drop-in for reference stereo_toolbox/loss_functions on HIP kernels: `split_mode` (loss_functions/split_mode.py:9-35, the twin
of the modal disparity estimators, csrc/estimators.hip) and the self-supervised objective -- `photometric_loss`, `auto_mask`,
`smoothness_loss` (csrc/selfsup_loss.hip).  The reference's import lines work with the package name changed:
`from stereo_toolbox_amd.loss_functions.photometric_loss import photometric_loss, warp_right_to_left, ssim`, and likewise
`.auto_mask` and `.smoothness_loss`.  Signatures and defaults are the reference's; `smoothness_loss` has one more keyword, `warn`.
The images are data: one that requires grad raises `StxError`; SSIM pads by reflection only."""
from ..ops import split_mode
from .auto_mask import auto_mask
from .photometric_loss import photometric_loss
from .smoothness_loss import smoothness_loss

__all__ = ["split_mode", "photometric_loss", "auto_mask", "smoothness_loss"]
