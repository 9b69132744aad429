from .corr import CorrBlock1D, CorrBlockFast1D  # noqa: F401
from .utils import (MonoAlignment, align_mono, apply_scale_shift, convex_upflow, estimate_all, estimate_left_confidence,  # noqa: F401
                    estimate_left_disparity, estimate_right_confidence, estimate_right_disparity, fuzzy_and, fuzzy_not, fuzzy_or,
                    generate_masks, handcrafted_mirror_detector, masked_volume, softlrc, truncate_corr_volume_v2, weighted_lsq)
from ..IGEVStereo.update import ConvGRU  # noqa: F401
from ..RAFTStereo.extractor import ResidualBlock  # noqa: F401
