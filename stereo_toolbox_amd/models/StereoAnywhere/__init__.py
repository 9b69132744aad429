from .corr import CorrBlock1D, CorrBlockFast1D  # noqa: F401
from .utils import (convex_upflow, estimate_all, estimate_left_confidence, estimate_left_disparity, estimate_right_confidence,  # noqa: F401
                    estimate_right_disparity, truncate_corr_volume_v2)
