from .aggregation import BasicConv, FeatureAtt, IGEVCostAggregation, hourglass  # noqa: F401
from .geometry import Combined_Geo_Encoding_Volume  # noqa: F401
from .submodule import (BasicConv_IN, Conv2x_IN, build_gwc_volume, context_upsample, disparity_regression, groupwise_correlation,  # noqa: F401
                        init_disparity, init_gwc_volume, upsample_disp_from_logits)
from .update import ConvGRU  # noqa: F401
from ..RAFTStereo.extractor import ResidualBlock  # noqa: F401  (the reference's IGEVStereo/extractor.py holds the same class)
