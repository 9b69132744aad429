"""Selective-IGEV (reference models/SelectiveStereo/SelectiveIGEV): its own recurrent unit and attention, and -- as the same
objects -- what it shares with IGEVStereo: the ConvGRU cell, the geometry encoding volume, the initial gwc volume and the
upsampling from super-pixel logits."""
from ..update import (ChannelAttentionEnhancement, RaftConvGRU, SelectiveConvGRU, SpatialAttentionExtractor,  # noqa: F401
                      contextual_spatial_attention)
from ...IGEVStereo import (Combined_Geo_Encoding_Volume, ConvGRU, build_gwc_volume, context_upsample,  # noqa: F401
                           disparity_regression, groupwise_correlation, upsample_disp_from_logits)
from ...IGEVStereo.submodule import BasicConv_IN, Conv2x_IN  # noqa: F401
from ...RAFTStereo.extractor import ResidualBlock  # noqa: F401
