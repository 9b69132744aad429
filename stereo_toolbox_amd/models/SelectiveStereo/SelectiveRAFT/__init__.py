"""Selective-RAFT (reference models/SelectiveStereo/SelectiveRAFT): its own recurrent unit and attention, and -- as the same
objects -- what it shares with RAFTStereo: the 1-D correlation blocks and the convex upsampling from the mask head's logits."""
from ..update import (ChannelAttentionEnhancement, RaftConvGRU, SelectiveConvGRU, SpatialAttentionExtractor,  # noqa: F401
                      contextual_spatial_attention)
from ...IGEVStereo import ConvGRU, context_upsample  # noqa: F401
from ...RAFTStereo import CorrBlock1D, CorrBlockFast1D, PytorchAlternateCorrBlock1D, upsample_flow  # noqa: F401
from ...IGEVStereo.submodule import BasicConv_IN, Conv2x_IN  # noqa: F401
from ...RAFTStereo.extractor import ResidualBlock  # noqa: F401
