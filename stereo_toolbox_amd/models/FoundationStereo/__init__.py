from .submodule import (Conv3dNormActReduced, CostVolumeDisparityAttention, FlashAttentionTransformerEncoderLayer,  # noqa: F401
                        FlashMultiheadAttention, PositionalEmbedding, build_concat_volume, build_gwc_volume, disparity_regression,
                        groupwise_correlation, init_comb_volume)
from ..IGEVStereo.update import ConvGRU  # noqa: F401
from ..IGEVStereo.submodule import BasicConv_IN  # noqa: F401
