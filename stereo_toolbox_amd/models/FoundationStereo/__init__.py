from .submodule import (Conv3dNormActReduced, build_concat_volume, build_gwc_volume, disparity_regression,  # noqa: F401
                        groupwise_correlation, init_comb_volume)
from ..IGEVStereo.update import ConvGRU  # noqa: F401
