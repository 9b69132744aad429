from .corr import CorrBlock1D, CorrBlockFast1D, PytorchAlternateCorrBlock1D  # noqa: F401
from .upsample import upsample_flow  # noqa: F401
from ..IGEVStereo.update import ConvGRU  # noqa: F401
from .extractor import ResidualBlock  # noqa: F401
