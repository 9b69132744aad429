from .corr import CorrBlock1D  # noqa: F401
from .upsample import upsample_flow  # noqa: F401
from ..IGEVStereo.update import ConvGRU  # noqa: F401
from ..RAFTStereo.extractor import ResidualBlock  # noqa: F401
