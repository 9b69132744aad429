from .monster import align_mono_disp, compute_scale_shift, mutual_flaws, refinement_flaws  # noqa: F401
from .warp import disp_warp  # noqa: F401
from ..IGEVStereo.aggregation import FeatureAtt  # noqa: F401
from ..IGEVStereo.geometry import Combined_Geo_Encoding_Volume  # noqa: F401
from ..IGEVStereo.submodule import build_gwc_volume, context_upsample, upsample_disp_from_logits  # noqa: F401
from ..IGEVStereo.update import ConvGRU  # noqa: F401
from ..RAFTStereo.extractor import ResidualBlock  # noqa: F401
from ..IGEVStereo.submodule import BasicConv_IN, Conv2x_IN  # noqa: F401
