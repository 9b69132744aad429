"""SelectiveStereo (reference models/SelectiveStereo): the selective recurrent unit and the contextual spatial attention on the
gfx950 kernels, with the sub-package layout of the reference.  Both sub-packages export the same class objects."""
from . import SelectiveIGEV, SelectiveRAFT  # noqa: F401
from .update import (ChannelAttentionEnhancement, RaftConvGRU, SelectiveConvGRU, SpatialAttentionExtractor,  # noqa: F401
                     contextual_spatial_attention)
