from .attention import MultiheadAttentionRelative  # noqa: F401
from .pos_encoder import PositionEncodingSine1DRelative, build_position_encoding, no_pos_encoding  # noqa: F401
from .regression_head import RegressionHead  # noqa: F401
from .transformer import Transformer, TransformerCrossAttnLayer, TransformerSelfAttnLayer, build_transformer  # noqa: F401
from .utilities import NestedTensor, batched_index_select, torch_1d_sample  # noqa: F401
