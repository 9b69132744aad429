from .regression_head import RegressionHead  # noqa: F401
from .utilities import NestedTensor, batched_index_select, torch_1d_sample  # noqa: F401
