"""`DEFOMStereo.upsample_flow` (reference models/DEFOMStereo/defom_stereo.py:83) on the fused kernel of csrc/convex_upsample.hip."""
from ... import ops


def upsample_flow(flow, mask, n_downsample=2):
    """flow [N,D,H,W], mask [N,9*4^n,H,W] (the mask head's logits) -> [N,D,2^n H,2^n W]: soft-max over the nine taps and the convex
    combination of the 3x3 neighbourhood of 2^n * flow.  The reference reads `n_downsample` from `self.args`; here it is an argument."""
    return ops.convex_upsample(flow, mask, n_downsample=n_downsample, use_scale_factor=True)
