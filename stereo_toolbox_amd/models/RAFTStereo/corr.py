"""The correlation blocks of RAFT-Stereo (reference models/RAFTStereo/corr.py:31-156; Selective-RAFT uses the same classes) on
the HIP kernels of csrc/corr1d.hip -- the object `RAFTStereo.forward` builds from the two feature maps (raft_stereo.py:121-139)
and calls once per GRU iteration (:155):

    corr_fn = CorrBlock1D(fmap1.float(), fmap2.float(), radius=args.corr_radius, num_levels=args.corr_levels)
    ...
    corr = corr_fn(coords1)                      # [B, num_levels * (2 radius + 1), H, W]

Same constructor arguments, call arguments, shapes, dtypes and channel order as the reference.  Inside, the pyramid is one
pixel-major buffer written by one launch (the all-pairs correlation runs on the matrix cores and writes its pooled levels in
the same pass), and a lookup is ONE launch for all levels instead of about a dozen ATen operators per level.  The lookup is
differentiated with respect to the two feature maps; its backward adds into per-pixel rows without atomics (bitwise
reproducible) and all lookups of one backward pass accumulate into one gradient buffer (ops._PyramidGrads), which reaches the
public `corr_pyramid` tensor complete, so it may have other consumers.  `coords` carries no gradient -- the reference detaches
it before every call (raft_stereo.py:154) -- and a tensor that requires grad is refused rather than silently given zeros.

All three `corr_implementation`s of the reference are this one object:
* `"reg"`       CorrBlock1D.
* `"reg_cuda"`  CorrBlockFast1D: the `corr_sampler` extension's semantics are the same linear interpolation with zero padding.
* `"alt"`       PytorchAlternateCorrBlock1D: it pools `fmap2` and correlates per call; by linearity that is pooling the
                correlation, and its reason to exist is the memory of the volume (62 MB at 144x240, nothing on this card).
"""
from ... import ops


class CorrBlock1D:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        """fmap1 [B, C, H, W1], fmap2 [B, C, H, W2] (NCHW or channels-last; fp16 / bf16 under autocast).  num_levels 1..4,
        radius 1..8, and the last level must keep two positions: W2 >> (num_levels - 1) >= 2."""
        self.num_levels = num_levels
        self.radius = radius
        self._build(fmap1, fmap2)

    @ops.fp32_region
    def _build(self, fmap1, fmap2):
        who = type(self).__name__
        if fmap1.dim() != 4 or fmap2.dim() != 4:
            raise ops.StxError(f"{who}: feature maps must be [B, C, H, W], got {tuple(fmap1.shape)} / {tuple(fmap2.shape)}")
        b, _, h, w1 = fmap1.shape
        self._grads = ops._PyramidGrads()
        # the flat pixel-major pyramid: level i is corr_pyramid[offset_i:].view(B * H * W1, W2 >> i)
        self.corr_pyramid = ops.corr1d_pyramid(fmap1, fmap2, self.num_levels, who)
        # what the lookups read: an alias of the public tensor that nothing else consumes (ops._PyramidGrads)
        self._lookup_pyramid = ops.corr1d_lookup_pyramid(self.corr_pyramid, self._grads)
        self._cfg = (b, h, w1, fmap2.shape[3], self.num_levels)
        self._jobs = tuple((i, self.radius, 0.0, 2.0 ** -i) for i in range(self.num_levels))

    @ops.fp32_region
    def __call__(self, coords):
        """coords [B, 2 or 1, H, W]: channel 0 is the sampling column -> [B, num_levels * (2 radius + 1), H, W] fp32."""
        if coords.dim() != 4:
            raise ops.StxError(f"{type(self).__name__}: coords must be [B, 2 or 1, H, W], got {tuple(coords.shape)}")
        return ops.corr1d_lookup(self._lookup_pyramid, coords[:, 0], None, self._jobs, self._cfg, self._grads, type(self).__name__)

    @staticmethod
    def corr(fmap1, fmap2):
        """[B, C, H, W1] x [B, C, H, W2] -> [B, H, W1, 1, W2], sum over C divided by sqrt(C)."""
        b, _, h, w1 = fmap1.shape
        return ops.corr1d_pyramid(fmap1, fmap2, 1).view(b, h, w1, 1, fmap2.shape[3])


class CorrBlockFast1D(CorrBlock1D):
    """`corr_implementation="reg_cuda"` (corr.py:31-61): the same kernels; no `corr_sampler` extension is needed."""


class PytorchAlternateCorrBlock1D(CorrBlock1D):
    """`corr_implementation="alt"` (corr.py:64-107): the same object again.  As in the model, `coords` must carry the row index in
    channel 1 -- [B, 2, H, W] with coords[:, 1] = the pixel's own row -- because the reference samples `fmap2` at (x, y) and this
    class reads the row the pixel lies in; only channel 0 is looked at."""

    @ops.fp32_region
    def __call__(self, coords):
        if coords.dim() != 4 or coords.shape[1] != 2:
            raise ops.StxError(f"PytorchAlternateCorrBlock1D: coords must be [B, 2, H, W] (column, row), got {tuple(coords.shape)}")
        return super().__call__(coords)
