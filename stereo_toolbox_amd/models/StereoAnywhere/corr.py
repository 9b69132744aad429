"""The correlation block of StereoAnywhere (reference models/StereoAnywhere/corr.py:75-132) on the HIP kernels of csrc/allpairs.hip
and csrc/corr1d.hip.  Unlike the RAFT block it is built from a VOLUME, not from feature maps -- the model builds two per forward,
from an aggregated volume and from a raw volume times a truncation mask (stereoanywhere.py:285-291):

    corr_fn = CorrBlock1D(fullcorr, radius=args.corr_radius, num_levels=args.corr_levels, pad=args.vol_pad)
    ...
    corr = corr_fn(coords1)                      # [B, num_levels * (2 radius + 1), H, W - pad[0] - pad[1]]

Same constructor arguments, call arguments, output shape, dtype and channel order as the reference: `coords + pad[0]` is the
lookup base and the crop along W happens after the lookup.  Inside, the pyramid is one pixel-major buffer written by one launch
and a lookup is one launch for all levels (ops.corr1d_lookup, the RAFT family's kernel).  The block is differentiated with respect
to `fullcorr` (it comes out of a trainable Conv3d); the lookups of one backward pass accumulate into one gradient buffer
(ops._PyramidGrads), which reaches the public `corr_pyramid` tensor complete, so it may have other consumers.  `coords` carries no
gradient; a tensor that requires grad is refused rather than silently given zeros.

Differences from the reference, all in what is kept, none in what a call returns:
* `corr_pyramid` is ONE flat tensor of `num_levels` levels: level i is corr_pyramid[offset_i:][:B*H*W1 * (W2 >> i)].view(B*H*W1,
  W2 >> i), offset_i = B*H*W1 * sum_{j<i} (W2 >> j).  The reference keeps a list of [B*H*W1, 1, 1, W2 >> i] tensors with one
  extra pooled level (num_levels + 1 entries) that no lookup reads; it is not built here.
* Extension: `truncate=(disp_left, conf_left, attenuation_gain)` multiplies the volume by the truncation mask inside the pyramid
  launch, equal to passing `truncate_corr_volume_v2(disp_left, conf_left, conf_th=None, attenuation_gain) * fullcorr` without
  the two volume-sized temporaries; the two maps carry no gradient, as the model detaches the mask (stereoanywhere.py:235).
"""
import torch

from ... import ops


class CorrBlock1D:
    def __init__(self, fullcorr, num_levels=4, radius=4, pad=[0, 0], truncate=None):
        """fullcorr [B, H, W1, 1, W2] fp32 (fp16 / bf16 under autocast).  num_levels 1..4, radius 1..8, and the last level must
        keep two positions: W2 >> (num_levels - 1) >= 2."""
        self.num_levels = num_levels
        self.radius = radius
        self.pad = pad
        self.fullcorr = fullcorr
        self._build(fullcorr, truncate)

    @ops.fp32_region
    def _build(self, fullcorr, truncate):
        who = type(self).__name__
        if fullcorr.dim() != 5 or fullcorr.shape[3] != 1:
            raise ops.StxError(f"{who}: fullcorr must be [B, H, W1, 1, W2], got {tuple(fullcorr.shape)}")
        b, h, w1, _, w2 = fullcorr.shape
        self._grads = ops._PyramidGrads()
        self.corr_pyramid = ops.corr1d_volume_pyramid(fullcorr, self.num_levels, truncate, who)
        # what the lookups read: an alias of the public tensor that nothing else consumes (ops._PyramidGrads)
        self._lookup_pyramid = ops.corr1d_lookup_pyramid(self.corr_pyramid, self._grads)
        self._cfg = (b, h, w1, w2, self.num_levels)
        self._jobs = tuple((i, self.radius, 0.0, 2.0 ** -i) for i in range(self.num_levels))

    @ops.fp32_region
    def __call__(self, coords):
        """coords [B, 2 or 1, H, W1]: channel 0 is the sampling column before the shift by pad[0]
        -> [B, num_levels * (2 radius + 1), H, W1 - pad[0] - pad[1]] fp32."""
        who = type(self).__name__
        if coords.dim() != 4:
            raise ops.StxError(f"{who}: coords must be [B, 2 or 1, H, W], got {tuple(coords.shape)}")
        if torch.is_grad_enabled() and coords.requires_grad:
            raise ops.StxError(f"{who}: coords must not require grad -- the lookup is differentiated with respect to the volume "
                               "only; pass coords.detach()")
        w1 = self._cfg[2]
        base = coords[:, 0] + self.pad[0]                               # real coords are shifted by pad[0] (corr.py:96)
        out = ops.corr1d_lookup(self._lookup_pyramid, base, None, self._jobs, self._cfg, self._grads, who)
        if self.pad[0] or self.pad[1]:
            out = out[:, :, :, self.pad[0]:w1 - self.pad[1]].contiguous()
        return out

    @staticmethod
    def corr(fmap2, fmap3):
        """[B, C, H, W2] x [B, C, H, W3] -> [B, H, W2, 1, W3], sum over C divided by sqrt(C); any C (the model's 3-channel
        normals included)."""
        b, _, h, w2 = fmap2.shape
        return ops.corr1d_pyramid(fmap2, fmap3, 1).view(b, h, w2, 1, fmap3.shape[3])


class CorrBlockFast1D(CorrBlock1D):
    """The reference's `CorrBlockFast1D` (corr.py:31-69) needs the `corr_sampler` extension and its `__call__` is not runnable
    as written (`out_pyramid.append()` without an argument, corr.py:56); what it means to compute is the same linear
    interpolation with zero padding, so it is this same object."""
