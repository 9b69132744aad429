"""`Combined_Geo_Encoding_Volume` of the IGEV family (reference models/IGEVStereo/geometry.py:7-70; used unchanged by MonSter,
Selective-IGEV and FoundationStereo) on the HIP kernels of csrc/geo_lookup.hip -- the object `IGEVStereo.forward` builds from
`geo_encoding_volume` and the two matching feature maps (igev_stereo.py:229-230) and calls once per GRU iteration (:239):

    geo_fn = Combined_Geo_Encoding_Volume(match_left.float(), match_right.float(), geo_encoding_volume.float(),
                                          radius=args.corr_radius, num_levels=args.corr_levels)
    ...
    geo_feat = geo_fn(disp, coords)              # [B, num_levels * (C + 1) * (2 radius + 1), H/4, W/4]

Same constructor arguments, call arguments, shapes, dtypes and channel order as the reference.  What differs is inside: both
pyramids are stored pixel-major in one buffer each (one pixel's whole search window is one contiguous run), built by two
launches (the all-pairs correlation runs on the matrix cores and writes its pooled levels in the same pass), and one lookup is
ONE launch instead of about twenty ATen operators with volume-sized temporaries.  The lookup is differentiated with respect to
`geo_volume`, `init_fmap1` and `init_fmap2`; its backward adds into per-pixel rows without atomics (bitwise reproducible), and
all lookups of one backward pass accumulate into one gradient buffer per pyramid (ops._PyramidGrads), which reaches the
public `geo_volume_pyramid` / `init_corr_pyramid` tensors complete, so they may have other consumers.  `disp` and `coords`
carry no gradient -- the reference detaches `disp` before every call (igev_stereo.py:238) -- and a tensor that requires
grad is refused rather than silently given a zero gradient.
"""
from ... import ops


class Combined_Geo_Encoding_Volume:
    def __init__(self, init_fmap1, init_fmap2, geo_volume, num_levels=2, radius=4):
        """init_fmap1 [B, Cf, H, W1], init_fmap2 [B, Cf, H, W2]; geo_volume [B, C, D, H, W1] (NCDHW-contiguous, or the
        channels-last view `IGEVCostAggregation` returns, which is taken as it is, without a copy)."""
        if geo_volume.dim() != 5:
            raise ops.StxError(f"Combined_Geo_Encoding_Volume: geo_volume must be [B, C, D, H, W], got {tuple(geo_volume.shape)}")
        if not 1 <= num_levels <= 3 or not 1 <= radius <= 8:
            raise ops.StxError(f"Combined_Geo_Encoding_Volume: num_levels {num_levels} (1..3) / radius {radius} (1..8) not supported")
        self.num_levels = num_levels
        self.radius = radius
        self._build(init_fmap1, init_fmap2, geo_volume)

    @ops.fp32_region
    def _build(self, init_fmap1, init_fmap2, geo_volume):
        b, c, d, h, w = geo_volume.shape
        vol = geo_volume.permute(0, 2, 3, 4, 1)                        # dense already for the aggregation's own output
        if not vol.is_contiguous():
            vol = vol.contiguous()
        self._grads = ops._PyramidGrads()
        self.geo_volume_pyramid, self.init_corr_pyramid = ops.geo_pyramids(vol, init_fmap1, init_fmap2, self.num_levels)
        # what the lookups read: aliases of the two public tensors that nothing else consumes (ops._PyramidGrads)
        self._lookup_pyramids = ops.geo_lookup_pyramids(self.geo_volume_pyramid, self.init_corr_pyramid, self._grads)
        self._cfg = (b, h, w, d, c, init_fmap2.shape[3], self.num_levels, self.radius)

    @ops.fp32_region
    def __call__(self, disp, coords):
        return ops.geo_lookup(*self._lookup_pyramids, disp, coords, self._cfg, self._grads)

    @staticmethod
    def corr(fmap1, fmap2):
        """[B, C, H, W1] x [B, C, H, W2] -> [B, H, W1, 1, W2], sum over C (no normalisation)."""
        return ops.geo_corr(fmap1, fmap2)
