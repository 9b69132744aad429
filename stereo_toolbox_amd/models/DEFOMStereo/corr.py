"""The disparity-indexed correlation block of DEFOM-Stereo (reference models/DEFOMStereo/corr.py:113-181) on the HIP kernels of
csrc/corr1d.hip: built once from the two feature maps and the pixels' columns (defom_stereo.py:118-127) and called once per GRU
iteration with the detached disparity (:142-150) -- `scaling=True` in the scale-update iterations, which sample level 0 at
`coords - s * disp` for every `s` of `scale_list`.

Same constructor arguments, call arguments, shapes, dtypes and channel order as the reference; the pyramid, the one-launch
lookup and the gradient flow are those of `models.RAFTStereo.CorrBlock1D`.  `coords` and `disp` carry no gradient: a tensor
that requires grad is refused rather than silently given zeros.
"""
import torch

from ... import ops


class CorrBlock1D:
    def __init__(self, fmap1, fmap2, coords, num_levels=4, radius=4, scale_list=(0.25, 0.5, 2.0, 4.0), scale_corr_radius=4):
        """fmap1 [B, C, H, W1], fmap2 [B, C, H, W2]; coords: B * H * W1 values, the column each pixel's disparity is taken
        from.  num_levels 1..4, radius and scale_corr_radius 1..8, at most 8 scales, W2 >> (num_levels - 1) >= 2."""
        self.num_levels = num_levels
        self.radius = radius
        self.scale_list = list(scale_list)
        self.scale_corr_radius = scale_corr_radius
        self._build(fmap1, fmap2, coords)

    @ops.fp32_region
    def _build(self, fmap1, fmap2, coords):
        if fmap1.dim() != 4 or fmap2.dim() != 4:
            raise ops.StxError(f"CorrBlock1D: feature maps must be [B, C, H, W], got {tuple(fmap1.shape)} / {tuple(fmap2.shape)}")
        b, _, h, w1 = fmap1.shape
        self.batch, self.h1, self.w1, self.w2 = b, h, w1, fmap2.shape[3]
        if torch.is_grad_enabled() and coords.requires_grad:
            raise ops.StxError("CorrBlock1D: `coords` must not require grad (defom_stereo.py builds it from coords_grid); pass "
                               "coords.detach()")
        self.coords = coords.detach().reshape(-1)
        self._grads = ops._PyramidGrads()
        self.corr_pyramid = ops.corr1d_pyramid(fmap1, fmap2, self.num_levels, "CorrBlock1D")
        self._lookup_pyramid = ops.corr1d_lookup_pyramid(self.corr_pyramid, self._grads)
        self._cfg = (b, h, w1, self.w2, self.num_levels)
        self._jobs = tuple((i, self.radius, 1.0, 2.0 ** -i) for i in range(self.num_levels))
        self._scale_jobs = tuple((0, self.scale_corr_radius, s, 1.0) for s in self.scale_list)

    @ops.fp32_region
    def __call__(self, disp, scaling=False):
        """disp [B, 1, H, W] -> [B, num_levels * (2 radius + 1), H, W], or with scaling
        [B, len(scale_list) * (2 scale_corr_radius + 1), H, W]; fp32."""
        jobs = self._scale_jobs if scaling else self._jobs
        return ops.corr1d_lookup(self._lookup_pyramid, self.coords, disp, jobs, self._cfg, self._grads, "CorrBlock1D")

    @staticmethod
    def corr(fmap1, fmap2):
        """[B, C, H, W1] x [B, C, H, W2] -> [B, H, W1, 1, W2], sum over C divided by sqrt(C)."""
        b, _, h, w1 = fmap1.shape
        return ops.corr1d_pyramid(fmap1, fmap2, 1).view(b, h, w1, 1, fmap2.shape[3])

