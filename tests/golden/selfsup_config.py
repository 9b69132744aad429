"""Case table and seeded inputs shared by tests/golden/make_golden_selfsup.py (build container, runs the reference) and
tests/test_selfsup_loss.py (runs everywhere: this module imports nothing from the reference tree).

Shapes (B, C, H, W), the smallest at which each mechanism of csrc/selfsup_loss.hip can fail:
  s4        (1, 3, 4, 4)     smallest legal for window 7: every pixel is a reflection source on both sides.
  b2_9x13   (2, 3, 9, 13)    odd H -- the row h = (H - 1) / 2 samples at an exact integer y; batch stride.  SSIM also with windows 3, 11.
  r37x70    (1, 3, 37, 70)   crosses a tile (16 x 64) and a 64-lane boundary in both directions, ragged remainders.
  c1_5x130  (1, 1, 5, 130)   single channel, wide: more than two column strips.
  g96x320   (1, 3, 96, 320)  GPU only; the fixture keeps d_ref, max|fp64| and `subsample` of each fp64 tensor, the test compares with
                             the restatement evaluated in fp64.
Inputs.  Images: uniform noise smoothed by a 5 x 5 replicate-padded mean (left and right independent, so the reprojection and the
identity error of auto_mask win about equally often).  Disparities are built FROM the sampling coordinate: xi an integer in
[-3, W + 2), fr in [0.05, 0.95], disp = w - (xi + fr + 1/2) (W - 1) / W -- every pixel's x stays 0.05 px clear of the integers where
the bilinear derivative jumps, and both borders see all three regimes (outside, the partly valid border column, inside).
smoothness_loss takes |disp| + 1 (the per-image mean away from zero).  Loss weights are drawn in fp32 and cast.
"""
import torch

from stereo_toolbox_amd.utils import synthetic_tensor

CASES = {
    "s4": (1, 3, 4, 4),
    "b2_9x13": (2, 3, 9, 13),
    "r37x70": (1, 3, 37, 70),
    "c1_5x130": (1, 1, 5, 130),
    "g96x320": (1, 3, 96, 320),
}
GPU_ONLY = ("g96x320",)
WHOLE = tuple(t for t in CASES if t not in GPU_ONLY)          # tensors stored whole
SSIM_WINDOW_CASES = {"b2_9x13": (3, 11)}                      # on top of the default 7 of every case
AUTO_MASK_CASES = ("b2_9x13", "r37x70", "c1_5x130")           # (s4 has no true pixel)
AUTO_MASK_DENORM = ("b2_9x13",)
AUTO_MASK_MARGIN = 1e-5                                       # |reproj - identity| in fp64 below which a pixel may be skipped
AUTO_MASK_MAX_SKIPPED = 0.01
AUTO_MASK_MIN_SHARE = 0.05
FD_SHAPE = (1, 3, 9, 13)
SSIM_WEIGHT = 0.85
SUBSAMPLE = 512

# the public surface: module -> function -> ((parameter, default), ...); `REQUIRED` marks a parameter without a default
REQUIRED = "<required>"
SURFACE = {
    "photometric_loss": {
        "warp_right_to_left": (("right_image", REQUIRED), ("disp", REQUIRED)),
        "ssim": (("x", REQUIRED), ("y", REQUIRED), ("window_size", 7), ("pad_mode", "reflect")),
        "photometric_loss": (("left_image", REQUIRED), ("right_image", REQUIRED), ("disp", None), ("ssim_weight", 0.85),
                             ("enable_mask", True)),
    },
    "auto_mask": {"auto_mask": (("left_image", REQUIRED), ("right_image", REQUIRED), ("disp", REQUIRED), ("denorm", False))},
    "smoothness_loss": {"smoothness_loss": (("disp", REQUIRED), ("img", REQUIRED), ("warn", True))},   # `warn` is this project's
}
PACKAGE_EXPORTS = ("split_mode", "photometric_loss", "auto_mask", "smoothness_loss")


def subsample(t):
    """At least SUBSAMPLE elements of t (all of a smaller tensor) at a fixed odd stride over the flattened tensor."""
    flat = t.reshape(-1)
    stride = max(1, flat.numel() // SUBSAMPLE)
    return flat[::stride - 1 + stride % 2]


def _seed(tag):
    return 4000 + 50 * list(CASES).index(tag)


def smooth_image(shape, seed):
    """uniform [0, 1) noise under a 5 x 5 replicate-padded mean"""
    raw = synthetic_tensor(shape, seed, lo=0.0, hi=1.0)
    padded = torch.nn.functional.pad(raw, (2, 2, 2, 2), mode="replicate")
    return torch.nn.functional.avg_pool2d(padded, 5, stride=1).contiguous()


def disparity(B, H, W, seed):
    """[B, 1, H, W] from the sampling coordinate (see the module docstring); formed in fp64, stored in fp32"""
    u = synthetic_tensor((B, 1, H, W), seed, lo=0.0, hi=1.0).double()
    xi = torch.floor(u * (W + 5)).clamp(max=W + 4) - 3
    fr = synthetic_tensor((B, 1, H, W), seed, stream=1, lo=0.05, hi=0.95).double()
    w = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    return (w - (xi + fr + 0.5) * (W - 1) / W).float()


def images(shape, seed):
    return smooth_image(shape, seed), smooth_image(shape, seed + 1)


def inputs(tag):
    """dict: left, right [B, C, H, W]; disp, sdisp (= |disp| + 1, for smoothness_loss) [B, 1, H, W]; loss weights gw_c [B, C, H, W]
    (warp, ssim) and gw_1 [B, 1, H, W] (photometric), all fp32"""
    B, C, H, W = CASES[tag]
    seed = _seed(tag)
    left, right = images((B, C, H, W), seed)
    disp = disparity(B, H, W, seed + 2)
    return {"left": left, "right": right, "disp": disp, "sdisp": disp.abs() + 1,
            "gw_c": synthetic_tensor((B, C, H, W), seed + 4), "gw_1": synthetic_tensor((B, 1, H, W), seed + 5)}


def normalised(img):
    """(img - mean) / std of ImageNet, fp32: what auto_mask(denorm=True) undoes (3 channels)"""
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).view(1, 3, 1, 1)
    return ((img - mean) / std).contiguous()


def fd_inputs():
    B, C, H, W = FD_SHAPE
    left, right = images(FD_SHAPE, 4900)
    disp = disparity(B, H, W, 4902)
    return left, right, disp
