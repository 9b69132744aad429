"""Case table and seeded inputs shared by tests/golden/make_golden_monster.py (build container, runs the reference) and
tests/test_monster.py (runs everywhere: this module imports nothing from the reference tree).

Flaw cases (B, C, H, W), the smallest shapes at which each mechanism of csrc/monster.hip can fail:
  odd       (2, 5, 6, 37)      odd sizes under a wave; disparities in [-3, 12]: both borders clip.
  wave96    (1, 96, 4, 70)     crosses a wave, the model's channel count: the channel-chunk loops.
  wide      (1, 3, 5, 300)     more columns than a workgroup has lanes (REMP's three channels).
  collide   (1, 4, 3, 40)      d = x - 7.3 (and x - 20.6): every pixel of a row samples one place, a list of W entries on two lanes.
  clipped   (1, 4, 3, 40)      d = x + 5 (and x + 9): everything clipped onto column 0, the disparity gradient exactly zero.
  min       (1, 4, 2, 2)       the smallest legal map: both rows clip.
  zeros     (2, 3, 5, 21)      padding 'zeros' with a non-trivial validity map.
  integer   (1, 3, 4, 19)      exact integer disparities: values only (the gradient to the disparity jumps there).
  single    (1, 2, 3, 9)       one disparity (disp_b = None).
  g144x240  (1, 96, 144, 240)  GPU only, the model's 1/4-resolution map.
Of `SUBSAMPLED` cases the fixture keeps d_ref, max|fp64| and `subsample` of each fp64 tensor (whole, they would not fit a
committed file); the test compares with the restatement evaluated in fp64.
Disparities of the random cases are drawn uniformly and then moved so that every sample coordinate ix keeps `KINK_MARGIN_DRAWN`
from the integers (the bilinear derivative and the clip limits 0 and W - 1 jump there); `kink_margin` measures what the fp32
disparities keep, and every gradient case must keep KINK_MARGIN (asserted by `check_flaw_inputs`, run when the fixture is made and
by the test).  The constructed cases (collide, clipped) sit at ix = 6.987 / 20.628 and outside the image.

Fit cases: mono, gt [B, 1, H, W] (and a caller's mask):
  n222 (6 x 37), n34560 (144 x 240), b3 (three different images), ties (mono in steps of 0.25: many values tie with the rank
  threshold and the strict `>` decides), holes (gt <= 0 at a fifth of the pixels, mono below 1e-2 at a tenth), negative (mono in
  [-3, 5]), mask (a caller's mask), empty (gt <= 0 everywhere: exactly (0, 0)).
Except `empty`, every image keeps at least a quarter of its pixels and at least 32 (`check_fit_inputs`); no mono value lies
within 1e-4 of the 1e-2 limit (fp32 and fp64 compare it with different constants).
"""
import torch

from stereo_toolbox_amd.utils import synthetic_tensor

FLAW_CASES = {
    # tag: (shape, padding, (lo, hi) of the drawn disparities or None = constructed, gradients compared)
    "odd": ((2, 5, 6, 37), "border", (-3.0, 12.0), True),
    "wave96": ((1, 96, 4, 70), "border", (-2.0, 20.0), True),
    "wide": ((1, 3, 5, 300), "border", (-4.0, 40.0), True),
    "collide": ((1, 4, 3, 40), "border", None, True),
    "clipped": ((1, 4, 3, 40), "border", None, True),
    "min": ((1, 4, 2, 2), "border", (-1.0, 1.5), True),
    "zeros": ((2, 3, 5, 21), "zeros", (-4.0, 8.0), True),
    "integer": ((1, 3, 4, 19), "border", (-2.0, 6.0), False),
    "single": ((1, 2, 3, 9), "border", (-2.0, 4.0), True),
    "g144x240": ((1, 96, 144, 240), "border", (-3.0, 60.0), True),
}
GPU_ONLY = ("g144x240",)
SUBSAMPLED = ("wave96", "g144x240")
ONE_DISPARITY = ("single",)
CONSTRUCTED = {"collide": (-7.3, -20.6), "clipped": (5.0, 9.0)}          # d = x + offset
# exact in fp32 and fp64 alike, d_ref = 0 (clipped: H = 3 puts every row coordinate on an integer, the sample is a copy of column 0)
ZERO_DREF = {"clipped": ("warped_a", "g_disp_a", "g_disp_b"), "single": ("g_left",)}
VALUE_KEYS = ("warped_a", "flaw_a", "flaw_b")
GRAD_KEYS = ("g_left", "g_right", "g_disp_a", "g_disp_b")
KINK_MARGIN_DRAWN = 0.05
KINK_MARGIN = 1e-3
SUBSAMPLE = 512
FD_CASE = "odd"

FIT_CASES = {
    # tag: (B, H, W)
    "n222": (1, 6, 37),
    "n34560": (1, 144, 240),
    "b3": (3, 9, 31),
    "ties": (1, 12, 40),
    "holes": (2, 10, 33),
    "negative": (1, 11, 29),
    "mask": (2, 8, 30),
    "empty": (1, 5, 20),
}
FIT_SUBSAMPLED = ("n34560",)
FIT_MIN_SHARE, FIT_MIN_COUNT = 0.25, 32
MIN_MONO = 1e-2

# the public surface of models.MonSter: disp_warp's parameters as the reference has them, and the names shared with IGEVStereo
REQUIRED = "<required>"
DISP_WARP_SIGNATURE = (("img", REQUIRED), ("disp", REQUIRED), ("padding_mode", "border"))
OWN_EXPORTS = ("disp_warp", "compute_scale_shift", "align_mono_disp", "mutual_flaws", "refinement_flaws")
SHARED_WITH_IGEV = ("Combined_Geo_Encoding_Volume", "build_gwc_volume", "context_upsample", "upsample_disp_from_logits", "ConvGRU",
                    "FeatureAtt")


def subsample(t):
    """At least SUBSAMPLE elements of t (all of a smaller tensor) at a fixed odd stride over the flattened tensor."""
    flat = t.reshape(-1)
    stride = max(1, flat.numel() // SUBSAMPLE)
    return flat[::stride - 1 + stride % 2]


def _seed(tag, table, base):
    return base + 50 * list(table).index(tag)


def _coordinate(disp, W):
    w = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    return (w - disp.double()) * (W / (W - 1)) - 0.5


def _drawn(B, H, W, seed, lo, hi, integer):
    d = synthetic_tensor((B, 1, H, W), seed, lo=lo, hi=hi).double()
    if integer:
        return torch.round(d).float()
    return _clear_of_kinks(d, W)


def _clear_of_kinks(d, W):
    ix = _coordinate(d, W)
    x0 = torch.floor(ix)
    fr = (ix - x0).clamp(KINK_MARGIN_DRAWN, 1 - KINK_MARGIN_DRAWN)
    w = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    return (w - (x0 + fr + 0.5) * (W - 1) / W).float()


def kink_margin(disp, W, padding):
    """min distance of the sample coordinate (in double, of the fp32 disparity) from an integer (which covers the clip limits)"""
    ix = _coordinate(disp, W)
    return (ix - torch.round(ix)).abs().min().item()


def flaw_inputs(tag):
    """dict: left, right [B, C, H, W]; disp_a, disp_b [B, 1, H, W] (disp_b None for a one-disparity case); loss weights gw_a, gw_b
    [B, C, H, W]; padding -- all fp32"""
    (B, C, H, W), padding, rng, _ = FLAW_CASES[tag]
    seed = _seed(tag, FLAW_CASES, 6000)
    if rng is None:
        x = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, 1, H, W)
        da, db = ((x + off).contiguous() for off in CONSTRUCTED[tag])
    else:
        lo, hi = rng
        da = _drawn(B, H, W, seed + 2, lo, hi, tag == "integer")
        db = _drawn(B, H, W, seed + 3, lo - 1.5, 0.6 * hi, tag == "integer")
        if tag == "min":                                                  # disp_a inside the image at every pixel, disp_b mostly clipped
            x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
            da = _clear_of_kinks(x - synthetic_tensor((B, 1, H, W), seed + 2, lo=0.3, hi=0.7).double(), W)
    return {"left": synthetic_tensor((B, C, H, W), seed), "right": synthetic_tensor((B, C, H, W), seed + 1), "disp_a": da,
            "disp_b": None if tag in ONE_DISPARITY else db, "gw_a": synthetic_tensor((B, C, H, W), seed + 4),
            "gw_b": synthetic_tensor((B, C, H, W), seed + 5), "padding": padding}


def check_flaw_inputs(tag):
    (_, _, _, W), padding, _, grads = FLAW_CASES[tag]
    t = flaw_inputs(tag)
    if grads:
        for k in ("disp_a", "disp_b"):
            if t[k] is not None:
                m = kink_margin(t[k], W, padding)
                assert m >= KINK_MARGIN, (tag, k, m)
    return t


def fit_inputs(tag):
    """-> (mono, gt [B, 1, H, W] fp32, mask (bool [B, 1, H, W]) or None, loss weight for the aligned map)"""
    B, H, W = FIT_CASES[tag]
    seed = _seed(tag, FIT_CASES, 7000)
    shape = (B, 1, H, W)
    lo, hi = (-3.0, 5.0) if tag == "negative" else (0.5, 6.0)
    mono = synthetic_tensor(shape, seed, lo=lo, hi=hi)
    if tag == "ties":
        mono = torch.round(mono * 4) / 4
    per_image = torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1)
    gt = (1.2 + 0.5 * per_image) * mono + 0.4 * per_image + synthetic_tensor(shape, seed + 1, lo=-0.3, hi=0.3)
    if tag == "negative":
        gt = gt.abs() + 0.1
    mask = None
    if tag == "holes":
        u = synthetic_tensor(shape, seed + 2, lo=0.0, hi=1.0)
        gt = torch.where(u < 0.2, -gt * (u < 0.1), gt)                    # zeros and negative values
        v = synthetic_tensor(shape, seed + 3, lo=0.0, hi=1.0)
        mono = torch.where(v < 0.1, 0.001 + 0.08 * v, mono)               # 0.001 .. 0.009
    if tag == "mask":
        mask = synthetic_tensor(shape, seed + 2, lo=0.0, hi=1.0) < 0.5
    if tag == "empty":
        gt = -gt.abs()
    return mono.contiguous(), gt.contiguous(), mask, synthetic_tensor(shape, seed + 4)


def fit_mask(mono, gt, mask):
    """the reference's mask of one image (monster.py:45-51), restated with kthvalue in place of the full sort -> (mask, threshold)"""
    flat = mono.reshape(-1)
    thr = torch.kthvalue(flat, int(0.2 * flat.numel()) + 1).values
    if mask is None:
        mask = (gt > 0) & (mono > MIN_MONO) & (mono > thr)
    return mask, thr


def check_fit_inputs(tag):
    mono, gt, mask, gw = fit_inputs(tag)
    assert ((mono - MIN_MONO).abs() > 1e-4).all(), tag
    for b in range(mono.shape[0]):
        kept = int(fit_mask(mono[b], gt[b], None if mask is None else mask[b])[0].sum())
        if tag == "empty":
            assert kept == 0, (tag, kept)
        else:
            assert kept >= FIT_MIN_COUNT and kept >= FIT_MIN_SHARE * mono[b].numel(), (tag, b, kept)
    return mono, gt, mask, gw
