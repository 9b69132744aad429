"""Case table and seeded inputs shared by tests/golden/make_golden_convex_upsample.py (runs the reference) and
tests/test_convex_upsample.py (runs everywhere: this module imports nothing from the reference tree).

RAFT-layout case: N, D, H, W, n_downsample, use_scale_factor, mask kind.  A workgroup of csrc/convex_upsample.hip holds 64 cells
p = y W + x, so H W = 66, 70 and 335 are no multiple of it and cross one or five workgroup borders; the flow channels are walked in
register chunks of two, so D = 3 reaches the second chunk and the plain-load path of the mask gradient.
  mask kinds   noise  seeded noise, unit variance, times 2
               large  noise times 3 plus an offset of +90 or -90 that is constant over the nine taps of a cell: the soft-max is the
                      one of the noise alone, but a naive exp(logit) overflows (exp(88.8) > FLT_MAX)
               const  constant over the nine taps (the output is the mean of the 3 x 3 neighbourhood; g_mask is not zero)
Pixel-layout case: B, h, w (logits [B, 9, 4h, 4w]); the reference call is context_upsample(disp * 4., softmax(logits, 1)).
"""
import math

import torch

from stereo_toolbox_amd.utils import synthetic_tensor

#                      N  D  H  W   n  scale  mask
CASES = {
    "b2_d2_5x7_n2": (2, 2, 5, 7, 2, True, "noise"),           # batch stride, D = 2, f = 4
    "d1_2x33_n3": (1, 1, 2, 33, 3, True, "noise"),            # f = 8, H W = 66
    "d2_4x5_n1": (1, 2, 4, 5, 1, True, "noise"),              # f = 2
    "d1_5x67_n1_noscale": (1, 1, 5, 67, 1, False, "noise"),   # H W = 335: six workgroups; use_scale_factor=False
    "h1_n2": (1, 2, 1, 9, 2, True, "noise"),                  # H = 1: the rows above and below are outside
    "w1_n1": (2, 1, 6, 1, 1, True, "noise"),                  # W = 1
    "large_2x35_n2": (1, 1, 2, 35, 2, True, "large"),         # logits around +-90, H W = 70
    "const_3x5_n2": (1, 2, 3, 5, 2, True, "const"),
    "d3_5x14_n1": (1, 3, 5, 14, 1, True, "noise"),            # D = 3: second register chunk; H W = 70
}
PIXEL_CASES = {"1x1": (1, 1, 1), "b2_3x17": (2, 3, 17), "5x67": (1, 5, 67)}
PIXEL_SCALE = 4.0

# sequence loss: the trainer's step on 22 predictions plus the initial disparity (train_iters = 22), 2 x 7 x 67 pixels
LOSS_SHAPE = (2, 7, 67)
LOSS_MAXDISP = 64
LOSS_PREDICTIONS = 22
LOSS_GAMMA = 0.9
LOSS_KS = (1, 2, 23, 33)


def inputs(tag):
    """(flow [N,D,H,W], mask logits [N,9 f f,H,W], loss weights [N,D,fH,fW])"""
    N, D, H, W, n, _, kind = CASES[tag]
    f = 2 ** n
    seed = 3000 + 10 * list(CASES).index(tag)
    flow = synthetic_tensor((N, D, H, W), seed, lo=-20.0, hi=20.0)
    noise = synthetic_tensor((N, 9, f, f, H, W), seed + 1)
    if kind == "noise":
        mask = 2.0 * noise
    elif kind == "large":
        sign = synthetic_tensor((N, 1, f, f, H, W), seed + 3)
        mask = 3.0 * noise + torch.where(sign > 0, 90.0, -90.0)
    else:
        mask = synthetic_tensor((N, 1, f, f, H, W), seed + 3).expand(N, 9, f, f, H, W)
    gw = synthetic_tensor((N, D, f * H, f * W), seed + 2)
    return flow, mask.reshape(N, 9 * f * f, H, W).contiguous(), gw


def pixel_inputs(tag):
    """(disp_low [B,1,h,w], logits [B,9,4h,4w], loss weights [B,4h,4w])"""
    B, h, w = PIXEL_CASES[tag]
    seed = 3200 + 10 * list(PIXEL_CASES).index(tag)
    disp = synthetic_tensor((B, 1, h, w), seed, lo=0.0, hi=40.0)
    logits = 2.0 * synthetic_tensor((B, 9, 4 * h, 4 * w), seed + 1)
    gw = synthetic_tensor((B, 4 * h, 4 * w), seed + 2)
    return disp, logits, gw


def loss_inputs(K=LOSS_PREDICTIONS + 1):
    """(gt [B,H,W], [K predictions [B,1,H,W]]): the first prediction plays the initial disparity.  gt is seeded noise over
    [-6, maxdisp + 6] rounded to quarters (so residuals of exactly +-1 exist in fp32 and fp64 alike) with planted pixels: zeros, values
    at and above maxdisp - 1, a NaN and an inf.  Residuals are noise over [-3, 3]; four valid pixels get exactly +1, -1, +0.5, -2."""
    B, H, W = LOSS_SHAPE
    gt = (synthetic_tensor((B, H, W), 3400, lo=-6.0, hi=LOSS_MAXDISP + 6.0) * 4).round() / 4
    gt = gt.clone()
    gt[0, 0, :8] = torch.tensor([0.0, 0.0, LOSS_MAXDISP - 1.0, LOSS_MAXDISP + 0.0, float("nan"), float("inf"), -float("inf"), 2.0 * LOSS_MAXDISP])
    gt[0, 1, :4] = torch.tensor([10.0, 20.25, 30.5, 40.0])
    gt[1, 6, 66] = LOSS_MAXDISP - 1.25                       # the last pixel is valid
    base = torch.where(torch.isfinite(gt), gt, torch.zeros(()))
    preds = []
    for k in range(K):
        p = base + synthetic_tensor((B, H, W), 3410 + k, lo=-3.0, hi=3.0)
        p[0, 1, :4] = gt[0, 1, :4] + torch.tensor([1.0, -1.0, 0.5, -2.0])
        preds.append(p.unsqueeze(1).contiguous())
    return gt, preds


def trainer_weights(n_predictions, loss_gamma=LOSS_GAMMA):
    """[1 for the initial disparity] + the trainer's gamma_adj ^ (n - i - 1) (trainer_torchrun.py:281-283), as Python floats."""
    adjusted = loss_gamma ** (15 / (n_predictions - 1))
    return [1.0] + [adjusted ** (n_predictions - i - 1) for i in range(n_predictions)]


assert all(math.prod(c[:4]) > 0 for c in CASES.values())
