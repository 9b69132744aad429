"""Case table and seeded inputs shared by tests/golden/make_golden_geo.py (build container, runs the reference) and
tests/test_geo_lookup.py (runs everywhere: this module imports nothing from the reference tree).

A lookup case: B, C (geometry channels), D, H, W (= W1), W2, Cf (feature channels), num_levels, radius.  The shapes are
tiny (a few hundred pixels) but ragged on purpose: W is never a multiple of 16, `r2_l3_odd` has an odd D and an odd W2 at
two levels (13 -> 6 -> 3, 21 -> 10 -> 5: pooling drops the tail twice) and B = 2.  No pooled level is shorter than 2: the
reference's grid normalisation divides by (length - 1).
Every case is called TWICE on one object with different disparities and the two losses are summed (the GRU-iteration
pattern).  Both disparity maps are seeded noise over [-3, D + 3] with planted pixels: exact integers (0, 3, D - 1), a negative
value, values beyond D - 1, and values that push coords - disp below 0 and above W2 - 1.
"""
import torch

from stereo_toolbox_amd.utils import synthetic_tensor

#            B  C  D   H  W   W2  Cf  levels radius
CASES = {
    "igev_r4_l2": (1, 8, 12, 5, 20, 20, 12, 2, 4),
    "r2_l3_odd": (2, 8, 13, 3, 18, 21, 8, 3, 2),
    "l1_r3": (1, 4, 9, 2, 17, 17, 8, 1, 3),
}
UPSAMPLE_CASES = {"b2_5x7": (2, 5, 7), "b1_3x18": (1, 3, 18)}         # B, h, w -> output [B, 4h, 4w]


def out_channels(tag):
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    return L * (C + 1) * (2 * r + 1)


def _disp(tag, call):
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    seed = 500 + 10 * list(CASES).index(tag) + call
    d = synthetic_tensor((B, 1, H, W), seed, lo=-3.0, hi=D + 3.0).clone()
    row = d[0, 0, 0]
    row[0] = 0.0
    row[1] = 3.0
    row[2] = float(D - 1)
    row[3] = -2.5
    row[4] = D + 1.25
    row[5] = float(D - 1) + 0.5
    row[W - 1] = -6.5 - call                  # coords - disp > W2 - 1 for W2 <= W + 5
    row[6] = 9.75 + call                      # coords - disp < 0
    d[-1, 0, -1, 0] = 7.0                     # an integer that leaves the correlation row on the left
    return d


def inputs(tag):
    """(geo_volume [B,C,D,H,W], fmap1 [B,Cf,H,W], fmap2 [B,Cf,H,W2], coords [B,1,H,W], (disp_a, disp_b),
    (loss weights of call a, call b))"""
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    seed = 400 + 10 * list(CASES).index(tag)
    geo = synthetic_tensor((B, C, D, H, W), seed)
    f1 = synthetic_tensor((B, Cf, H, W), seed + 1)
    f2 = synthetic_tensor((B, Cf, H, W2), seed + 2)
    coords = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).repeat(B, 1, H, 1)
    n = out_channels(tag)
    gws = (synthetic_tensor((B, n, H, W), seed + 3), synthetic_tensor((B, n, H, W), seed + 4))
    return geo, f1, f2, coords, (_disp(tag, 0), _disp(tag, 1)), gws


def upsample_inputs(tag):
    """(disp_low [B,1,h,w], up_weights [B,9,4h,4w] (positive, summing to one over the 9 taps like the mask head's softmax;
    built from additions and one division so that every machine regenerates the same bits), loss weights [B,4h,4w])"""
    B, h, w = UPSAMPLE_CASES[tag]
    seed = 600 + 10 * list(UPSAMPLE_CASES).index(tag)
    disp = synthetic_tensor((B, 1, h, w), seed, lo=0.0, hi=40.0)
    u = synthetic_tensor((B, 9, 4 * h, 4 * w), seed + 1, lo=0.02, hi=1.0)
    total = u[:, 0]
    for t in range(1, 9):
        total = total + u[:, t]
    wts = (u / total.unsqueeze(1)).contiguous()
    gw = synthetic_tensor((B, 4 * h, 4 * w), seed + 2)
    return disp, wts, gw
