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


# ------------------------------------------------------------------------------------------------------------------------
# Second table (tests/test_geo_lookup_shapes.py, fixture geo_lookup_shapes.npz): shapes that reach the size-dependent branches
# of csrc/geo_lookup.hip.  Same layout of a row as CASES.  Whole tensors at these sizes do not belong in git: the fixture keeps
# per tensor d_ref = max|fp32 - fp64| of the reference, max|fp64| and `subsample` of the fp64 tensor.
#
# geo_pyramid_launch halves the pixel tile WT from 16 until D * (WT * C + C) * 4 bytes <= 65536, i.e. WT + 1 <= 16384 / (D * C):
#   D * C = 48 * 8 = 384    -> 42.6 : WT = 16        (wide, production)
#   D * C = 192 * 8 = 1536  -> 10.6 : WT = 8         (deep_wt8;  W = 21 = 2 * 8 + 5: partial last tile)
#   D * C = 192 * 16 = 3072 -> 5.3  : WT = 4         (deep_wt4;  W = 11 = 2 * 4 + 3)
#   D * C = 400 * 8 = 3200  -> 5.1  : WT = 4         (deep_d400; W = 7 = 4 + 3; 400 -> 200 -> 100)
#   D * C = 1032 * 8 = 8256 -> 1.98 : refused        (REFUSED_PYRAMID: does not fit at WT = 1)
# wide: W2 = 301 = 256 + 45 (second w2_0 round of wave 0 only, ragged: tiles 256, 272 full, 288 partial), pooled lengths
#   150 and 75; W1 = 77 = 4 * 16 + 13; the backward sums over 301 (19 trips) and over 77 (5 trips); Cf = 96: two channel rounds.
# many_px: 2 * 32 * 65 = 4160 pixels = 33 lookup workgroups of 128; the batch boundary (pixel 2080 = 16 * 128 + 32) lies
#   inside workgroup 16.
#               B  C   D    H    W    W2   Cf  levels radius
SHAPE_CASES = {
    "wide": (1, 8, 48, 2, 77, 301, 96, 3, 4),
    "deep_wt8": (1, 8, 192, 2, 21, 24, 8, 3, 4),
    "deep_wt4": (1, 16, 192, 2, 11, 24, 8, 3, 4),
    "deep_d400": (1, 8, 400, 2, 7, 19, 8, 3, 4),
    "c12": (2, 12, 13, 3, 18, 21, 8, 2, 3),
    "many_px": (2, 8, 12, 32, 65, 65, 8, 2, 2),
    "production_rows": (1, 8, 48, 3, 240, 240, 96, 2, 4),            # the README's shape cut to three rows (emulator)
    "production": (1, 8, 48, 144, 240, 240, 96, 2, 4),               # 576x960 -> 144x240: product run gpu-marked only
}
GPU_ONLY_SHAPE_CASES = ("production",)
REFUSED_PYRAMID = (1, 8, 1032, 1, 3)                                  # B, C, D, H, W
SHAPE_UPSAMPLE_CASES = {"b2_12x23": (2, 12, 23), "production": (1, 144, 240)}     # 276 low-resolution pixels per image, B = 2
GPU_ONLY_SHAPE_UPSAMPLE_CASES = ("production",)
ITER_CASE = (1, 8, 12, 5, 20, 20, 12, 2, 4)                           # the shape of igev_r4_l2
ITER_CALLS = 22                                                       # lookups of one training step (igev_stereo.py:101)
EXTRA_CALLS = 4                                                       # the extra-consumer case: the first four of them
SUBSAMPLE = 512


def subsample(t):
    """At least SUBSAMPLE elements of t (all of a smaller tensor) at a fixed odd stride over the flattened tensor."""
    flat = t.reshape(-1)
    stride = max(1, flat.numel() // SUBSAMPLE)
    return flat[::stride - 1 + stride % 2]


def shape_out_channels(case):
    B, C, D, H, W, W2, Cf, L, r = case
    return L * (C + 1) * (2 * r + 1)


def shape_coords(case):
    """The pixel's column, stretched over the right image's row where W2 > W (a multiple of 0.25 per column, so the pooled
    levels see fractional positions): 3.75 per column at wide, i.e. 0 .. 285 of 0 .. 300."""
    B, C, D, H, W, W2, Cf, L, r = case
    step = max(1.0, int(4 * (W2 - 1) / (W - 1)) / 4)
    return (torch.arange(W, dtype=torch.float32) * step).view(1, 1, 1, W).repeat(B, 1, H, 1)


def shape_disp(case, seed, call):
    """Seeded noise over [-3, D + 3] with the planted pixels of `_disp`, the two that must leave the correlation row placed
    relative to this case's coords and W2."""
    B, C, D, H, W, W2, Cf, L, r = case
    c = shape_coords(case)[0, 0, 0]
    d = synthetic_tensor((B, 1, H, W), seed, lo=-3.0, hi=D + 3.0).clone()
    row = d[0, 0, 0]
    row[0] = 0.0
    row[1] = 3.0
    row[2] = float(D - 1)
    row[3] = -2.5
    row[4] = D + 1.25
    row[5] = float(D - 1) + 0.5
    if W > 8:
        row[7] = float(c[7]) - (W2 - 1.5)                # the window straddles the right end of the correlation row
    row[W - 1] = float(c[W - 1]) - (W2 + 5.5 + call)     # coords - disp = W2 + 5.5 + call > W2 - 1
    if W > 6:
        row[6] = float(c[6]) + 3.75 + call               # coords - disp < 0
    d[-1, 0, -1, 0] = 7.0                                # an integer that leaves the correlation row on the left
    return d


def shape_inputs(tag):
    """As `inputs`, for SHAPE_CASES."""
    case = SHAPE_CASES[tag]
    B, C, D, H, W, W2, Cf, L, r = case
    seed = 1000 + 20 * list(SHAPE_CASES).index(tag)
    geo = synthetic_tensor((B, C, D, H, W), seed)
    f1 = synthetic_tensor((B, Cf, H, W), seed + 1)
    f2 = synthetic_tensor((B, Cf, H, W2), seed + 2)
    n = shape_out_channels(case)
    gws = (synthetic_tensor((B, n, H, W), seed + 3), synthetic_tensor((B, n, H, W), seed + 4))
    return geo, f1, f2, shape_coords(case), (shape_disp(case, seed + 5, 0), shape_disp(case, seed + 6, 1)), gws


def iter_inputs():
    """The iteration pattern on one object: ITER_CALLS distinct disparities and loss weights; for the extra-consumer case the
    weights of a weighted sum of both pyramids, per level: geometry [B, H, W, C, D_i], correlation [B, H, W, W2_i]."""
    case = ITER_CASE
    B, C, D, H, W, W2, Cf, L, r = case
    geo = synthetic_tensor((B, C, D, H, W), 1400)
    f1 = synthetic_tensor((B, Cf, H, W), 1401)
    f2 = synthetic_tensor((B, Cf, H, W2), 1402)
    n = shape_out_channels(case)
    disps = [shape_disp(case, 1410 + i, i % 3) for i in range(ITER_CALLS)]
    gws = [synthetic_tensor((B, n, H, W), 1440 + i) for i in range(ITER_CALLS)]
    wg = [synthetic_tensor((B, H, W, C, D >> i), 1470 + i) for i in range(L)]
    wc = [synthetic_tensor((B, H, W, W2 >> i), 1480 + i) for i in range(L)]
    return geo, f1, f2, shape_coords(case), disps, gws, wg, wc


def shape_upsample_inputs(tag):
    """As `upsample_inputs`, for SHAPE_UPSAMPLE_CASES."""
    B, h, w = SHAPE_UPSAMPLE_CASES[tag]
    seed = 1600 + 10 * list(SHAPE_UPSAMPLE_CASES).index(tag)
    disp = synthetic_tensor((B, 1, h, w), seed, lo=0.0, hi=40.0)
    u = synthetic_tensor((B, 9, 4 * h, 4 * w), seed + 1, lo=0.02, hi=1.0)
    total = u[:, 0]
    for t in range(1, 9):
        total = total + u[:, t]
    wts = (u / total.unsqueeze(1)).contiguous()
    gw = synthetic_tensor((B, 4 * h, 4 * w), seed + 2)
    return disp, wts, gw
