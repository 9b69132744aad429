"""Case tables and seeded inputs shared by tests/golden/make_golden_stereoanywhere.py (build container, runs the reference) and
tests/test_stereoanywhere.py (runs everywhere: this module imports nothing from the reference tree).

Estimator cases: B, H, W1, W2, s -- the volume is a near-normal field times s (peaky enough that the softmax is not flat: the
reference's fp32 and fp64 runs then differ in every output, d_ref > 0).  The smallest shapes at which csrc/allpairs.hip can fail:
  b2_13    (2, 3, 13, 13)    below one wave, W2 no multiple of 4, B*H*W1 = 78 rows: the last workgroup of four rows is half empty.
  w70_66   (1, 2, 70, 66)    W1 != W2, more than one wave's width (a second register per lane, a second column strip of 2 lanes).
  w260     (1, 1, 260, 260)  more than 256 columns: five registers per lane, five column strips, 65 rows per wave.
  px37     (1, 5, 37, 37)    185 rows, no multiple of the workgroup's four.
Block cases: B, H, W1, W2, num_levels, radius, pad, truncate.  Three lookups on one object, the losses summed, plus a weighted sum
of every level of the public pyramid (another consumer of it).  The positions are the pixel's column plus seeded offsets with
planted pixels in row 0 (exact integers, every tap outside on either side, windows straddling both ends).
  l4_r4        37 -> 18 -> 9 -> 4: an odd tail is dropped at levels 0 and 2.
  l1_r1_pad    one level, radius 1, pad [2, 1], B = 2.
  trunc_pad    four levels, pad [2, 1], the volume multiplied by truncate_corr_volume_v2(..., conf_th=None) first.
Mask cases: truncate_corr_volume_v2 with conf_th None and 0.5.
"""
import torch

from stereo_toolbox_amd.utils import synthetic_tensor

#             B  H   W1   W2   s
EST_CASES = {
    "b2_13": (2, 3, 13, 13, 1.0),
    "w70_66": (1, 2, 70, 66, 4.0),
    "w260": (1, 1, 260, 260, 6.0),
    "px37": (1, 5, 37, 37, 4.0),
}
EST_WHOLE = ("b2_13",)                 # gradients stored whole; of the others d_ref, max|fp64| and `subsample` of the fp64 tensor
EST_GPU_ONLY = ()
OUTPUTS = ("disp_l", "conf_l", "disp_r", "conf_r")
#                B  H  W1  W2  L  r  pad     truncate
BLOCK_CASES = {
    "l4_r4": (1, 3, 37, 37, 4, 4, (0, 0), False),
    "l1_r1_pad": (2, 2, 20, 20, 1, 1, (2, 1), False),
    "trunc_pad": (1, 2, 37, 37, 4, 4, (2, 1), True),
}
BLOCK_CALLS = 3
ATTENUATION = 0.1
MASK_SHAPE = (1, 2, 37)                # B, H, W
MASK_THRESHOLDS = {"mask_none": None, "mask_th": 0.5}
SUBSAMPLE = 512


def subsample(t):
    """At least SUBSAMPLE elements of t (all of a smaller tensor) at a fixed odd stride over the flattened tensor."""
    flat = t.reshape(-1)
    stride = max(1, flat.numel() // SUBSAMPLE)
    return flat[::stride - 1 + stride % 2]


def _normal(shape, seed):
    """Near-normal, unit variance: three uniform fields summed."""
    return sum(synthetic_tensor(shape, seed, stream=k) for k in range(3)) / 3.0 ** 0.5


def est_inputs(tag):
    """(volume [B, 1, H, W1, W2], loss weights of the four outputs: [B, 1, H, W1] x 2, [B, 1, H, W2] x 2)"""
    B, H, W1, W2, s = EST_CASES[tag]
    seed = 3000 + 20 * list(EST_CASES).index(tag)
    vol = _normal((B, 1, H, W1, W2), seed) * s
    gws = tuple(synthetic_tensor((B, 1, H, W2 if i >= 2 else W1), seed + 1 + i) for i in range(4))
    return vol, gws


def truncation_maps(B, H, W, seed):
    """(disp_left, conf_left) [B, 1, H, W]: disparities 0 .. 12, confidences 0 .. 1 on both sides of 0.5"""
    return (synthetic_tensor((B, 1, H, W), seed, lo=0.0, hi=12.0), synthetic_tensor((B, 1, H, W), seed + 1, lo=0.0, hi=1.0))


def block_out_width(tag):
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES[tag]
    return W1 - pad[0] - pad[1]


def block_inputs(tag):
    """(fullcorr [B, H, W1, 1, W2], truncation maps or None, coords of the calls [B, 2, H, W1], loss weights of the calls
    [B, L (2r + 1), H, W1 - pad0 - pad1], weights of the pyramid levels [B, H, W1, W2 >> i])"""
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES[tag]
    seed = 3200 + 40 * list(BLOCK_CASES).index(tag)
    vol = _normal((B, H, W1, 1, W2), seed) * 2.0
    maps = truncation_maps(B, H, W1, seed + 1) if trunc else None
    cols = torch.arange(W1, dtype=torch.float32).view(1, 1, 1, W1).repeat(B, 1, H, 1)
    rows = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).repeat(B, 1, 1, W1)
    coords = []
    for call in range(BLOCK_CALLS):
        x = cols + synthetic_tensor((B, 1, H, W1), seed + 5 + call, lo=-6.0, hi=6.0)
        row = x[0, 0, 0]                          # planted before the shift by pad[0]; columns pad[0] .. survive the crop
        row[3] = 0.0 - pad[0]                     # exact integers
        row[4] = float(W2 - 1) - pad[0]
        row[5] = -(r + 1.5) - call - pad[0]       # every tap outside on the left
        row[6] = W2 - 1 + r + 1.25 + call         # ... and on the right
        row[7] = -0.5 - call - pad[0]             # the window straddles the left end
        row[8] = W2 - 1.5 + call - pad[0]         # ... and the right end
        coords.append(torch.cat([x, rows], dim=1))
    n = L * (2 * r + 1)
    gws = [synthetic_tensor((B, n, H, block_out_width(tag)), seed + 10 + i) for i in range(BLOCK_CALLS)]
    wc = [synthetic_tensor((B, H, W1, W2 >> i), seed + 20 + i) for i in range(L)]
    return vol, maps, coords, gws, wc


def mask_inputs():
    B, H, W = MASK_SHAPE
    return truncation_maps(B, H, W, 3400)
