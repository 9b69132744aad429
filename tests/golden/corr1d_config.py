"""Case table and seeded inputs shared by tests/golden/make_golden_corr1d.py (build container, runs the reference) and
tests/test_corr1d.py (runs everywhere: this module imports nothing from the reference tree).

A case: kind, B, Cf (feature channels), H, W1, W2, num_levels, radius.  They are the smallest shapes at which each branch of
csrc/corr1d.hip can fail:
  raft_l4_r4     levels 27 -> 13 -> 6 -> 3: an odd tail is dropped at levels 0 and 1; all four levels, W1 = 20 = 16 + 4.
  raft_b2_l3_r2  B = 2, three levels (21 -> 10 -> 5), W1 = 18.
  wide           W2 = 301 = 256 + 45 (a second w2 round of wave 0, ragged tiles; -> 150 -> 75 -> 37: an odd tail at level 2),
                 W1 = 77 = 4 * 16 + 13, Cf = 96 (two channel rounds of the backward).
  many_px        2 * 32 * 65 = 4160 pixels = 33 lookup workgroups; the batch boundary (pixel 2080 = 16 * 128 + 32) lies inside one.
  defom          the disparity-indexed block with the model's eight scales (defom_stereo.py: scale_list, scale_corr_radius 2),
                 called without and with `scaling`.
  production     576x960 at 1/4: Cf 256, 144x240, four levels, radius 4 (GPU only; `production_rows` is its cut to three rows
                 for the emulator).
Every case is called TWICE on one object with different positions and the two losses are summed (the GRU-iteration pattern).
The positions are the pixel's column (stretched over the right row where W2 > W1) plus seeded sub-pixel offsets, with planted
pixels in row 0: exact integers, x < -r, x > len - 1 + r, windows straddling each end of the row, and one position of +-1e9.
"""
import torch

from stereo_toolbox_amd.utils import synthetic_tensor

DEFOM_SCALES = (0.125, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0)          # the model's scale_list (defom_stereo.py:41-42)
DEFOM_SCALE_RADIUS = 2

#                  kind    B  Cf   H   W1   W2  L  r
CASES = {
    "raft_l4_r4": ("raft", 1, 12, 3, 20, 27, 4, 4),
    "raft_b2_l3_r2": ("raft", 2, 8, 2, 18, 21, 3, 2),
    "defom": ("defom", 1, 8, 3, 20, 20, 2, 4),
}
#  whole tensors at these sizes do not belong in git: the fixture keeps d_ref, max|fp64| and `subsample` of the fp64 tensor
SHAPE_CASES = {
    "wide": ("raft", 1, 96, 2, 77, 301, 4, 4),
    "many_px": ("raft", 2, 8, 32, 65, 65, 2, 2),
    "production_rows": ("raft", 1, 256, 3, 240, 240, 4, 4),
    "production": ("raft", 1, 256, 144, 240, 240, 4, 4),
}
GPU_ONLY_CASES = ("production",)
ALL_CASES = {**CASES, **SHAPE_CASES}
ITER_CASE = "raft_l4_r4"
ITER_CALLS = 32                                                       # lookups of one validation pass (raft_stereo.py: iters)
SUBSAMPLE = 512


def subsample(t):
    """At least SUBSAMPLE elements of t (all of a smaller tensor) at a fixed odd stride over the flattened tensor."""
    flat = t.reshape(-1)
    stride = max(1, flat.numel() // SUBSAMPLE)
    return flat[::stride - 1 + stride % 2]


def out_channels(tag, scaling=False):
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    return len(DEFOM_SCALES) * (2 * DEFOM_SCALE_RADIUS + 1) if scaling else L * (2 * r + 1)


def columns(tag):
    """[B, 1, H, W1]: the pixel's column, stretched over the right image's row where W2 > W1 (a multiple of 0.25 per column)."""
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    step = max(1.0, int(4 * (W2 - 1) / (W1 - 1)) / 4)
    return (torch.arange(W1, dtype=torch.float32) * step).view(1, 1, 1, W1).repeat(B, 1, H, 1)


def _planted(tag, x, call):
    """x [B, 1, H, W1]: sampling positions at level 0; plants the edge pixels in row 0 of image 0."""
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    row = x[0, 0, 0]
    row[0] = 0.0                               # exact integers
    row[1] = 3.0
    row[2] = float(W2 - 1)
    row[3] = -(r + 1.5) - call                 # x < -r: every tap outside on the left
    row[4] = W2 - 1 + r + 1.25 + call          # x > len - 1 + r
    row[5] = -0.5 - call                       # the window straddles the left end
    row[6] = W2 - 1.5 + call                   # ... and the right end
    row[7] = 1.0e9 if call == 0 else -1.0e9    # must not overflow the integer window
    row[8] = (W2 >> (L - 1)) * 2.0 ** (L - 1) - 0.25      # the dropped tail of the last level
    x[-1, 0, -1, 0] = 7.0
    return x


def positions(tag, call):
    """RAFT cases: coords [B, 2, H, W1] -- channel 0 the sampling column, channel 1 the pixel's own row (as the model passes)."""
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    seed = 2000 + 20 * list(ALL_CASES).index(tag)
    x = columns(tag) + synthetic_tensor((B, 1, H, W1), seed + 5 + call, lo=-6.0, hi=6.0)
    x = _planted(tag, x.clone(), call)
    rows = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).repeat(B, 1, 1, W1)
    return torch.cat([x, rows], dim=1)


def disparities(tag, call):
    """DEFOM cases: disp [B, 1, H, W1] such that columns - disp are the planted positions."""
    return columns(tag) - positions(tag, call)[:, :1]


def inputs(tag):
    """(fmap1 [B,Cf,H,W1], fmap2 [B,Cf,H,W2], (positions of call a, call b), (loss weights of call a, call b)); the positions
    are coords for a RAFT case, disparities for a DEFOM case; a DEFOM case's call b is the `scaling=True` call."""
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    seed = 2000 + 20 * list(ALL_CASES).index(tag)
    f1 = synthetic_tensor((B, Cf, H, W1), seed + 1)
    f2 = synthetic_tensor((B, Cf, H, W2), seed + 2)
    if kind == "raft":
        pos = (positions(tag, 0), positions(tag, 1))
        n = (out_channels(tag), out_channels(tag))
    else:
        pos = (disparities(tag, 0), disparities(tag, 1))
        n = (out_channels(tag), out_channels(tag, scaling=True))
    gws = tuple(synthetic_tensor((B, n[i], H, W1), seed + 3 + i) for i in range(2))
    return f1, f2, pos, gws


def iter_inputs():
    """ITER_CALLS lookups on one object of ITER_CASE, plus the weights of a weighted sum of every pyramid level [B,H,W1,W2_i]
    (another consumer of the public pyramid)."""
    tag = ITER_CASE
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    f1 = synthetic_tensor((B, Cf, H, W1), 2401)
    f2 = synthetic_tensor((B, Cf, H, W2), 2402)
    coords = []
    for i in range(ITER_CALLS):
        x = columns(tag) + synthetic_tensor((B, 1, H, W1), 2410 + i, lo=-6.0, hi=6.0)
        coords.append(_planted(tag, x.clone(), i % 3))
    gws = [synthetic_tensor((B, out_channels(tag), H, W1), 2450 + i) for i in range(ITER_CALLS)]
    wc = [synthetic_tensor((B, H, W1, W2 >> i), 2490 + i) for i in range(L)]
    return f1, f2, coords, gws, wc
