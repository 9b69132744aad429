"""Cases and inputs of the axial-planar convolution tests (tests/test_apc.py) and of their fixture generator
(make_golden_apc.py): FoundationStereo's Conv3dNormActReduced, reference FoundationStereo/submodule.py:89-114.

Inputs and loss weights come from the hash generator, weights from fill_state_dict: the tests regenerate them, the fixture
stores only what the reference computed.  The fp64 tensors of the four cases total 2.6 MB, more than one committed file may
hold: the generator deals the keys to `apc.npz` and as many `apc_<n>.npz` parts as it needs (PARTS), the tests read them as one
mapping (`load_gold`).
"""
import os

import numpy as np

from stereo_toolbox_amd.utils import synthetic_tensor

HERE = os.path.dirname(os.path.abspath(__file__))

# tag -> (B, C_in, hidden, C_out, kernel_disp, D, H, W); hidden None = C_out (the reference's default)
CASES = {
    "vol28": (2, 28, None, 28, 17, 19, 3, 5),     # the model's 1/4-resolution width; ragged N; D just above the kernel
    "d13": (1, 56, None, 56, 17, 13, 2, 33),      # D below the kernel length (the real 1/32 depth); W across a 32-tile
    "short": (1, 8, 16, 24, 5, 3, 4, 7),          # Cin != hidden != Cout; kd > D
    "wide": (1, 8, 136, 8, 17, 6, 3, 4),          # more than 128 channels as Cout of conv1 and as Cin of conv2
}
SEED_X, SEED_G = 7, 8                              # first seeds the generator tries (input, loss weights)
PARTS = ("apc.npz", "apc_1.npz", "apc_2.npz", "apc_3.npz")
PART_BYTES = 900 * 1024

# kernel-level shapes (B, D, H, W, Cin, Cout[, kd]) of the fp64 F.conv3d comparison
PLANAR_SHAPES = [(1, 2, 3, 5, 28, 28), (2, 1, 1, 1, 8, 8), (1, 2, 5, 35, 56, 56), (1, 3, 33, 2, 112, 112), (1, 1, 2, 3, 168, 168)]
AXIAL_SHAPES = [(1, 19, 3, 5, 28, 28, 17), (1, 5, 2, 3, 56, 56, 17), (1, 1, 1, 1, 8, 8, 17), (1, 40, 1, 33, 8, 16, 17),
                (1, 13, 2, 3, 168, 168, 17), (1, 3, 4, 7, 16, 24, 5)]


def block_args(tag):
    B, Cin, hidden, Cout, kdisp, D, H, W = CASES[tag]
    return dict(C_in=Cin, C_out=Cout, hidden=hidden, kernel_size=3, kernel_disp=kdisp)


def inputs(tag, seed_x=SEED_X, seed_g=SEED_G):
    """x [B, C_in, D, H, W] and the loss weights g [B, C_out, D, H, W] of `loss = (y * g).sum()`."""
    B, Cin, hidden, Cout, kdisp, D, H, W = CASES[tag]
    return synthetic_tensor((B, Cin, D, H, W), seed_x), synthetic_tensor((B, Cout, D, H, W), seed_g)


def load_gold():
    gold = {}
    for name in PARTS:
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            with np.load(path) as part:
                gold.update({k: part[k] for k in part.files})
    return gold
