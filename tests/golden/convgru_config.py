"""Cases, inputs and the plain-torch restatement of the ConvGRU cell tests (tests/test_convgru.py) and of their fixture generator
(make_golden_convgru.py): the reference class IGEVStereo/update.py:25-40.

Inputs and loss weights come from the hash generator, weights from fill_state_dict: the tests regenerate them, the fixture stores
only what the reference computed (`tag/key:f64`, `tag/key:f32`, `tag/key:dref`).  The cell is smooth, so no condition on the
seeds is needed.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from stereo_toolbox_amd.utils import synthetic_tensor

HERE = os.path.dirname(os.path.abspath(__file__))

# tag -> (B, hidden, x channels, H, W, iterations)
CASES = {
    "one_src": (2, 16, (16,), 5, 19, 1),       # batch stride; W across a 16-pixel tile edge, H below a tile
    "two_src": (1, 16, (16, 16), 9, 7, 1),     # source seams in K; H across a tile edge
    "ragged": (1, 16, (20, 4, 8), 3, 33, 1),   # channel counts that are no multiple of a K group; three x sources
    "wide_n": (1, 32, (32,), 4, 6, 1),         # N = 64 in the zr launch
    "loop3": (1, 16, (8,), 4, 6, 3),           # one module three times, h fed back, loss over all states
}
SEED = 31
PARTS = ("convgru.npz", "convgru_1.npz", "convgru_2.npz")
PART_BYTES = 900 * 1024

# the real width, no fixture: (B, H, W, hidden, x channels); the last one runs on the GPU only
WIDE_SHAPES = [(1, 3, 17, 128, (128, 128)), (1, 2, 5, 128, (128,)), (1, 24, 40, 128, (128, 128))]
PARAMS = ("convz.weight", "convz.bias", "convr.weight", "convr.bias", "convq.weight", "convq.bias")


def cell_inputs(B, hidden, cx, H, W, seed=SEED, iters=1):
    """h, cz, cr, cq, the x sources and one loss-weight tensor per iteration, all logical NCHW fp32."""
    t = lambda c, k, lo=-1.0, hi=1.0: synthetic_tensor((B, c, H, W), seed, stream=k, lo=lo, hi=hi)   # noqa: E731
    h = torch.tanh(t(hidden, 0, -2.0, 2.0))                   # a state is a convex mix of tanh values
    cz, cr, cq = t(hidden, 1), t(hidden, 2), t(hidden, 3)
    xs = [t(c, 10 + i) for i, c in enumerate(cx)]
    gs = [t(hidden, 20 + i) for i in range(iters)]
    return h, cz, cr, cq, xs, gs


def inputs(tag):
    B, hidden, cx, H, W, iters = CASES[tag]
    return cell_inputs(B, hidden, cx, H, W, iters=iters)


def module_args(tag):
    B, hidden, cx, H, W, iters = CASES[tag]
    return dict(hidden_dim=hidden, input_dim=sum(cx))


def cell(h, cz, cr, cq, xs, wz, bz, wr, br, wq, bq):
    """The cell in plain torch, any dtype: gates from [h | x], candidate from [r h | x], convex update."""
    x = torch.cat(list(xs), 1)
    zero = lambda c: 0 if c is None else c                    # noqa: E731
    hx = torch.cat([h, x], 1)
    z = torch.sigmoid(F.conv2d(hx, wz, bz, padding=1) + zero(cz))
    r = torch.sigmoid(F.conv2d(hx, wr, br, padding=1) + zero(cr))
    q = torch.tanh(F.conv2d(torch.cat([r * h, x], 1), wq, bq, padding=1) + zero(cq))
    return (1 - z) * h + z * q


def run_case(step, params, tag, dtype):
    """`step(h, cz, cr, cq, xs)` iterated as the case says with loss = sum_i (h_i * g_i).sum(); returns the tensors the fixture
    stores: the last state `h`, and the gradients `g_h`, `g_cz`, `g_cr`, `g_cq`, `g_x<i>`, `grad/<parameter>`."""
    h, cz, cr, cq, xs, gs = inputs(tag)
    leaves = [t.to(dtype).requires_grad_() for t in [h, cz, cr, cq] + xs]
    state, loss = leaves[0], 0
    for g in gs:
        state = step(state, leaves[1], leaves[2], leaves[3], leaves[4:])
        loss = loss + (state * g.to(dtype)).sum()
    loss.backward()
    out = {"h": state.detach()}
    for name, t in zip(["g_h", "g_cz", "g_cr", "g_cq"] + [f"g_x{i}" for i in range(len(xs))], leaves):
        out[name] = t.grad
    for name, p in params.items():
        out["grad/" + name] = p.grad
    return out


def load_gold():
    gold = {}
    for name in PARTS:
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            with np.load(path) as part:
                gold.update({k: part[k] for k in part.files})
    return gold
