"""Cases, inputs and the plain-torch restatement of the SelectiveStereo tests (tests/test_selective.py) and of their fixture
generator (make_golden_selective.py): the reference classes SelectiveStereo/SelectiveRAFT/update.py:15-30 (RaftConvGRU), :61-71
(SelectiveConvGRU), :106-121 (ChannelAttentionEnhancement) and :123-135 (SpatialAttentionExtractor).

Inputs and loss weights come from the hash generator, weights from fill_state_dict: the tests regenerate them, the fixture stores
only what the reference computed (`tag/key:f64`, `tag/key:f32`, `tag/key:dref`).  The cell is smooth.  The attention is not: a
ReLU and two kinds of max sit in it, so the generator asserts margins on its fp64 run (CSA_MARGINS) and the seed is chosen to
meet them.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from stereo_toolbox_amd.utils import synthetic_tensor

HERE = os.path.dirname(os.path.abspath(__file__))

# ------------------------------------------------------------------------------------------ the selective cell
# tag -> (B, hidden, x channels, H, W, iterations)
CELL_CASES = {
    "one_src": (2, 16, (16,), 5, 19, 1),       # batch stride; pixels across a 64-pixel tile edge
    "two_src": (1, 16, (16, 16), 9, 7, 1),     # source seams in K
    "ragged": (1, 16, (20, 4, 8), 3, 33, 1),   # channel counts that are no multiple of a K group; three x sources
    "wide_n": (1, 32, (32,), 4, 6, 1),         # N = 64 in the zr launches
    "loop3": (1, 16, (8,), 4, 6, 3),           # one module three times, h fed back, att fixed, loss over all states
}
CELL_SEED = 37
PARTS = ("selective.npz", "selective_1.npz", "selective_2.npz")
PART_BYTES = 900 * 1024

# the real width, no fixture: (B, H, W, hidden, x channels); the third runs on the GPU only; the last crosses the tile-size
# switch of both GEMM launchers (8-row tiles from 256 workgroups: 4 x 9 x 9 of the 3x3 kernel, 263 of the 1x1 kernel)
WIDE_SHAPES = [(1, 3, 17, 128, (256, 128)), (1, 2, 5, 128, (128, 128)), (1, 24, 40, 128, (256, 128)), (4, 65, 129, 16, (8,))]
CELLS = ("small_gru", "large_gru")
CELL_PARAMS = tuple(f"{c}.{n}" for c in CELLS for n in ("convz.weight", "convz.bias", "convr.weight", "convr.bias", "convq.weight",
                                                        "convq.bias"))


def cell_inputs(B, hidden, cx, H, W, seed=CELL_SEED, iters=1):
    """att, h, the x sources and one loss-weight tensor per iteration, all logical NCHW fp32."""
    t = lambda c, k, lo=-1.0, hi=1.0: synthetic_tensor((B, c, H, W), seed, stream=k, lo=lo, hi=hi)   # noqa: E731
    att = t(1, 5, 0.05, 0.95)
    h = torch.tanh(t(hidden, 0, -2.0, 2.0))                   # a state is a convex mix of tanh values
    xs = [t(c, 10 + i) for i, c in enumerate(cx)]
    gs = [t(hidden, 20 + i) for i in range(iters)]
    return att, h, xs, gs


def inputs(tag):
    B, hidden, cx, H, W, iters = CELL_CASES[tag]
    return cell_inputs(B, hidden, cx, H, W, iters=iters)


def module_args(tag):
    B, hidden, cx, H, W, iters = CELL_CASES[tag]
    return dict(hidden_dim=hidden, input_dim=sum(cx))


def raft_cell(h, xs, wz, bz, wr, br, wq, bq):
    """RaftConvGRU in plain torch, any dtype; the kernel size is the weights'."""
    pad = wz.shape[-1] // 2
    x = torch.cat(list(xs), 1)
    hx = torch.cat([h, x], 1)
    z = torch.sigmoid(F.conv2d(hx, wz, bz, padding=pad))
    r = torch.sigmoid(F.conv2d(hx, wr, br, padding=pad))
    q = torch.tanh(F.conv2d(torch.cat([r * h, x], 1), wq, bq, padding=pad))
    return (1 - z) * h + z * q


def cell(att, h, xs, params):
    """SelectiveConvGRU in plain torch: `params` are the twelve tensors of CELL_PARAMS."""
    return raft_cell(h, xs, *params[:6]) * att + raft_cell(h, xs, *params[6:]) * (1 - att)


def run_cell_case(step, params, tag, dtype):
    """`step(att, h, xs)` iterated as the case says with loss = sum_i (h_i * g_i).sum(); returns the tensors the fixture stores:
    the last state `h` and the gradients `g_att`, `g_h`, `g_x<i>`, `grad/<parameter>`."""
    att, h, xs, gs = inputs(tag)
    leaves = [t.to(dtype).requires_grad_() for t in [att, h] + xs]
    state, loss = leaves[1], 0
    for g in gs:
        state = step(leaves[0], state, leaves[2:])
        loss = loss + (state * g.to(dtype)).sum()
    loss.backward()
    out = {"h": state.detach()}
    for name, t in zip(["g_att", "g_h"] + [f"g_x{i}" for i in range(len(xs))], leaves):
        out[name] = t.grad
    for name, p in params.items():
        out["grad/" + name] = p.grad
    return out


# ------------------------------------------------------------------------------------------ contextual spatial attention
# tag -> (B, C, H, W); two are smaller than the 7x7 halo in one direction
CSA_CASES = {
    "c16": (2, 16, 5, 19),
    "c32": (1, 32, 9, 7),
    "c48": (1, 48, 4, 33),
    "c128": (1, 128, 3, 17),
}
CSA_GPU_CASE = ("c128_big", (2, 128, 36, 60))          # no fixture: the restatement in fp64 against its own fp32 run
# (94: the first seed from 71 up that meets CSA_MARGINS at the GPU-only shape)
CSA_SEED = {"c16": 71, "c32": 71, "c48": 71, "c128": 71, "c128_big": 94}
CSA_KERNEL = 7
CSA_PARAMS = ("cam/fc.0.weight", "cam/fc.2.weight", "sam/samconv.weight")
# what the generator asserts on the fp64 run: |MLP pre-activation|, gap of the two best values of a global max pool, of a
# per-pixel channel max
CSA_MARGINS = (1e-4, 1e-5, 1e-5)


def csa_shape(tag):
    return CSA_GPU_CASE[1] if tag == CSA_GPU_CASE[0] else CSA_CASES[tag]


def csa_inputs(tag):
    """x and the loss weights of x' and att, logical NCHW fp32."""
    B, C, H, W = csa_shape(tag)
    seed = CSA_SEED[tag]
    x = synthetic_tensor((B, C, H, W), seed, stream=0, lo=-1.0, hi=1.0)
    return x, synthetic_tensor((B, C, H, W), seed, stream=1), synthetic_tensor((B, 1, H, W), seed, stream=2)


def csa_gate(x, w1, w2):
    """ChannelAttentionEnhancement.forward in plain torch."""
    fc = lambda v: F.conv2d(torch.relu(F.conv2d(v, w1)), w2)   # noqa: E731
    return torch.sigmoid(fc(F.adaptive_avg_pool2d(x, 1)) + fc(F.adaptive_max_pool2d(x, 1)))


def csa_spatial(x, w):
    """SpatialAttentionExtractor.forward in plain torch."""
    m = torch.cat([x.mean(1, keepdim=True), x.max(1, keepdim=True)[0]], 1)
    return torch.sigmoid(F.conv2d(m, w, padding=w.shape[-1] // 2))


def csa(x, w1, w2, w_sam):
    """(x', att) = (cam(x) * x, sam(x')): reference SelectiveIGEV/igev_stereo.py:225-226 on one map."""
    xp = csa_gate(x, w1, w2) * x
    return xp, csa_spatial(xp, w_sam)


def csa_margins(x, w1, w2):
    """The three margins of CSA_MARGINS on a (fp64) input."""
    pools = torch.cat([F.adaptive_avg_pool2d(x, 1), F.adaptive_max_pool2d(x, 1)], 0)
    pre = F.conv2d(pools, w1).abs().min().item()
    xp = csa_gate(x, w1, w2) * x
    top = x.flatten(2).topk(min(2, x.shape[2] * x.shape[3]), dim=2)[0]
    gap_pool = (top[..., 0] - top[..., -1]).min().item() if top.shape[-1] > 1 else float("inf")
    topc = xp.topk(2, dim=1)[0]
    return pre, gap_pool, (topc[:, 0] - topc[:, 1]).min().item()


def run_csa_case(step, params, tag, dtype):
    """`step(x) -> (x', att)` with loss = (x' g1).sum() + (att g2).sum(); returns `xp`, `att`, `g_x`, `grad/<parameter>`."""
    x, g1, g2 = csa_inputs(tag)
    leaf = x.to(dtype).requires_grad_()
    xp, att = step(leaf)
    ((xp * g1.to(dtype)).sum() + (att * g2.to(dtype)).sum()).backward()
    out = {"xp": xp.detach(), "att": att.detach(), "g_x": leaf.grad}
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
