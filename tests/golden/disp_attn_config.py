"""Cases, inputs, the plain-torch restatement and the numpy restatement of the dropout generator for the disparity-transformer
tests (tests/test_disp_attention.py) and their fixture generator (make_golden_disp_attn.py): the reference classes
FoundationStereo/submodule.py `CostVolumeDisparityAttention` / `FlashAttentionTransformerEncoderLayer`.

Inputs and loss weights come from the hash generator, weights from fill_state_dict: the tests regenerate them, the fixture stores
only what the reference computed (`tag/key:f64`, `tag/key:f32`, `tag/key:dref`).
"""
import math
import os

import numpy as np
import torch

from stereo_toolbox_amd.utils import synthetic_tensor

HERE = os.path.dirname(os.path.abspath(__file__))

# tag -> (B, C, heads, feed-forward, layers, D, H, W)
CASES = {
    "model": (1, 28, 4, 28, 4, 26, 3, 5),      # the model's widths: head dim 7, L = 26, 15 sequences
    "ragged": (2, 12, 3, 20, 2, 5, 2, 3),      # head dim 4, ff != C, L far below a tile, batch stride
    "limits": (1, 32, 4, 32, 1, 32, 2, 2),     # every served maximum
    "one_token": (1, 28, 4, 28, 4, 1, 2, 3),   # soft-max over one key: q_proj / k_proj gradients are exactly zero
}
# GPU only, no fixture: the model's own sequence count at 576 x 960
FULL = (1, 28, 4, 28, 4, 26, 36, 60)
SEED = 71
MAX_LEN = 32
MIN_VARIANCE = 1e-2                            # of every LayerNorm input of the fixture's fp64 run, per token (a condition, not a tolerance)
PARTS = ("disp_attn.npz", "disp_attn_1.npz")
PART_BYTES = 900 * 1024
TENSORS = ("self_attn.q_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.weight", "self_attn.k_proj.bias",
           "self_attn.v_proj.weight", "self_attn.v_proj.bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
           "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
           "norm2.bias")


def module_args(shape, dropout=0.0):
    B, C, heads, ff, layers, D, H, W = shape
    return dict(d_model=C, nhead=heads, dim_feedforward=ff, dropout=dropout, num_transformer=layers, max_len=MAX_LEN)


def param_names(layers):
    return [f"sa.{i}.{n}" for i in range(layers) for n in TENSORS]


def volume_inputs(shape, seed=SEED):
    """cv and the loss weights g, logical [B, C, D, H, W] fp32 (contiguous NCDHW)."""
    B, C, heads, ff, layers, D, H, W = shape
    return synthetic_tensor((B, C, D, H, W), seed, stream=0), synthetic_tensor((B, C, D, H, W), seed, stream=1)


def sinusoid(L, C, dtype):
    """The reference's table (submodule.py:477-484) computed in fp32 as there, first L rows."""
    position = torch.arange(0, MAX_LEN).float().unsqueeze(1)
    div_term = (torch.arange(0, C, 2).float() * -(math.log(10000.0) / C)).exp()[None]
    pe = torch.zeros(MAX_LEN, C)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe[:L].to(dtype)


def encoder(x, pe, params, heads, eps=1e-5, masks=None, scale=1.0, norm_inputs=None):
    """The layers in plain torch, any dtype: tests/restated.py::disp_encoder (shared with the kernel-level parity module)."""
    from tests.restated import disp_encoder
    return disp_encoder(x, pe, params, heads, eps=eps, masks=masks, scale=scale, norm_inputs=norm_inputs)


def to_sequences(cv):
    """[B, C, D, H, W] -> [B H W, D, C], the reference's permute + reshape."""
    B, C, D, H, W = cv.shape
    return cv.permute(0, 3, 4, 2, 1).reshape(B * H * W, D, C)


def from_sequences(x, B, H, W):
    N, D, C = x.shape
    return x.reshape(B, H, W, D, C).permute(0, 4, 3, 1, 2)


def restated(cv, params, heads, masks=None, scale=1.0, norm_inputs=None):
    """`CostVolumeDisparityAttention.forward` in plain torch."""
    B, C, D, H, W = cv.shape
    x = encoder(to_sequences(cv), sinusoid(D, C, cv.dtype), params, heads, masks=masks, scale=scale, norm_inputs=norm_inputs)
    return from_sequences(x, B, H, W)


def run_case(step, params, shape, dtype, seed=SEED):
    """y = step(cv), loss = (y * g).sum(); returns what the fixture stores: `y`, `gx` and `grad/<name>` for `params` (name -> tensor)."""
    cv, g = volume_inputs(shape, seed)
    cv = cv.to(dtype).requires_grad_()
    y = step(cv)
    (y * g.to(dtype).to(y.device)).sum().backward()
    out = {"y": y.detach(), "gx": cv.grad}
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


# ------------------------------------------------------------------------------------------ the dropout generator, restated
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays that hold 32-bit words; returns the four output words."""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
    return c0, c1, c2, c3


def keep_masks(seed, p, N, L, C, ff, layers):
    """The documented counter layout (include/stx_hip.h): key = (seed low word, seed high word), counter = (sequence, token >> 2,
    4 * layer + site, channel), word (token & 3); kept iff word >= floor(p * 2^32) with p taken as fp32.
    -> uint8 [layers, 3, N, L, max(C, ff)]."""
    s = int(seed) & (2 ** 64 - 1)
    thr = np.uint64(math.floor(float(np.float32(p)) * 4294967296.0))
    Cm = max(C, ff)
    ls, n, t, ch = np.meshgrid(np.arange(layers * 3, dtype=np.uint64), np.arange(N, dtype=np.uint64), np.arange(L, dtype=np.uint64),
                               np.arange(Cm, dtype=np.uint64), indexing="ij")
    site = ls % np.uint64(3)
    layer = ls // np.uint64(3)
    words = philox4x32_10(n, t >> np.uint64(2), np.uint64(4) * layer + site, ch, s & 0xFFFFFFFF, s >> 32)
    word = np.select([(t & np.uint64(3)) == np.uint64(r) for r in range(4)], words)
    return (word >= thr).astype(np.uint8).reshape(layers, 3, N, L, Cm)
