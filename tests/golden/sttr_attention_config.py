"""Case tables and seeded inputs shared by tests/golden/make_golden_sttr_attention.py (build container, runs the reference) and
tests/test_sttr_attention.py (runs everywhere: this module imports nothing from the reference tree).

Core records: ONE `MultiheadAttentionRelative` call -- kind (self: query = key = value; cross: key = value), C, heads E, W, rows B,
the causal mask of the last layer, and the table ('pos' the sine table, 'flip' the table flipped as in the right update, 'none').
The smallest shapes at which csrc/sttr_attention.hip can fail:
  w2    W = 2: the lower limit; one tile, 14 of 16 rows and columns padding, table rows outside [0, 2W-2] in every window.
  w17   one row past a 16-wide tile, 8 heads (the reference's 128 / 8), three rows b; every variant.
  w65   one query past the 64 queries of a workgroup: a second workgroup, five tiles.
GPU only:
  w320  the working width of 960 / 3, 8 heads.
Transformer records: `Transformer.forward(feat_left, feat_right, pos)` with N = 1 -- hidden, heads, layers, H, W.
Inputs: near-normal unit-variance features (what the LayerNorm in front of every attention produces), weights N(0, 1) / sqrt(fan_in),
biases 0.3 N(0, 1) (the default 0 would hide bias-gradient bugs), LayerNorm weights 1 + 0.1 N(0, 1).
"""
import zlib

import torch

from stereo_toolbox_amd.utils import synthetic_tensor
from tests.golden.sttr_config import SUBSAMPLE, WHOLE, is_whole, subsample  # noqa: F401

#                     kind     C    E  W    B  causal  table
CORE = {
    "w2": ("cross", 32, 2, 2, 1, False, "pos"),
    "w2_causal": ("cross", 32, 2, 2, 1, True, "pos"),
    "w17_self": ("self", 128, 8, 17, 3, False, "pos"),
    "w17_self_causal": ("self", 128, 8, 17, 3, True, "pos"),
    "w17_cross": ("cross", 128, 8, 17, 3, False, "pos"),
    "w17_cross_causal": ("cross", 128, 8, 17, 3, True, "pos"),
    "w17_cross_nopos": ("cross", 128, 8, 17, 3, False, "none"),
    "w17_cross_flip": ("cross", 128, 8, 17, 3, False, "flip"),
    "w65_causal": ("cross", 32, 2, 65, 2, True, "pos"),
    "w320_causal": ("cross", 128, 8, 320, 2, True, "pos"),
}
CORE_GPU_ONLY = ("w320_causal",)
#                 hidden heads layers H  W
TRANSFORMER = {
    "t17": (128, 8, 2, 3, 17),
    "t33": (32, 2, 2, 4, 33),
    "t70": (128, 8, 6, 2, 70),
    "t17b": (128, 8, 2, 3, 17),        # the parameters of t17, other features: the second sample of the N = 2 test
}
TRANSFORMER_GPU_ONLY = ("t70",)
PARAMETERS_OF = {"t17b": "t17"}
SEEDS = {tag: 7000 + 40 * k for k, tag in enumerate(list(CORE) + list(TRANSFORMER))}


def parameter_seed(tag):
    return SEEDS[PARAMETERS_OF.get(tag, tag)]


def normal(shape, seed, stream=0):
    """Near-normal, unit variance: three uniform fields summed."""
    return sum(synthetic_tensor(shape, seed, stream=3 * stream + k) for k in range(3)) / 3.0 ** 0.5


def sine_table(W, C, dtype=torch.float32):
    """The relative sine encoding of reference pos_encoder.py for a full-resolution row of W columns: [2W-1, C], fp32 like the
    reference forms it (also in an fp64 run, where it is cast afterwards)."""
    dist = torch.linspace(W - 1, -W + 1, 2 * W - 1, dtype=torch.float32)
    dim_t = torch.arange(C, dtype=torch.float32)
    dim_t = 10000 ** (2 * (dim_t // 2) / C)
    pos = dist[:, None] / dim_t
    return torch.stack((pos[:, 0::2].sin(), pos[:, 1::2].cos()), dim=2).flatten(1).to(dtype)


def fill_parameters(module, seed):
    """Seeded, by parameter name: matrices N(0, 1) / sqrt(fan_in), LayerNorm weights 1 + 0.1 N(0, 1), biases 0.3 N(0, 1)."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            x = normal(tuple(p.shape), seed, stream=zlib.crc32(name.encode()) % 100003)
            if p.dim() >= 2:
                x = x * p.shape[-1] ** -0.5
            elif name.endswith("weight"):
                x = 1.0 + 0.1 * x
            else:
                x = 0.3 * x
            p.copy_(x.to(p.dtype))
    return module


def core_inputs(tag):
    """dict: query, key [W, B, C] (self: the same tensor), pos [2W-1, C] or None, g_vo [W, B, C], g_raw [B, W, W]"""
    kind, C, E, W, B, causal, table = CORE[tag]
    seed = SEEDS[tag]
    query = normal((W, B, C), seed, 1)
    pos = None if table == "none" else sine_table(W, C)
    return {"query": query, "key": query if kind == "self" else normal((W, B, C), seed, 2),
            "pos": torch.flip(pos, [0]).contiguous() if table == "flip" else pos,
            "g_vo": normal((W, B, C), seed, 3), "g_raw": normal((B, W, W), seed, 4)}


def core_layout(tag):
    """[(key, shape)] of a core record in storage order; the gradients are those of sum(v_o g_vo) + sum(finite raw_attn g_raw)."""
    kind, C, E, W, B, causal, table = CORE[tag]
    rec = [("v_o", (W, B, C)), ("raw_attn", (B, W, W)), ("attn", (B, W, W)), ("g_query", (W, B, C))]
    if kind == "cross":
        rec.append(("g_key", (W, B, C)))
    return rec + [("g_in_proj_weight", (3 * C, C)), ("g_in_proj_bias", (3 * C,)), ("g_out_proj.weight", (C, C)), ("g_out_proj.bias", (C,))]


def transformer_inputs(tag):
    """dict: feat_left, feat_right [1, C, H, W], pos [2W-1, C], g_attn [1, H, W, W]"""
    C, E, L, H, W = TRANSFORMER[tag]
    seed = SEEDS[tag]
    return {"feat_left": normal((1, C, H, W), seed, 1), "feat_right": normal((1, C, H, W), seed, 2), "pos": sine_table(W, C),
            "g_attn": normal((1, H, W, W), seed, 3)}


def transformer_parameters(tag):
    """[(name, shape)] in state-dict order; `norm.*` (last) receive no gradient in the reference."""
    C, E, L, H, W = TRANSFORMER[tag]
    attn = [("in_proj_weight", (3 * C, C)), ("in_proj_bias", (3 * C,)), ("out_proj.weight", (C, C)), ("out_proj.bias", (C,))]
    norm = lambda n: [(n + ".weight", (C,)), (n + ".bias", (C,))]  # noqa: E731
    names = []
    for layer in range(L):
        names += [(f"self_attn_layers.{layer}.self_attn.{k}", s) for k, s in attn] + [(f"self_attn_layers.{layer}.{k}", s) for k, s in norm("norm1")]
    for layer in range(L):
        names += [(f"cross_attn_layers.{layer}.cross_attn.{k}", s) for k, s in attn]
        names += [(f"cross_attn_layers.{layer}.{k}", s) for k, s in norm("norm1") + norm("norm2")]
    return names + norm("norm")


def transformer_layout(tag):
    """[(key, shape)]: attn_weight, the two feature gradients and every parameter gradient but `norm.*` (absent: None)."""
    C, E, L, H, W = TRANSFORMER[tag]
    rec = [("attn_weight", (1, H, W, W)), ("g_feat_left", (1, C, H, W)), ("g_feat_right", (1, C, H, W))]
    return rec + [("g:" + n, s) for n, s in transformer_parameters(tag) if not n.startswith("norm.")]
