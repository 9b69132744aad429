"""STTR's relative sine encoding (reference models/STTR/pos_encoder.py): a few stock ops under no_grad, any device."""
import math

import torch
from torch import nn


class PositionEncodingSine1DRelative(nn.Module):
    """Sine / cosine features of every relative distance W-1 .. -(W-1): [2W-1, num_pos_feats], sin and cos interleaved."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        self.num_pos_feats, self.temperature, self.normalize = num_pos_feats, temperature, normalize
        self.scale = 2 * math.pi if scale is None else scale

    @torch.no_grad()
    def forward(self, inputs):
        """inputs: a NestedTensor (left [N, C, H, W]; sampled_cols [N, W'] shrinks the width and stretches the distances)"""
        x = inputs.left
        w = x.size(-1) if inputs.sampled_cols is None else inputs.sampled_cols.size(-1)
        dist = torch.linspace(w - 1, -w + 1, 2 * w - 1, dtype=torch.float32, device=x.device)
        if inputs.sampled_cols is not None:
            dist = dist * (x.size(-1) / float(w))
        if self.normalize:
            dist = dist * self.scale
        dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32, device=x.device)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_pos_feats)
        pos = dist[:, None] / dim_t
        return torch.stack((pos[:, 0::2].sin(), pos[:, 1::2].cos()), dim=2).flatten(1)


def no_pos_encoding(x):
    return None


def build_position_encoding(args):
    mode = args.position_encoding
    if mode == "sine1d_rel":
        return PositionEncodingSine1DRelative(args.channel_dim, normalize=False)
    if mode == "none":
        return no_pos_encoding
    raise ValueError(f"not supported {mode}")
