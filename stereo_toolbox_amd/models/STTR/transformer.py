"""STTR's transformer (reference models/STTR/transformer.py): alternating self and cross attention over the image rows, the
attention cores on csrc/sttr_attention.hip.  Same classes, signatures and state-dict keys.  Differences:
  * no torch.utils.checkpoint: the fused attention saves nothing matrix-sized, so there is nothing to trade for recomputation;
  * only the last layer's left update asks for raw_attn, and the head-averaged softmax is never formed;
  * the left / right split of the concatenated features is at H * N (the reference splits at H, which only holds for N = 1).
"""
import copy
from typing import Optional

import torch
from torch import Tensor, nn

from .attention import MultiheadAttentionRelative, causal_mask


def get_clones(module, n):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(n)])


class TransformerSelfAttnLayer(nn.Module):
    def __init__(self, hidden_dim: int, nhead: int):
        super().__init__()
        self.self_attn = MultiheadAttentionRelative(hidden_dim, nhead)
        self.norm1 = nn.LayerNorm(hidden_dim)

    def forward(self, feat: Tensor, pos: Optional[Tensor] = None, pos_indexes: Optional[Tensor] = None):
        """feat [W, 2HN, C], pos [2W-1, C] -> feat + self-attention of its normalised rows"""
        feat2 = self.norm1(feat)
        feat2 = self.self_attn(query=feat2, key=feat2, value=feat2, pos_enc=pos, pos_indexes=pos_indexes, need_attn=False,
                               need_raw=False)[0]
        return feat + feat2


class TransformerCrossAttnLayer(nn.Module):
    def __init__(self, hidden_dim: int, nhead: int):
        super().__init__()
        self.cross_attn = MultiheadAttentionRelative(hidden_dim, nhead)
        self.norm1 = nn.LayerNorm(hidden_dim)
        self.norm2 = nn.LayerNorm(hidden_dim)

    def forward(self, feat_left: Tensor, feat_right: Tensor, pos: Optional[Tensor] = None, pos_indexes: Optional[Tensor] = None,
                last_layer: Optional[bool] = False):
        """feat_left, feat_right [W, HN, C] -> (the updated features concatenated [W, 2HN, C], raw_attn [HN, W, W] of the left
        update in the last layer, else None)"""
        left2, right2 = self.norm1(feat_left), self.norm1(feat_right)
        # the right image attends to the left one: relative positions mirrored
        pos_flipped = None if pos is None else torch.flip(pos, [0])
        feat_right = feat_right + self.cross_attn(query=right2, key=left2, value=left2, pos_enc=pos_flipped, pos_indexes=pos_indexes,
                                                  need_attn=False, need_raw=False)[0]
        # the left image attends to the updated right one; in the last layer a left pixel sees no right pixel beyond itself
        mask = self._generate_square_subsequent_mask(feat_left.size(0), feat_left.device) if last_layer else None
        right2 = self.norm2(feat_right)
        left2, _, raw_attn = self.cross_attn(query=left2, key=right2, value=right2, attn_mask=mask, pos_enc=pos, pos_indexes=pos_indexes,
                                             need_attn=False, need_raw=bool(last_layer))
        feat_left = feat_left + left2
        return torch.cat([feat_left, feat_right], dim=1), raw_attn

    @torch.no_grad()
    def _generate_square_subsequent_mask(self, sz: int, device=None):
        return causal_mask(sz, device)


class Transformer(nn.Module):
    """Self (within an image) and cross (between the images) attention, `num_attn_layers` times."""

    def __init__(self, hidden_dim: int = 128, nhead: int = 8, num_attn_layers: int = 6):
        super().__init__()
        self.self_attn_layers = get_clones(TransformerSelfAttnLayer(hidden_dim, nhead), num_attn_layers)
        self.cross_attn_layers = get_clones(TransformerCrossAttnLayer(hidden_dim, nhead), num_attn_layers)
        self.norm = nn.LayerNorm(hidden_dim)                             # (unused by the reference's forward as well: a state-dict key)
        self.hidden_dim, self.nhead, self.num_attn_layers = hidden_dim, nhead, num_attn_layers

    def _alternating_attn(self, feat: Tensor, pos_enc: Optional[Tensor], pos_indexes: Optional[Tensor], hn: int):
        attn_weight = None
        for idx, (self_attn, cross_attn) in enumerate(zip(self.self_attn_layers, self.cross_attn_layers)):
            feat = self_attn(feat, pos_enc, pos_indexes)
            feat, attn_weight = cross_attn(feat[:, :hn], feat[:, hn:], pos_enc, pos_indexes, idx == self.num_attn_layers - 1)
        return attn_weight

    def forward(self, feat_left: Tensor, feat_right: Tensor, pos_enc: Optional[Tensor] = None):
        """feat_left, feat_right [N, C, H, W], pos_enc [2W-1, C] or None -> the raw cross attention [N, H, W, W] (dim 2 the left
        position, dim 3 the right one; -inf where right > left)"""
        bs, c, h, w = feat_left.shape
        feat_left = feat_left.permute(1, 3, 2, 0).flatten(2).permute(1, 2, 0)        # [W, HN, C], row index h * N + n
        feat_right = feat_right.permute(1, 3, 2, 0).flatten(2).permute(1, 2, 0)
        attn_weight = self._alternating_attn(torch.cat([feat_left, feat_right], dim=1), pos_enc, None, h * bs)
        return attn_weight.view(h, bs, w, w).permute(1, 0, 2, 3)


def build_transformer(args):
    return Transformer(hidden_dim=args.channel_dim, nhead=args.nheads, num_attn_layers=args.num_attn_layers)
