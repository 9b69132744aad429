"""STTR's attention with relative positional encoding (reference models/STTR/attention.py) on csrc/sttr_attention.hip.

The reference gathers the [2W-1, C] table into [W, W, C] with `pos_indexes`, projects that and forms three [B, E, W, W] einsums.
Here the [2W-1, C] table itself is projected (two stock linear layers, so autograd carries the table gradients into
`in_proj_weight` / `in_proj_bias`) and `ops.sttr_rel_attention` reads row (W-1-w) + v of it for the pair (w, v): the product
ASSUMES the reference's index pattern pos_indexes[w, v] = (W-1-w) + v, which is the only one `Transformer` ever builds;
`pos_indexes` itself is accepted and ignored.  The q / k / v, table and output projections stay stock ops (rocBLAS).
"""
import torch
import torch.nn.functional as F
from torch import nn

from ... import ops


def causal_mask(w, device=None):
    """The reference's `_generate_square_subsequent_mask`: [w, w], -inf strictly above the diagonal, 0 elsewhere.  The tensor is
    tagged so that `MultiheadAttentionRelative.forward` recognises it without comparing W x W values."""
    mask = torch.zeros(w, w, device=device).masked_fill_(torch.ones(w, w, dtype=torch.bool, device=device).triu_(1), float("-inf"))
    mask._stx_causal = True
    return mask


class MultiheadAttentionRelative(nn.MultiheadAttention):
    """Multi-head attention with relative positional encoding; the state-dict keys are nn.MultiheadAttention's
    (`in_proj_weight`, `in_proj_bias`, `out_proj.weight`, `out_proj.bias`).  Head dim 16 only (128 / 8, 32 / 2)."""

    def __init__(self, embed_dim, num_heads):
        super().__init__(embed_dim, num_heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None)

    def forward(self, query, key, value, attn_mask=None, pos_enc=None, pos_indexes=None, *, need_attn=True, need_raw=True):
        """query, key, value [W, B, C]; attn_mask None or the upper-triangular -inf mask [W, W] (any other mask is refused);
        pos_enc [2W-1, C] or None -> (v_o [W, B, C], attn [B, W, W] = the softmax averaged over the heads, raw_attn [B, W, W] =
        the scores summed over the heads, -inf where masked).  `attn` is a debugging output without a gradient; need_attn /
        need_raw = False leave the two matrices unwritten (None)."""
        w, bsz, c = query.shape
        heads, hd = self.num_heads, c // self.num_heads
        if hd * heads != c:
            raise ops.StxError(f"MultiheadAttentionRelative: embed_dim {c} is not divisible by num_heads {heads}")
        causal = False
        if attn_mask is not None:
            if tuple(attn_mask.shape) != (w, w) or not (getattr(attn_mask, "_stx_causal", False)
                                                       or torch.equal(attn_mask.float().cpu(), causal_mask(w))):
                raise ops.StxError("MultiheadAttentionRelative: attn_mask must be None or the upper-triangular -inf mask "
                                   f"[{w}, {w}] of the reference's last layer; other masks are not supported")
            causal = True
        wq, wk, wv = self.in_proj_weight[:c], self.in_proj_weight[c:2 * c], self.in_proj_weight[2 * c:]
        bq, bk, bv = self.in_proj_bias[:c], self.in_proj_bias[c:2 * c], self.in_proj_bias[2 * c:]
        scaling = float(hd) ** -0.5
        q = (F.linear(query, wq, bq) * scaling).view(w, bsz, heads, hd)
        k = F.linear(key, wk, bk).view(w, bsz, heads, hd)
        v = F.linear(value, wv, bv).view(w, bsz, heads, hd)
        q_r = k_r = None
        if pos_enc is not None:
            if tuple(pos_enc.shape) != (2 * w - 1, c):
                raise ops.StxError(f"MultiheadAttentionRelative: pos_enc must be [2W-1, C] = [{2 * w - 1}, {c}], got "
                                   f"{tuple(pos_enc.shape)}")
            q_r = (F.linear(pos_enc, wq, bq) * scaling).view(2 * w - 1, heads, hd)
            k_r = F.linear(pos_enc, wk, bk).view(2 * w - 1, heads, hd)
        o, raw, avg = ops.sttr_rel_attention(q, k, v, q_r, k_r, causal, need_raw, need_attn)
        v_o = F.linear(o.reshape(w, bsz, c), self.out_proj.weight, self.out_proj.bias)
        return v_o, avg, raw
