"""STTR's regression head (reference models/STTR/regression_head.py) on the HIP kernels of csrc/sttr_head.hip.

`forward` runs the fused pair (`ops.sttr_regress`): dustbins, Sinkhorn or softmax, the 3-pixel regression, the occlusion, the
ground-truth response and the dustbin responses in one launch and one backward launch; the transported matrix is never written.
`_optimal_transport` / `_softmax` return the dense matrix (`ops.sttr_optimal_transport` / `ops.sttr_softmax`) and the `_compute_*`
methods work on it in plain torch, for callers that use the reference's steps one by one.  `_sinkhorn` is the plain-torch
iteration (forward does not use it).  `_upsample` is plain torch on the device around `cal`, whatever module the caller passes.
The transformer, the tokenizer, the backbone and the `build_*` functions are not part of this package.
"""
import torch
import torch.nn.functional as F
from torch import nn

from ... import ops
from .utilities import batched_index_select, torch_1d_sample

SINKHORN_ITERS = 10                                                      # regression_head.py:244


class RegressionHead(nn.Module):
    """Disparity and occlusion from the last cross-attention; parameters: `phi` (the dustbin cost) and `cal.*`."""

    def __init__(self, cal, ot=True):
        super().__init__()
        self.cal = cal
        self.ot = ot
        self.phi = nn.Parameter(torch.tensor(0.0))

    # -------------------------------------------------------------------------------- the dense steps
    def _compute_unscaled_pos_shift(self, w, device):
        """[1, 1, W, W]: left position minus right position, negative differences as 0"""
        pos = torch.arange(w, dtype=torch.float32, device=device)
        return (pos[:, None] - pos[None, :]).clamp_min(0)[None, None]

    def _compute_low_res_disp(self, pos_shift, attn_weight, occ_mask):
        """attn_weight [N, H, W, W] -> (disparity [N, H, W], window sum [N, H, W, 1]): the first arg-max and its two
        neighbours (0 outside the row), re-normalised by their sum -- by 1, a constant, where occ_mask is set or, without a
        mask, where the sum is below 0.1"""
        W = attn_weight.shape[-1]
        cols = attn_weight.argmax(dim=-1, keepdim=True) + torch.arange(-1, 2, device=attn_weight.device)
        inside = ((cols >= 0) & (cols < W)).to(attn_weight.dtype)
        cols = cols.clamp(0, W - 1)
        taps = torch.gather(attn_weight, -1, cols) * inside
        shifts = torch.gather(pos_shift.to(attn_weight.dtype).expand_as(attn_weight), -1, cols) * inside
        norm = taps.sum(-1, keepdim=True)
        forced = norm < 0.1 if occ_mask is None else occ_mask.unsqueeze(-1)
        norm = torch.where(forced, torch.ones_like(norm), norm)
        return (taps / norm * shifts).sum(-1), norm

    def _compute_low_res_occ(self, matched_attn):
        return (1.0 - matched_attn).squeeze(-1)

    @staticmethod
    def _target(scale, sampled_cols, sampled_rows, disp):
        """[N, H', W', 1]: the ground-truth right position of every sampled pixel in low-resolution columns"""
        w = disp.shape[-1]
        target = (torch.linspace(0, w - 1, w)[None].to(disp.device) - disp).unsqueeze(-1)
        if sampled_cols is not None:
            target = batched_index_select(target, 2, sampled_cols)
        if sampled_rows is not None:
            target = batched_index_select(target, 1, sampled_rows)
        return target / scale

    def _compute_gt_location(self, scale, sampled_cols, sampled_rows, attn_weight, disp):
        target = self._target(scale, sampled_cols, sampled_rows, disp)
        return torch_1d_sample(attn_weight, target, "linear"), target

    def _upsample(self, x, disp_pred, occ_pred, scale):
        """Low-resolution predictions -> (adjusted disparity, raw upsampled disparity, occlusion) at the size of x.left"""
        h, w = x.left.shape[2:]
        disp_attn = disp_pred * scale
        disp_up = F.interpolate(disp_attn[None], size=(h, w), mode="nearest")
        occ_up = F.interpolate(occ_pred[None], size=(h, w), mode="nearest")
        if self.cal is None:
            return disp_up.squeeze(1).squeeze(1), disp_attn.squeeze(1).squeeze(1), occ_up.squeeze(1)
        mean, std = disp_up.mean(), disp_up.std() + 1e-6
        disp_adj, occ_adj = self.cal((disp_up - mean) / std, (occ_up - 0.5) / 0.5, x.left)
        return (disp_adj * std + mean).squeeze(1), disp_attn.squeeze(1), occ_adj.squeeze(1)

    def _sinkhorn(self, attn, log_mu, log_nu, iters):
        """Log-space Sinkhorn scaling of attn [N, H, W+1, W+1], columns first: rows end up summing to mu"""
        u = torch.zeros_like(log_mu)
        v = torch.zeros_like(log_nu)
        for _ in range(iters):
            v = log_nu - torch.logsumexp(attn + u.unsqueeze(3), dim=2)
            u = log_mu - torch.logsumexp(attn + v.unsqueeze(2), dim=3)
        return attn + u.unsqueeze(3) + v.unsqueeze(2)

    def _optimal_transport(self, attn, iters):
        """attn [N, H, W, W] -> the transported matrix with dustbins [N, H, W+1, W+1] (dense HIP pair)"""
        return ops.sttr_optimal_transport(attn, self.phi, iters)

    def _softmax(self, attn):
        """attn [N, H, W, W] -> the row softmax with dustbins [N, H, W+1, W+1] (dense HIP pair)"""
        return ops.sttr_softmax(attn, self.phi)

    # -------------------------------------------------------------------------------- the fused head
    def forward(self, attn_weight, x):
        """attn_weight [N, H, W, W] raw attention, x a NestedTensor -> the reference's dictionary"""
        output = {}
        cols, rows = x.sampled_cols, x.sampled_rows
        scale = x.left.size(-1) / float(cols.size(-1)) if cols is not None else 1.0
        target = None
        if x.disp is not None:
            target = self._target(scale, cols, rows, x.disp).squeeze(-1)
        occ_mask, occ_mask_right = x.occ_mask, x.occ_mask_right
        if occ_mask is not None:
            if cols is not None:
                occ_mask = batched_index_select(occ_mask, 2, cols)
                occ_mask_right = batched_index_select(occ_mask_right, 2, cols)
            if rows is not None:
                occ_mask = batched_index_select(occ_mask, 1, rows)
                occ_mask_right = batched_index_select(occ_mask_right, 1, rows)
        disp, occ, gt_response, bin_left, bin_right, _ = ops.sttr_regress(attn_weight, self.phi, self.ot, SINKHORN_ITERS,
                                                                         occ_mask, target)
        output["gt_response"] = gt_response
        output["gt_response_occ_left"] = bin_left[occ_mask] if occ_mask is not None else None
        output["gt_response_occ_right"] = bin_right[occ_mask_right] if occ_mask is not None else None
        if cols is not None:
            output["disp_pred"], output["disp_pred_low_res"], output["occ_pred"] = self._upsample(x, disp, occ, scale)
        else:
            output["disp_pred"], output["occ_pred"] = disp, occ
        return output
