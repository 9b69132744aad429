"""The helpers of reference models/STTR/utilities/misc.py that the regression head uses, restated: plain torch, any device."""
import torch


class NestedTensor(object):
    """The head's input record: the image pair and, optionally, the ground truth and the subsampling index vectors."""

    def __init__(self, left, right, disp=None, sampled_cols=None, sampled_rows=None, occ_mask=None, occ_mask_right=None):
        self.left, self.right = left, right
        self.disp = disp
        self.occ_mask, self.occ_mask_right = occ_mask, occ_mask_right
        self.sampled_cols, self.sampled_rows = sampled_cols, sampled_rows


def batched_index_select(source, dim, index):
    """source [N, ...], index [N, K] -> source with axis `dim` (>= 1) reduced to each batch element's own K indices."""
    shape = [1] * source.dim()
    shape[0], shape[dim] = source.shape[0], -1
    size = list(source.shape)
    size[dim] = index.shape[-1]
    return torch.gather(source, dim, index.view(shape).expand(size))


def torch_1d_sample(source, sample_points, mode="linear"):
    """source [..., L] sampled along its last axis at sample_points [..., 1] -> [...].  'linear': the taps are the floor and
    the ceil clamped to [0, L - 1], the right weight is the point minus the CLAMPED floor (so a point left of 0 extrapolates);
    'sum': the left tap plus the right tap where the point is not an integer."""
    last = source.size(-1) - 1
    left = torch.floor(sample_points).long().clamp(0, last)
    right = torch.ceil(sample_points).long().clamp(0, last)
    if mode == "linear":
        w_right = sample_points - left
        w_left = 1 - w_right
    elif mode == "sum":
        w_right = (right != left).int()
        w_left = 1
    else:
        raise ValueError(f"torch_1d_sample: unknown mode {mode!r}")
    return (torch.gather(source, -1, left) * w_left + torch.gather(source, -1, right) * w_right).squeeze(-1)
