"""Plain-torch restatements of reference code that more than one test module compares with: the gather form (no grid_sample)
of IGEV's geometry lookup (reference models/IGEVStereo/geometry.py:7-70) and convex upsampling (submodule.py:243-255), and
StereoAnywhere's truncation mask (utils/utils.py:216-238).  A restatement used by a single test module lives in that module.
"""
import math

import torch


def pool(x):
    """avg_pool2d(x, [1, 2], stride=[1, 2]) along the last axis: pairs (2j, 2j+1), an odd tail dropped."""
    n = x.shape[-1] // 2
    return (x[..., 0:2 * n:2] + x[..., 1:2 * n:2]) / 2


def pyramids(geo, f1, f2, levels):
    """geo [B,C,D,H,W], f1 [B,Cf,H,W], f2 [B,Cf,H,W2] -> ([B,H,W,C,D_i]), ([B,H,W,W2_i])"""
    gp = [geo.permute(0, 3, 4, 1, 2)]
    cp = [torch.einsum("aijk,aijh->ajkh", f1, f2)]
    for _ in range(levels - 1):
        gp.append(pool(gp[-1]))
        cp.append(pool(cp[-1]))
    return gp, cp


def sample(rows, x):
    """rows [..., n], x [..., K] positions -> linear interpolation between floor(x) and floor(x) + 1, zero outside [0, n-1]."""
    n = rows.shape[-1]
    x0 = torch.floor(x)
    f = x - x0
    i0 = x0.long()

    def tap(i):
        ok = (i >= 0) & (i < n)
        return torch.gather(rows, -1, i.clamp(0, n - 1)) * ok.to(rows.dtype)
    return (1 - f) * tap(i0) + f * tap(i0 + 1)


def lookup(gp, cp, disp, coords, radius):
    B, _, H, W = disp.shape
    dx = torch.arange(-radius, radius + 1, dtype=disp.dtype, device=disp.device)
    d, c = disp.reshape(B, H, W, 1), coords.reshape(B, H, W, 1)
    out = []
    for i, (g, r) in enumerate(zip(gp, cp)):
        C = g.shape[3]
        xg = (d / 2 ** i + dx).unsqueeze(3).expand(B, H, W, C, 2 * radius + 1)
        out.append(sample(g, xg).reshape(B, H, W, -1))
        out.append(sample(r, c / 2 ** i - d / 2 ** i + dx))
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def upsample(disp_low, wts):
    B, _, h, w = disp_low.shape
    p = torch.nn.functional.pad(disp_low[:, 0], (1, 1, 1, 1))
    out = 0
    for t in range(9):
        tap = p[:, t // 3:t // 3 + h, t % 3:t % 3 + w]
        out = out + wts[:, t] * tap.repeat_interleave(4, 1).repeat_interleave(4, 2)
    return out


def corr1d_pyramid(f1, f2, levels):
    """f1 [B,C,H,W1], f2 [B,C,H,W2] -> [[B,H,W1,W2_i]]: einsum / sqrt(C), then pairwise averages along the last axis
    (reference models/RAFTStereo/corr.py:31-156)."""
    cp = [torch.einsum("aijk,aijh->ajkh", f1, f2) / torch.sqrt(torch.tensor(float(f1.shape[1]), dtype=f1.dtype))]
    for _ in range(levels - 1):
        cp.append(pool(cp[-1]))
    return cp


def convex(flow, mask, f, scale):
    """out[n, d, f y + j, f x + i] = sum_t softmax_t(mask[n, (t f + j) f + i, y, x]) * scale * flow[n, d, y + t/3 - 1, x + t%3 - 1]"""
    N, D, H, W = flow.shape
    s = torch.softmax(mask.view(N, 9, f, f, H, W), dim=1)
    p = torch.nn.functional.pad(scale * flow, (1, 1, 1, 1))
    out = 0
    for t in range(9):
        tap = p[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W]
        out = out + s[:, t].unsqueeze(1) * tap.view(N, D, 1, 1, H, W)
    return out.permute(0, 1, 4, 2, 5, 3).reshape(N, D, f * H, f * W)


def estimates(volume):
    """[B,1,H,W1,W2] -> (disp_l, conf_l, disp_r, conf_r), StereoAnywhere utils/utils.py:112-170 without the repeats and meshgrids"""
    v = volume.squeeze(1)
    W1, W2 = v.shape[2:]
    a1, a2 = torch.arange(W1, dtype=v.dtype), torch.arange(W2, dtype=v.dtype)
    pl, pr = torch.softmax(v, dim=3), torch.softmax(v, dim=2)
    disp_l = a1.view(1, 1, W1) - torch.sum(pl * a2, 3)
    disp_r = torch.sum(pr * a1.view(1, 1, W1, 1), 2) - a2
    conf_l = 1 - (-torch.sum(pl * torch.log2(pl + 1e-6), dim=3) / math.log2(W2))
    conf_r = 1 - (-torch.sum(pr * torch.log2(pr + 1e-6), dim=2) / math.log2(W1))
    return tuple(t.unsqueeze(1) for t in (disp_l, conf_l, disp_r, conf_r))


def _pack(levels_list):
    """pixel-major levels ([rows..., len_i(, C)]) -> the flat pyramid buffer of include/stx_hip.h"""
    return torch.cat([t.reshape(-1) for t in levels_list])


def truncation_mask(disp, conf, conf_th, atten):
    """[B,1,H,W] x 2 -> [B,1,H,W,W], utils/utils.py:216-238"""
    W = disp.shape[3]
    a = torch.arange(W, dtype=disp.dtype)
    c = (conf if conf_th is None else (conf > conf_th).to(disp.dtype)).unsqueeze(4)
    x = (a.view(1, 1, 1, W) - disp).unsqueeze(4) - a.view(1, 1, 1, 1, W)
    return 1 * (1 - c) + c * (torch.sigmoid(x) * (1 - atten) + atten)
