"""Plain-torch restatements of reference code that more than one test module compares with: the gather form (no grid_sample)
of IGEV's geometry lookup (reference models/IGEVStereo/geometry.py:7-70) and convex upsampling (submodule.py:243-255), and
StereoAnywhere's truncation mask (utils/utils.py:216-238), STTR's attention with relative positions (models/STTR/attention.py) and its
matching head (models/STTR/regression_head.py), the encoder layers of FoundationStereo's disparity transformer (submodule.py
`FlashAttentionTransformerEncoderLayer`).  A restatement used by a single test module lives in that module.
"""
import math

import torch
import torch.nn.functional as F

from tests.golden.sttr_config import SCALE as STTR_SCALE


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


# ------------------------------------------------------------------------------------------ STTR: attention
NINF = float("-inf")


def relative_index(W, device=None):
    """[W * W]: the row (W - 1 - w) + v of the [2W-1] positional table that the pair (query w, key v) reads"""
    return (torch.arange(W - 1, -1, -1, device=device).view(W, 1) + torch.arange(W, device=device).view(1, W)).view(-1)


def attention_core(q, k, v, q_r, k_r, causal):
    """STTR's attention between the projections (reference models/STTR/attention.py): q (scaled), k, v [W, B, E, hd]; q_r, k_r
    [W, W, E, hd] the projected positional rows of every pair, or both None -> (o [W, B, E, hd], softmax [B, E, W, W], the scores
    [B, E, W, W] with -inf above the diagonal when causal)."""
    W, B, E, hd = q.shape
    attn = torch.einsum("wnec,vnec->newv", q, k)
    if q_r is not None:
        attn = attn + torch.einsum("wnec,wvec->newv", q, k_r) + torch.einsum("vnec,wvec->newv", k, q_r)
    if causal:
        attn = attn + torch.triu(torch.full((W, W), NINF, dtype=attn.dtype, device=attn.device), 1)
    raw = attn
    attn = F.softmax(attn, dim=-1)
    v_o = torch.bmm(attn.view(B * E, W, W), v.permute(1, 2, 0, 3).reshape(B * E, W, hd))
    return v_o.reshape(B, E, W, hd).permute(2, 0, 1, 3), attn, raw


def attention(form, P, prefix, query, key, causal, pos, E):
    """One MultiheadAttentionRelative call with key = value -> (v_o, attn, raw_attn).  P: parameters by name."""
    W, B, C = query.shape
    hd = C // E
    w_in, b_in = P[prefix + "in_proj_weight"], P[prefix + "in_proj_bias"]
    if query is key:
        q, k, v = F.linear(query, w_in, b_in).chunk(3, dim=-1)
    else:
        q = F.linear(query, w_in[:C], b_in[:C])
        k, v = F.linear(key, w_in[C:], b_in[C:]).chunk(2, dim=-1)
    scaling = float(hd) ** -0.5
    q = (q * scaling).contiguous().view(W, B, E, hd)
    k, v = k.contiguous().view(W, B, E, hd), v.contiguous().view(W, B, E, hd)
    q_r = k_r = None
    if pos is not None:
        idx = relative_index(W, query.device)
        if form == "stock":
            q_r, k_r = F.linear(torch.index_select(pos, 0, idx).view(W, W, -1), w_in[:2 * C], b_in[:2 * C]).chunk(2, dim=-1)
            q_r, k_r = (q_r * scaling).contiguous().view(W, W, E, hd), k_r.contiguous().view(W, W, E, hd)
        else:
            q_r = (F.linear(pos, w_in[:C], b_in[:C]) * scaling)[idx].view(W, W, E, hd)
            k_r = F.linear(pos, w_in[C:2 * C], b_in[C:2 * C])[idx].view(W, W, E, hd)
    v_o, attn, raw = attention_core(q, k, v, q_r, k_r, causal)
    v_o = F.linear(v_o.reshape(W, B, C), P[prefix + "out_proj.weight"], P[prefix + "out_proj.bias"])
    return v_o, attn.sum(dim=1) / E, raw.sum(dim=1)


# ------------------------------------------------------------------------------------------ STTR: matching head
def constants(W):
    """log mu = log nu and log 2W: fp32 host tensors, in an fp64 run as well"""
    return (torch.cat([torch.ones(W), torch.tensor([W]).float()]) / (2 * W)).log(), torch.log(torch.tensor([2.0 * W]))


def transported(attn, phi, ot, iters):
    """[N, H, W, W] -> P [N, H, W+1, W+1]"""
    N, H, W, _ = attn.shape
    S = torch.cat([torch.cat([attn, phi.expand(N, H, W, 1)], -1), phi.expand(N, H, 1, W + 1)], -2)
    if not ot:
        return torch.softmax(S, dim=-1)
    lm, l2w = constants(W)
    u = torch.zeros(N, H, W + 1, dtype=attn.dtype)
    for _ in range(iters):
        v = lm - torch.logsumexp(S + u.unsqueeze(3), dim=2)
        u = lm - torch.logsumexp(S + v.unsqueeze(2), dim=3)
    return (S + u.unsqueeze(3) + v.unsqueeze(2) + l2w).exp()


def target_of(disp_gt):
    """full-resolution ground truth [N, 3H, 3W] -> the right position of every sampled pixel in low-resolution columns"""
    w = disp_gt.shape[-1]
    return (torch.arange(w, dtype=torch.float32) - disp_gt)[..., 1::STTR_SCALE, 1::STTR_SCALE] / float(STTR_SCALE)


def regress(P, mask, target):
    """P [N, H, W+1, W+1] -> the five outputs ('gt' only with a target) and 'norm', the arg-max and where norm was forced.  The steps come in
    the order of the reference's forward (ground-truth response, regression, dustbins): autograd then adds the gradients that
    meet in P in the same order, and the fp32 run agrees with the reference's to the last bit or two."""
    inner = P[..., :-1, :-1]
    W = inner.shape[-1]
    out = {}
    if target is not None:
        t = target.to(P.dtype).unsqueeze(-1)
        left, right = torch.floor(t).long().clamp(0, W - 1), torch.ceil(t).long().clamp(0, W - 1)
        w_right = t - left
        out["gt"] = (torch.gather(inner, -1, left) * (1 - w_right) + torch.gather(inner, -1, right) * w_right).squeeze(-1)
    cols = inner.argmax(-1, keepdim=True) + torch.arange(-1, 2)
    inside = ((cols >= 0) & (cols < W)).to(P.dtype)
    taps = torch.gather(inner, -1, cols.clamp(0, W - 1)) * inside
    shift = (torch.arange(W).view(W, 1) - cols).clamp_min(0).to(torch.float32) * inside.float()
    raw = taps.sum(-1, keepdim=True)
    forced = mask.unsqueeze(-1) if mask is not None else raw.detach() < 0.1
    norm = torch.where(forced, torch.ones_like(raw), raw)
    out["disp"] = (taps / norm * shift).sum(-1)
    out["occ"] = (1.0 - norm).squeeze(-1)
    out["norm"] = norm.squeeze(-1)
    out["bin_l"], out["bin_r"] = P[..., :-1, -1], P[..., -1, :-1]
    return out, cols[..., 1], forced.squeeze(-1)


# ------------------------------------------------------------------------------------------ FoundationStereo: disparity transformer
DISP_ENCODER_MISSES = ("unbiased", "tanh_gelu", "over_hd", "pe_every_layer", "pre_norm", "query_softmax", "site1_at_site2")


def disp_encoder(x, pe, params, heads, eps=1e-5, masks=None, scale=1.0, norm_inputs=None, miss=None):
    """The layers in plain torch, any dtype.  x [N, L, C]; params: 16 tensors per layer in state-dict order; masks: None or
    [layers, 3, N, L, max(C, ff)] keep decisions, applied with `scale` = 1 / (1 - p).  `norm_inputs`: a list that receives every
    LayerNorm input.  `miss`: None, or one of DISP_ENCODER_MISSES -- a subtly different layer that the parity rule has to refuse
    (unbiased LayerNorm variance; tanh GELU; scores over hd instead of sqrt(hd); pe in front of every layer; pre-norm order;
    soft-max over the query axis; the masks of site 1 used at site 2)."""
    assert miss is None or miss in DISP_ENCODER_MISSES, miss
    N, L, C = x.shape
    hd = C // heads

    def norm(z, g, e):
        if norm_inputs is not None:
            norm_inputs.append(z)
        if miss != "unbiased":
            return F.layer_norm(z, (C,), g, e, eps)
        return (z - z.mean(-1, keepdim=True)) / torch.sqrt(z.var(-1, unbiased=True, keepdim=True) + eps) * g + e
    if pe is not None and miss != "pe_every_layer":
        x = x + pe[None]
    for i in range(len(params) // 16):
        qw, qb, kw, kb, vw, vb, ow, ob, w1, b1, w2, b2, g1, e1, g2, e2 = params[16 * i:16 * i + 16]
        ff = w1.shape[0]

        def drop(t, site, width):
            return t if masks is None else t * (masks[i, site, :, :, :width].to(t.dtype) * scale)

        def attend(t):
            q = F.linear(t, qw, qb).view(N, L, heads, hd).transpose(1, 2)
            k = F.linear(t, kw, kb).view(N, L, heads, hd).transpose(1, 2)
            v = F.linear(t, vw, vb).view(N, L, heads, hd).transpose(1, 2)
            s = q @ k.transpose(-1, -2) / (hd if miss == "over_hd" else math.sqrt(hd))
            a = torch.softmax(s, dim=-2 if miss == "query_softmax" else -1) @ v
            return drop(F.linear(a.transpose(1, 2).reshape(N, L, C), ow, ob), 0, C)

        def feed(t):
            h = F.linear(t, w1, b1)
            h = F.gelu(h, approximate="tanh") if miss == "tanh_gelu" else F.gelu(h)
            return drop(F.linear(drop(h, 1, ff), w2, b2), 1 if miss == "site1_at_site2" else 2, C)
        if pe is not None and miss == "pe_every_layer":
            x = x + pe[None]
        if miss == "pre_norm":
            x = x + attend(norm(x, g1, e1))
            x = x + feed(norm(x, g2, e2))
            continue
        x = norm(x + attend(x), g1, e1)
        x = norm(x + feed(x), g2, e2)
    return x
