"""FoundationStereo's initial cost volume on the HIP kernels -- drop-in functions of reference
models/FoundationStereo/submodule.py:388-427 and the four lines of `FoundationStereo.forward` that build the combined volume
(foundation_stereo.py:243-248).  NOT the same arithmetic as the IGEV / MonSter volume (VERDICT r5 "Missing" 2):

  * `groupwise_correlation` is a per-group COSINE similarity: both maps are L2-normalised over each group's channels at every
    pixel (`F.normalize(fea.float(), dim=2)`, eps 1e-12) and the products are SUMMED, not averaged; the reference computes it
    outside autocast in fp32 (:394-395) -- so does this (ops.fp32_region);
  * `build_concat_volume` leaves the LEFT half unmasked (:418-424, like ACVNet's), the right half is the shifted copy.

The norm of a pixel does not depend on the disparity, so the normalised volume is the plain group-wise correlation volume of the
two normalised maps: one HBM-bound pre-pass per map (csrc/group_normalize.hip), then the MFMA builder (20 / 28 channels per
group for the 160 / 224-channel maps of the vitb / vitl backbones, 16 for vits).

Behind the volume, `Conv3dNormActReduced` -- the "axial-planar convolution" that makes up twelve layers of the reference's
`hourglass` (foundation_stereo.py:46-124) -- runs on csrc/conv3d_axial.hip, and the disparity transformer of its 1/16 branch
(`CostVolumeDisparityAttention` with its layer classes; the reference needs the `flash_attn` package for it) on
csrc/disp_attention.hip: all layers in one launch, dropout drawn inside the kernel.  NOT built: the two ends of that branch
(`conv_patch` and the trilinear upsampling), the composed `hourglass` / `corr_stem` / `classifier` (the classifier's 7x7x7
convolution is another unsupported shape), attention windows other than (-1, -1), the GRU update block and the DepthAnything
backbone.  `corr_stem` etc. take the dense NDHWC volume of `init_comb_volume` through aggregation.conv_block like the IGEV
aggregation does.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...aggregation import axial_conv_block


def groupwise_correlation(fea1, fea2, num_groups):
    """reference FoundationStereo/submodule.py:388-397 -> [B, G, H, W]: sum_c normalize(fea1)[g,c] * normalize(fea2)[g,c]."""
    B, C, H, W = fea1.shape
    assert C % num_groups == 0, f"C:{C}, num_groups:{num_groups}"
    cost = ops.cost_volume(fea1, fea2, None, None, 1, num_groups, normalize=True)          # [B,1,H,W,G]
    cost = cost.reshape(B, H, W, num_groups).permute(0, 3, 1, 2)
    assert cost.shape == (B, num_groups, H, W)
    return cost


def build_gwc_volume(refimg_fea, targetimg_fea, maxdisp, num_groups, stride=1):
    """reference :399-413 -> [B, G, D, H, W] (zero where w < d); `stride` is accepted and unused, as in the reference."""
    B, C, H, W = refimg_fea.shape
    assert C % num_groups == 0, f"C:{C}, num_groups:{num_groups}"
    return ops.to_ncdhw(ops.cost_volume(refimg_fea, targetimg_fea, None, None, maxdisp, num_groups, normalize=True))


def build_concat_volume(refimg_fea, targetimg_fea, maxdisp):
    """reference :416-427 -> [B, 2C, D, H, W]: left half = the left map at every disparity (NOT masked), right half shifted."""
    return ops.to_ncdhw(ops.cost_volume(None, None, refimg_fea, targetimg_fea, maxdisp, 0, mask_left=False))


def disparity_regression(x, maxdisp):
    """reference FoundationStereo/submodule.py `disparity_regression`: sum_d d * x[b,d,h,w], keepdim -> [B,1,H,W]."""
    return ops.softargmax(x, maxdisp, keepdim=True)


def init_comb_volume(features_left, features_right, left_tmp, right_tmp, max_disp, cv_group=8):
    """foundation_stereo.py:243-248 in one pass: cat(build_gwc_volume(features[0]), build_concat_volume(proj_cmb(features[0])))
    written straight into the dense channels-last volume [B, max_disp/4, H/4, W/4, cv_group + 2 * 12] that `corr_stem` reads
    (`ops.to_ncdhw` gives the reference's [B, C, D, H, W] view)."""
    return ops.cost_volume(features_left, features_right, left_tmp, right_tmp, max_disp // 4, cv_group, mask_left=False,
                           normalize=True)


class Conv3dNormActReduced(nn.Module):
    """reference FoundationStereo/submodule.py:89-114: Conv3d (1,k,k) + norm + ReLU, then Conv3d (kernel_disp,1,1) + norm + ReLU,
    both convolutions with a bias -- same signature, same state-dict keys (`conv1.0.weight`, `conv1.0.bias`, `conv1.1.*`,
    `conv2.0.*`, `conv2.1.*`), shapes and order.  The nn modules are parameter containers; the arithmetic runs on the
    axial-planar MFMA kernels (aggregation.axial_conv_block), in fp32 also under autocast.

    Served: kernel_size 3, kernel_disp odd up to 17, stride 1, norm = BatchNorm3d (SyncBatchNorm after conversion).  Anything else
    raises StxError at construction; there is no CPU fallback.

    The gradient of `conv*.0.bias` under a train-mode BatchNorm is analytically zero (the batch mean removes the bias); the
    block returns exact zeros for it, where the reference's autograd leaves rounding noise (1e-14 in fp64).  With eval-mode
    BatchNorm and gradients enabled it is the channel sum of the raw output's gradient."""

    def __init__(self, C_in, C_out, hidden=None, kernel_size=3, kernel_disp=None, stride=1, norm=nn.BatchNorm3d):
        super().__init__()
        if kernel_disp is None:
            kernel_disp = kernel_size
        if hidden is None:
            hidden = C_out
        if stride != 1:
            raise ops.StxError(f"Conv3dNormActReduced: stride {stride} is not served (stride 1 only)")
        if kernel_size != 3:
            raise ops.StxError(f"Conv3dNormActReduced: kernel_size {kernel_size} is not served (3 only)")
        if kernel_disp % 2 != 1 or not 3 <= kernel_disp <= ops.AXIAL_MAX_TAPS:
            raise ops.StxError(f"Conv3dNormActReduced: kernel_disp {kernel_disp} is not served (odd, 3..{ops.AXIAL_MAX_TAPS})")
        if not (isinstance(norm, type) and issubclass(norm, nn.modules.batchnorm._BatchNorm)):
            raise ops.StxError(f"Conv3dNormActReduced: norm {getattr(norm, '__name__', norm)} is not a BatchNorm")
        if max(C_in, hidden, C_out) > ops.AXIAL_MAX_CHANNELS:
            raise ops.StxError(f"Conv3dNormActReduced: more than {ops.AXIAL_MAX_CHANNELS} channels are not served")
        self.conv1 = nn.Sequential(
            nn.Conv3d(C_in, hidden, kernel_size=(1, kernel_size, kernel_size), padding=(0, kernel_size // 2, kernel_size // 2),
                      stride=(1, stride, stride)),
            norm(hidden),
            nn.ReLU(),
        )
        self.conv2 = nn.Sequential(
            nn.Conv3d(hidden, C_out, kernel_size=(kernel_disp, 1, 1), padding=(kernel_disp // 2, 0, 0), stride=(stride, 1, 1)),
            norm(C_out),
            nn.ReLU(),
        )

    def run(self, x):
        """x: dense [B, D, H, W, C] on a ROCm device -> dense [B, D, H, W, C_out]."""
        x = axial_conv_block(x, self.conv1[0], self.conv1[1])
        return axial_conv_block(x, self.conv2[0], self.conv2[1])

    @ops.fp32_region
    def forward(self, x):
        """x: logical [B, C, D, H, W] (any strides; a view of a dense NDHWC tensor costs no copy) -> logical [B, C_out, D, H, W]."""
        if x.dim() != 5:
            raise ops.StxError(f"Conv3dNormActReduced: expected [B, C, D, H, W], got shape {tuple(x.shape)}")
        return ops.to_ncdhw(self.run(ops.to_ndhwc(x)))


# ---------------------------------------------------------------------------------------------------- disparity transformer
def _unbounded(window_size, who):
    if tuple(window_size) != (-1, -1):
        raise ops.StxError(f"{who}: window_size {tuple(window_size)} is not served, only (-1, -1) (attention over every token)")


class PositionalEmbedding(nn.Module):
    """reference FoundationStereo/submodule.py:472-502: the fixed sinusoid table pe [1, max_len, d_model] (sin on the even
    channels, cos on the odd ones, frequencies 10000^(-2i / d_model)), a plain attribute and not a buffer, as there.  `forward`
    adds it to [B, N, D] with stock torch (not a hot path: `CostVolumeDisparityAttention` hands `table()` to the kernel)."""

    def __init__(self, d_model, max_len=512):
        super().__init__()
        position = torch.arange(0, max_len).float().unsqueeze(1)
        div_term = (torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model)).exp()[None]
        pe = torch.zeros(max_len, d_model).float()
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.pe = pe.unsqueeze(0)

    def table(self, length, device, dtype=torch.float32, resize_embed=False):
        """The first `length` rows [length, d_model]; a table that is too short is interpolated (linear, as the reference does)
        with `resize_embed`, and refused without."""
        self.pe = self.pe.to(device).to(dtype)
        pe = self.pe
        if pe.shape[1] < length:
            if not resize_embed:
                raise RuntimeError(f"PositionalEmbedding: {length} tokens, table of {pe.shape[1]} rows (pass resize_embed=True)")
            pe = F.interpolate(pe.permute(0, 2, 1), size=length, mode="linear", align_corners=False).permute(0, 2, 1)
        return pe[0, :length]

    def forward(self, x, resize_embed=False):
        return x + self.table(x.shape[1], x.device, x.dtype, resize_embed)[None]


class FlashMultiheadAttention(nn.Module):
    """reference :198-229: the four projections of a layer -- a parameter container here.  The attention alone is not served:
    it runs inside `FlashAttentionTransformerEncoderLayer`."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.embed_dim = embed_dim
        self.head_dim = embed_dim // num_heads
        if self.head_dim * num_heads != embed_dim:
            raise ops.StxError(f"FlashMultiheadAttention: embed_dim {embed_dim} must be divisible by num_heads {num_heads}")
        self.q_proj = nn.Linear(embed_dim, embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim)
        self.v_proj = nn.Linear(embed_dim, embed_dim)
        self.out_proj = nn.Linear(embed_dim, embed_dim)

    def forward(self, query, key, value, attn_mask=None, window_size=(-1, -1)):
        raise ops.StxError("FlashMultiheadAttention: the attention alone is not served; run FlashAttentionTransformerEncoderLayer (one "
                           "fused layer) or CostVolumeDisparityAttention (all layers in one launch)")


class FlashAttentionTransformerEncoderLayer(nn.Module):
    """reference :233-257, the post-norm encoder layer: same signature, same state-dict keys, shapes and order (`self_attn.{q,k,v,
    out}_proj.*`, `linear1.*`, `linear2.*`, `norm1.*`, `norm2.*`).  The nn modules are parameter containers; the arithmetic is one
    launch of csrc/disp_attention.hip (ops.disp_attention), dropout included, in fp32 also under autocast.
    Served: embed_dim and dim_feedforward multiples of 4 up to 32, head dim <= 8, act = nn.GELU, norm = nn.LayerNorm, sequences of
    at most 32 tokens; anything else raises StxError.  There is no CPU fallback."""

    def __init__(self, embed_dim, num_heads, dim_feedforward, dropout=0.1, act=nn.GELU, norm=nn.LayerNorm):
        super().__init__()
        who = "FlashAttentionTransformerEncoderLayer"
        if act is not nn.GELU:
            raise ops.StxError(f"{who}: act {getattr(act, '__name__', act)} is not served (nn.GELU only)")
        if norm is not nn.LayerNorm:
            raise ops.StxError(f"{who}: norm {getattr(norm, '__name__', norm)} is not served (nn.LayerNorm only)")
        if not ops.disp_attention_served(embed_dim, num_heads, dim_feedforward):
            raise ops.StxError(f"{who}: embed_dim {embed_dim}, {num_heads} heads, dim_feedforward {dim_feedforward} is not served "
                               f"(multiples of 4 up to {ops.DISP_ATTN_MAX_C}, head dim <= {ops.DISP_ATTN_MAX_HEAD_DIM})")
        self.self_attn = FlashMultiheadAttention(embed_dim, num_heads)
        self.act = act()
        self.linear1 = nn.Linear(embed_dim, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, embed_dim)
        self.norm1 = norm(embed_dim)
        self.norm2 = norm(embed_dim)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)

    def tensors(self):
        """The 16 tensors in state-dict order, as ops.disp_attention takes them."""
        a = self.self_attn
        mods = (a.q_proj, a.k_proj, a.v_proj, a.out_proj, self.linear1, self.linear2, self.norm1, self.norm2)
        return [t for m in mods for t in (m.weight, m.bias)]

    def settings(self):
        """(dropout probability, LayerNorm eps): one value each for the whole layer."""
        ps = {self.dropout.p, self.dropout1.p, self.dropout2.p}
        es = {self.norm1.eps, self.norm2.eps}
        if len(ps) != 1 or len(es) != 1:
            raise ops.StxError(f"FlashAttentionTransformerEncoderLayer: one dropout probability and one eps per layer are served, got "
                               f"{sorted(ps)} and {sorted(es)}")
        return ps.pop(), es.pop()

    def forward(self, src, src_mask=None, window_size=(-1, -1)):
        """src [N, L, C] -> [N, L, C]."""
        who = "FlashAttentionTransformerEncoderLayer"
        _unbounded(window_size, who)
        if src.dim() != 3:
            raise ops.StxError(f"{who}: expected [N, L, C], got shape {tuple(src.shape)}")
        p, eps = self.settings()
        return _run_layers(src, None, [self], p, eps, self.training)


def _run_layers(x, pe, layers, p, eps, training):
    seed = None
    if training and p > 0:
        # drawn on the input's device from torch's default generator: torch.manual_seed reproduces a step, nothing is read back
        seed = torch.randint(-2 ** 62, 2 ** 62, (1,), dtype=torch.int64, device=x.device)
    params = [t for layer in layers for t in layer.tensors()]
    return ops.disp_attention(x, pe, params, layers[0].self_attn.num_heads, p=p, seed=seed, training=training, eps=eps)


class CostVolumeDisparityAttention(nn.Module):
    """reference :506-528, the transformer over the disparity axis of the 1/16 volume: same signature, same state-dict keys
    (`sa.{i}.*`, 16 tensors per layer); `pos_embed0.pe` is a plain attribute.  All `num_transformer` layers run in one launch
    that reads the sequences of the channels-last volume in place; `norm_first` is accepted and ignored, as in the reference."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout=0.1, act=nn.GELU, norm_first=False, num_transformer=6, max_len=512,
                 resize_embed=False):
        super().__init__()
        if not 1 <= num_transformer <= ops.DISP_ATTN_MAX_LAYERS:
            raise ops.StxError(f"CostVolumeDisparityAttention: {num_transformer} layers are not served (1..{ops.DISP_ATTN_MAX_LAYERS})")
        self.resize_embed = resize_embed
        self.sa = nn.ModuleList([])
        for _ in range(num_transformer):
            self.sa.append(FlashAttentionTransformerEncoderLayer(embed_dim=d_model, num_heads=nhead, dim_feedforward=dim_feedforward,
                                                                 act=act, dropout=dropout))
        self.pos_embed0 = PositionalEmbedding(d_model, max_len=max_len)

    @ops.fp32_region
    def forward(self, cv, window_size=(-1, -1)):
        """cv: logical [B, C, D, H, W] (a view of a dense NDHWC tensor costs no copy) -> logical [B, C, D, H, W] over a dense
        NDHWC result."""
        who = "CostVolumeDisparityAttention"
        _unbounded(window_size, who)
        if cv.dim() != 5:
            raise ops.StxError(f"{who}: expected [B, C, D, H, W], got shape {tuple(cv.shape)}")
        if not ops.on_device(cv):
            raise ops.StxError(f"{who}: expected a ROCm device tensor, got {cv.device} -- there is no CPU fallback")
        D = cv.shape[2]
        if D > ops.DISP_ATTN_MAX_L:
            raise ops.StxError(f"{who}: {D} disparity tokens are not served (at most {ops.DISP_ATTN_MAX_L})")
        settings = {layer.settings() for layer in self.sa}
        if len(settings) != 1:
            raise ops.StxError(f"{who}: one dropout probability and one eps for all layers are served, got {sorted(settings)}")
        p, eps = settings.pop()
        pe = self.pos_embed0.table(D, cv.device, torch.float32, self.resize_embed)
        return ops.to_ncdhw(_run_layers(ops.to_ndhwc(cv), pe, list(self.sa), p, eps, self.training))
