"""Tensor-level host side of the HIP kernels: argument checking, workspaces, autograd.

Everything here launches hand-written gfx950 kernels through the C-ABI (include/stx_hip.h) on the
caller's current HIP stream.  There is no CPU or stock-torch fallback for these ops: tensors that
are not fp32 on a ROCm device raise, and a missing library raises at first use.

Activation convention inside the 3-D path: dense channels-last tensors of shape [B, D, H, W, C]
("NDHWC").  `to_ncdhw` / `to_ndhwc` give zero-copy logical views for the public API.
"""
import ctypes

import torch

from ._capi import StxError, get_lib

_P = ctypes.c_void_p


# --------------------------------------------------------------------------------------- plumbing
class _DevPtr(ctypes.c_void_p):
    """A device pointer that remembers the device of the tensor it came from: _call() reads the launch device off its
    own arguments, so nothing survives between launches (an exception between building the arguments and the launch
    cannot leak state into the next one)."""


def _stream(dev=None):
    return _P(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    if t is None:
        return None
    p = _DevPtr(t.data_ptr())
    p.dev = t.device
    return p


def on_device(t):
    """Whether `t` lives where the kernels of this library run (a ROCm device)."""
    return t.is_cuda


def _chk(t, name, dims=None):
    if t is None:
        return
    if not t.is_cuda:
        raise StxError(f"{name}: expected a ROCm device tensor, got {t.device} -- the cost-volume hot path has "
                       "no CPU fallback (the CPU oracle lives in oracle/ and is test-only)")
    if t.dtype != torch.float32:
        raise StxError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise StxError(f"{name}: expected a dense contiguous tensor, strides {t.stride()}")
    if dims is not None and t.dim() != dims:
        raise StxError(f"{name}: expected {dims} dims, got shape {tuple(t.shape)}")


def _call(name, *args):
    """Launch one C-ABI entry point on the device that OWNS the operands, on that device's current stream
    (`model.to('cuda:1')` without `torch.cuda.set_device(1)` -- the way evaluation/sceneflow_test.py:22 and
    generalization_eval.py use `device=` -- must not launch on cuda:0's stream).  Operands on different devices raise."""
    dev = None
    for a in args:
        if isinstance(a, _DevPtr):
            if dev is None:
                dev = a.dev
            elif a.dev != dev:
                raise StxError(f"{name}: operands live on different devices ({dev} and {a.dev})")
    if dev is not None and dev.type == "cuda" and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            get_lib().call(name, *args, _stream(dev))
    else:
        get_lib().call(name, *args, _stream(dev))


# ------------------------------------------------------------------------- mixed-precision callers
_LOW = (torch.float16, torch.bfloat16)


def _to_fp32(v):
    if isinstance(v, torch.Tensor):
        return v.float() if v.dtype in _LOW else v          # a differentiable cast: the gradient goes back in the caller's dtype
    if isinstance(v, dict):
        return {k: _to_fp32(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_to_fp32(x) for x in v)
    return v


def autocast_active():
    return torch.is_autocast_enabled("cuda") or torch.is_autocast_enabled("cpu")


def fp32_region(fn):
    """The hot path computes in fp32 (north_star; the reference's own FoundationStereo builds its volume outside autocast for
    the same reason, FoundationStereo/submodule.py:388-397).  Under `torch.amp.autocast` -- the reference Trainer's `--amp`,
    trainer/trainer_torchrun.py:219,274,286-294 -- the stock 2-D CNN hands over fp16 / bf16 feature maps: a decorated entry
    point casts its low-precision tensor arguments (also inside dicts / lists) to fp32 and runs with autocast switched off,
    like the operators on autocast's own fp32 list; outputs are fp32.  The casts are ordinary autograd nodes, so a
    `GradScaler`-scaled loss back-propagates through the fp32 kernels and reaches the 2-D CNN in its own dtype.  Outside
    autocast nothing changes: a low-precision tensor is still refused by `_chk` (there is no fp16 kernel to fall back to)."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        if not autocast_active():
            return fn(*args, **kwargs)
        with torch.autocast("cuda", enabled=False), torch.autocast("cpu", enabled=False):
            return fn(*_to_fp32(args), **_to_fp32(kwargs))
    return wrapped


def to_ncdhw(x):
    """[B,D,H,W,C] dense -> logical [B,C,D,H,W] view (channels_last_3d strides, no copy)."""
    return x.permute(0, 4, 1, 2, 3)


def to_ndhwc(x):
    """logical [B,C,D,H,W] (any strides) -> dense [B,D,H,W,C]."""
    return x.permute(0, 2, 3, 4, 1).contiguous()


class _Workspace:
    """Grow-only scratch buffers per (device, stream, tag): wgrad slabs, BN partial sums."""

    def __init__(self):
        self.bufs = {}

    def get(self, tag, nfloats, device):
        # keyed by the launching stream as well: two streams (or autograd threads on different streams) must not
        # share a slab whose contents live from one launch to the next
        sid = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        key = (device.index, sid, tag)
        b = self.bufs.get(key)
        if b is None or b.numel() < nfloats:
            b = torch.empty(int(nfloats), dtype=torch.float32, device=device)
            self.bufs[key] = b
        return b


_WS = _Workspace()


_CACHE_ENABLED = True


def set_weight_cache(enabled):
    """Turn the inference-time caches (packed conv weights, folded eval-mode BatchNorm) on or off.  They are keyed by
    the owner tensors' autograd version counters and storage addresses, which every regular update moves (optimizer
    steps, `load_state_dict`, `copy_`, in-place ops on the parameter).  An in-place edit THROUGH `.data`
    (`p.data.mul_()`, `bn.running_var.data.fill_()`: EMA / weight-surgery code) does not move them: call
    `invalidate_caches(model)` after such edits, or switch the caches off here while doing them."""
    global _CACHE_ENABLED
    _CACHE_ENABLED = bool(enabled)


def invalidate_caches(model):
    """Drop every cached packed weight / folded BatchNorm of `model` (see set_weight_cache)."""
    for m in model.modules():
        m.__dict__.pop("_stx_fold", None)
    for p in model.parameters():
        p.__dict__.pop("_stx_packed", None)


def pack_weight(w, mode, owner=None):
    """Device-side re-layout of a torch conv weight [A][B][k,k,k] into MFMA B-operand order.
    mode 0: conv fwd / deconv dgrad;  1: stride-1 conv dgrad;  2: deconv fwd / stride-2 conv dgrad.
    `owner` (the nn.Parameter) enables caching for inference: the packed copy is stored ON the
    parameter object (so it dies with it -- a dict keyed by data_ptr would hand stale weights to a
    new model whose storage reuses the address) and is refreshed when the version counter moves
    (`.data` edits do not move it: see set_weight_cache / invalidate_caches)."""
    _chk(w, "weight", 5)
    if owner is not None and _CACHE_ENABLED:
        cache = owner.__dict__.setdefault("_stx_packed", {})
        hit = cache.get(mode)
        if hit is not None and hit[0] == (owner._version, owner.data_ptr()):
            return hit[1]
    A, Bd = w.shape[0], w.shape[1]
    T = w.shape[2] * w.shape[3] * w.shape[4]
    K, N = (Bd, A) if mode == 0 else (A, Bd)
    n = get_lib().raw("stx_conv3d_packed_floats")(K, N, T)
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    _call("stx_conv3d_pack_weight", _p(w), _p(wp), A, Bd, T, mode)
    if owner is not None and _CACHE_ENABLED:
        cache[mode] = ((owner._version, owner.data_ptr()), wp)
    return wp


def _pad_channels(t, C):
    """Zero-pad the last (channel) axis of an NDHWC tensor / dim 0 or 1 of a weight."""
    if t.shape[-1] == C:
        return t
    out = t.new_zeros(*t.shape[:-1], C)
    out[..., : t.shape[-1]] = t
    return out


def pad_input_channels(x, w):
    """Zero-pad the channel axis of an NDHWC activation and dim 1 of a conv weight [Cout, Cin, k, k, k] to the next
    multiple of 8 (the implicit-GEMM kernels take K in steps of 8)."""
    Cin = x.shape[-1]
    Cp = (Cin + 7) // 8 * 8
    if Cp == Cin:
        return x, w
    wp = w.new_zeros(w.shape[0], Cp, *w.shape[2:])
    wp[:, :Cin] = w
    return _pad_channels(x, Cp), wp


def pad_weight_channels(w, Cp):
    """Zero-pad dim 1 (input channels) of a conv weight [Cout, Cin, k, k, k] to Cp."""
    if w.shape[1] == Cp:
        return w
    wp = w.new_zeros(w.shape[0], Cp, *w.shape[2:])
    wp[:, : w.shape[1]] = w
    return wp


# --------------------------------------------------------------------------------------- raw convs
def conv_out_dims(D, H, W, ks, stride):
    pad = ks // 2
    return tuple((d + 2 * pad - ks) // stride + 1 for d in (D, H, W))


def conv3d_forward(x, wp, Cout, ks, stride, scale=None, bias=None, residual=None, relu=False, want_stats=False):
    """out = act(conv(x) * scale + bias + residual); optional BN partial sums of the raw output."""
    _chk(x, "x", 5)
    B, D, H, W, Cin = x.shape
    Do, Ho, Wo = conv_out_dims(D, H, W, ks, stride)
    out = torch.empty(B, Do, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    stats = None
    if want_stats:
        rows = get_lib().raw("stx_conv3d_fwd_stat_rows")(B, D, H, W, Cin, Cout, ks, stride)   # (exactly the rows the launch writes)
        stats = torch.empty(rows, 2, Cout, dtype=torch.float32, device=x.device)
    _call("stx_conv3d_fwd", _p(x), _p(wp), _p(out), _p(scale), _p(bias), _p(residual), _p(stats), B, D, H, W, Cin,
          Cout, ks, stride, int(relu))
    return out, stats


def deconv3d_forward(x, wp, Cout, out_dims=None, scale=None, bias=None, residual=None, relu=False, want_stats=False):
    """ConvTranspose3d(k3, s2, p1, op1) (out = 2*in), same fused epilogue as conv3d_forward."""
    _chk(x, "x", 5)
    B, D, H, W, Cin = x.shape
    Do, Ho, Wo = out_dims if out_dims is not None else (2 * D, 2 * H, 2 * W)
    if Cout > 64:
        # The transposed-conv kernel keeps 4 parity-class accumulators per 32-column block and is instantiated for
        # N <= 64.  Wider outputs (PCWNet: ConvTranspose3d(128, 128), dgrad of Conv3d(128, 128, s2)) run as 64-channel
        # slices of the packed weights [tap][K/8][N/32][256] and are concatenated (small 1/16-1/32-resolution volumes).
        if Cout % 64 != 0:
            raise StxError(f"deconv3d_forward: Cout={Cout} > 64 must be a multiple of 64")
        nt = Cout // 32
        wv = wp.view(-1, Cin // 8, nt, 256)
        outs, sts = [], []
        for h in range(Cout // 64):
            sl = slice(64 * h, 64 * h + 64)
            o, st_ = deconv3d_forward(x, wv[:, :, 2 * h:2 * h + 2].contiguous(), 64, (Do, Ho, Wo),
                                      None if scale is None else scale[sl].contiguous(),
                                      None if bias is None else bias[sl].contiguous(),
                                      None if residual is None else residual[..., sl].contiguous(), relu, want_stats)
            outs.append(o)
            sts.append(st_)
        return torch.cat(outs, -1), (torch.cat(sts, -1) if want_stats else None)
    out = torch.empty(B, Do, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    stats = None
    if want_stats:
        nb = get_lib().raw("stx_deconv3d_fwd_blocks")(D, H, W)
        stats = torch.empty(B * nb, 2, Cout, dtype=torch.float32, device=x.device)
    _call("stx_deconv3d_fwd", _p(x), _p(wp), _p(out), _p(scale), _p(bias), _p(residual), _p(stats), B, D, H, W, Cin,
          Cout, Do, Ho, Wo, int(relu))
    return out, stats


def conv3d_wgrad(fine, coarse, ks, stride):
    """G[cc][cf][tap] = sum_o fine[S*o+tap-pad][cf] * coarse[o][cc] (see conv3d.hip)."""
    B, Df, Hf, Wf, CF = fine.shape
    _, Dc, Hc, Wc, CC = coarse.shape
    n = get_lib().raw("stx_conv3d_wgrad_workspace_floats")(B, Dc, Hc, Wc, CF, CC, ks, stride)
    ws = _WS.get("wgrad", n, fine.device)
    dw = torch.empty(CC, CF, ks ** 3, dtype=torch.float32, device=fine.device)
    _call("stx_conv3d_wgrad", _p(fine), _p(coarse), _p(dw), _p(ws), B, Df, Hf, Wf, CF, Dc, Hc, Wc, CC, ks, stride)
    return dw


def conv3d_wgrad_bn(x, gy, pend):
    """Weight gradient of a 3x3x3 stride-1 convolution from the gradient BEHIND its train-mode BatchNorm (+ ReLU): returns
    (dw [CC, CF, 27], dz) -- see stx_conv3d_wgrad_bn.  `pend` = the record BnActFn.backward left (_PendingBn)."""
    B, D, H, W, CF = x.shape
    CC = gy.shape[-1]
    n = get_lib().raw("stx_conv3d_wgrad_workspace_floats")(B, D, H, W, CF, CC, 3, 1)
    ws = _WS.get("wgrad", n, x.device)
    dw = torch.empty(CC, CF, 27, dtype=torch.float32, device=x.device)
    dz = torch.empty_like(gy)
    _call("stx_conv3d_wgrad_bn", _p(x), _p(gy), _p(pend.z), _p(pend.scale), _p(pend.shift), _p(pend.mean), _p(pend.invstd),
          _p(pend.gamma), _p(pend.sums), float(pend.inv_n), int(pend.act), _p(dz), _p(dw), _p(ws), B, D, H, W, CF, CC)
    return dw, dz


class _PendingBn:
    """What BnActFn.backward hands to the backward of the convolution that produced its input when the BatchNorm's
    `bn_bwd_apply` pass is folded into that convolution's weight-gradient kernel (conv_block decides: `defer`): the
    operands of dz = gamma invstd (gy' - sum_g / n - xhat sum_gx / n).  Attached to the gradient tensor it describes."""
    __slots__ = ("g", "z", "scale", "shift", "mean", "invstd", "gamma", "sums", "inv_n", "act")

    def materialize(self):
        """The BatchNorm-backward apply pass on its own (a consumer that cannot fold it: frozen weights, other kernels)."""
        C = self.z.shape[-1]
        nvox = self.z.numel() // C
        dz = torch.empty_like(self.z)
        _call("stx_bn_bwd_apply2", _p(self.g), None, _p(self.z), _p(self.mean), _p(self.invstd), _p(self.gamma), None, None,
              None, None, _p(self.scale), _p(self.shift), None, None, _p(self.sums), _p(dz), None, None, nvox, C, int(self.act), 1)
        return dz


# Safety net of the deferral: a record that no convolution backward consumed means that convolution differentiated the
# UN-normalised gradient.  Every backward pass that defers queues one end-of-pass callback that raises in that case.
_BN_DEFER = {"outstanding": 0, "armed": False}


def _bn_defer_check():
    n, _BN_DEFER["outstanding"], _BN_DEFER["armed"] = _BN_DEFER["outstanding"], 0, False
    if n:
        raise StxError(f"{n} deferred BatchNorm-backward record(s) were not consumed by their convolution's backward node: "
                       "the gradients of this backward pass are wrong (set STX_BN_BWD_IN_WGRAD=0 and report)")


def _defer_pending_bn(g, pend):
    g._stx_pending_bn = pend
    _BN_DEFER["outstanding"] += 1
    if not _BN_DEFER["armed"]:
        _BN_DEFER["armed"] = True
        torch.autograd.Variable._execution_engine.queue_callback(_bn_defer_check)


def bn_defer_reset_if_stale():
    """Called from the FORWARD side of a deferring block (aggregation.conv_block): a backward pass that died with an exception
    after a deferral (out of memory, a user hook) never ran its end-of-pass callback and left the counters armed -- the
    safety net would stay off for the rest of the process.  Outside a backward pass nothing can be legitimately
    outstanding, so the state is reset."""
    if not _BN_DEFER["armed"]:
        return
    task_id = getattr(torch._C, "_current_graph_task_id", None)       # (a private accessor: a torch build without it skips the reset
    if task_id is None or task_id() == -1:                           #  outside-backward check and resets whenever a forward starts)
        _BN_DEFER["outstanding"], _BN_DEFER["armed"] = 0, False


def _take_pending_bn(g):
    """The deferred-BatchNorm record BnActFn.backward attached to gradient tensor `g`, if any (it travels ON the tensor object:
    no global table to leak when a backward pass is interrupted, nothing shared between threads)."""
    pend = getattr(g, "_stx_pending_bn", None) if g is not None else None
    if pend is not None:
        del g._stx_pending_bn
        _BN_DEFER["outstanding"] -= 1
        if pend.g is not g:                        # (cannot happen; a stale record must never be applied to another tensor)
            raise StxError("deferred BatchNorm backward: record attached to a different gradient tensor")
    return pend


def _is_c1(w, ks, stride, transposed):
    """Classifier tail Conv3d(Cin, 1, 3, padding=1): served by the VALU kernels of conv_c1.hip."""
    return (not transposed) and ks == 3 and stride == 1 and w.shape[0] == 1 and w.shape[1] % 16 == 0 and w.shape[1] <= 64


def conv3d_c1_forward(x, w, residual=None):
    """x [B,D,H,W,Cin], w [1,Cin,3,3,3] -> [B,D,H,W,1] (+ residual [B,D,H,W,1])."""
    _chk(x, "x", 5)
    _chk(w, "weight", 5)
    B, D, H, W, Cin = x.shape
    out = torch.empty(B, D, H, W, 1, dtype=torch.float32, device=x.device)
    _call("stx_conv3d_c1_fwd", _p(x), _p(w), _p(residual), _p(out), B, D, H, W, Cin)
    return out


def conv3d_c1_wgrad(x, gy):
    B, D, H, W, Cin = x.shape
    ws = _WS.get("c1wgrad", get_lib().raw("stx_conv3d_c1_wgrad_workspace_floats")(Cin), x.device)
    dw = torch.empty(1, Cin, 3, 3, 3, dtype=torch.float32, device=x.device)
    _call("stx_conv3d_c1_wgrad", _p(x), _p(gy), _p(dw), _p(ws), B, D, H, W, Cin)
    return dw


def conv3d_c1_dgrad(gy, w, Cin):
    """gy [B,D,H,W,1], w [1,Cin,3,3,3] -> gx [B,D,H,W,Cin]."""
    B, D, H, W, _ = gy.shape
    gx = torch.empty(B, D, H, W, Cin, dtype=torch.float32, device=gy.device)
    _call("stx_conv3d_c1_dgrad", _p(gy), _p(w), _p(gx), B, D, H, W, Cin)
    return gx


class ConvRawFn(torch.autograd.Function):
    """z = conv(x, w) (or transposed conv), raw output + BN partial sums; backward = dgrad + wgrad
    on the same MFMA kernels with re-packed weights."""

    @staticmethod
    def forward(ctx, x, w, ks, stride, transposed, want_stats):
        _chk(x, "x", 5)
        ctx.cin_true = None
        ctx.x_prepadded = False
        if not transposed and x.shape[-1] != w.shape[1]:
            # an activation that already carries zero pad channels up to the GEMM-K step (ops.sampled_volume): pad the
            # weight only; the pad channels' input gradient is returned (and ignored by the producer)
            if x.shape[-1] != (w.shape[1] + 7) // 8 * 8:
                raise StxError(f"conv: input has {x.shape[-1]} channels, weight expects {w.shape[1]}")
            ctx.cin_true, ctx.x_prepadded = w.shape[1], True
            w = pad_weight_channels(w, x.shape[-1])
        elif not transposed and x.shape[-1] % 8 != 0:
            # GEMM-K (input channels) in steps of 8: zero-pad odd widths (CFNet's 65- and 33-channel cascade volumes)
            ctx.cin_true = x.shape[-1]
            x, w = pad_input_channels(x, w)
        if _is_c1(w, ks, stride, transposed) and not want_stats:
            z, stats = conv3d_c1_forward(x, w.contiguous()), None
        elif transposed:
            Cout = w.shape[1]
            z, stats = deconv3d_forward(x, pack_weight(w, 2), Cout, want_stats=want_stats)
        else:
            Cout = w.shape[0]
            z, stats = conv3d_forward(x, pack_weight(w, 0), Cout, ks, stride, want_stats=want_stats)
        ctx.save_for_backward(x, w)
        ctx.cfg = (ks, stride, transposed)
        if stats is None:
            stats = x.new_empty(0)
        ctx.mark_non_differentiable(stats)
        return z, stats

    @staticmethod
    def backward(ctx, gz, _gstats):
        x, w = ctx.saved_tensors
        ks, stride, transposed = ctx.cfg
        pend = _take_pending_bn(gz)
        gx = gw = None
        B, D, H, W, Cin = x.shape
        if pend is not None:
            # gz is the gradient BEHIND this convolution's BatchNorm (BnActFn deferred its apply pass): the march weight
            # gradient forms dz itself and writes it for the data gradient below
            if (ctx.needs_input_grad[1] and not transposed and ks == 3 and stride == 1 and ctx.cin_true is None
                    and get_lib().raw("stx_conv3d_wgrad_bn_supported")(B, D, H, W, Cin, w.shape[0])):
                gw_pre, gz = conv3d_wgrad_bn(x, gz, pend)
                gw_pre = gw_pre.reshape(w.shape)
            else:
                gw_pre, gz = None, pend.materialize()
        else:
            gw_pre = None
        gz = gz.contiguous()
        if transposed:
            Ci, Co = w.shape[0], w.shape[1]
            if ctx.needs_input_grad[0]:   # stride-2 conv of gz with the deconv weight read as [Cout'][Cin']
                gx, _ = conv3d_forward(gz, pack_weight(w, 0), Ci, 3, 2)
            if ctx.needs_input_grad[1]:   # the wgrad kernel works on 32-channel pairs: pad CFNet's 16-wide deconvs
                gz_w = gz if Co % 32 == 0 else _pad_channels(gz, (Co + 31) // 32 * 32)
                x_w = x if Ci % 32 == 0 else _pad_channels(x, (Ci + 31) // 32 * 32)
                gw = conv3d_wgrad(gz_w, x_w, 3, 2)[:Ci, :Co].reshape(w.shape)
        else:
            Co, Ci = w.shape[0], w.shape[1]
            c1 = _is_c1(w, ks, stride, transposed)
            gz_k, w_k = gz, w
            if Co % 8 != 0 and not c1:    # pad GEMM-K to 8
                Cp = (Co + 7) // 8 * 8
                gz_k = _pad_channels(gz, Cp)
                w_k = w.new_zeros(Cp, *w.shape[1:])
                w_k[:Co] = w
            if ctx.needs_input_grad[0]:
                if c1:                    # classifier tail Conv3d(32 -> 1): streaming VALU kernel
                    gx = conv3d_c1_dgrad(gz, w.contiguous(), Ci)
                elif stride == 1 and Ci > 128:
                    # the conv kernels produce at most 128 output channels per launch: wide inputs (PCWNet's 192-channel
                    # fusion convs) get their gradient in slices of the weight's input-channel axis
                    parts = []
                    for lo in range(0, Ci, 128):
                        hi = min(Ci, lo + 128)
                        g, _ = conv3d_forward(gz_k, pack_weight(w_k[:, lo:hi].contiguous(), 1), hi - lo, ks, 1)
                        parts.append(g)
                    gx = torch.cat(parts, -1)
                elif stride == 1:
                    gx, _ = conv3d_forward(gz_k, pack_weight(w_k, 1), Ci, ks, 1)
                else:                     # stride-2 dgrad = transposed conv of gz (its kernel takes GEMM-K in steps of 32)
                    if Co % 32:
                        Cp = (Co + 31) // 32 * 32
                        gz_k = _pad_channels(gz, Cp)
                        w_k = w.new_zeros(Cp, *w.shape[1:])
                        w_k[:Co] = w
                    gx, _ = deconv3d_forward(gz_k, pack_weight(w_k, 2), Ci, out_dims=(D, H, W))
            if gw_pre is not None:
                gw = gw_pre
            elif ctx.needs_input_grad[1]:
                if c1:
                    gw = conv3d_c1_wgrad(x, gz)
                else:
                    gz_w = gz if Co % 32 == 0 else _pad_channels(gz, (Co + 31) // 32 * 32)
                    x_w = x if Ci % 32 == 0 else _pad_channels(x, (Ci + 31) // 32 * 32)
                    gw = conv3d_wgrad(x_w, gz_w, ks, stride)[:Co, :Ci].reshape(w.shape)
        if ctx.cin_true is not None:
            if gx is not None and not ctx.x_prepadded:
                gx = gx[..., :ctx.cin_true].contiguous()
            if gw is not None:
                gw = gw[:, :ctx.cin_true].contiguous()
        return gx, gw, None, None, None, None


# ------------------------------------------------------------------- axial-planar convolutions (conv3d_axial.hip)
AXIAL_MAX_CHANNELS = 192
AXIAL_MAX_TAPS = 17


def _axial_kernel(w, who):
    """(kd, kh, kw) of a weight [Cout, Cin, kd, kh, kw] the axial-planar kernels serve: (1,3,3) or (kd,1,1), kd odd, 3..17."""
    if w.dim() != 5:
        raise StxError(f"{who}: expected a weight [Cout, Cin, kd, kh, kw], got shape {tuple(w.shape)}")
    kd, kh, kw = (int(k) for k in w.shape[2:])
    planar = (kd, kh, kw) == (1, 3, 3)
    axial = kh == 1 and kw == 1 and kd % 2 == 1 and 3 <= kd <= AXIAL_MAX_TAPS
    if not (planar or axial):
        raise StxError(f"{who}: kernel {(kd, kh, kw)} is not served -- (1,3,3) or (kd,1,1) with kd odd, 3 <= kd <= {AXIAL_MAX_TAPS}")
    if w.shape[0] > AXIAL_MAX_CHANNELS or w.shape[1] > AXIAL_MAX_CHANNELS:
        raise StxError(f"{who}: {w.shape[1]} -> {w.shape[0]} channels, at most {AXIAL_MAX_CHANNELS} are served")
    return kd, kh, kw


def pack_weight_axial(w, mode, owner=None):
    """Packed copy of a torch weight [A][B][kd,kh,kw] for stx_conv3d_axial_fwd (mode 0: forward, 1: data gradient); cached on
    `owner` like pack_weight."""
    _chk(w, "weight", 5)
    kd, kh, kw = _axial_kernel(w, "pack_weight_axial")
    if owner is not None and _CACHE_ENABLED:
        cache = owner.__dict__.setdefault("_stx_packed", {})
        hit = cache.get(("axial", mode))
        if hit is not None and hit[0] == (owner._version, owner.data_ptr()):
            return hit[1]
    A, Bd = w.shape[0], w.shape[1]
    K, N = (Bd, A) if mode == 0 else (A, Bd)
    n = get_lib().raw("stx_conv3d_axial_packed_floats")(K, N, kd, kh, kw)
    if n <= 0:
        raise StxError(f"pack_weight_axial: GEMM-K {K} (a multiple of 4), N {N}, kernel {(kd, kh, kw)} unsupported")
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    _call("stx_conv3d_axial_pack_weight", _p(w), _p(wp), A, Bd, kd, kh, kw, mode)
    if owner is not None and _CACHE_ENABLED:
        cache[("axial", mode)] = ((owner._version, owner.data_ptr()), wp)
    return wp


def conv3d_axial_forward(x, wp, Cout, kernel, scale=None, bias=None, residual=None, act=0, want_stats=False):
    """out = act(conv(x) * scale + bias + residual) for a (1,3,3) / (kd,1,1) stride-1 "same" convolution of a dense NDHWC
    tensor; optional BatchNorm partial rows of the raw output (exactly the rows the launch writes)."""
    _chk(x, "x", 5)
    B, D, H, W, Cin = x.shape
    kd, kh, kw = kernel
    out = torch.empty(B, D, H, W, Cout, dtype=torch.float32, device=x.device)
    stats = None
    if want_stats:
        rows = get_lib().raw("stx_conv3d_axial_fwd_stat_rows")(B, D, H, W, Cin, Cout, kd, kh, kw)
        stats = torch.empty(rows, 2, Cout, dtype=torch.float32, device=x.device)
    _call("stx_conv3d_axial_fwd", _p(x), _p(wp), _p(out), _p(scale), _p(bias), _p(residual), _p(stats), B, D, H, W, Cin, Cout,
          kd, kh, kw, int(act))
    return out, stats


def conv3d_axial_wgrad(x, gz, kernel):
    """dw [CC, CF, taps] = sum_vox x[vox + t - pad][cf] * gz[vox][cc] (fixed-order reduction of a workspace slab)."""
    B, D, H, W, CF = x.shape
    CC = gz.shape[-1]
    kd, kh, kw = kernel
    n = get_lib().raw("stx_conv3d_axial_wgrad_workspace_floats")(B, D, H, W, CF, CC, kd, kh, kw)
    if n <= 0:
        raise StxError(f"conv3d_axial_wgrad: {CF} x {CC} channels, kernel {kernel} unsupported")
    ws = _WS.get("axwgrad", n, x.device)
    dw = torch.empty(CC, CF, kd * kh * kw, dtype=torch.float32, device=x.device)
    _call("stx_conv3d_axial_wgrad", _p(x), _p(gz), _p(dw), _p(ws), B, D, H, W, CF, CC, kd, kh, kw)
    return dw


def _pad4(C):
    return (C + 3) // 4 * 4


def _axial_prepare(x, w, who):
    """Checks of an axial-planar call and its operands in kernel form: input channels zero-padded to a multiple of 4."""
    _chk(x, "x", 5)
    _chk(w, "weight", 5)
    kernel = _axial_kernel(w, who)
    if x.shape[-1] != w.shape[1]:
        raise StxError(f"{who}: input has {x.shape[-1]} channels, weight expects {w.shape[1]}")
    Cp = _pad4(w.shape[1])
    if Cp != w.shape[1]:
        x, w = _pad_channels(x, Cp), pad_weight_channels(w, Cp)
    return x, w, kernel


def _axial_backward(x, w, kernel, gz, cin_true, need_x, need_w):
    """Data and weight gradient of z = conv(x, w) on the axial-planar kernels (x, w as _axial_prepare left them)."""
    gz = gz.contiguous()
    Co, Ci = w.shape[0], w.shape[1]
    gz_k, w_k = gz, w
    if Co % 4:                          # GEMM-K of the data gradient / the gz operand of the weight gradient in steps of 4
        Cp = _pad4(Co)
        gz_k = _pad_channels(gz, Cp)
        w_k = w.new_zeros(Cp, *w.shape[1:])
        w_k[:Co] = w
    gx = gw = None
    if need_x:
        gx, _ = conv3d_axial_forward(gz_k, pack_weight_axial(w_k, 1), Ci, kernel)
        if Ci != cin_true:
            gx = gx[..., :cin_true].contiguous()
    if need_w:
        gw = conv3d_axial_wgrad(x, gz_k, kernel)[:Co, :cin_true].reshape(Co, cin_true, *kernel)
        if not gw.is_contiguous():
            gw = gw.contiguous()
    return gx, gw


class AxialConvRawFn(torch.autograd.Function):
    """z = conv(x, w) for the (1,3,3) / (kd,1,1) stride-1 convolutions, raw output + BatchNorm partial rows -- the twin of
    ConvRawFn on csrc/conv3d_axial.hip.  x: dense NDHWC; w: the torch parameter [Cout, Cin, kd, kh, kw].  backward = data
    gradient (the forward kernel on flipped / transposed weights) + weight gradient."""

    @staticmethod
    def forward(ctx, x, w, want_stats):
        ctx.cin_true = w.shape[1]
        x, w, kernel = _axial_prepare(x, w, "AxialConvRawFn")
        z, stats = conv3d_axial_forward(x, pack_weight_axial(w, 0), w.shape[0], kernel, want_stats=want_stats)
        ctx.save_for_backward(x, w)
        ctx.kernel = kernel
        if stats is None:
            stats = x.new_empty(0)
        ctx.mark_non_differentiable(stats)
        return z, stats

    @staticmethod
    def backward(ctx, gz, _gstats):
        x, w = ctx.saved_tensors
        gx, gw = _axial_backward(x, w, ctx.kernel, gz, ctx.cin_true, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, None


class _AxialConvBiasFn(torch.autograd.Function):
    """ops.conv3d_axial with a bias under autograd: the bias rides in the forward kernel's epilogue; its gradient is the
    channel sum of gz (a torch reduction)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.cin_true = w.shape[1]
        x, w, kernel = _axial_prepare(x, w, "conv3d_axial")
        z, _ = conv3d_axial_forward(x, pack_weight_axial(w, 0), w.shape[0], kernel, bias=bias.contiguous())
        ctx.save_for_backward(x, w)
        ctx.kernel = kernel
        return z

    @staticmethod
    def backward(ctx, gz):
        x, w = ctx.saved_tensors
        gx, gw = _axial_backward(x, w, ctx.kernel, gz, ctx.cin_true, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        gb = gz.sum((0, 1, 2, 3)) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


class ZeroGradBiasFn(torch.autograd.Function):
    """z unchanged, with `bias` tied into the graph: a convolution bias in front of a batch-statistics BatchNorm cancels in the
    output, its gradient is analytically zero -- returned as exact zeros instead of a volume-sized reduction."""

    @staticmethod
    def forward(ctx, z, bias):
        ctx.save_for_backward(bias)
        return z.view_as(z)

    @staticmethod
    def backward(ctx, gz):
        (bias,) = ctx.saved_tensors
        return gz, torch.zeros_like(bias)


@fp32_region
def conv3d_axial(x, weight, bias=None):
    """Stride-1 "same" Conv3d with a (1,3,3) or (kd,1,1) kernel (kd odd, 3..17) on the gfx950 MFMA kernels, with autograd.
    x: dense channels-last [B, D, H, W, Cin] (`to_ndhwc`); weight: [Cout, Cin, kd, kh, kw]; bias: [Cout] or None.
    Returns [B, D, H, W, Cout].  Raises StxError for CPU tensors, non-fp32 input outside autocast, non-contiguous input and any
    other kernel shape; there is no fallback."""
    _chk(x, "x", 5)
    _chk(weight, "weight", 5)
    _chk(bias, "bias", 1)
    _axial_kernel(weight, "conv3d_axial")
    if bias is not None and bias.shape[0] != weight.shape[0]:
        raise StxError(f"conv3d_axial: bias of {bias.shape[0]} for {weight.shape[0]} output channels")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias)):
        if bias is None:
            return AxialConvRawFn.apply(x, weight, False)[0]
        return _AxialConvBiasFn.apply(x, weight, bias)
    xk, wk, kernel = _axial_prepare(x, weight.detach(), "conv3d_axial")
    return conv3d_axial_forward(xk, pack_weight_axial(wk, 0), weight.shape[0], kernel, bias=None if bias is None else bias.detach())[0]


# ------------------------------------------------------------------------------ ConvGRU cell (convgru.hip)
CONVGRU_MAX_HIDDEN = 128
CONVGRU_MAX_K = 512
CONVGRU_MAX_X = 3            # a launch takes 4 sources: h (or r h) and up to three x
CONVGRU_PACKS = 0            # pack launches so far (tests: a training step packs once per weight and mode, not once per iteration)


def _cl_pitch(t):
    """Pixel pitch in floats if the memory of the logical NCHW tensor `t` is channels-last [B][H][W][pitch >= C] the kernels can
    read in place (a channel slice of a wider map included), else None."""
    B, C, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    if C > 1 and sc != 1:
        return None
    pitch = sw if W > 1 else (sh if H > 1 else (sb if B > 1 else C))      # (the stride of a size-1 dim says nothing)
    if pitch < C or pitch % 4 or t.data_ptr() % 16:
        return None
    if (W > 1 and sw != pitch) or (H > 1 and sh != W * pitch) or (B > 1 and sb != H * W * pitch):
        return None
    return pitch


def _cl_source(t):
    """(tensor, pitch) of a logical NCHW tensor for the channels-last kernels: in place where its memory allows, else one copy."""
    pitch = _cl_pitch(t)
    if pitch is None:
        t = t.contiguous(memory_format=torch.channels_last)
        pitch = _cl_pitch(t)
        if pitch is None:                                    # (size-1 dims leave the strides of the copy unspecified)
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            pitch = t.shape[1]
    return t, pitch


def _convgru_chk(t, name, like=None, channels=None, who="convgru"):
    if t is None:
        return
    if not on_device(t):
        raise StxError(f"{who}: {name}: expected a ROCm device tensor, got {t.device} -- the cell has no CPU fallback")
    if t.dtype != torch.float32:
        raise StxError(f"{who}: {name}: expected float32, got {t.dtype}")
    if like is not None:
        if t.dim() != 4 or t.shape[0] != like.shape[0] or tuple(t.shape[2:]) != tuple(like.shape[2:]):
            raise StxError(f"{who}: {name} has shape {tuple(t.shape)}, h has {tuple(like.shape)} (batch, H and W must agree)")
        if channels is not None and t.shape[1] != channels:
            raise StxError(f"{who}: {name} has {t.shape[1]} channels, expected {channels}")


def _convgru_pack(w0, w1, mode):
    """Packed copy of one or two ConvGRU weights [hidden][K][3][3] (mode 0: forward, 1: data gradient); cached on `w0` under
    the rules of set_weight_cache, keyed by the versions and addresses of both."""
    global CONVGRU_PACKS
    key = tuple(v for w in (w0, w1) if w is not None for v in (w._version, w.data_ptr()))
    tag = ("convgru", mode, w1 is not None)
    if _CACHE_ENABLED:
        cache = w0.__dict__.setdefault("_stx_packed", {})
        hit = cache.get(tag)
        if hit is not None and hit[0] == key:
            return hit[1]
    A, Bd = w0.shape[0], w0.shape[1]
    nw = 1 if w1 is None else 2
    K, N = (Bd, nw * A) if mode == 0 else (nw * A, Bd)
    n = get_lib().raw("stx_convgru_packed_floats")(K, N)
    if n <= 0:
        raise StxError(f"convgru: GEMM-K {K} (a multiple of 4, <= {CONVGRU_MAX_K}) x N {N} unsupported")
    wp = torch.empty(n, dtype=torch.float32, device=w0.device)
    w0c, w1c = w0.detach().contiguous(), None if w1 is None else w1.detach().contiguous()
    _call("stx_convgru_pack_weight", _p(w0c), _p(w1c), _p(wp), A, Bd, mode)
    CONVGRU_PACKS += 1
    if _CACHE_ENABLED:
        cache[tag] = (key, wp)
    return wp


def _src_args(srcs):
    """The flat (pointer, channels, pitch) x 4 form of a source list [(tensor NCHW-logical, pitch)]."""
    out = []
    for t, pitch in srcs:
        out += [_p(t), t.shape[1], pitch]
    for _ in range(4 - len(srcs)):
        out += [None, 0, 0]
    return out


def convgru_gemm(srcs, wp, N, B, H, W, epi=0, split=0, bias0=None, bias1=None, add0=None, add1=None, h=None, z=None, out0=None,
                 out1=None, out2=None, out_pitch=0):
    """One launch of the ConvGRU implicit-GEMM kernel (include/stx_hip.h: stx_convgru_gemm).  srcs / add0 / add1 / h:
    (tensor, pitch) pairs or None."""
    a0, a0p = add0 if add0 is not None else (None, 0)
    a1, a1p = add1 if add1 is not None else (None, 0)
    ht, hp = h if h is not None else (None, 0)
    _call("stx_convgru_gemm", *_src_args(srcs), _p(wp), N, epi, split, _p(bias0), _p(bias1), _p(a0), a0p, _p(a1), a1p, _p(ht), hp,
          _p(z), _p(out0), _p(out1), _p(out2), out_pitch, B, H, W)


def _nchw(t):
    """Logical NCHW view of a dense channels-last buffer [B][H][W][C] (or of a channel slice of one)."""
    return t.permute(0, 3, 1, 2)


class ConvGRUFn(torch.autograd.Function):
    """h' = ConvGRU(h, cz, cr, cq, x..) as one node on csrc/convgru.hip.  Forward: the zr launch and the q launch.  Backward: gate
    backward, data gradient of the q convolution, reset backward, data gradient of the z and r convolutions with the running
    [dL/dh | g_x] as addend, two weight gradients and the bias-row sums; nothing is accumulated by autograd afterwards.
    Saved: h and the x sources by reference, z, r, q and r h (4 x pixels x hidden floats per call)."""

    @staticmethod
    def forward(ctx, h, cz, cr, cq, wz, bz, wr, br, wq, bq, *xs):
        B, hidden, H, W = h.shape
        dev = h.device
        need = any(ctx.needs_input_grad)                      # (all False under no_grad: r and q are then not written)
        hs = _cl_source(h.detach())
        xsrc = [_cl_source(x.detach()) for x in xs]
        cs = [None if c is None else _cl_source(c.detach()) for c in (cz, cr, cq)]
        new = lambda: torch.empty(B, H, W, hidden, dtype=torch.float32, device=dev)       # noqa: E731
        z, rh, hn = new(), new(), new()
        r = new() if need else None
        q = new() if need else None
        bzc, brc, bqc = (None if b is None else b.detach().contiguous() for b in (bz, br, bq))
        convgru_gemm([hs] + xsrc, _convgru_pack(wz, wr, 0), 2 * hidden, B, H, W, epi=1, split=hidden, bias0=bzc, bias1=brc,
                     add0=cs[0], add1=cs[1], h=hs, out0=z, out1=rh, out2=r)
        convgru_gemm([(_nchw(rh), hidden)] + xsrc, _convgru_pack(wq, None, 0), hidden, B, H, W, epi=2, split=hidden, bias0=bqc,
                     add0=cs[2], h=hs, z=z, out0=hn, out1=q)
        if need:
            ctx.save_for_backward(hs[0], z, r, q, rh, wz, wr, wq, *[t for t, _ in xsrc])
            ctx.pitches = (hs[1], [p for _, p in xsrc])
            ctx.has_c = [c is not None for c in (cz, cr, cq)]
            ctx.has_b = [b is not None for b in (bz, br, bq)]
        return _nchw(hn)

    @staticmethod
    def backward(ctx, g):
        h, z, r, q, rh, wz, wr, wq, *xt = ctx.saved_tensors
        hp, xp = ctx.pitches
        B, hidden, H, W = h.shape
        dev = h.device
        P = B * H * W
        need = ctx.needs_input_grad
        need_x = any(need[10:])
        need_w = any(need[i] for i in (4, 6, 8))
        need_b = any(need[i] for i in (5, 7, 9)) and any(ctx.has_b)
        cx = [t.shape[1] for t in xt]
        K = hidden + sum(cx)
        Ndg = K if need_x else hidden                         # data gradients: [g_rh | g_x], or g_rh alone when no x wants one
        gt, gp = _cl_source(g)
        new = lambda: torch.empty(B, H, W, hidden, dtype=torch.float32, device=dev)       # noqa: E731
        gq, gz, gr = new(), new(), new()
        nrows = get_lib().raw("stx_convgru_gate_rows")(P, hidden)
        rows_g = torch.empty(nrows, 2, hidden, dtype=torch.float32, device=dev) if need_b else None
        rows_r = torch.empty(nrows, hidden, dtype=torch.float32, device=dev) if need_b else None
        _call("stx_convgru_gate_bwd", _p(gt), gp, _p(z), _p(q), _p(h), hp, _p(gq), _p(gz), _p(rows_g), P, hidden)
        buf = torch.empty(B, H, W, Ndg, dtype=torch.float32, device=dev)
        if need_x:
            wq1, wzr1 = _convgru_pack(wq, None, 1), _convgru_pack(wz, wr, 1)
        else:                                                 # (a pack is laid out for its own N: the h columns alone)
            wq1, wzr1 = _convgru_pack_head(wq, None, hidden), _convgru_pack_head(wz, wr, hidden)
        convgru_gemm([(_nchw(gq), hidden)], wq1, Ndg, B, H, W, out0=buf, out_pitch=Ndg)
        _call("stx_convgru_reset_bwd", _p(buf), Ndg, _p(gt), gp, _p(z), _p(r), _p(h), hp, _p(gr), _p(rows_r), P, hidden)
        convgru_gemm([(_nchw(gz), hidden), (_nchw(gr), hidden)], wzr1, Ndg, B, H, W, add0=(buf, Ndg), out0=buf, out_pitch=Ndg)
        grads = [None] * len(need)
        if need[0]:
            grads[0] = _nchw(buf[..., :hidden])
        for i, (gc, has) in enumerate(zip((gz, gr, gq), ctx.has_c)):
            if has and need[1 + i]:
                grads[1 + i] = _nchw(gc)
        off = hidden
        for i, c in enumerate(cx):
            if need[10 + i]:
                grads[10 + i] = _nchw(buf[..., off:off + c])
            off += c
        if need_w:
            xsrc = list(zip(xt, xp))
            if need[4] or need[6]:
                dzr = _convgru_wgrad([(h, hp)] + xsrc, gz, gr, B, H, W)
                if need[4]:
                    grads[4] = dzr[:hidden].view(hidden, K, 3, 3)
                if need[6]:
                    grads[6] = dzr[hidden:].view(hidden, K, 3, 3)
            if need[8]:
                grads[8] = _convgru_wgrad([(_nchw(rh), hidden)] + xsrc, gq, None, B, H, W).view(hidden, K, 3, 3)
        if need_b:
            sums = torch.empty(3, hidden, dtype=torch.float32, device=dev)         # gq | gz | gr
            _call("stx_convgru_row_sum", _p(rows_g), _p(sums), nrows, 2 * hidden)
            _call("stx_convgru_row_sum", _p(rows_r), _p(sums[2]), nrows, hidden)
            for i, k in ((5, 1), (7, 2), (9, 0)):
                if need[i] and ctx.has_b[(i - 5) // 2]:
                    grads[i] = sums[k]
        return tuple(grads)


def _convgru_pack_head(w0, w1, n_out):
    """Mode-1 packed weights restricted to the first `n_out` output channels (the data gradient of h alone, when no x source
    wants a gradient); cached like the full pack."""
    global CONVGRU_PACKS
    key = tuple(v for w in (w0, w1) if w is not None for v in (w._version, w.data_ptr()))
    tag = ("convgru_head", n_out, w1 is not None)
    if _CACHE_ENABLED:
        cache = w0.__dict__.setdefault("_stx_packed", {})
        hit = cache.get(tag)
        if hit is not None and hit[0] == key:
            return hit[1]
    w0h = w0.detach()[:, :n_out].contiguous()
    w1h = None if w1 is None else w1.detach()[:, :n_out].contiguous()
    A = w0h.shape[0]
    nw = 1 if w1 is None else 2
    wp = torch.empty(get_lib().raw("stx_convgru_packed_floats")(nw * A, n_out), dtype=torch.float32, device=w0.device)
    _call("stx_convgru_pack_weight", _p(w0h), _p(w1h), _p(wp), A, n_out, 1)
    CONVGRU_PACKS += 1
    if _CACHE_ENABLED:
        cache[tag] = (key, wp)
    return wp


def _convgru_wgrad(srcs, g0, g1, B, H, W):
    """dW [(1 or 2) hidden][K][9] of the source list against one or two dense gradient maps [B][H][W][hidden]."""
    CG = g0.shape[-1]
    K = sum(t.shape[1] for t, _ in srcs)
    CC = CG if g1 is None else 2 * CG
    n = get_lib().raw("stx_convgru_wgrad_workspace_floats")(B, H, W, K, CC)
    if n <= 0:
        raise StxError(f"convgru: weight gradient of {K} x {CC} channels unsupported")
    ws = _WS.get("convgru_wgrad", n, g0.device)
    dw = torch.empty(CC, K, 9, dtype=torch.float32, device=g0.device)
    _call("stx_convgru_wgrad", *_src_args(srcs), _p(g0), _p(g1), CG, _p(dw), _p(ws), B, H, W)
    return dw


@fp32_region
def convgru(h, cz, cr, cq, x_list, wz, bz, wr, br, wq, bq):
    """The ConvGRU cell of the iterative families (reference IGEVStereo/update.py:25-40) on the gfx950 kernels, one autograd node:
        z = sigmoid(conv(wz, [h, x..]) + bz + cz),  r = sigmoid(conv(wr, [h, x..]) + br + cr),
        q = tanh(conv(wq, [r h, x..]) + bq + cq),   h' = (1 - z) h + z q.
    h, cz, cr, cq: logical NCHW [B, hidden, H, W] (each c* may be None = zero); x_list: 1..3 tensors [B, C_i, H, W]; weights
    [hidden, hidden + sum C_i, 3, 3], biases [hidden] or None.  Tensors whose memory is channels-last -- channel slices of a
    wider channels-last map included -- are read in place, others are converted once.  Returns h' as an NCHW view of
    channels-last storage, fp32 (under autocast: the fp32 path on the cast-up inputs).  Served: hidden a multiple of 16 up to
    128, every C_i a multiple of 4, hidden + sum C_i <= 512; anything else raises StxError and launches nothing."""
    x_list = list(x_list)
    if h is None or h.dim() != 4:
        raise StxError("convgru: h must be a tensor [B, hidden, H, W]")
    _convgru_chk(h, "h")
    B, hidden, H, W = h.shape
    if not 1 <= len(x_list) <= CONVGRU_MAX_X:
        raise StxError(f"convgru: {len(x_list)} x sources; 1..{CONVGRU_MAX_X} are served (4 sources with h)")
    for i, x in enumerate(x_list):
        _convgru_chk(x, f"x[{i}]", like=h)
    for name, c in (("cz", cz), ("cr", cr), ("cq", cq)):
        _convgru_chk(c, name, like=h, channels=hidden)
    cx = [int(x.shape[1]) for x in x_list]
    K = hidden + sum(cx)
    for name, w, b in (("wz", wz, bz), ("wr", wr, br), ("wq", wq, bq)):
        _convgru_chk(w, name)
        _convgru_chk(b, "bias of " + name)
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
            raise StxError(f"convgru: {name} has shape {tuple(w.shape)}; only 3x3 kernels are served")
        if tuple(w.shape[:2]) != (hidden, K):
            raise StxError(f"convgru: {name} has shape {tuple(w.shape)}, expected {(hidden, K, 3, 3)}")
        if b is not None and tuple(b.shape) != (hidden,):
            raise StxError(f"convgru: bias of {name} has shape {tuple(b.shape)}, expected {(hidden,)}")
    if not get_lib().raw("stx_convgru_supported")(hidden, len(cx), *(cx + [0] * (3 - len(cx))), 3):
        raise StxError(f"convgru: hidden {hidden} (a multiple of 16, <= {CONVGRU_MAX_HIDDEN}) with x channels {cx} (multiples of 4, "
                       f"hidden + sum <= {CONVGRU_MAX_K}) is not served")
    return ConvGRUFn.apply(h, cz, cr, cq, wz, bz, wr, br, wq, bq, *x_list)


# ------------------------------------------------------------------------------ SelectiveStereo cells (selgru.hip + convgru.hip)
SELGRU_PACKS = 0             # pack launches of 1x1 weights so far (the 3x3 ones count in CONVGRU_PACKS)


def _selgru_pack(w0, w1, mode, n_out=None):
    """Packed copy of one or two 1x1 RaftConvGRU weights [hidden][K][1][1] (mode 0: forward, 1: data gradient; `n_out`: mode 1
    restricted to the first n_out output channels, the data gradient of h alone); cached like the ConvGRU packs."""
    global SELGRU_PACKS
    key = tuple(v for w in (w0, w1) if w is not None for v in (w._version, w.data_ptr()))
    tag = ("selgru", mode, w1 is not None, n_out)
    if _CACHE_ENABLED:
        cache = w0.__dict__.setdefault("_stx_packed", {})
        hit = cache.get(tag)
        if hit is not None and hit[0] == key:
            return hit[1]
    cut = lambda w: None if w is None else (w.detach() if n_out is None else w.detach()[:, :n_out]).contiguous()   # noqa: E731
    w0c, w1c = cut(w0), cut(w1)
    A, Bd = w0c.shape[0], w0c.shape[1]
    nw = 1 if w1 is None else 2
    K, N = (Bd, nw * A) if mode == 0 else (nw * A, Bd)
    n = get_lib().raw("stx_selgru_packed_floats")(K, N)
    if n <= 0:
        raise StxError(f"raft_convgru: GEMM-K {K} (a multiple of 4, <= {CONVGRU_MAX_K}) x N {N} unsupported")
    wp = torch.empty(n, dtype=torch.float32, device=w0.device)
    _call("stx_selgru_pack_weight", _p(w0c), _p(w1c), _p(wp), A, Bd, mode)
    SELGRU_PACKS += 1
    if _CACHE_ENABLED:
        cache[tag] = (key, wp)
    return wp


def _raft_pack(ks, w0, w1, mode, n_out=None):
    if ks == 1:
        return _selgru_pack(w0, w1, mode, n_out)
    return _convgru_pack(w0, w1, mode) if n_out is None else _convgru_pack_head(w0, w1, n_out)


def _raft_gemm(ks, srcs, wp, N, B, H, W, epi=0, split=0, bias0=None, bias1=None, add0=None, add1=None, h=None, z=None, att=None,
               other=None, blend=0, out0=None, out1=None, out2=None, out_pitch=0):
    """One GEMM launch of a RaftConvGRU cell: the 3x3 kernel of convgru.hip or the 1x1 kernel of selgru.hip (which alone takes a
    second raw addend and the blend)."""
    if ks == 3:
        assert blend == 0 and add1 is None
        return convgru_gemm(srcs, wp, N, B, H, W, epi=epi, split=split, bias0=bias0, bias1=bias1, add0=add0, h=h, z=z, out0=out0,
                            out1=out1, out2=out2, out_pitch=out_pitch)
    a0, a0p = add0 if add0 is not None else (None, 0)
    a1, a1p = add1 if add1 is not None else (None, 0)
    ht, hp = h if h is not None else (None, 0)
    _call("stx_selgru_gemm", *_src_args(srcs), _p(wp), N, epi, split, _p(bias0), _p(bias1), _p(a0), a0p, _p(a1), a1p, _p(ht), hp,
          _p(z), _p(att), _p(other), blend, _p(out0), _p(out1), _p(out2), out_pitch, B * H * W)


def _raft_cell_fwd(ks, hs, xsrc, w, need, att=None, other=None, blend=0):
    """z, r, q, r h and the new state of one RaftConvGRU cell (r, q only with `need`); with `blend` the state is blended with
    `other` in place (stx_selgru_gemm)."""
    wz, bz, wr, br, wq, bq = w
    B, hidden, H, W = hs[0].shape
    new = lambda: torch.empty(B, H, W, hidden, dtype=torch.float32, device=hs[0].device)       # noqa: E731
    z, rh = new(), new()
    r = new() if need else None
    q = new() if need else None
    hn = other if blend else new()
    bzc, brc, bqc = (None if b is None else b.detach().contiguous() for b in (bz, br, bq))
    _raft_gemm(ks, [hs] + xsrc, _raft_pack(ks, wz, wr, 0), 2 * hidden, B, H, W, epi=1, split=hidden, bias0=bzc, bias1=brc, h=hs,
               out0=z, out1=rh, out2=r)
    _raft_gemm(ks, [(_nchw(rh), hidden)] + xsrc, _raft_pack(ks, wq, None, 0), hidden, B, H, W, epi=2, split=hidden, bias0=bqc,
               h=hs, z=z, att=att, other=other if blend else None, blend=blend, out0=hn, out1=q)
    return z, r, q, rh, hn


def _raft_cell_bwd(ks, g, h, z, r, q, rh, xsrc, w, need_x, need_w, need_b, prev=None):
    """The backward chain of one RaftConvGRU cell for the incoming gradient g (tensor, pitch): gate backward, q data gradient,
    reset backward, z | r data gradient, weight gradients, bias gradients as column sums of gq, gz, gr.  Returns buf [B][H][W][hidden (+ K_x with need_x)] = [dL/dh | g_x] -- with `prev` (1x1
    cells only) the other cell's buffer is added: (product + own partial) + prev --, the weight gradients (wz, wr, wq) and the
    bias gradients (bz, br, bq), None where not needed."""
    gt, gp = g
    ht, hp = h
    wz, wr, wq = w
    B, hidden, H, W = ht.shape
    dev = ht.device
    P = B * H * W
    K = hidden + sum(t.shape[1] for t, _ in xsrc)
    Ndg = K if need_x else hidden
    new = lambda: torch.empty(B, H, W, hidden, dtype=torch.float32, device=dev)       # noqa: E731
    gq, gz, gr = new(), new(), new()
    _call("stx_convgru_gate_bwd", _p(gt), gp, _p(z), _p(q), _p(ht), hp, _p(gq), _p(gz), None, P, hidden)
    buf = torch.empty(B, H, W, Ndg, dtype=torch.float32, device=dev)
    n_out = None if need_x else hidden
    _raft_gemm(ks, [(_nchw(gq), hidden)], _raft_pack(ks, wq, None, 1, n_out), Ndg, B, H, W, out0=buf, out_pitch=Ndg)
    _call("stx_convgru_reset_bwd", _p(buf), Ndg, _p(gt), gp, _p(z), _p(r), _p(ht), hp, _p(gr), None, P, hidden)
    _raft_gemm(ks, [(_nchw(gz), hidden), (_nchw(gr), hidden)], _raft_pack(ks, wz, wr, 1, n_out), Ndg, B, H, W, add0=(buf, Ndg),
               add1=None if prev is None else (prev, Ndg), out0=buf, out_pitch=Ndg)
    dw = [None, None, None]
    if need_w[0] or need_w[1]:
        dzr = _raft_wgrad(ks, [h] + xsrc, gz, gr)
        if need_w[0]:
            dw[0] = dzr[:hidden].view(hidden, K, ks, ks)
        if need_w[1]:
            dw[1] = dzr[hidden:].view(hidden, K, ks, ks)
    if need_w[2]:
        dw[2] = _raft_wgrad(ks, [(_nchw(rh), hidden)] + xsrc, gq, None).view(hidden, K, ks, ks)
    db = [None, None, None]
    if any(need_b):                                          # column sums in double: at 3 x 10^4 pixels the fp32 partial rows of
        sums = torch.empty(3, hidden, dtype=torch.float32, device=dev)             # the ConvGRU node sit at the rule's edge
        ws = _WS.get("selgru_col_sum", get_lib().raw("stx_selgru_col_sum_workspace_floats")(P, hidden), dev)
        _call("stx_selgru_col_sum", _p(gq), _p(gz), _p(gr), _p(sums), _p(ws), P, hidden)
        db = [sums[k] if n else None for k, n in zip((1, 2, 0), need_b)]
    return buf, dw, db


def _raft_wgrad(ks, srcs, g0, g1):
    """dW [(1 or 2) hidden][K][ks ks] of the source list against one or two dense gradient maps [B][H][W][hidden]."""
    B, H, W, CG = g0.shape
    if ks == 3:
        return _convgru_wgrad(srcs, g0, g1, B, H, W)
    K = sum(t.shape[1] for t, _ in srcs)
    CC = CG if g1 is None else 2 * CG
    n = get_lib().raw("stx_selgru_wgrad_workspace_floats")(B * H * W, K, CC)
    if n <= 0:
        raise StxError(f"raft_convgru: weight gradient of {K} x {CC} channels unsupported")
    ws = _WS.get("selgru_wgrad", n, g0.device)
    dw = torch.empty(CC, K, dtype=torch.float32, device=g0.device)
    _call("stx_selgru_wgrad", *_src_args(srcs), _p(g0), _p(g1), CG, _p(dw), _p(ws), B * H * W)
    return dw


def _x_grads(buf, hidden, cx, need):
    out, off = [], hidden
    for c, n in zip(cx, need):
        out.append(_nchw(buf[..., off:off + c]) if n else None)
        off += c
    return out


class RaftConvGRU1x1Fn(torch.autograd.Function):
    """h' = RaftConvGRU(h, x..) with 1x1 kernels as one node on csrc/selgru.hip; the chain of ConvGRUFn without context biases.
    Saved: h and the x sources by reference, z, r, q and r h.  The last argument is the caller's grad mode (a forward always runs
    with it switched off, and needs_input_grad follows requires_grad alone): without it r and q are not written."""

    @staticmethod
    def forward(ctx, h, wz, bz, wr, br, wq, bq, *xs):
        *xs, track = xs
        need = track and any(ctx.needs_input_grad)
        hs = _cl_source(h.detach())
        xsrc = [_cl_source(x.detach()) for x in xs]
        z, r, q, rh, hn = _raft_cell_fwd(1, hs, xsrc, (wz, bz, wr, br, wq, bq), need)
        if need:
            ctx.save_for_backward(hs[0], z, r, q, rh, wz, wr, wq, *[t for t, _ in xsrc])
            ctx.pitches = (hs[1], [p for _, p in xsrc])
            ctx.has_b = [b is not None for b in (bz, br, bq)]
        return _nchw(hn)

    @staticmethod
    def backward(ctx, g):
        h, z, r, q, rh, wz, wr, wq, *xt = ctx.saved_tensors
        hp, xp = ctx.pitches
        need = ctx.needs_input_grad
        hidden = h.shape[1]
        need_b = [need[i] and has for i, has in zip((2, 4, 6), ctx.has_b)]
        buf, dw, db = _raft_cell_bwd(1, _cl_source(g), (h, hp), z, r, q, rh, list(zip(xt, xp)), (wz, wr, wq), any(need[7:-1]),
                                     [need[1], need[3], need[5]], need_b)
        gh = _nchw(buf[..., :hidden]) if need[0] else None
        return (gh, dw[0], db[0], dw[1], db[1], dw[2], db[2], *_x_grads(buf, hidden, [t.shape[1] for t in xt], need[7:-1]), None)


class SelectiveConvGRUFn(torch.autograd.Function):
    """h' = att small_gru(h, x..) + (1 - att) large_gru(h, x..) as one node.  Forward: the cell with 3x3 kernels first (both 1x1:
    the large one), then the 1x1 cell, whose q epilogue forms the blend in place: neither cell's own state is kept.  Backward:
    stx_selgru_blend_bwd (g_s, g_l and, if att wants it, g_att from the re-formed states), then the two cells' chains in the same
    order; the second chain's last launch adds the first chain's [dL/dh | g_x] buffer as a second raw addend, so the sum has one
    fixed order and autograd accumulates nothing.  Saved: h, att and the x sources by reference, z, r, q, r h of each cell."""

    @staticmethod
    def forward(ctx, att, h, *rest):
        ws, wl, xs, track = rest[:6], rest[6:12], rest[12:-1], rest[-1]        # (track: the caller's grad mode, as above)
        ks_s, ks_l = ws[0].shape[-1], wl[0].shape[-1]
        need = track and any(ctx.needs_input_grad)
        hs = _cl_source(h.detach())
        xsrc = [_cl_source(x.detach()) for x in xs]
        attc = att.detach().contiguous()
        small_last = ks_s == 1
        first, last = ((ks_l, wl), (ks_s, ws)) if small_last else ((ks_s, ws), (ks_l, wl))
        f = _raft_cell_fwd(first[0], hs, xsrc, first[1], need)
        l = _raft_cell_fwd(last[0], hs, xsrc, last[1], need, att=attc, other=f[4], blend=1 if small_last else 2)   # noqa: E741
        if need:
            ctx.save_for_backward(hs[0], attc, *f[:4], *l[:4], first[1][0], first[1][2], first[1][4], last[1][0], last[1][2],
                                  last[1][4], *[t for t, _ in xsrc])
            ctx.pitches = (hs[1], [p for _, p in xsrc])
            ctx.small_last = small_last
            ctx.ks = (first[0], last[0])
            ctx.has_b = [[w[i] is not None for i in (1, 3, 5)] for w in (first[1], last[1])]
        return _nchw(l[4])

    @staticmethod
    def backward(ctx, g):
        h, att, zf, rf, qf, rhf, zl, rl, ql, rhl, wzf, wrf, wqf, wzl, wrl, wql, *xt = ctx.saved_tensors
        hp, xp = ctx.pitches
        need = ctx.needs_input_grad
        B, hidden, H, W = h.shape
        dev = h.device
        P = B * H * W
        gt, gp = _cl_source(g)
        new = lambda: torch.empty(B, H, W, hidden, dtype=torch.float32, device=dev)       # noqa: E731
        g_s, g_l = new(), new()
        gatt = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev) if need[0] else None
        (zs, qs), (zb, qb) = ((zl, ql), (zf, qf)) if ctx.small_last else ((zf, qf), (zl, ql))       # small cell, large cell
        _call("stx_selgru_blend_bwd", _p(gt), gp, _p(att), _p(zs), _p(qs), _p(zb), _p(qb), _p(h), hp, _p(g_s), _p(g_l), _p(gatt),
              P, hidden)
        g_first, g_last = (g_l, g_s) if ctx.small_last else (g_s, g_l)
        o_first, o_last = (8, 2) if ctx.small_last else (2, 8)               # where each cell's parameters sit in the inputs
        xsrc = list(zip(xt, xp))
        need_x = any(need[14:-1])
        outs = [None] * len(need)
        buf = None
        for ks, gc, o, has_b, (z, r, q, rh), w in ((ctx.ks[0], g_first, o_first, ctx.has_b[0], (zf, rf, qf, rhf), (wzf, wrf, wqf)),
                                                   (ctx.ks[1], g_last, o_last, ctx.has_b[1], (zl, rl, ql, rhl), (wzl, wrl, wql))):
            need_b = [need[o + i] and hb for i, hb in zip((1, 3, 5), has_b)]
            buf, dw, db = _raft_cell_bwd(ks, (_nchw(gc), hidden), (h, hp), z, r, q, rh, xsrc, w, need_x,
                                         [need[o], need[o + 2], need[o + 4]], need_b, prev=buf)
            outs[o:o + 6] = [dw[0], db[0], dw[1], db[1], dw[2], db[2]]
        outs[0] = gatt
        if need[1]:
            outs[1] = _nchw(buf[..., :hidden])
        outs[14:-1] = _x_grads(buf, hidden, [t.shape[1] for t in xt], need[14:-1])
        return tuple(outs)


def _raft_chk(who, h, x_list, cells):
    """Argument checks of the RaftConvGRU ops; returns the kernel sizes of `cells` (tuples wz, bz, wr, br, wq, bq)."""
    x_list = list(x_list)
    if h is None or h.dim() != 4:
        raise StxError(f"{who}: h must be a tensor [B, hidden, H, W]")
    _convgru_chk(h, "h", who=who)
    hidden = h.shape[1]
    if not 1 <= len(x_list) <= CONVGRU_MAX_X:
        raise StxError(f"{who}: {len(x_list)} x sources; 1..{CONVGRU_MAX_X} are served (4 sources with h)")
    for i, x in enumerate(x_list):
        _convgru_chk(x, f"x[{i}]", like=h, who=who)
    cx = [int(x.shape[1]) for x in x_list]
    K = hidden + sum(cx)
    sizes = []
    for cell in cells:
        if len(cell) != 6 or cell[0] is None or cell[0].dim() != 4:
            raise StxError(f"{who}: a cell is (wz, bz, wr, br, wq, bq) with weights [hidden, K, k, k]")
        ks = int(cell[0].shape[-1])
        if ks not in (1, 3):
            raise StxError(f"{who}: kernel size {ks}; 1x1 and 3x3 cells are served")
        for name, w, b in zip(("wz", "wr", "wq"), cell[0::2], cell[1::2]):
            _convgru_chk(w, name, who=who)
            _convgru_chk(b, "bias of " + name, who=who)
            if w.dim() != 4 or tuple(w.shape) != (hidden, K, ks, ks):
                raise StxError(f"{who}: {name} has shape {tuple(w.shape)}, expected {(hidden, K, ks, ks)}")
            if b is not None and tuple(b.shape) != (hidden,):
                raise StxError(f"{who}: bias of {name} has shape {tuple(b.shape)}, expected {(hidden,)}")
        sizes.append(ks)
    cx3 = cx + [0] * (3 - len(cx))
    lib = get_lib()
    if not (lib.raw("stx_selgru_supported")(hidden, len(cx), *cx3) and lib.raw("stx_convgru_supported")(hidden, len(cx), *cx3, 3)):
        raise StxError(f"{who}: hidden {hidden} (a multiple of 16, <= {CONVGRU_MAX_HIDDEN}) with x channels {cx} (multiples of 4, "
                       f"hidden + sum <= {CONVGRU_MAX_K}) is not served")
    return sizes


@fp32_region
def raft_convgru(h, x_list, wz, bz, wr, br, wq, bq):
    """RaftConvGRU of SelectiveStereo (reference SelectiveStereo/SelectiveRAFT/update.py:15-30) on the gfx950 kernels, one autograd
    node: the ConvGRU cell without context biases, its kernel size (1 or 3) read from the weights.  For 3x3 it is
    `convgru(h, None, None, None, x_list, ...)` to the bit; 1x1 runs on csrc/selgru.hip.  Shapes, strides, limits and refusals as
    `convgru`."""
    ks, = _raft_chk("raft_convgru", h, x_list, [(wz, bz, wr, br, wq, bq)])
    if ks == 3:
        return ConvGRUFn.apply(h, None, None, None, wz, bz, wr, br, wq, bq, *x_list)
    return RaftConvGRU1x1Fn.apply(h, wz, bz, wr, br, wq, bq, *x_list, torch.is_grad_enabled())


@fp32_region
def selective_convgru(att, h, x_list, small, large):
    """SelectiveConvGRU of SelectiveStereo (reference SelectiveStereo/SelectiveRAFT/update.py:61-71), one autograd node:
        h' = att * RaftConvGRU_small(h, x..) + (1 - att) * RaftConvGRU_large(h, x..)
    att [B, 1, H, W]; h, x_list as `convgru`; small / large = (wz, bz, wr, br, wq, bq) of the two cells, kernel sizes 1 or 3 read
    from the weights, at least one of them 1 (the blend lives in the 1x1 kernel's epilogue).  The blend is formed in double from
    the 1x1 cell's unrounded state and rounded once; neither cell's own state is materialised beyond the call.  Returns h' as an
    NCHW view of channels-last storage, fp32.  Anything not served raises StxError and launches nothing."""
    who = "selective_convgru"
    small, large = tuple(small), tuple(large)
    ks_s, ks_l = _raft_chk(who, h, x_list, [small, large])
    if ks_s != 1 and ks_l != 1:
        raise StxError(f"{who}: kernel sizes {ks_s} and {ks_l}; one of the two cells must be 1x1")
    if att is None or att.dim() != 4:
        raise StxError(f"{who}: att must be a tensor [B, 1, H, W]")
    _convgru_chk(att, "att", like=h, channels=1, who=who)
    return SelectiveConvGRUFn.apply(att, h, *small, *large, *x_list, torch.is_grad_enabled())


# ------------------------------------------------------------------------------ contextual spatial attention (csa.hip)
CSA_MAX_C = 256
CSA_MAX_KERNEL = 7


def _csa_chk(who, x, w1=None, w2=None, w_sam=None):
    """Argument checks of the CSA ops; returns (B, C, H, W, kernel size or None)."""
    for name, t in (("x", x), ("w1", w1), ("w2", w2), ("w_sam", w_sam)):
        if t is None:
            continue
        if not on_device(t):
            raise StxError(f"{who}: {name}: expected a ROCm device tensor, got {t.device} -- the attention has no CPU fallback")
        if t.dtype != torch.float32:
            raise StxError(f"{who}: {name}: expected float32, got {t.dtype}")
        if t.dim() != 4:
            raise StxError(f"{who}: {name} has shape {tuple(t.shape)}, expected 4 dims")
    B, C, H, W = x.shape
    k = None if w_sam is None else int(w_sam.shape[-1])
    if min(B, H, W) < 1 or not get_lib().raw("stx_csa_supported")(C, 1 if k is None else k):
        raise StxError(f"{who}: {C} channels (a multiple of 16, <= {CSA_MAX_C}) with a {k} x {k} kernel (odd, <= {CSA_MAX_KERNEL}) on "
                       f"{tuple(x.shape)} is not served")
    if w1 is not None and (tuple(w1.shape) != (C // 16, C, 1, 1) or w2 is None or tuple(w2.shape) != (C, C // 16, 1, 1)):
        raise StxError(f"{who}: the MLP weights have shapes {tuple(w1.shape)} and {None if w2 is None else tuple(w2.shape)}, expected "
                       f"{(C // 16, C, 1, 1)} and {(C, C // 16, 1, 1)}")
    if w_sam is not None and tuple(w_sam.shape) != (1, 2, k, k):
        raise StxError(f"{who}: w_sam has shape {tuple(w_sam.shape)}, expected {(1, 2, k, k)}")
    return B, C, H, W, k


def _csa_pool(xs, pitch, B, C, HW):
    nblk = get_lib().raw("stx_csa_blocks")(HW, C)
    dev = xs.device
    psum = torch.empty(B, nblk, C, dtype=torch.float64, device=dev)
    pmax = torch.empty(B, nblk, C, dtype=torch.float32, device=dev)
    pidx = torch.empty(B, nblk, C, dtype=torch.int32, device=dev)
    _call("stx_csa_pool", _p(xs), pitch, _p(psum), _p(pmax), _p(pidx), B, HW, C)
    return nblk, psum, pmax, pidx


def _csa_gate_state(B, C, dev):
    return (torch.empty(B, C, dtype=torch.float32, device=dev), torch.empty(B, 2, C, dtype=torch.float64, device=dev),
            torch.empty(B, C, dtype=torch.int32, device=dev))


def _csa_sam_bwd(g, att, cmap, w, need_w):
    """gmap [B][H][W][2] and dw [1][2][k][k] (None without need_w) from the gradient of att."""
    B, _, H, W = att.shape
    k = w.shape[-1]
    dev = att.device
    gc = g.contiguous()
    gpre = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    gmap = torch.empty(B, H, W, 2, dtype=torch.float32, device=dev)
    dw = torch.empty(1, 2, k, k, dtype=torch.float32, device=dev) if need_w else None
    ws = _WS.get("csa_sam_bwd", get_lib().raw("stx_csa_sam_bwd_workspace_floats")(B, H, W, k), dev) if need_w else None
    _call("stx_csa_sam_bwd", _p(gc), _p(att), _p(cmap), _p(w), _p(gpre), _p(gmap), _p(dw), _p(ws), B, H, W, k)
    return gmap, dw


def _csa_gate_bwd(pgate, nblk, gg, pooled, argp, w1, w2, gx, accumulate, need_w1, need_w2, need_x, HW):
    """Backward of the MLP and of the two global pools; gx [B][H][W][C] receives (or is added) the pools' gradient."""
    B, C = argp.shape
    dev = argp.device
    dw1 = torch.empty(C // 16, C, 1, 1, dtype=torch.float32, device=dev) if need_w1 else None
    dw2 = torch.empty(C, C // 16, 1, 1, dtype=torch.float32, device=dev) if need_w2 else None
    gavg = torch.empty(B, C, dtype=torch.float32, device=dev)
    gmx = torch.empty(B, C, dtype=torch.float32, device=dev)
    _call("stx_csa_gate_bwd", _p(pgate), nblk, _p(gg), _p(pooled), _p(w1), _p(w2), _p(dw1), _p(dw2), _p(gavg), _p(gmx), B, HW, C)
    if need_x:
        _call("stx_csa_pool_bwd", _p(gx), _p(gavg), _p(gmx), _p(argp), 1 if accumulate else 0, B, HW, C)
    return dw1, dw2


class CsaFn(torch.autograd.Function):
    """(x', att) = (cam(x) x, sam(x')) in three launches (csrc/csa.hip); the backward pass in its fixed-order partials.  Saved: x by
    reference, the gate, the pooled vectors (double), the two arg max maps (int32), the 2-channel map and att."""

    @staticmethod
    def forward(ctx, x, w1, w2, w_sam, track):
        B, C, H, W = x.shape
        k = w_sam.shape[-1]
        dev = x.device
        need = track and any(ctx.needs_input_grad)           # (track: the caller's grad mode, as in the cells)
        xs, pitch = _cl_source(x.detach())
        w1c, w2c, wsc = w1.detach().contiguous(), w2.detach().contiguous(), w_sam.detach().contiguous()
        nblk, psum, pmax, pidx = _csa_pool(xs, pitch, B, C, H * W)
        xp = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        cmap = torch.empty(B, H, W, 2, dtype=torch.float32, device=dev)
        argc = torch.empty(B, H, W, dtype=torch.int32, device=dev) if need else None
        gate, pooled, argp = _csa_gate_state(B, C, dev) if need else (None, None, None)
        _call("stx_csa_apply", _p(xs), pitch, _p(psum), _p(pmax), _p(pidx), nblk, _p(w1c), _p(w2c), _p(xp), _p(cmap), _p(argc),
              _p(gate), _p(pooled), _p(argp), B, H * W, C)
        att = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
        _call("stx_csa_sam", _p(cmap), _p(wsc), _p(att), B, H, W, k)
        if need:
            ctx.save_for_backward(xs, gate, pooled, argp, argc, cmap, att, w1c, w2c, wsc)
            ctx.pitch, ctx.nblk = pitch, nblk
            ctx.set_materialize_grads(False)
        return _nchw(xp), att

    @staticmethod
    def backward(ctx, gxp, gatt):
        xs, gate, pooled, argp, argc, cmap, att, w1, w2, wsam = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, C, H, W = xs.shape
        dev = xs.device
        gmap = dws = None
        if gatt is not None:
            gmap, dws = _csa_sam_bwd(gatt, att, cmap, wsam, need[3])
        if not any(need[:3]) or (gxp is None and gmap is None):
            return None, None, None, dws, None
        gs, gpitch = _cl_source(gxp) if gxp is not None else (None, 0)
        gx = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        pgate = torch.empty(B, ctx.nblk, C, dtype=torch.float64, device=dev)
        _call("stx_csa_apply_bwd", _p(xs), ctx.pitch, _p(gate), _p(gs), gpitch, _p(gmap), _p(argc), _p(gx), _p(pgate), B, H * W, C)
        dw1, dw2 = _csa_gate_bwd(pgate, ctx.nblk, None, pooled, argp, w1, w2, gx, True, need[1], need[2], need[0], H * W)
        return _nchw(gx) if need[0] else None, dw1, dw2, dws, None


class CsaGateFn(torch.autograd.Function):
    """gate = ChannelAttentionEnhancement(x) [B, C, 1, 1]: the pooled partials and a one-workgroup finish."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        B, C, H, W = x.shape
        dev = x.device
        xs, pitch = _cl_source(x.detach())
        w1c, w2c = w1.detach().contiguous(), w2.detach().contiguous()
        nblk, psum, pmax, pidx = _csa_pool(xs, pitch, B, C, H * W)
        gate, pooled, argp = _csa_gate_state(B, C, dev)
        _call("stx_csa_gate", _p(psum), _p(pmax), _p(pidx), nblk, _p(w1c), _p(w2c), _p(gate), _p(pooled), _p(argp), B, H * W, C)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(pooled, argp, w1c, w2c)
            ctx.hw = (H, W)
        return gate.view(B, C, 1, 1)

    @staticmethod
    def backward(ctx, g):
        pooled, argp, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, C = argp.shape
        H, W = ctx.hw
        gg = g.reshape(B, C).contiguous()
        gx = torch.empty(B, H, W, C, dtype=torch.float32, device=argp.device) if need[0] else None
        dw1, dw2 = _csa_gate_bwd(None, 0, gg, pooled, argp, w1, w2, gx, False, need[1], need[2], need[0], H * W)
        return None if gx is None else _nchw(gx), dw1, dw2


class CsaSpatialFn(torch.autograd.Function):
    """att = SpatialAttentionExtractor(x) [B, 1, H, W]: the map sweep without a gate, then the k x k convolution."""

    @staticmethod
    def forward(ctx, x, w, track):
        B, C, H, W = x.shape
        k = w.shape[-1]
        dev = x.device
        need = track and any(ctx.needs_input_grad)
        xs, pitch = _cl_source(x.detach())
        wc = w.detach().contiguous()
        cmap = torch.empty(B, H, W, 2, dtype=torch.float32, device=dev)
        argc = torch.empty(B, H, W, dtype=torch.int32, device=dev) if need else None
        _call("stx_csa_apply", _p(xs), pitch, None, None, None, 0, None, None, None, _p(cmap), _p(argc), None, None, None, B, H * W, C)
        att = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
        _call("stx_csa_sam", _p(cmap), _p(wc), _p(att), B, H, W, k)
        if need:
            ctx.save_for_backward(argc, cmap, att, wc)
            ctx.C = C
        return att

    @staticmethod
    def backward(ctx, g):
        argc, cmap, att, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, _, H, W = att.shape
        gmap, dw = _csa_sam_bwd(g, att, cmap, w, need[1])
        gx = None
        if need[0]:
            gx = torch.empty(B, H, W, ctx.C, dtype=torch.float32, device=att.device)
            _call("stx_csa_apply_bwd", None, 0, None, None, 0, _p(gmap), _p(argc), _p(gx), None, B, H * W, ctx.C)
        return None if gx is None else _nchw(gx), dw, None


@fp32_region
def csa_gate(x, w1, w2):
    """ChannelAttentionEnhancement.forward of SelectiveStereo (reference SelectiveRAFT/update.py:106-121): sigmoid(fc(avgpool(x)) +
    fc(maxpool(x))) with fc = w2 relu(w1 .), w1 [C/16, C, 1, 1], w2 [C, C/16, 1, 1]; returns [B, C, 1, 1] fp32.  x logical NCHW,
    channels-last memory is read in place.  Served: C a multiple of 16 up to 256; anything else raises StxError."""
    _csa_chk("csa_gate", x, w1, w2)
    return CsaGateFn.apply(x, w1, w2)


@fp32_region
def csa_spatial(x, w):
    """SpatialAttentionExtractor.forward (reference SelectiveRAFT/update.py:123-135): sigmoid(conv([mean_c x | max_c x], w)) with
    w [1, 2, k, k], k odd up to 7, zero padding k // 2; returns [B, 1, H, W] fp32."""
    _csa_chk("csa_spatial", x, w_sam=w)
    return CsaSpatialFn.apply(x, w, torch.is_grad_enabled())


@fp32_region
def csa(x, w1, w2, w_sam):
    """The contextual spatial attention of one context map (reference SelectiveIGEV/igev_stereo.py:225-226), fused:
    x' = csa_gate(x, w1, w2) * x and att = csa_spatial(x', w_sam), to the bit, in three launches.  Returns (x' as an NCHW view of
    channels-last storage, att [B, 1, H, W])."""
    _csa_chk("csa", x, w1, w2, w_sam)
    return CsaFn.apply(x, w1, w2, w_sam, torch.is_grad_enabled())


class SharedInputConvsFn(torch.autograd.Function):
    """Raw outputs (+ BN partial sums) of SEVERAL plain convolutions of ONE activation -- the tensors with more than one
    convolution consumer in the reference graphs: the hourglass input (conv1 stride 2 + redir1 1x1x1, gwcnet.py:85,103) together
    with the classifier head that reads the same volume (gwcnet.py:192-195), conv2's output (conv3 + redir2).  Forward = the
    same launches ConvRawFn makes.  Backward: autograd would sum the consumers' input gradients with one volume-sized `add`
    per extra consumer (three passes over a 212 MB volume each: 0.65 ms per GwcNet_GC train step); here every gradient after
    the first is accumulated in the epilogue of the kernel that produces it (`residual` operand: one extra read).  Order: the
    3x3x3 stride-1 layer first (its march kernel keeps its straight-line epilogue), then stride 2, then 1x1x1.
    cfgs: one (ks, stride, want_stats) per convolution; weights [Cout, Cin, k, k, k], Cin % 8 == 0, Cout % 8 == 0."""

    @staticmethod
    def forward(ctx, x, cfgs, *ws):
        _chk(x, "x", 5)
        outs = []
        for (ks, stride, want), w in zip(cfgs, ws):
            if x.shape[-1] != w.shape[1] or w.shape[1] % 8 or w.shape[0] % 8 or _is_c1(w, ks, stride, False):
                raise StxError(f"SharedInputConvsFn: weight {tuple(w.shape)} on an input of {x.shape[-1]} channels")
            z, stats = conv3d_forward(x, pack_weight(w, 0), w.shape[0], ks, stride, want_stats=want)
            if stats is None:
                stats = x.new_empty(0)
            ctx.mark_non_differentiable(stats)
            outs += [z, stats]
        ctx.save_for_backward(x, *ws)
        ctx.cfgs = cfgs
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        x, ws = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        B, D, H, W, Ci = x.shape
        gws = [None] * len(ws)
        gzs = []
        for k, g in enumerate(grads[0::2]):
            pend = _take_pending_bn(g)
            if pend is not None:                       # (see ConvRawFn.backward)
                ks, stride, _ = ctx.cfgs[k]
                if (ctx.needs_input_grad[2 + k] and ks == 3 and stride == 1
                        and get_lib().raw("stx_conv3d_wgrad_bn_supported")(B, D, H, W, Ci, ws[k].shape[0])):
                    gw, g = conv3d_wgrad_bn(x, g, pend)
                    gws[k] = gw.reshape(ws[k].shape)
                else:
                    g = pend.materialize()
            gzs.append(None if g is None else g.contiguous())
        gx = None
        if ctx.needs_input_grad[0]:
            rank = lambda k: (0 if ctx.cfgs[k][0] == 3 and ctx.cfgs[k][1] == 1 else (1 if ctx.cfgs[k][1] == 2 else 2))
            for k in sorted((k for k in range(len(ws)) if gzs[k] is not None), key=rank):
                (ks, stride, _), w, gz = ctx.cfgs[k], ws[k], gzs[k]
                if stride == 1:
                    gx, _ = conv3d_forward(gz, pack_weight(w, 1), Ci, ks, 1, residual=gx)
                else:                     # stride-2 dgrad = transposed conv of gz (its kernel takes GEMM-K in steps of 32)
                    Co = w.shape[0]
                    gz_k, w_k = gz, w
                    if Co % 32:
                        Cp = (Co + 31) // 32 * 32
                        gz_k = _pad_channels(gz, Cp)
                        w_k = w.new_zeros(Cp, *w.shape[1:])
                        w_k[:Co] = w
                    gx, _ = deconv3d_forward(gz_k, pack_weight(w_k, 2), Ci, out_dims=(D, H, W), residual=gx)
        for k, (w, gz) in enumerate(zip(ws, gzs)):
            if gz is None or not ctx.needs_input_grad[2 + k] or gws[k] is not None:
                continue
            ks, stride, _ = ctx.cfgs[k]
            Co = w.shape[0]
            gz_w = gz if Co % 32 == 0 else _pad_channels(gz, (Co + 31) // 32 * 32)
            x_w = x if Ci % 32 == 0 else _pad_channels(x, (Ci + 31) // 32 * 32)
            gws[k] = conv3d_wgrad(x_w, gz_w, ks, stride)[:Co, :Ci].reshape(w.shape)
        return (gx, None, *gws)


# --------------------------------------------------------------------------------------- ConvTranspose3d(k4, s2, p1)
_D4_SEL = ((3, 1, 4), (4, 2, 0))       # per axis and output parity p: the k4 tap at offsets -1, 0, +1 (4 = the zero slice)


def embed_deconv4_weight(w):
    """ConvTranspose3d(k=4, s=2, p=1) weight [Cin, Cout, 4, 4, 4] -> the weight [8 Cout, Cin, 3, 3, 3] of ONE stride-1
    3x3x3 convolution whose output channel (4 pd + 2 ph + pw) Cout + c is parity class (pd, ph, pw) of output channel c:
    per axis  out[2j + p] = x[j] w[1 + p] + x[j - 1 + 2p] w[3 - 3p], i.e. offsets (-1, 0, +1) take taps (3, 1, -) for
    p = 0 and (-, 2, 0) for p = 1 (reference IGEVStereo/igev_stereo.py:44-51 `conv*_up`).  Pure indexing: differentiable."""
    Ci, Co = w.shape[0], w.shape[1]
    wz = torch.cat((w, w.new_zeros(Ci, Co, 1, 4, 4)), 2)
    wz = torch.cat((wz, wz.new_zeros(Ci, Co, 5, 1, 4)), 3)
    wz = torch.cat((wz, wz.new_zeros(Ci, Co, 5, 5, 1)), 4)
    parts = []
    for pd in (0, 1):
        for ph in (0, 1):
            for pw in (0, 1):
                sel = wz[:, :, list(_D4_SEL[pd])][:, :, :, list(_D4_SEL[ph])][:, :, :, :, list(_D4_SEL[pw])]
                parts.append(sel.transpose(0, 1))
    return torch.cat(parts, 0).contiguous()


class DepthToSpaceFn(torch.autograd.Function):
    """[B, D, H, W, 8 C] (parity-class-major channels) -> [B, 2D, 2H, 2W, C]; backward = the inverse map."""

    @staticmethod
    def forward(ctx, y):
        y = y.contiguous()
        _chk(y, "y", 5)
        B, D, H, W, C8 = y.shape
        C = C8 // 8
        out = torch.empty(B, 2 * D, 2 * H, 2 * W, C, dtype=torch.float32, device=y.device)
        _call("stx_depth_to_space", _p(y), _p(out), B, D, H, W, C, 0)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, D2, H2, W2, C = g.shape
        gy = torch.empty(B, D2 // 2, H2 // 2, W2 // 2, 8 * C, dtype=torch.float32, device=g.device)
        _call("stx_depth_to_space", _p(g), _p(gy), B, D2 // 2, H2 // 2, W2 // 2, C, 1)
        return gy


def _d4_chunks(Co):
    """Parity classes per launch: the convolution kernels produce at most 128 output channels."""
    per = max(1, min(8, 128 // Co))
    return [(c0, min(8, c0 + per)) for c0 in range(0, 8, per)]


def deconv4_raw(x, w, want_stats):
    """Autograd path of ConvTranspose3d(k4, s2, p1): raw output z [B, 2D, 2H, 2W, Cout] (+ BatchNorm partial rows).
    One (or a few, for 8 Cout > 128) stride-1 3x3x3 MFMA convolutions on the embedded weight + the class interleave;
    data and weight gradients flow back through the same kernels (ConvRawFn) and the indexing above."""
    Co = w.shape[1]
    if Co % 4:
        raise StxError(f"ConvTranspose3d(k4): {Co} output channels (need a multiple of 4)")
    w3 = embed_deconv4_weight(w)
    ys = [ConvRawFn.apply(x, w3[c0 * Co:c1 * Co], 3, 1, False, False)[0] for c0, c1 in _d4_chunks(Co)]
    z = DepthToSpaceFn.apply(ys[0] if len(ys) == 1 else torch.cat(ys, -1))
    return z, (bn_stats(z.detach()) if want_stats else z.new_empty(0))


@fp32_region
def deconv4_forward(x, w, scale=None, bias=None, relu=0, owner=None):
    """Inference path of ConvTranspose3d(k4, s2, p1) with the folded BatchNorm / activation in the convolution epilogue
    (scale / bias repeated per parity class), then the class interleave.  Packed weights cached on `owner`."""
    _chk(x, "x", 5)
    Co = w.shape[1]
    if Co % 4:
        raise StxError(f"ConvTranspose3d(k4): {Co} output channels (need a multiple of 4)")
    cache = owner.__dict__.setdefault("_stx_packed", {}) if (owner is not None and _CACHE_ENABLED) else None
    key = (owner._version, owner.data_ptr()) if owner is not None else None
    hit = cache.get("d4") if cache is not None else None
    if hit is not None and hit[0] == key:
        packed = hit[1]
    else:
        w3 = embed_deconv4_weight(w)
        packed = [pack_weight(w3[c0 * Co:c1 * Co].contiguous(), 0) for c0, c1 in _d4_chunks(Co)]
        if cache is not None:
            cache["d4"] = (key, packed)
    ys = []
    for (c0, c1), wp in zip(_d4_chunks(Co), packed):
        n = c1 - c0
        ys.append(conv3d_forward(x, wp, n * Co, 3, 1, None if scale is None else scale.repeat(n),
                                 None if bias is None else bias.repeat(n), None, relu)[0])
    B, D, H, W, _ = x.shape
    y = ys[0] if len(ys) == 1 else torch.cat(ys, -1)
    out = torch.empty(B, 2 * D, 2 * H, 2 * W, Co, dtype=torch.float32, device=x.device)
    _call("stx_depth_to_space", _p(y), _p(out), B, D, H, W, Co, 0)
    return out


# --------------------------------------------------------------------------------------- FeatureAtt gate
class GateFn(torch.autograd.Function):
    """cv [B, D, H, W, C] * sigmoid(att [B, H, W, C]) (reference IGEVStereo/submodule.py:238-240), one pass; backward one
    pass over (g, cv) with the gate's gradient summed over D in registers."""

    @staticmethod
    def forward(ctx, cv, att):
        out = gate(cv.detach(), att.detach())
        ctx.save_for_backward(cv, att)
        return out

    @staticmethod
    def backward(ctx, g):
        cv, att = ctx.saved_tensors
        g = g.contiguous()
        B, D, H, W, C = cv.shape
        gcv = torch.empty_like(cv) if ctx.needs_input_grad[0] else None
        gatt = torch.empty_like(att) if ctx.needs_input_grad[1] else None
        if gcv is not None or gatt is not None:
            _call("stx_gate_bwd", _p(g), _p(cv), _p(att), _p(gcv), _p(gatt), B, D, H * W, C)
        return gcv, gatt


@fp32_region
def gate(cv, att):
    """cv [B, D, H, W, C] (dense NDHWC) * sigmoid(att [B, H, W, C]) broadcast over D; differentiable."""
    if torch.is_grad_enabled() and (cv.requires_grad or att.requires_grad):
        return GateFn.apply(cv.contiguous(), att.contiguous())
    cv, att = cv.contiguous(), att.contiguous()
    _chk(cv, "cv", 5)
    _chk(att, "att", 4)
    B, D, H, W, C = cv.shape
    if att.shape != (B, H, W, C) or C % 4:
        raise StxError(f"gate: volume {tuple(cv.shape)} vs gate {tuple(att.shape)} (need [B,H,W,C], C % 4 == 0)")
    out = torch.empty_like(cv)
    _call("stx_gate_fwd", _p(cv), _p(att), _p(out), B, D, H * W, C)
    return out


# --------------------------------------------------------------------------------------- channels-last <-> channel-major
class ChannelMajorFn(torch.autograd.Function):
    """NCHW-logical tensor stored channels-last (dense [B, H, W, C]) -> the same values stored NCHW-contiguous, through the
    tiled transpose kernel (stx_transpose); backward: the inverse transpose, so the gradient goes back dense in the
    producer's layout (torch's `contiguous()` takes its generic strided copy both ways: 0.10 ms per 320 x 144 x 240 map, and
    its backward hands the producer an NCHW gradient that every channels-last consumer re-lays again)."""

    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        out = torch.empty((B, C, H, W), dtype=x.dtype, device=x.device)
        _call("stx_transpose", _p(x.permute(0, 2, 3, 1)), _p(out), B, H * W, C)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, C, H, W = g.shape
        gx = torch.empty((B, H, W, C), dtype=g.dtype, device=g.device)
        _call("stx_transpose", _p(g), _p(gx), B, C, H * W)
        return gx.permute(0, 3, 1, 2)


@fp32_region
def channel_major(x):
    """`x.contiguous()` for a 4-D NCHW-logical tensor: a no-op for NCHW-contiguous input, the transpose kernel for dense
    channels-last fp32 input whose H*W and C are multiples of 4, torch's copy otherwise."""
    if x.is_contiguous():
        return x
    if (x.dim() == 4 and x.dtype == torch.float32 and on_device(x) and x.is_contiguous(memory_format=torch.channels_last)
            and x.shape[1] % 4 == 0 and (x.shape[2] * x.shape[3]) % 4 == 0):
        return ChannelMajorFn.apply(x)
    return x.contiguous()


# --------------------------------------------------------------------------------------- channel concatenation
class CatChannelsFn(torch.autograd.Function):
    """Dense channels-last tensors [..., C_k] -> [..., sum C_k] in one coalesced pass (stx_concat_channels); backward: one
    pass that writes the dense per-part gradients (stx_split_channels).  Reference: `torch.cat(..., dim=1)` of the feature
    extractors (gwcnet.py:59, acv.py:48)."""

    @staticmethod
    def forward(ctx, *parts):
        ctx.cs = [int(p.shape[-1]) for p in parts]
        nvox = parts[0].numel() // ctx.cs[0]
        out = parts[0].new_empty(*parts[0].shape[:-1], sum(ctx.cs))
        ptrs = [_p(p) for p in parts] + [None] * (4 - len(parts))
        cs = ctx.cs + [0] * (4 - len(parts))
        _call("stx_concat_channels", *ptrs, *cs, _p(out), nvox)
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        nvox = g.numel() // g.shape[-1]
        outs = [g.new_empty(*g.shape[:-1], c) if need else None for c, need in zip(ctx.cs, ctx.needs_input_grad)]
        if any(o is not None for o in outs):
            # (a part that needs no gradient still gets a destination: the kernel writes every part)
            dst = [o if o is not None else g.new_empty(*g.shape[:-1], c) for o, c in zip(outs, ctx.cs)]
            ptrs = [_p(o) for o in dst] + [None] * (4 - len(dst))
            cs = ctx.cs + [0] * (4 - len(dst))
            _call("stx_split_channels", _p(g), *ptrs, *cs, nvox)
        return tuple(outs)


@fp32_region
def cat_channels(parts):
    """Concatenate 2-4 dense channels-last tensors of equal leading shape along their LAST (channel) axis; every width a
    multiple of 4.  Differentiable."""
    parts = [p.contiguous() for p in parts]
    if not 2 <= len(parts) <= 4:
        raise StxError(f"cat_channels: {len(parts)} parts (2 to 4)")
    lead = parts[0].shape[:-1]
    for p in parts:
        if p.shape[:-1] != lead or p.shape[-1] % 4 or p.dtype != torch.float32 or p.device != parts[0].device:
            raise StxError(f"cat_channels: parts {[tuple(q.shape) for q in parts]} (equal leading shape, fp32, widths % 4 == 0)")
    return CatChannelsFn.apply(*parts)


# --------------------------------------------------------------------------------------- 2-D convolution (feature CNN)
def conv2d_supported(conv):
    """Whether an nn.Conv2d is one csrc/conv2d.hip serves in BOTH directions: 3x3, stride 1, padding 1, dilation 1, dense, no
    bias, 32 or 64 input AND output channels (the data gradient's GEMM-K is the layer's output width)."""
    return (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.in_channels in (32, 64) and conv.out_channels in (32, 64))


def _ohwi(w):
    """[Co][Ci][3][3] parameter -> dense [Co][3][3][Ci] (a view when the parameter is stored channels_last, as the extractors
    keep theirs: features2d.channels_last_weights_)."""
    v = w.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def conv2d_forward(x, w, dgrad=False, groups=1, want_stats=False):
    """x dense [B, H, W, Cin]; w the layer's parameter [Co][Ci][3][3].  dgrad=False: conv(x, w) -> [B, H, W, Co]; dgrad=True: x is
    the output gradient [B, H, W, Co] -> the input gradient [B, H, W, Ci].  want_stats: also the per-workgroup (sum, sum of
    squares) rows of the raw output, [rows, 2, C] ([groups, rows / groups, 2, C]: per-view statistics) -> bn_finalize."""
    _chk(x, "x", 4)
    wo = _ohwi(w)
    _chk(wo, "weight", 4)
    B, H, W, Cin = x.shape
    Co, Ci = w.shape[0], w.shape[1]
    Kin, Nout = (Co, Ci) if dgrad else (Ci, Co)
    if Cin != Kin or B % groups:
        raise StxError(f"conv2d: input {tuple(x.shape)} against weight {tuple(w.shape)} (dgrad={dgrad}, groups={groups})")
    out = torch.empty(B, H, W, Nout, dtype=torch.float32, device=x.device)
    part = None
    if want_stats:
        rows = int(get_lib().raw("stx_conv2d_stat_rows")(groups))
        part = torch.empty(rows, 2, Nout, dtype=torch.float32, device=x.device)
    _call("stx_conv2d_fwd", _p(x), _p(wo), _p(out), _p(part), B, H, W, Kin, Nout, int(dgrad), groups)
    if part is not None and groups > 1:
        part = part.view(groups, rows // groups, 2, Nout)
    return out, part


class Conv2dFn(torch.autograd.Function):
    """z = conv2d(x, w) (3x3, stride 1, padding 1) of the 2-D feature CNN's BasicBlocks on csrc/conv2d.hip: forward and data
    gradient hand-written, the weight gradient stays MIOpen's (aten.convolution_backward).  x NCHW-logical channels_last;
    returns z as dense [B, H, W, Co] and the BatchNorm statistics rows of z (not differentiable)."""

    @staticmethod
    def forward(ctx, x, w, groups):
        xl = x.permute(0, 2, 3, 1)
        if not xl.is_contiguous():
            xl = xl.contiguous()
        z, part = conv2d_forward(xl, w, False, groups, True)
        ctx.save_for_backward(x, w)
        ctx.mark_non_differentiable(part)
        return z, part

    @staticmethod
    def backward(ctx, gz, _gpart):
        x, w = ctx.saved_tensors
        gz = gz.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = conv2d_forward(gz, w, True)[0].permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            gw = torch.ops.aten.convolution_backward(gz.permute(0, 3, 1, 2), x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                     (False, True, False))[1]
        return gx, gw, None


# --------------------------------------------------------------------------------------- batch norm
def bn_finalize(partials, count, gamma, beta, running_mean, running_var, momentum, eps, groups=1):
    """partials [rows, 2, C] ([groups, rows, 2, C] for groups > 1) -> scale, shift, mean, invstd ([C] each, [groups, C] for
    groups > 1: one launch, running statistics updated slab after slab)."""
    C = partials.shape[-1]
    out = torch.empty(4, groups, C, dtype=torch.float32, device=partials.device)
    _call("stx_bn_finalize_groups", _p(partials), partials.shape[-3], C, float(count), _p(gamma), _p(beta),
          _p(running_mean), _p(running_var), float(momentum), float(eps), _p(out), groups)
    return list(out.unbind(0)) if groups > 1 else list(out[:, 0].unbind(0))   # scale, shift, mean, invstd


@fp32_region
def bn_stats(z, groups=1):
    """Per-workgroup (sum, sum of squares) rows of a dense channels-last activation [..., C] -> [rows, 2, C]
    ([groups, rows, 2, C] for groups > 1: the leading axis of z splits into `groups` equal slabs with their own
    statistics): the batch statistics input of bn_finalize for producers without a fused epilogue (the 2-D feature
    CNN's MIOpen convolutions)."""
    _chk(z, "z")
    C = z.shape[-1]
    nvox = z.numel() // C // groups
    if groups < 1 or z.shape[0] % groups:
        raise StxError(f"bn_stats: leading axis {z.shape[0]} does not split into {groups} groups")
    rows = get_lib().raw("stx_bn_stats_rows")(nvox, C)
    if rows <= 0:
        raise StxError(f"bn_stats: C={C} unsupported")
    part = torch.empty(groups, rows, 2, C, dtype=torch.float32, device=z.device)
    _call("stx_bn_stats", _p(z), _p(part), nvox, C, groups)
    return part if groups > 1 else part[0]


def _sync_bn_partials(partials, count, group, world):
    """SyncBatchNorm forward: sum the conv-epilogue partials (sum z, sum z^2 per channel) over the replicas.
    The local rows are reduced in fp64, all-reduced in fp64 (2C values: latency-bound, RCCL), and handed to
    stx_bn_finalize as two fp32 rows hi + lo so that its fp64 accumulation sees the exact global sums
    (E[z^2] - mean^2 cancels badly on single-precision totals).  Equal per-replica batches are assumed, as
    DistributedSampler(drop_last=True) guarantees (trainer_torchrun.py:130-136)."""
    import torch.distributed as dist
    tot = partials.double().sum(0)                 # [2, C]
    dist.all_reduce(tot, group=group)
    hi = tot.float()
    lo = (tot - hi.double()).float()
    return torch.stack((hi, lo)).contiguous(), count * world


@fp32_region
def bn_apply(z1, scale1, shift1, z2=None, scale2=None, shift2=None, relu=False, groups=1):
    out = torch.empty_like(z1)
    C = z1.shape[-1]
    _call("stx_bn_apply", _p(z1), _p(scale1), _p(shift1), _p(z2), _p(scale2), _p(shift2), _p(out),
          z1.numel() // C // groups, C, int(relu), groups)
    return out


class BnActFn(torch.autograd.Function):
    """y = act(BN1(z1) [+ BN2(z2)] [+ residual]) with batch statistics (train) or running statistics
    (eval with grad).  `bn1`/`bn2` are dicts: gamma, beta, running_mean, running_var, momentum, eps,
    training, partials (conv-epilogue sums) and count.
    groups > 1: the leading axis of z1 (z2, residual) splits into `groups` equal slabs with their OWN batch statistics
    (partials [groups, rows, 2, C], count = voxels per slab); the running statistics are updated slab after slab, as
    separate forward calls would (the two views of the 2-D feature CNN, reference gwcnet.py:172-173)."""

    @staticmethod
    def forward(ctx, z1, gamma1, beta1, z2, gamma2, beta2, residual, relu, bn1, bn2, groups=1, defer=False):
        G = int(groups)
        # defer: z1 is the raw output of a 3x3x3 stride-1 convolution whose backward node folds this BatchNorm's
        # backward-apply pass into its weight-gradient kernel (conv_block sets it; see _PendingBn)
        ctx.defer = bool(defer)

        def affine(gamma, beta, bn):
            if bn["training"]:
                partials, count = bn["partials"], bn["count"]
                if bn.get("sync"):
                    if G > 1:
                        raise StxError("BnActFn: SyncBatchNorm with groups is not wired (SyncBN runs the views separately)")
                    partials, count = _sync_bn_partials(partials, count, *bn["sync"])
                return bn_finalize(partials, count, gamma, beta, bn["running_mean"], bn["running_var"], bn["momentum"],
                                   bn["eps"], G)                                              # [C] each ([G, C] for G > 1)
            invstd = torch.rsqrt(bn["running_var"] + bn["eps"])
            scale = gamma * invstd
            res = (scale, beta - bn["running_mean"] * scale, bn["running_mean"].clone(), invstd)
            return res if G == 1 else [t.unsqueeze(0).expand(G, -1).contiguous() for t in res]

        relu = int(relu)                                  # activation code: 0 none, 1 ReLU, 2 Mish
        if relu == 2 and residual is not None:            # (before anything is launched or any running statistic moves)
            raise StxError("BnActFn: Mish with a plain residual is not wired (no model of the family uses it)")
        if G < 1 or z1.shape[0] % G:
            raise StxError(f"BnActFn: leading axis {z1.shape[0]} does not split into {G} groups")
        sc1, sh1, m1, i1 = affine(gamma1, beta1, bn1)
        two = z2 is not None
        if two:
            sc2, sh2, m2, i2 = affine(gamma2, beta2, bn2)
            y = bn_apply(z1, sc1, sh1, z2, sc2, sh2, relu, G)
        else:
            sc2 = sh2 = m2 = i2 = None
            y = bn_apply(z1, sc1, sh1, residual, None, None, relu, G)
        ctx.relu, ctx.two, ctx.has_res, ctx.groups = relu, two, residual is not None, G
        ctx.train1 = bn1["training"]
        ctx.train2 = bn2["training"] if two else False
        ctx.sync = bn1.get("sync") or (bn2.get("sync") if two else None)
        # ReLU mask for the backward pass: a block without a plain residual recomputes sign(y) from z1 / z2 and the
        # scale / shift vectors used above (bit-identical expression, operands the backward kernels read anyway), so
        # the activated volume is not kept alive by this node and not re-read by its two backward passes
        ctx.remask = bool(relu) and residual is None
        keep_y = y if (relu and not ctx.remask) else None
        ctx.save_for_backward(z1, gamma1, m1, i1, z2, gamma2, m2, i2, keep_y, sc1 if ctx.remask else None,
                              sh1 if ctx.remask else None, sc2 if (ctx.remask and two) else None,
                              sh2 if (ctx.remask and two) else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        z1, gamma1, m1, i1, z2, gamma2, m2, i2, y, sc1, sh1, sc2, sh2 = ctx.saved_tensors
        gy = gy.contiguous()
        G = ctx.groups
        C = z1.shape[-1]
        nvox = z1.numel() // C // G                       # voxels per group
        lib = get_lib()
        NB = lib.raw("stx_bn_reduce_blocks")()
        part = _WS.get("bnred", G * NB * 3 * C, z1.device)
        # (groups > 1: one more slab = the total over the groups, written by the same launch)
        sums_all = torch.empty(G + (1 if G > 1 else 0), 3, C, dtype=torch.float32, device=z1.device)
        sums = sums_all[:G]
        _call("stx_bn_bwd_reduce2", _p(gy), _p(y), _p(z1), _p(m1), _p(i1), _p(z2) if ctx.two else None,
              _p(m2) if ctx.two else None, _p(i2) if ctx.two else None, _p(sc1), _p(sh1), _p(sc2), _p(sh2), _p(part),
              _p(sums_all), nvox, C, int(ctx.relu), G)
        if not ctx.needs_input_grad[0] and not ctx.two and not ctx.has_res:
            # nobody differentiates z1 (frozen convolution weight AND an input without gradient, e.g. a BatchNorm-only
            # fine-tune behind a frozen backbone): only the gamma / beta gradients are wanted -- no apply pass, and in
            # particular no deferred record that no convolution backward would ever consume
            tot = sums_all[G] if G > 1 else sums_all[0]
            return (None, tot[1], tot[0], None, None, None, None, None, None, None, None, None)
        if (ctx.defer and not ctx.two and not ctx.has_res and ctx.relu in (0, 1) and ctx.train1 and not ctx.sync and G == 1
                and (not ctx.relu or ctx.remask)):
            # the record travels on a FRESH alias of the gradient: only the node that receives this very return value (z1's
            # producer) can see it -- `gy` itself may also be delivered to other nodes by an add's fan-out
            alias = gy.view_as(gy)
            pend = _PendingBn()
            pend.g, pend.z, pend.scale, pend.shift, pend.mean, pend.invstd = alias, z1, sc1, sh1, m1, i1
            pend.gamma, pend.sums, pend.inv_n, pend.act = gamma1, sums, 1.0 / nvox, int(ctx.relu)
            if pend.scale is None:                     # (no activation: the mask operands were not saved; any finite pair does)
                pend.scale = pend.shift = m1
            _defer_pending_bn(alias, pend)
            tot = sums_all[0]
            return (alias, tot[1], tot[0], None, None, None, None, None, None, None, None, None)
        dz1 = torch.empty_like(z1)
        dz2 = torch.empty_like(z2) if ctx.two else None
        gres = torch.empty_like(z1) if (ctx.has_res and ctx.relu) else None
        use = sums
        if ctx.sync:
            # SyncBatchNorm: the centering terms are means over ALL replicas; the kernel divides by the local voxel
            # count, so hand it (sum over replicas) / world.  Parameter gradients stay local (DDP averages them).
            import torch.distributed as dist
            use = sums.clone()
            dist.all_reduce(use, group=ctx.sync[0])
            use /= ctx.sync[1]
        if not ctx.train1 or (ctx.two and not ctx.train2):
            # running-stat BN: no centering terms (mixed train/eval pairs are not used by these models)
            use = torch.zeros_like(sums)
        _call("stx_bn_bwd_apply2", _p(gy), _p(y), _p(z1), _p(m1), _p(i1), _p(gamma1), _p(z2) if ctx.two else None,
              _p(m2) if ctx.two else None, _p(i2) if ctx.two else None, _p(gamma2) if ctx.two else None, _p(sc1), _p(sh1),
              _p(sc2), _p(sh2), _p(use), _p(dz1), _p(dz2), _p(gres), nvox, C, int(ctx.relu), G)
        if ctx.has_res and not ctx.relu:
            gres = gy
        tot = sums_all[G] if G > 1 else sums_all[0]       # gamma / beta are shared between the groups
        # (beta2's gradient equals beta1's; it gets its OWN memory: two parameters whose .grad alias one buffer are scaled twice
        # by every in-place pass over the gradients -- GradScaler.unscale_, clip_grad_norm_ -- found by tests/test_amp.py)
        return (dz1, tot[1], tot[0], dz2, tot[2] if ctx.two else None, tot[0].clone() if ctx.two else None, gres,
                None, None, None, None, None)


# --------------------------------------------------------------------------------------- activations
class MishFn(torch.autograd.Function):
    """y = x * tanh(softplus(x)) (PCWNet/CFNet `Mish` / `FMish`, models/PCWNet/submodule.py:11-18,178-190)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _chk(x, "x")
        y = torch.empty_like(x)
        _call("stx_mish_fwd", _p(x), _p(y), x.numel())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        _call("stx_mish_bwd", _p(gy), _p(x), _p(gx), x.numel())
        return gx


@fp32_region
def mish(x):
    """Mish on a dense fp32 tensor with numel % 4 == 0 (every channels-last activation of these models)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return MishFn.apply(x)
    x = x.contiguous()
    _chk(x, "x")
    y = torch.empty_like(x)
    _call("stx_mish_fwd", _p(x), _p(y), x.numel())
    return y


# --------------------------------------------------------------------------------------- cost volume
def _cv_shapes(Lg, Lc, num_groups):
    ref = Lg if Lg is not None else Lc
    B, _, H, W = ref.shape
    Cg = Lg.shape[1] if Lg is not None else 0
    Cc = Lc.shape[1] if Lc is not None else 0
    G = num_groups if Lg is not None else 0
    return B, H, W, Cg, G, Cc


@fp32_region
def cost_volume_forward(Lg, Rg, Lc, Rc, maxdisp, num_groups, mask_left=True, scale=None):
    for n, t in (("ref gwc", Lg), ("tgt gwc", Rg), ("ref concat", Lc), ("tgt concat", Rc)):
        _chk(t, n, 4)
    B, H, W, Cg, G, Cc = _cv_shapes(Lg, Lc, num_groups)
    if G:
        assert Cg % G == 0   # reference models/GwcNet/submodule.py:46
    vol = torch.empty(B, maxdisp, H, W, G + 2 * Cc, dtype=torch.float32, device=(Lg if Lg is not None else Lc).device)
    _call("stx_cost_volume_fwd", _p(Lg), _p(Rg), Cg, G, _p(Lc), _p(Rc), Cc, _p(scale), _p(vol), B, H, W, maxdisp,
          int(mask_left))
    return vol


class CostVolumeFn(torch.autograd.Function):
    """Fused gwc + concat volume, NDHWC output [B, D, H, W, G + 2*Cc]."""

    @staticmethod
    def forward(ctx, Lg, Rg, Lc, Rc, maxdisp, num_groups, mask_left):
        ctx.save_for_backward(Lg, Rg)
        ctx.cfg = (maxdisp, num_groups, mask_left, None if Lc is None else Lc.shape)
        return cost_volume_forward(Lg, Rg, Lc, Rc, maxdisp, num_groups, mask_left)

    @staticmethod
    def backward(ctx, gvol):
        Lg, Rg = ctx.saved_tensors
        maxdisp, num_groups, mask_left, cshape = ctx.cfg
        gvol = gvol.contiguous()
        B, D, H, W, CT = gvol.shape
        Cg = Lg.shape[1] if Lg is not None else 0
        G = num_groups if Lg is not None else 0
        Cc = cshape[1] if cshape is not None else 0
        gLg = torch.empty_like(Lg) if G else None
        gRg = torch.empty_like(Rg) if G else None
        gLc = gvol.new_empty(cshape) if Cc else None
        gRc = gvol.new_empty(cshape) if Cc else None
        _call("stx_cost_volume_bwd", _p(gvol), _p(Lg), _p(Rg), Cg, G, Cc, _p(gLg), _p(gRg), _p(gLc), _p(gRc), B, H, W,
              D, int(mask_left))
        return gLg, gRg, gLc, gRc, None, None, None


class GroupNormalizeFn(torch.autograd.Function):
    """y = out_scale * x / max(||x||_2 over each group's channels, 1e-12), per pixel (stx_group_normalize_fwd / _bwd):
    F.normalize(x.view(B, G, C/G, H, W), dim=2) of FoundationStereo's group-wise correlation (submodule.py:388-397)."""

    @staticmethod
    def forward(ctx, x, num_groups, out_scale):
        x = x.contiguous()
        _chk(x, "x", 4)
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        _call("stx_group_normalize_fwd", _p(x), _p(y), B, C, num_groups, H * W, float(out_scale))
        ctx.save_for_backward(x)
        ctx.cfg = (num_groups, float(out_scale))
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = gy.contiguous()
        B, C, H, W = x.shape
        gx = torch.empty_like(x)
        _call("stx_group_normalize_bwd", _p(x), _p(gy), _p(gx), B, C, ctx.cfg[0], H * W, ctx.cfg[1])
        return gx, None, None


@fp32_region
def group_normalize(x, num_groups, out_scale=1.0):
    """[B, C, H, W] -> every group of C / num_groups channels scaled to unit L2 norm at every pixel (times out_scale)."""
    assert x.dim() == 4 and x.shape[1] % num_groups == 0, f"C:{x.shape[1]}, num_groups:{num_groups}"   # submodule.py:390
    return GroupNormalizeFn.apply(channel_major(x), num_groups, out_scale)


@fp32_region
def cost_volume(Lg, Rg, Lc, Rc, maxdisp, num_groups, mask_left=True, normalize=False):
    """normalize=True: FoundationStereo's volume (submodule.py:388-413) -- cosine similarity per group (unit-norm groups,
    group SUM): the two gwc maps go through group_normalize first, the left one scaled by C/G so that the builder's group
    mean is the sum."""
    if normalize and Lg is not None:
        Lg = group_normalize(Lg, num_groups, float(Lg.shape[1] // num_groups))
        Rg = group_normalize(Rg, num_groups, 1.0)
    ts = [channel_major(t) if t is not None else None for t in (Lg, Rg, Lc, Rc)]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        return CostVolumeFn.apply(*ts, maxdisp, num_groups, mask_left)
    return cost_volume_forward(*ts, maxdisp, num_groups, mask_left)


class SampledVolumeFn(torch.autograd.Function):
    """CFNet cascade-stage volume (stx_sampled_volume_fwd / _bwd): NDHWC [B, S, H, W, CTp], channels = G group
    correlations | Cc left concat | Cc warped right concat | the hypothesis itself | zero pad to a multiple of 8."""

    @staticmethod
    def forward(ctx, Lg, Rg, Lc, Rc, samples, num_groups):
        B, H, W, Cg, G, Cc = _cv_shapes(Lg, Lc, num_groups)
        S = samples.shape[1]
        CTp = (G + 2 * Cc + 1 + 7) // 8 * 8
        vol = torch.empty(B, S, H, W, CTp, dtype=torch.float32, device=samples.device)
        _call("stx_sampled_volume_fwd", _p(Lg), _p(Rg), Cg, G, _p(Lc), _p(Rc), Cc, _p(samples), _p(vol), B, H, W, S, CTp)
        ctx.save_for_backward(Lg, Rg, samples)
        ctx.cfg = (G, Cg, Cc, None if Lc is None else Lc.shape)
        return vol

    @staticmethod
    def backward(ctx, gvol):
        Lg, Rg, samples = ctx.saved_tensors
        G, Cg, Cc, cshape = ctx.cfg
        gvol = gvol.contiguous()
        B, S, H, W, CTp = gvol.shape
        gLg = torch.empty_like(Lg) if G else None
        gRg = torch.empty_like(Rg) if G else None
        gLc = gvol.new_empty(cshape) if Cc else None
        gRc = gvol.new_empty(cshape) if Cc else None
        _call("stx_sampled_volume_bwd", _p(gvol), _p(Lg), _p(Rg), Cg, G, Cc, _p(samples), _p(gLg), _p(gRg), _p(gLc),
              _p(gRc), B, H, W, S, CTp)
        return gLg, gRg, gLc, gRc, None, None


@fp32_region
def sampled_volume(Lg, Rg, Lc, Rc, samples, num_groups):
    """Cascade-stage cost volume from per-pixel disparity hypotheses `samples` [B, S, H, W] (integer-valued floats, no
    gradient): see include/stx_hip.h.  The channel axis is padded with zeros to a multiple of 8; `conv_block` accepts
    such a volume for a convolution whose weight has the un-padded input width."""
    ts = [channel_major(t) if t is not None else None for t in (Lg, Rg, Lc, Rc)]
    for n, t in (("ref gwc", ts[0]), ("tgt gwc", ts[1]), ("ref concat", ts[2]), ("tgt concat", ts[3])):
        _chk(t, n, 4)
    samples = samples.detach().contiguous()
    _chk(samples, "samples", 4)
    if ts[0] is not None:
        assert ts[0].shape[1] % num_groups == 0   # reference models/CFNet/submodule.py:165
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        return SampledVolumeFn.apply(*ts, samples, num_groups)
    return SampledVolumeFn.forward(_NoCtx(), *ts, samples, num_groups)


class _NoCtx:
    """Stand-in for the autograd context when a Function's forward is used without a graph."""

    def save_for_backward(self, *a):
        pass

    def mark_non_differentiable(self, *a):
        pass


# --------------------------------------------------------------------------------------- PCWNet / CFNet 2-D helpers (row f-1)
class WarpFn(torch.autograd.Function):
    """reference PCWNet/submodule.py:137-176 (`warp`): stx_warp_fwd / stx_warp_bwd."""

    @staticmethod
    def forward(ctx, x, disp):
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        _call("stx_warp_fwd", _p(x), _p(disp), _p(out), B, C, H, W)
        ctx.save_for_backward(x, disp)
        return out

    @staticmethod
    def backward(ctx, g):
        x, disp = ctx.saved_tensors
        B, C, H, W = x.shape
        g = g.contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gd = torch.empty_like(disp) if ctx.needs_input_grad[1] else None
        _call("stx_warp_bwd", _p(g), _p(x), _p(disp), _p(gx), _p(gd), B, C, H, W)
        return gx, gd


@fp32_region
def warp(x, disp):
    """x [B,C,H,W] sampled at column w - disp[B,1,H,W] (bilinear, the reference's grid), zeroed where the footprint leaves
    the image.  Differentiable in x and disp like the reference."""
    x, disp = x.contiguous(), disp.contiguous()
    _chk(x, "x", 4)
    _chk(disp, "disp", 4)
    if disp.shape != (x.shape[0], 1, x.shape[2], x.shape[3]):
        raise StxError(f"warp: disp {tuple(disp.shape)} does not match x {tuple(x.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or disp.requires_grad):
        return WarpFn.apply(x, disp)
    return WarpFn.forward(_NoCtx(), x, disp)


class CorrVolumeFn(torch.autograd.Function):
    """reference PCWNet/submodule.py:121-135 (`build_corrleation_volume`): stx_corr_volume_fwd / _bwd."""

    @staticmethod
    def forward(ctx, ref, tgt, maxdisp, groups):
        B, C, H, W = ref.shape
        vol = torch.empty(B, groups, 2 * maxdisp + 1, H, W, dtype=torch.float32, device=ref.device)
        _call("stx_corr_volume_fwd", _p(ref), _p(tgt), _p(vol), B, C, H, W, maxdisp, groups)
        ctx.save_for_backward(ref, tgt)
        ctx.cfg = (maxdisp, groups)
        return vol

    @staticmethod
    def backward(ctx, g):
        ref, tgt = ctx.saved_tensors
        B, C, H, W = ref.shape
        g = g.contiguous()
        gr = torch.empty_like(ref) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(tgt) if ctx.needs_input_grad[1] else None
        _call("stx_corr_volume_bwd", _p(g), _p(ref), _p(tgt), _p(gr), _p(gt), B, C, H, W, *ctx.cfg)
        return gr, gt, None, None


@fp32_region
def corr_volume(ref, tgt, maxdisp, groups):
    """[B,C,H,W] x 2 -> [B, groups, 2*maxdisp+1, H, W] (see include/stx_hip.h for the slice semantics)."""
    ref, tgt = ref.contiguous(), tgt.contiguous()
    _chk(ref, "ref", 4)
    _chk(tgt, "tgt", 4)
    if ref.shape != tgt.shape:
        raise StxError(f"corr_volume: ref {tuple(ref.shape)} vs tgt {tuple(tgt.shape)}")
    if torch.is_grad_enabled() and (ref.requires_grad or tgt.requires_grad):
        return CorrVolumeFn.apply(ref, tgt, int(maxdisp), int(groups))
    return CorrVolumeFn.forward(_NoCtx(), ref, tgt, int(maxdisp), int(groups))


class DisparityVarianceFn(torch.autograd.Function):
    """reference CFNet/submodule.py:128-140 (`disparity_variance`, `disparity_variance_confidence`)."""

    @staticmethod
    def forward(ctx, x, disp, samples):
        B, D = x.shape[0], x.shape[1]
        HW = x.shape[2] * x.shape[3]
        out = torch.empty(B, 1, x.shape[2], x.shape[3], dtype=torch.float32, device=x.device)
        _call("stx_disparity_variance_fwd", _p(x), _p(disp), _p(samples), _p(out), B, D, HW)
        ctx.save_for_backward(x, disp, samples)
        return out

    @staticmethod
    def backward(ctx, g):
        x, disp, samples = ctx.saved_tensors
        B, D = x.shape[0], x.shape[1]
        HW = x.shape[2] * x.shape[3]
        g = g.contiguous()
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[0] else None
        gd = torch.empty_like(disp) if need[1] else None
        gs = torch.empty_like(samples) if (samples is not None and need[2]) else None
        if gx is None and gd is None and gs is None:
            return None, None, None
        _call("stx_disparity_variance_bwd", _p(g), _p(x), _p(disp), _p(samples), _p(gx), _p(gd), _p(gs), B, D, HW)
        return gx, gd, gs


@fp32_region
def disparity_variance(x, disp, samples=None):
    """sum_d x_d (d - disp)^2 (samples None) or sum_d x_d (disp - samples_d)^2 -> [B,1,H,W]."""
    x, disp = x.contiguous(), disp.contiguous()
    _chk(x, "x", 4)
    _chk(disp, "disparity", 4)
    if disp.shape != (x.shape[0], 1, x.shape[2], x.shape[3]):
        raise StxError(f"disparity_variance: disparity {tuple(disp.shape)} does not match x {tuple(x.shape)}")
    if samples is not None:
        samples = samples.contiguous()
        _chk(samples, "samples", 4)
        if samples.shape != x.shape:
            raise StxError(f"disparity_variance: samples {tuple(samples.shape)} vs x {tuple(x.shape)}")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, disp, samples)):
        return DisparityVarianceFn.apply(x, disp, samples)
    return DisparityVarianceFn.forward(_NoCtx(), x, disp, samples)


class AcVolumeFn(torch.autograd.Function):
    """ACVNet attention concat volume: softmax(att, dim=2) * concat_volume (acv.py:196), left half
    unmasked (ACVNet/submodule.py:180-191).  prob: [B, D, H, W] softmax probabilities."""

    @staticmethod
    def forward(ctx, Lc, Rc, prob, maxdisp):
        ctx.save_for_backward(Lc, Rc, prob)
        ctx.maxdisp = maxdisp
        return cost_volume_forward(None, None, Lc, Rc, maxdisp, 0, mask_left=False, scale=prob)

    @staticmethod
    def backward(ctx, gvol):
        Lc, Rc, prob = ctx.saved_tensors
        gvol = gvol.contiguous()
        B, D, H, W, CT = gvol.shape
        Cc = Lc.shape[1]
        gprob = torch.empty_like(prob)
        gL, gR = torch.empty_like(Lc), torch.empty_like(Rc)
        if D * W * 4 <= 150 * 1024:
            # one pass over the gradient volume (the [D][W] image of gprob lives in LDS)
            _call("stx_ac_volume_bwd", _p(gvol), _p(Lc), _p(Rc), _p(prob), _p(gL), _p(gR), _p(gprob), B, Cc, H, W, D, 0)
            return gL, gR, gprob, None
        _call("stx_cost_volume_scale_bwd", _p(gvol), _p(Lc), _p(Rc), _p(gprob), B, Cc, H, W, D, 0)
        scaled = torch.empty_like(gvol)
        _call("stx_scale_channels", _p(gvol), _p(prob), _p(scaled), B * D * H * W, CT)
        _call("stx_cost_volume_bwd", _p(scaled), None, None, 0, 0, Cc, None, None, _p(gL), _p(gR), B, H, W, D, 0)
        return gL, gR, gprob, None


@fp32_region
def ac_volume(Lc, Rc, prob, maxdisp):
    Lc, Rc, prob = Lc.contiguous(), Rc.contiguous(), prob.contiguous()
    if torch.is_grad_enabled() and (Lc.requires_grad or Rc.requires_grad or prob.requires_grad):
        return AcVolumeFn.apply(Lc, Rc, prob, maxdisp)
    return cost_volume_forward(None, None, Lc, Rc, maxdisp, 0, mask_left=False, scale=prob)


class DwConvHWFn(torch.autograd.Function):
    """Depth-wise (1,3,3) convolution with per-channel-quad dilation on an NDHWC volume.
    w: [C, 9]; dil: int32 [C/4] device tensor."""

    @staticmethod
    def forward(ctx, x, w, dil):
        _chk(x, "x", 5)
        B, D, H, W, C = x.shape
        out = torch.empty_like(x)
        _call("stx_dwconv_hw_fwd", _p(x), _p(w), _p(dil), _p(out), B, D, H, W, C, 0)
        ctx.save_for_backward(x, w, dil)
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w, dil = ctx.saved_tensors
        gy = gy.contiguous()
        B, D, H, W, C = x.shape
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _call("stx_dwconv_hw_fwd", _p(gy), _p(w), _p(dil), _p(gx), B, D, H, W, C, 1)
        if ctx.needs_input_grad[1]:
            ws = _WS.get("dwwgrad", get_lib().raw("stx_dwconv_hw_wgrad_workspace_floats")(C), x.device)
            gw = torch.empty_like(w)
            _call("stx_dwconv_hw_wgrad", _p(x), _p(gy), _p(dil), _p(gw), _p(ws), B, D, H, W, C)
        return gx, gw, None


@fp32_region
def dwconv_hw(x, w, dil):
    w = w.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        return DwConvHWFn.apply(x, w, dil)
    B, D, H, W, C = x.shape
    out = torch.empty_like(x)
    _call("stx_dwconv_hw_fwd", _p(x), _p(w), _p(dil), _p(out), B, D, H, W, C, 0)
    return out


# --------------------------------------------------------------------------------------- head
class HeadFn(torch.autograd.Function):
    """trilinear upsample -> softmax over D -> soft-argmin, fused. cost: [B, D', H', W'] dense.
    align_corners=False: GwcNet / PSMNet / ACVNet heads; True: PCWNet / CFNet heads."""

    @staticmethod
    def forward(ctx, cost, maxdisp, H, W, align_corners=False):
        _chk(cost, "cost", 4)
        B, Dc, Hc, Wc = cost.shape
        disp = torch.empty(B, H, W, dtype=torch.float32, device=cost.device)
        stats = torch.empty(B, H, W, 2, dtype=torch.float32, device=cost.device)
        if align_corners:
            _call("stx_head_fwd2", _p(cost), _p(disp), _p(stats), B, Dc, Hc, Wc, maxdisp, H, W, 1)
        else:
            _call("stx_head_fwd", _p(cost), _p(disp), _p(stats), B, Dc, Hc, Wc, maxdisp, H, W)
        ctx.save_for_backward(cost, disp, stats)
        ctx.cfg = (maxdisp, H, W, bool(align_corners))
        return disp

    @staticmethod
    def backward(ctx, g):
        cost, disp, stats = ctx.saved_tensors
        maxdisp, H, W, ac = ctx.cfg
        B, Dc, Hc, Wc = cost.shape
        gc = torch.empty_like(cost)
        g = g.contiguous()      # keep the dense copy alive across the launch
        ws = _WS.get("headbwd", get_lib().raw("stx_head_bwd_workspace_floats")(B, Dc, H, W), cost.device)
        if ac:
            _call("stx_head_bwd2", _p(g), _p(cost), _p(disp), _p(stats), _p(gc), _p(ws), B, Dc, Hc, Wc, maxdisp, H, W, 1)
        else:
            _call("stx_head_bwd", _p(g), _p(cost), _p(disp), _p(stats), _p(gc), _p(ws), B, Dc, Hc, Wc, maxdisp, H, W)
        return gc, None, None, None, None


@fp32_region
def regression_head(cost, maxdisp, H, W, align_corners=False):
    """cost [B, D', H', W'] (or [B,1,D',H',W'] / NDHWC with C=1) -> disparity [B, H, W]."""
    if cost.dim() == 5:
        cost = cost.reshape(cost.shape[0], *_squeeze_c(cost))
    return HeadFn.apply(cost.contiguous(), maxdisp, H, W, align_corners)


def _squeeze_c(cost):
    """Shape of a 5-D single-channel cost ([B,1,D,H,W] or [B,D,H,W,1]) without the channel axis."""
    if cost.shape[1] == 1:
        return tuple(cost.shape[2:])
    if cost.shape[-1] == 1:
        return tuple(cost.shape[1:4])
    raise StxError(f"regression_head: expected a single-channel cost, got {tuple(cost.shape)}")


@fp32_region
def softargmax(x, maxdisp, keepdim):
    """sum_d d * x[b,d,h,w] (disparity_regression / disparityregression / softargmax estimator)."""
    assert len(x.shape) == 4   # reference models/GwcNet/submodule.py:24
    _chk(x.contiguous(), "x", 4)
    x = x.contiguous()
    B, D, H, W = x.shape
    if D != maxdisp:
        raise StxError(f"disparity_regression: volume has {D} disparities, maxdisp={maxdisp}")
    if torch.is_grad_enabled() and x.requires_grad:
        # linear map: gradient is d broadcast -- keep autograd simple with a tiny custom function
        out = _SoftArgmaxFn.apply(x)
    else:
        out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
        _call("stx_softargmax_fwd", _p(x), _p(out), B, D, H * W)
    return out.unsqueeze(1) if keepdim else out


class _SoftArgmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, D, H, W = x.shape
        out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
        _call("stx_softargmax_fwd", _p(x), _p(out), B, D, H * W)
        ctx.D = D
        return out

    @staticmethod
    def backward(ctx, g):
        d = torch.arange(ctx.D, dtype=g.dtype, device=g.device).view(1, ctx.D, 1, 1)
        return g.unsqueeze(1) * d


@fp32_region
def argmax_disparity(x):
    _chk(x.contiguous(), "x", 4)
    x = x.contiguous()
    B, D, H, W = x.shape
    out = torch.empty(B, 1, H, W, dtype=torch.int64, device=x.device)
    _call("stx_argmax_fwd", _p(x), _p(out), B, D, H * W)
    return out


class _ModalFn(torch.autograd.Function):
    """Modal estimators with autograd: the support mask is a constant of the graph (the reference multiplies by
    `mask.data` / boolean masks), so d out / d x_k = m_k (k - out) / S; the forward pass saves the support and its
    mass per pixel ([B,5,H,W]) for the backward kernel."""

    @staticmethod
    def forward(ctx, x, kind):
        B, D, H, W = x.shape
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device)
        aux = torch.empty(B, 5, H, W, dtype=torch.float32, device=x.device)
        _call("stx_modal_fwd", _p(x), _p(out), _p(aux), B, D, H * W, kind)
        ctx.save_for_backward(out, aux)
        ctx.D = D
        return out

    @staticmethod
    def backward(ctx, g):
        out, aux = ctx.saved_tensors
        B, _, H, W = out.shape
        g = g.contiguous()
        gx = torch.empty(B, ctx.D, H, W, dtype=torch.float32, device=out.device)
        _call("stx_modal_bwd", _p(g), _p(out), _p(aux), _p(gx), B, ctx.D, H * W)
        return gx, None


def _modal_estimator(kind, x, maxdisp):
    assert len(x.shape) == 4
    name = ("unimodal", "dominant_modal")[kind]
    x = x.contiguous()
    _chk(x, "x", 4)
    B, D, H, W = x.shape
    if D != maxdisp:
        raise StxError(f"{name}_disparity_estimator: volume has {D} disparities, maxdisp={maxdisp}")
    if torch.is_grad_enabled() and x.requires_grad:
        return _ModalFn.apply(x, kind)
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device)
    _call("stx_modal_fwd", _p(x), _p(out), None, B, D, H * W, kind)
    return out


@fp32_region
def unimodal_disparity(x, maxdisp):
    """Expectation over the mode containing the arg-max (unimodal_disparity_estimator.py:4-25) -> [B,1,H,W];
    differentiable w.r.t. x inside the (constant) mode mask, like the reference."""
    return _modal_estimator(0, x, maxdisp)


@fp32_region
def dominant_modal_disparity(x, maxdisp):
    """Expectation over the heavier of the two main modes of the blurred volume
    (dominant_modal_disparity_estimator.py:35-54) -> [B,1,H,W]; differentiable like the reference."""
    return _modal_estimator(1, x, maxdisp)


class _SplitModeFn(torch.autograd.Function):
    """mode = x * mask with the mask a constant of the graph (boolean in the reference): d mode / d x = mask."""

    @staticmethod
    def forward(ctx, x):
        B, D, H, W = x.shape
        mode = torch.empty_like(x)
        mask = torch.empty(B, D, H, W, dtype=torch.bool, device=x.device)
        _call("stx_split_mode", _p(x), _p(mode), _p(mask), B, D, H * W)
        ctx.save_for_backward(mask)
        ctx.mark_non_differentiable(mask)
        return mode, mask

    @staticmethod
    def backward(ctx, g, _gmask):
        (mask,) = ctx.saved_tensors
        return g * mask


@fp32_region
def split_mode(x, maxdisp=192):
    """(mode, mask) of loss_functions/split_mode.py:9-35: the support of the mode around the per-pixel arg-max of the
    probability volume x [B, D, H, W] (twin of the modal estimators' mask, on the raw volume) as a bool tensor, and
    mode = x * mask.  One kernel, the volume read once (the reference builds ~12 full-volume temporaries)."""
    assert len(x.shape) == 4
    x = x.contiguous()
    _chk(x, "x", 4)
    N, D, H, W = x.shape
    assert D == maxdisp
    if torch.is_grad_enabled() and x.requires_grad:
        return _SplitModeFn.apply(x)
    mode = torch.empty_like(x)
    mask = torch.empty(N, D, H, W, dtype=torch.bool, device=x.device)
    _call("stx_split_mode", _p(x), _p(mode), _p(mask), N, D, H * W)
    return mode, mask


@fp32_region
def softmax_over_d(x):
    """x [B, D, H, W] -> softmax over D."""
    _chk(x, "x", 4)
    B, D, H, W = x.shape
    y = torch.empty_like(x)
    _call("stx_softmax_d_fwd", _p(x), _p(y), B, D, H * W)
    return y


# --------------------------------------------------------------------------------------- IGEV geometry-encoding lookup
def geo_pyramid_floats(rows, length, channels, levels):
    """Floats of a pixel-major pyramid (include/stx_hip.h, geo_lookup.hip): level i is [rows][length >> i][channels]."""
    n = int(get_lib().raw("stx_geo_pyramid_floats")(rows, length, channels, levels))
    if n <= 0:
        raise StxError(f"geometry pyramid: bad shape rows={rows} length={length} channels={channels} levels={levels}")
    return n


class _PyramidGrads:
    """The gradient buffers of the two pyramids of one `Combined_Geo_Encoding_Volume` (or of the one pyramid of a RAFT-family
    `CorrBlock1D`, Corr1dLookupFn below), shared by all of its lookups within
    one backward pass: stx_geo_lookup_bwd ADDS into the rows a pixel owns, so the 22-32 lookups of a training step
    accumulate in place instead of handing autograd one dense pyramid-sized tensor per iteration.  The hand-off: the lookups
    do not read the pyramid tensors the build node returns (the public `geo_volume_pyramid` / `init_corr_pyramid`) but
    aliases of them behind an identity node (GeoPyramidHubFn) that nothing else can consume.  The lookup that runs first
    returns the buffers to that node, the others add into them and return nothing; the engine runs the identity node only
    after every lookup of the pass has run, and it alone passes the finished buffers on to the build node and drops them
    here.  Any other consumer of the public pyramid tensors therefore meets ONE complete gradient per pyramid at the build
    node and is summed with it in autograd's ordinary way.  Keyed by the autograd graph-task id: a second backward pass
    (retained graph) starts from zeros."""

    def __init__(self):
        self.task, self.bufs = None, None

    def take(self, device, *sizes):
        """(first lookup of this backward pass?, one zeroed buffer per size: (ggpyr, gcpyr) / (gcpyr,))"""
        task = torch._C._current_graph_task_id()
        first = self.bufs is None or task != self.task
        if first:
            self.task = task
            self.bufs = tuple(torch.zeros(n, dtype=torch.float32, device=device) for n in sizes)
        return first, self.bufs

    def release(self):
        self.bufs = None


class GeoPyramidFn(torch.autograd.Function):
    """geometry.py:14-30: all-pairs row correlation (MFMA) with its pooled levels, and the pixel-major pyramid of the
    geometry volume; vol dense [B, D, H, W, C], fmaps NCHW -> (gpyr, cpyr) flat buffers."""

    @staticmethod
    def forward(ctx, vol, f1, f2, levels):
        B, D, H, W, C = vol.shape
        Cf, W2 = f1.shape[1], f2.shape[3]
        gpyr = torch.empty(geo_pyramid_floats(B * H * W, D, C, levels), dtype=torch.float32, device=vol.device)
        cpyr = torch.empty(geo_pyramid_floats(B * H * W, W2, 1, levels), dtype=torch.float32, device=vol.device)
        _call("stx_geo_pyramid_fwd", _p(vol), _p(gpyr), B, D, H, W, C, levels)
        _call("stx_geo_corr_fwd", _p(f1), _p(f2), _p(cpyr), B, Cf, H, W, W2, levels)
        ctx.save_for_backward(f1, f2)
        ctx.cfg = (B, D, H, W, C, Cf, W2, levels)
        return gpyr, cpyr

    @staticmethod
    def backward(ctx, ggp, gcp):
        f1, f2 = ctx.saved_tensors
        B, D, H, W, C, Cf, W2, levels = ctx.cfg
        gvol = gf1 = gf2 = None
        if ggp is not None and ctx.needs_input_grad[0]:
            gvol = torch.empty(B, D, H, W, C, dtype=torch.float32, device=f1.device)
            _call("stx_geo_pyramid_bwd", _p(ggp.contiguous()), _p(gvol), B, D, H, W, C, levels)
        if gcp is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            gf1 = torch.empty_like(f1) if ctx.needs_input_grad[1] else None
            gf2 = torch.empty_like(f2) if ctx.needs_input_grad[2] else None
            _call("stx_geo_corr_bwd", _p(gcp.contiguous()), _p(f1), _p(f2), _p(gf1), _p(gf2), B, Cf, H, W, W2, levels)
        return gvol, gf1, gf2, None


class GeoPyramidHubFn(torch.autograd.Function):
    """Identity on the two pyramids, between the build node and the lookups of one object (see _PyramidGrads): the outputs
    alias the inputs (no copy, no launch) and are read by the lookups only, so this node receives the shared gradient
    buffers alone and hands them on once every lookup of the backward pass has added its part."""

    @staticmethod
    def forward(ctx, gpyr, cpyr, grads):
        ctx.grads = grads
        return gpyr.view_as(gpyr), cpyr.view_as(cpyr)

    @staticmethod
    def backward(ctx, ggp, gcp):
        ctx.grads.release()
        return ggp, gcp, None


def geo_lookup_pyramids(gpyr, cpyr, grads):
    """The pyramid tensors the lookups of one object read: (gpyr, cpyr) themselves where no graph is recorded, their aliases
    behind GeoPyramidHubFn otherwise."""
    if torch.is_grad_enabled() and (gpyr.requires_grad or cpyr.requires_grad):
        return GeoPyramidHubFn.apply(gpyr, cpyr, grads)
    return gpyr, cpyr


@fp32_region
def geo_pyramids(vol, fmap1, fmap2, levels):
    """vol: dense [B, D, H, W, C] geometry volume; fmap1 [B, Cf, H, W], fmap2 [B, Cf, H, W2] -> (gpyr, cpyr)."""
    f1, f2 = channel_major(fmap1), channel_major(fmap2)
    _chk(vol, "geo_volume", 5)
    _chk(f1, "init_fmap1", 4)
    _chk(f2, "init_fmap2", 4)
    B, D, H, W, C = vol.shape
    if f1.shape[0] != B or f1.shape[2:] != (H, W) or f2.shape[:3] != f1.shape[:3]:
        raise StxError(f"geometry encoding: volume {tuple(vol.shape)} (B, D, H, W, C) and feature maps {tuple(f1.shape)} / "
                       f"{tuple(f2.shape)} do not match")
    if C % 4:
        raise StxError(f"geometry encoding: the volume's channel count ({C}) must be a multiple of 4")
    if torch.is_grad_enabled() and (vol.requires_grad or f1.requires_grad or f2.requires_grad):
        return GeoPyramidFn.apply(vol, f1, f2, levels)
    return GeoPyramidFn.forward(_NoCtx(), vol, f1, f2, levels)


class GeoCorrFn(torch.autograd.Function):
    """Combined_Geo_Encoding_Volume.corr (geometry.py:62-70): [B, H, W1, 1, W2] all-pairs row correlation."""

    @staticmethod
    def forward(ctx, f1, f2):
        B, C, H, W1 = f1.shape
        W2 = f2.shape[3]
        corr = torch.empty(B, H, W1, 1, W2, dtype=torch.float32, device=f1.device)
        _call("stx_geo_corr_fwd", _p(f1), _p(f2), _p(corr), B, C, H, W1, W2, 1)
        ctx.save_for_backward(f1, f2)
        return corr

    @staticmethod
    def backward(ctx, g):
        f1, f2 = ctx.saved_tensors
        B, C, H, W1 = f1.shape
        gf1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        gf2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        _call("stx_geo_corr_bwd", _p(g.contiguous()), _p(f1), _p(f2), _p(gf1), _p(gf2), B, C, H, W1, f2.shape[3], 1)
        return gf1, gf2


@fp32_region
def geo_corr(fmap1, fmap2):
    f1, f2 = channel_major(fmap1), channel_major(fmap2)
    _chk(f1, "fmap1", 4)
    _chk(f2, "fmap2", 4)
    if f1.shape[:3] != f2.shape[:3]:
        raise StxError(f"corr: feature maps {tuple(f1.shape)} / {tuple(f2.shape)} do not match")
    if torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad):
        return GeoCorrFn.apply(f1, f2)
    return GeoCorrFn.forward(_NoCtx(), f1, f2)


class GeoLookupFn(torch.autograd.Function):
    """One call of Combined_Geo_Encoding_Volume (geometry.py:35-59) on stx_geo_lookup_fwd / _bwd.  cfg = (B, H, W, D, C, W2,
    levels, radius).  Gradients go to the two pyramids only, accumulated through `grads` (_PyramidGrads)."""

    @staticmethod
    def forward(ctx, gpyr, cpyr, disp, coords, cfg, grads):
        B, H, W, D, C, W2, levels, radius = cfg
        out = torch.empty(B, levels * (C + 1) * (2 * radius + 1), H, W, dtype=torch.float32, device=disp.device)
        _call("stx_geo_lookup_fwd", _p(gpyr), _p(cpyr), _p(disp), _p(coords), _p(out), *cfg)
        ctx.save_for_backward(disp, coords)
        ctx.cfg, ctx.grads, ctx.sizes = cfg, grads, (gpyr.numel(), cpyr.numel())
        return out

    @staticmethod
    def backward(ctx, gout):
        disp, coords = ctx.saved_tensors
        first, (ggp, gcp) = ctx.grads.take(disp.device, *ctx.sizes)
        _call("stx_geo_lookup_bwd", _p(gout.contiguous()), _p(disp), _p(coords), _p(ggp), _p(gcp), *ctx.cfg)
        if first:
            return ggp, gcp, None, None, None, None
        return None, None, None, None, None, None


@fp32_region
def geo_lookup(gpyr, cpyr, disp, coords, cfg, grads):
    """[B, levels * (C + 1) * (2 radius + 1), H, W]; disp [B, 1, H, W], coords: B * H * W values (the pixel's column)."""
    B, H, W = cfg[:3]
    if torch.is_grad_enabled() and (disp.requires_grad or coords.requires_grad):
        raise StxError("Combined_Geo_Encoding_Volume: `disp` / `coords` must not require grad -- the lookup is differentiated "
                       "with respect to the volumes only, as in the reference, which detaches disp before every call "
                       "(igev_stereo.py:238); pass disp.detach()")
    if disp.numel() != B * H * W or coords.numel() != B * H * W:
        raise StxError(f"Combined_Geo_Encoding_Volume: disp {tuple(disp.shape)} / coords {tuple(coords.shape)} do not match the "
                       f"volume's {B} x {H} x {W} pixels")
    disp, coords = disp.detach().contiguous(), coords.detach().contiguous()
    _chk(disp, "disp")
    _chk(coords, "coords")
    if torch.is_grad_enabled() and (gpyr.requires_grad or cpyr.requires_grad):
        return GeoLookupFn.apply(gpyr, cpyr, disp, coords, cfg, grads)
    return GeoLookupFn.forward(_NoCtx(), gpyr, cpyr, disp, coords, cfg, None)


# --------------------------------------------------------------------------------------- RAFT-family 1-D correlation lookup
def corr1d_pyramid_floats(rows, W2, levels):
    """Floats of the pixel-major correlation pyramid of csrc/corr1d.hip: level i is [rows][W2 >> i]."""
    n = int(get_lib().raw("stx_corr1d_pyramid_floats")(rows, W2, levels))
    if n <= 0:
        raise StxError(f"correlation pyramid: bad shape rows={rows} W2={W2} num_levels={levels} (1..4 levels)")
    return n


class Corr1dPyramidFn(torch.autograd.Function):
    """RAFTStereo/corr.py:110-125, 148-156: all-pairs row correlation / sqrt(C) (MFMA) with its pooled levels, one launch;
    fmaps NCHW -> the flat pixel-major pyramid."""

    @staticmethod
    def forward(ctx, f1, f2, levels):
        B, C, H, W1 = f1.shape
        W2 = f2.shape[3]
        scale = 1.0 / float(C) ** 0.5
        cpyr = torch.empty(corr1d_pyramid_floats(B * H * W1, W2, levels), dtype=torch.float32, device=f1.device)
        _call("stx_corr1d_pyramid_fwd", _p(f1), _p(f2), _p(cpyr), B, C, H, W1, W2, levels, scale)
        ctx.save_for_backward(f1, f2)
        ctx.cfg = (B, C, H, W1, W2, levels, scale)
        return cpyr

    @staticmethod
    def backward(ctx, gcp):
        f1, f2 = ctx.saved_tensors
        gf1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        gf2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        _call("stx_corr1d_pyramid_bwd", _p(gcp.contiguous()), _p(f1), _p(f2), _p(gf1), _p(gf2), *ctx.cfg)
        return gf1, gf2, None


class Corr1dHubFn(torch.autograd.Function):
    """GeoPyramidHubFn for the one pyramid of a CorrBlock1D: an alias that only the lookups read (see _PyramidGrads)."""

    @staticmethod
    def forward(ctx, cpyr, grads):
        ctx.grads = grads
        return cpyr.view_as(cpyr)

    @staticmethod
    def backward(ctx, gcp):
        ctx.grads.release()
        return gcp, None


def _corr1d_fmaps(fmap1, fmap2, who):
    f1, f2 = channel_major(fmap1), channel_major(fmap2)
    _chk(f1, "fmap1", 4)
    _chk(f2, "fmap2", 4)
    if f1.shape[:3] != f2.shape[:3]:
        raise StxError(f"{who}: feature maps {tuple(f1.shape)} / {tuple(f2.shape)} do not match")
    return f1, f2


@fp32_region
def corr1d_pyramid(fmap1, fmap2, levels, who="CorrBlock1D"):
    """fmap1 [B, C, H, W1], fmap2 [B, C, H, W2] -> the flat pyramid of `levels` levels (corr1d_pyramid_floats)."""
    f1, f2 = _corr1d_fmaps(fmap1, fmap2, who)
    if torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad):
        return Corr1dPyramidFn.apply(f1, f2, levels)
    return Corr1dPyramidFn.forward(_NoCtx(), f1, f2, levels)


def corr1d_lookup_pyramid(cpyr, grads):
    """The pyramid tensor the lookups of one object read: `cpyr` itself where no graph is recorded, its alias behind
    Corr1dHubFn otherwise."""
    if torch.is_grad_enabled() and cpyr.requires_grad:
        return Corr1dHubFn.apply(cpyr, grads)
    return cpyr


def _corr1d_jobs(jobs):
    """((level, radius, alpha, mult), ...) -> (the host array of the C-ABI, number of jobs, output channels)"""
    flat = [float(v) for job in jobs for v in job]
    return (ctypes.c_float * max(1, len(flat)))(*flat), len(jobs), sum(2 * int(job[1]) + 1 for job in jobs)


class Corr1dLookupFn(torch.autograd.Function):
    """One call of a RAFT-family correlation block on stx_corr1d_lookup_fwd / _bwd: every job of the call in one launch.
    cfg = (B, H, W1, W2, levels).  The gradient goes to the pyramid only, accumulated through `grads` (_PyramidGrads)."""

    @staticmethod
    def forward(ctx, cpyr, base, disp, jobs, cfg, grads):
        B, H, W1, W2, levels = cfg
        table, n, channels = _corr1d_jobs(jobs)
        out = torch.empty(B, channels, H, W1, dtype=torch.float32, device=base.device)
        _call("stx_corr1d_lookup_fwd", _p(cpyr), _p(base), _p(disp), table, n, _p(out), *cfg)
        ctx.save_for_backward(base, disp)
        ctx.cfg, ctx.jobs, ctx.grads, ctx.size = cfg, jobs, grads, cpyr.numel()
        return out

    @staticmethod
    def backward(ctx, gout):
        base, disp = ctx.saved_tensors
        table, n, _ = _corr1d_jobs(ctx.jobs)
        first, (gcp,) = ctx.grads.take(base.device, ctx.size)
        _call("stx_corr1d_lookup_bwd", _p(gout.contiguous()), _p(base), _p(disp), table, n, _p(gcp), *ctx.cfg)
        return (gcp if first else None), None, None, None, None, None


@fp32_region
def corr1d_lookup(cpyr, base, disp, jobs, cfg, grads, who="CorrBlock1D"):
    """[B, sum_j (2 r_j + 1), H, W1]; base (and disp, or None): B * H * W1 values; jobs: ((level, radius, alpha, mult), ...),
    sample positions (base - alpha * disp) * mult + k of the pixel's row of that level."""
    B, H, W1 = cfg[:3]
    for t in (base, disp):
        if t is not None and torch.is_grad_enabled() and t.requires_grad:
            raise StxError(f"{who}: the sampling positions must not require grad -- the lookup is differentiated with respect to "
                           "the feature maps only, as in the reference, which detaches them before every call "
                           "(raft_stereo.py:154, defom_stereo.py:142); pass coords.detach() / disp.detach()")
        if t is not None and t.numel() != B * H * W1:
            raise StxError(f"{who}: positions {tuple(t.shape)} do not match the pyramid's {B} x {H} x {W1} pixels")
    base = base.detach().contiguous()
    disp = None if disp is None else disp.detach().contiguous()
    _chk(base, "coords")
    _chk(disp, "disp")
    if torch.is_grad_enabled() and cpyr.requires_grad:
        return Corr1dLookupFn.apply(cpyr, base, disp, jobs, cfg, grads)
    return Corr1dLookupFn.forward(_NoCtx(), cpyr, base, disp, jobs, cfg, None)


# --------------------------------------------------------------------------------------- StereoAnywhere volume stage
ALLPAIRS_DISP_LEFT, ALLPAIRS_CONF_LEFT, ALLPAIRS_DISP_RIGHT, ALLPAIRS_CONF_RIGHT = 1, 2, 4, 8
ALLPAIRS_ALL = 15
ALLPAIRS_MAX_W = 512                                                     # csrc/allpairs.hip AP_MAX_W


class AllpairsEstimatesFn(torch.autograd.Function):
    """The estimates of StereoAnywhere/utils/utils.py:112-170 named by the bit mask `which`, from vol [B, H, W1, W2], on
    stx_allpairs_estimates_fwd / _bwd: one tensor per set bit, in bit order ([B, H, W1] left, [B, H, W2] right); ONE backward
    launch for all of them."""

    @staticmethod
    def forward(ctx, vol, which):
        B, H, W1, W2 = vol.shape
        outs = [torch.empty(B, H, W2 if bit & 12 else W1, dtype=torch.float32, device=vol.device) if which & bit else None
                for bit in (1, 2, 4, 8)]
        stats = None
        if not isinstance(ctx, _NoCtx):
            stats = torch.empty(4 * (B * H * W1 + B * H * W2), dtype=torch.float32, device=vol.device)
            ctx.set_materialize_grads(False)                             # an output the loss does not use: NULL, not zeros
        _call("stx_allpairs_estimates_fwd", _p(vol), which, *(_p(o) for o in outs), _p(stats), B, H, W1, W2)
        ctx.save_for_backward(vol, stats)
        ctx.which = which
        return tuple(o for o in outs if o is not None)

    @staticmethod
    def backward(ctx, *gouts):
        vol, stats = ctx.saved_tensors
        B, H, W1, W2 = vol.shape
        it = iter(gouts)
        grads = [next(it) if ctx.which & bit else None for bit in (1, 2, 4, 8)]
        grads = [None if g is None else g.contiguous() for g in grads]
        gvol = torch.empty_like(vol)
        _call("stx_allpairs_estimates_bwd", *(_p(g) for g in grads), _p(vol), _p(stats), _p(gvol), B, H, W1, W2)
        return gvol, None


@fp32_region
def allpairs_estimates(volume, which=ALLPAIRS_ALL):
    """volume [B, 1, H, W1, W2] (or [B, H, W1, W2]) -> (disp_left, conf_left, disp_right, conf_right), each [B, 1, H, W1] (left)
    / [B, 1, H, W2] (right) or None where its bit of `which` (ALLPAIRS_*) is not set.  2 <= W1, W2 <= 512."""
    if volume.dim() == 5 and volume.shape[1] == 1:
        vol = volume[:, 0]
    elif volume.dim() == 4:
        vol = volume
    else:
        raise StxError(f"allpairs_estimates: the volume must be [B, 1, H, W1, W2], got {tuple(volume.shape)}")
    if not isinstance(which, int) or not 0 < which <= ALLPAIRS_ALL:
        raise StxError(f"allpairs_estimates: `which` must be a mask of ALLPAIRS_* bits (1..15), got {which!r}")
    vol = vol.contiguous()
    _chk(vol, "volume", 4)
    W1, W2 = vol.shape[2:]
    if not (2 <= W1 <= ALLPAIRS_MAX_W and 2 <= W2 <= ALLPAIRS_MAX_W):
        raise StxError(f"allpairs_estimates: W1={W1} / W2={W2} outside the supported 2..{ALLPAIRS_MAX_W}")
    if torch.is_grad_enabled() and vol.requires_grad:
        got = AllpairsEstimatesFn.apply(vol, which)
    else:
        got = AllpairsEstimatesFn.forward(_NoCtx(), vol, which)
    it = iter(got)
    return tuple(next(it).unsqueeze(1) if which & bit else None for bit in (1, 2, 4, 8))


def _truncate_args(truncate, B, H, W1, who):
    """(disp_left, conf_left, attenuation_gain) -> (tdisp, tconf, atten): detached dense fp32 [B*H*W1] maps."""
    if truncate is None:
        return None, None, 0.0
    disp, conf, atten = truncate
    for t, name in ((disp, "disp_left"), (conf, "conf_left")):
        if t.numel() != B * H * W1:
            raise StxError(f"{who}: truncate {name} {tuple(t.shape)} does not match the volume's {B} x {H} x {W1} pixels")
    disp, conf = disp.detach().contiguous(), conf.detach().contiguous()
    _chk(disp, "disp_left")
    _chk(conf, "conf_left")
    return disp, conf, float(atten)


class Corr1dVolumePyramidFn(torch.autograd.Function):
    """StereoAnywhere/corr.py:85-91: the flat pixel-major pyramid whose level 0 is the given volume [B, H, W1, W2] (times the
    truncation factor where tdisp / tconf are given), one launch; differentiated with respect to the volume."""

    @staticmethod
    def forward(ctx, vol, tdisp, tconf, atten, levels):
        B, H, W1, W2 = vol.shape
        cpyr = torch.empty(corr1d_pyramid_floats(B * H * W1, W2, levels), dtype=torch.float32, device=vol.device)
        _call("stx_corr1d_volume_pyramid_fwd", _p(vol), _p(tdisp), _p(tconf), atten, _p(cpyr), B, H, W1, W2, levels)
        ctx.save_for_backward(tdisp, tconf)
        ctx.cfg = (atten, B, H, W1, W2, levels)
        return cpyr

    @staticmethod
    def backward(ctx, gcp):
        tdisp, tconf = ctx.saved_tensors
        atten, B, H, W1, W2, levels = ctx.cfg
        gvol = torch.empty(B, H, W1, W2, dtype=torch.float32, device=gcp.device)
        _call("stx_corr1d_volume_pyramid_bwd", _p(gcp.contiguous()), _p(tdisp), _p(tconf), atten, _p(gvol), B, H, W1, W2, levels)
        return gvol, None, None, None, None


@fp32_region
def corr1d_volume_pyramid(volume, levels, truncate=None, who="CorrBlock1D"):
    """volume [B, H, W1, 1, W2] (or [B, H, W1, W2]) -> the flat pyramid of `levels` levels (corr1d_pyramid_floats) with level 0 =
    the volume; truncate = (disp_left, conf_left, attenuation_gain) multiplies it by truncate_mask(..., conf_th=None) on the fly
    (the maps carry no gradient)."""
    if volume.dim() == 5 and volume.shape[3] == 1:
        vol = volume.squeeze(3)
    elif volume.dim() == 4:
        vol = volume
    else:
        raise StxError(f"{who}: the volume must be [B, H, W1, 1, W2], got {tuple(volume.shape)}")
    vol = vol.contiguous()
    _chk(vol, "fullcorr", 4)
    B, H, W1, W2 = vol.shape
    tdisp, tconf, atten = _truncate_args(truncate, B, H, W1, who)
    if torch.is_grad_enabled() and vol.requires_grad:
        return Corr1dVolumePyramidFn.apply(vol, tdisp, tconf, atten, levels)
    return Corr1dVolumePyramidFn.forward(_NoCtx(), vol, tdisp, tconf, atten, levels)


@fp32_region
def truncate_mask(disp_left, conf_left, conf_th=0.5, attenuation_gain=0.1):
    """truncate_corr_volume_v2 (StereoAnywhere/utils/utils.py:216-238): disp_left, conf_left [B, 1, H, W] -> [B, 1, H, W, W]
    (1 - c) + c (sigmoid((w - disp) - w') (1 - gain) + gain), c = conf_left or, with a threshold, conf_left > conf_th.  No
    gradient: the model detaches the mask (stereoanywhere.py:235)."""
    if disp_left.dim() != 4 or disp_left.shape[1] != 1 or conf_left.shape != disp_left.shape:
        raise StxError(f"truncate_mask: disp_left / conf_left must be [B, 1, H, W], got {tuple(disp_left.shape)} / "
                       f"{tuple(conf_left.shape)}")
    B, _, H, W = disp_left.shape
    disp, conf, atten = _truncate_args((disp_left, conf_left, attenuation_gain), B, H, W, "truncate_mask")
    mask = torch.empty(B, 1, H, W, W, dtype=torch.float32, device=disp.device)
    _call("stx_truncate_mask_fwd", _p(disp), _p(conf), int(conf_th is not None), float(conf_th or 0.0), atten, _p(mask), B, H, W)
    return mask


# --------------------------------------------------------------------------------------- StereoAnywhere mono-stereo alignment
MASKS_MAX_N = 64                                                         # csrc/mono_align.hip MA_MAX_N
MASKED_VOLUME_MAX_W = 2048                                               # MA_MAX_W
SOFTLRC_MAX_TH = 20.0                                                    # the linear branch of F.softplus starts above
SOFTLRC_BWD_MAX_W = 1024                                                 # MA_LRC_MAX_W
WEIGHTED_LSQ_MAX_N = 1 << 24                                             # torch.quantile's own limit


def _maps(who, shape_of, **maps):
    """Dense fp32 device maps of one shape [B, C, H, W] (`shape_of` names the first); refuses before any launch."""
    out, want = [], None
    for name, t in maps.items():
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or (shape_of == 1 and t.shape[1] != 1):
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise StxError(f"{who}: {name} must be [B, {'1' if shape_of == 1 else 'C'}, H, W], got {got}")
        if want is None:
            want = t.shape
        elif t.shape != want:
            raise StxError(f"{who}: {name} {tuple(t.shape)} does not match {tuple(want)}")
        t = t.contiguous()
        _chk(t, name, 4)
        out.append(t)
    return out


def _n_masks(who, N):
    if not isinstance(N, int) or isinstance(N, bool) or not 1 <= N <= MASKS_MAX_N:
        raise StxError(f"{who}: the number of masks must be an int in 1..{MASKS_MAX_N}, got {N!r}")
    return N


def generate_masks(mde, N=16):
    """generate_masks (StereoAnywhere/utils/utils.py:48-54): mde [B, 1, H, W] -> one-hot fp16 masks [B, N, H, W], channel i where
    f32(i / N) <= mde < f32((i + 1) / N) compared in fp32; values >= 1, negative values and NaN fall in no bin.  No gradient."""
    N = _n_masks("generate_masks", N)
    mde, = _maps("generate_masks", 1, mde=mde.detach() if isinstance(mde, torch.Tensor) else mde)
    B, _, H, W = mde.shape
    masks = torch.empty(B, N, H, W, dtype=torch.float16, device=mde.device)
    _call("stx_generate_masks_fwd", _p(mde), _p(masks), B, N, H, W)
    return masks


class MaskedVolumeFn(torch.autograd.Function):
    """volume * left_masks.unsqueeze(4) * right_masks.unsqueeze(3) (stereoanywhere.py:180,193) on stx_masked_volume_fwd / _bwd: the
    volume row is read once, the N output rows are written once; the backward gathers one channel row."""

    @staticmethod
    def forward(ctx, vol, ml, mr, N):
        B, H, W2, W3 = vol.shape
        out = torch.empty(B, N, H, W2, W3, dtype=torch.float32, device=vol.device)
        _call("stx_masked_volume_fwd", _p(vol), _p(ml), _p(mr), _p(out), B, N, H, W2, W3)
        ctx.save_for_backward(ml, mr)
        ctx.cfg = (B, N, H, W2, W3)
        return out

    @staticmethod
    def backward(ctx, g):
        ml, mr = ctx.saved_tensors
        B, N, H, W2, W3 = ctx.cfg
        gvol = torch.empty(B, H, W2, W3, dtype=torch.float32, device=g.device)
        _call("stx_masked_volume_bwd", _p(g.contiguous()), _p(ml), _p(mr), _p(gvol), B, N, H, W2, W3)
        return gvol, None, None, None


@fp32_region
def masked_volume(volume, mde_left, mde_right, n_masks):
    """volume [B, 1, H, W2, W3], mde_left [B, 1, H, W2], mde_right [B, 1, H, W3] -> contiguous fp32 [B, N, H, W2, W3] equal to
    volume * generate_masks(mde_left, N).unsqueeze(4) * generate_masks(mde_right, N).unsqueeze(3): out[n] = volume where both
    bins are n, exact zero elsewhere -- also where the volume is not finite (the reference's product gives NaN there).
    Differentiated with respect to the volume; the maps carry no gradient (the reference's masks are fp16 constants).  The maps
    are at the volume's resolution: for the reference's vol_downsample > 0 path (nearest-interpolated masks) pass the strided maps."""
    N = _n_masks("masked_volume", n_masks)
    if not isinstance(volume, torch.Tensor) or volume.dim() != 5 or volume.shape[1] != 1:
        raise StxError(f"masked_volume: the volume must be [B, 1, H, W2, W3], got {tuple(getattr(volume, 'shape', ()))}")
    for name, t in (("mde_left", mde_left), ("mde_right", mde_right)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 1:
            raise StxError(f"masked_volume: {name} must be [B, 1, H, W], got {tuple(getattr(t, 'shape', ()))}")
    B, _, H, W2, W3 = volume.shape
    if tuple(mde_left.shape) != (B, 1, H, W2) or tuple(mde_right.shape) != (B, 1, H, W3):
        raise StxError(f"masked_volume: maps {tuple(mde_left.shape)} / {tuple(mde_right.shape)} do not match the volume "
                       f"{tuple(volume.shape)}")
    if W3 > MASKED_VOLUME_MAX_W:
        raise StxError(f"masked_volume: W3={W3} above the supported {MASKED_VOLUME_MAX_W}")
    vol, ml, mr = volume[:, 0].contiguous(), mde_left.detach().contiguous(), mde_right.detach().contiguous()
    _chk(vol, "volume", 4)
    _chk(ml, "mde_left", 4)
    _chk(mr, "mde_right", 4)
    if torch.is_grad_enabled() and vol.requires_grad:
        return MaskedVolumeFn.apply(vol, ml, mr, N)
    return MaskedVolumeFn.forward(_NoCtx(), vol, ml, mr, N)


class SoftLrcFn(torch.autograd.Function):
    """softlrc (StereoAnywhere/utils/utils.py:189-198) on stx_softlrc_fwd / _bwd: both maps from one launch; the backward
    (direct term, sampled value, sample coordinate through relu) in two launches without atomics."""

    @staticmethod
    def forward(ctx, d2, d3, th):
        B, _, H, W = d2.shape
        out2, out3 = torch.empty_like(d2), torch.empty_like(d2)
        _call("stx_softlrc_fwd", _p(d2), _p(d3), th, _p(out2), _p(out3), B, H, W)
        if not isinstance(ctx, _NoCtx):
            ctx.set_materialize_grads(False)
        ctx.save_for_backward(d2, d3)
        ctx.th = th
        return out2, out3

    @staticmethod
    def backward(ctx, g2, g3):
        d2, d3 = ctx.saved_tensors
        B, _, H, W = d2.shape
        if g2 is None and g3 is None:
            return None, None, None
        g2, g3 = (None if g is None else g.contiguous() for g in (g2, g3))
        ws = torch.empty(4 * B * H * W, dtype=torch.float64, device=d2.device)
        gd2, gd3 = torch.empty_like(d2), torch.empty_like(d3)
        _call("stx_softlrc_bwd", _p(g2), _p(g3), _p(d2), _p(d3), ctx.th, _p(ws), _p(gd2), _p(gd3), B, H, W)
        return gd2, gd3, None


@fp32_region
def softlrc(disp2, disp3, lrc_th=1.0):
    """disp2, disp3 [B, 1, H, W] -> (softlrc2, softlrc3) = softplus(lrc_th - |disp - warped other|) / log(1 + e^lrc_th), the warp
    the reference's disp_warping (bilinear in both directions, zeros outside, relu on the warping disparity).  lrc_th <= 20."""
    if isinstance(lrc_th, bool) or not isinstance(lrc_th, (int, float)) or not lrc_th <= SOFTLRC_MAX_TH:
        raise StxError(f"softlrc: lrc_th must be a number <= {SOFTLRC_MAX_TH} (above it F.softplus turns linear), got {lrc_th!r}")
    d2, d3 = _maps("softlrc", 1, disp2=disp2, disp3=disp3)
    if torch.is_grad_enabled() and (d2.requires_grad or d3.requires_grad):
        if d2.shape[3] > SOFTLRC_BWD_MAX_W:
            raise StxError(f"softlrc: W={d2.shape[3]} above the {SOFTLRC_BWD_MAX_W} the backward supports")
        return SoftLrcFn.apply(d2, d3, float(lrc_th))
    return SoftLrcFn.forward(_NoCtx(), d2, d3, float(lrc_th))


class WeightedLsqFn(torch.autograd.Function):
    """weighted_lsq (StereoAnywhere/utils/utils.py:345-384) on stx_weighted_lsq_fwd / _bwd: one workgroup per image selects the
    quantile thresholds, sums and solves; nothing is read back by the host."""

    @staticmethod
    def forward(ctx, mde, disp, conf, qmin, qmax):
        B = mde.shape[0]
        n = mde.numel() // B
        scale = torch.empty(B, dtype=torch.float32, device=mde.device)
        shift = torch.empty(B, dtype=torch.float32, device=mde.device)
        stats = torch.empty(B, 8, dtype=torch.float64, device=mde.device)
        _call("stx_weighted_lsq_fwd", _p(mde), _p(disp), _p(conf), qmin, qmax, _p(scale), _p(shift), _p(stats), B, n)
        if not isinstance(ctx, _NoCtx):
            ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(stats)
        ctx.save_for_backward(mde, disp, conf, stats)
        return scale, shift, stats

    @staticmethod
    def backward(ctx, g_scale, g_shift, _g_stats):
        mde, disp, conf, stats = ctx.saved_tensors
        if g_scale is None and g_shift is None:
            return None, None, None, None, None
        B = mde.shape[0]
        g_scale, g_shift = (None if g is None else g.contiguous() for g in (g_scale, g_shift))
        grads = [torch.empty_like(t) for t in (mde, disp, conf)]
        _call("stx_weighted_lsq_bwd", _p(g_scale), _p(g_shift), _p(mde), _p(disp), _p(conf), _p(stats), *(_p(g) for g in grads), B,
              mde.numel() // B)
        return (*grads, None, None)


def _weighted_lsq(mde, disp, conf, min_quantile, max_quantile):
    for name, q in (("min_quantile", min_quantile), ("max_quantile", max_quantile)):
        if isinstance(q, bool) or not isinstance(q, (int, float)) or not 0.0 <= q <= 1.0:
            raise StxError(f"weighted_lsq: {name} must be a number in 0..1, got {q!r}")
    mde, disp, conf = _maps("weighted_lsq", 0, mde=mde, disp=disp, conf=conf)
    n = mde.numel() // max(1, mde.shape[0])
    if not 0 < n < WEIGHTED_LSQ_MAX_N:
        raise StxError(f"weighted_lsq: {n} elements per image outside 1..2^24 - 1 (the limit of torch.quantile itself)")
    if torch.is_grad_enabled() and (mde.requires_grad or disp.requires_grad or conf.requires_grad):
        return WeightedLsqFn.apply(mde, disp, conf, float(min_quantile), float(max_quantile))
    return WeightedLsqFn.forward(_NoCtx(), mde, disp, conf, float(min_quantile), float(max_quantile))


@fp32_region
def weighted_lsq(mde, disp, conf, min_quantile=0.2, max_quantile=0.9):
    """mde, disp, conf [B, C, H, W] -> (scale, shift), each [B, 1, 1, 1]: per image the weighted least-squares fit
    relu(disp) ~ scale |mde| + shift with weights 0.9 |conf| + 0.1 over the elements whose relu(disp) lies between its
    min_quantile and max_quantile (torch.quantile's fp32 values, bit for bit), from the 2 x 2 normal equations -- the solution the
    reference gets by QR.  Where their determinant is 0 (one distinct |mde|): scale 0, shift the weighted mean of relu(disp)
    (the reference's lstsq result there depends on the driver).  Inputs must be finite.  No host synchronisation."""
    scale, shift, _ = _weighted_lsq(mde, disp, conf, min_quantile, max_quantile)
    B = scale.shape[0]
    return scale.view(B, 1, 1, 1), shift.view(B, 1, 1, 1)


@fp32_region
def quantile_thresholds(disp, min_quantile=0.2, max_quantile=0.9):
    """The two thresholds `weighted_lsq` masks with, [B, 2] fp32: torch.quantile(relu(disp[b]).flatten(), q) for both q."""
    with torch.no_grad():
        _, _, stats = _weighted_lsq(disp, disp, disp, min_quantile, max_quantile)
    return stats[:, 5:7].float()


class MirrorDetectorFn(torch.autograd.Function):
    """handcrafted_mirror_detector (StereoAnywhere/utils/utils.py:255-269) on stx_mirror_detector_fwd / _bwd."""

    @staticmethod
    def forward(ctx, sd, md, sc, mc, th, gain):
        out = torch.empty_like(sd)
        _call("stx_mirror_detector_fwd", _p(sd), _p(md), _p(sc), _p(mc), th, gain, _p(out), sd.numel())
        ctx.save_for_backward(sd, md, sc, mc)
        ctx.cfg = (th, gain)
        return out

    @staticmethod
    def backward(ctx, g):
        sd, md, sc, mc = ctx.saved_tensors
        grads = [torch.empty_like(sd) for _ in range(4)]
        _call("stx_mirror_detector_bwd", _p(g.contiguous()), _p(sd), _p(md), _p(sc), _p(mc), *ctx.cfg, *(_p(t) for t in grads),
              sd.numel())
        return (*grads, None, None)


@fp32_region
def mirror_detector(stereo_disp, mono_disp, stereo_conf, mono_conf, conf_th=0.5, step_gain=20):
    """Four maps of one shape [B, C, H, W] -> sigmoid(step_gain (fuzzy_or(a, b) - conf_th)) with a = stereo_conf mono_conf
    sigmoid(step_gain (mono_disp - stereo_disp)), b = (1 - stereo_conf) mono_conf; differentiated with respect to all four."""
    for name, v in (("conf_th", conf_th), ("step_gain", step_gain)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise StxError(f"mirror_detector: {name} must be a number, got {v!r}")
    maps = _maps("mirror_detector", 0, stereo_disp=stereo_disp, mono_disp=mono_disp, stereo_conf=stereo_conf, mono_conf=mono_conf)
    if torch.is_grad_enabled() and any(t.requires_grad for t in maps):
        return MirrorDetectorFn.apply(*maps, float(conf_th), float(step_gain))
    return MirrorDetectorFn.forward(_NoCtx(), *maps, float(conf_th), float(step_gain))


class ContextUpsampleFn(torch.autograd.Function):
    """context_upsample (IGEVStereo/submodule.py:243-255) on stx_context_upsample_fwd / _bwd."""

    @staticmethod
    def forward(ctx, disp_low, up_weights):
        B, _, h, w = disp_low.shape
        out = torch.empty(B, 4 * h, 4 * w, dtype=torch.float32, device=disp_low.device)
        _call("stx_context_upsample_fwd", _p(disp_low), _p(up_weights), _p(out), B, h, w)
        ctx.save_for_backward(disp_low, up_weights)
        return out

    @staticmethod
    def backward(ctx, g):
        disp_low, up_weights = ctx.saved_tensors
        B, _, h, w = disp_low.shape
        gd = torch.empty_like(disp_low) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(up_weights) if ctx.needs_input_grad[1] else None
        _call("stx_context_upsample_bwd", _p(g.contiguous()), _p(disp_low), _p(up_weights), _p(gd), _p(gw), B, h, w)
        return gd, gw


@fp32_region
def context_upsample(disp_low, up_weights):
    """disp_low [B, 1, h, w], up_weights [B, 9, 4h, 4w] -> [B, 4h, 4w]."""
    disp_low, up_weights = disp_low.contiguous(), up_weights.contiguous()
    _chk(disp_low, "disp_low", 4)
    _chk(up_weights, "up_weights", 4)
    B, c, h, w = disp_low.shape
    if c != 1 or up_weights.shape != (B, 9, 4 * h, 4 * w):
        raise StxError(f"context_upsample: disp_low {tuple(disp_low.shape)} wants up_weights [B, 9, 4h, 4w], got "
                       f"{tuple(up_weights.shape)}")
    if torch.is_grad_enabled() and (disp_low.requires_grad or up_weights.requires_grad):
        return ContextUpsampleFn.apply(disp_low, up_weights)
    return ContextUpsampleFn.forward(_NoCtx(), disp_low, up_weights)


# --------------------------------------------------------------------------------------- convex upsampling from logits, sequence loss
CONVEX_FACTORS = (2, 4, 8)                                               # csrc/convex_upsample.hip


def _aligned16(t):
    """The kernels move whole output rows as 16-byte vectors: a dense tensor that starts inside a larger storage is copied."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class ConvexUpsampleFn(torch.autograd.Function):
    """upsample_flow / convex_upflow / upsample_disp (RAFTStereo/raft_stereo.py:81-93, StereoAnywhere/utils/utils.py:97-110,
    SelectiveRAFT/raft.py:72-84) on stx_convex_upsample_fwd / _bwd.  Saves the two inputs only: the backward re-forms the soft-max."""

    @staticmethod
    def forward(ctx, flow, mask, f, scale):
        N, D, H, W = flow.shape
        out = torch.empty(N, D, f * H, f * W, dtype=torch.float32, device=flow.device)
        _call("stx_convex_upsample_fwd", _p(flow), _p(mask), _p(out), N, D, H, W, mask.shape[1], f, scale)
        ctx.save_for_backward(flow, mask)
        ctx.cfg = (f, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        flow, mask = ctx.saved_tensors
        f, scale = ctx.cfg
        N, D, H, W = flow.shape
        gf = torch.empty_like(flow) if ctx.needs_input_grad[0] else None
        gm = torch.empty_like(mask) if ctx.needs_input_grad[1] else None
        ws = None
        if gf is not None:
            ws = _WS.get("convex_upsample_bwd", get_lib().raw("stx_convex_upsample_bwd_workspace_floats")(N, D, H, W), flow.device)
        _call("stx_convex_upsample_bwd", _p(_aligned16(g.contiguous())), _p(flow), _p(mask), _p(gf), _p(gm), _p(ws), N, D, H, W,
              mask.shape[1], f, scale)
        return gf, gm, None, None


@fp32_region
def convex_upsample(flow, mask, n_downsample=2, use_scale_factor=True):
    """flow [N, D, H, W], mask [N, 9 * 4^n, H, W] (the LOGITS of the mask head) -> [N, D, 2^n H, 2^n W]: the soft-max over the nine
    taps and the convex combination of the 3 x 3 neighbourhood of 2^n * flow (flow itself with use_scale_factor=False), one launch.
    n_downsample 1, 2 or 3.  A fp16 / bf16 mask (the reference's autocast) is taken as its fp32 cast and gets its gradient back in
    its own dtype; the flow is fp32.  Differentiable in both."""
    who = "convex_upsample"
    if flow.dim() != 4 or mask.dim() != 4:
        raise StxError(f"{who}: flow must be [N, D, H, W] and mask [N, 9 * 4^n, H, W], got {tuple(flow.shape)} / {tuple(mask.shape)}")
    if not isinstance(n_downsample, int) or 2 ** n_downsample not in CONVEX_FACTORS:
        raise StxError(f"{who}: n_downsample {n_downsample!r} is not built (factors {CONVEX_FACTORS}); flow {tuple(flow.shape)}, "
                       f"mask {tuple(mask.shape)}")
    f = 2 ** n_downsample
    N, D, H, W = flow.shape
    if D < 1 or mask.shape != (N, 9 * f * f, H, W):
        raise StxError(f"{who}: flow {tuple(flow.shape)} at n_downsample={n_downsample} wants mask {(N, 9 * f * f, H, W)}, got "
                       f"{tuple(mask.shape)}")
    if mask.dtype in _LOW:
        mask = mask.float()
    flow, mask = flow.contiguous(), mask.contiguous()
    _chk(flow, "flow", 4)
    _chk(mask, "mask", 4)
    scale = float(f) if use_scale_factor else 1.0
    if torch.is_grad_enabled() and (flow.requires_grad or mask.requires_grad):
        return ConvexUpsampleFn.apply(flow, mask, f, scale)
    return ConvexUpsampleFn.forward(_NoCtx(), flow, mask, f, scale)


class SoftmaxContextUpsampleFn(torch.autograd.Function):
    """context_upsample(scale * disp_low, softmax(logits, 1)) (IGEVStereo/igev_stereo.py:158-166) on
    stx_softmax_context_upsample_fwd / _bwd."""

    @staticmethod
    def forward(ctx, disp_low, logits, scale):
        B, _, h, w = disp_low.shape
        out = torch.empty(B, 4 * h, 4 * w, dtype=torch.float32, device=disp_low.device)
        _call("stx_softmax_context_upsample_fwd", _p(disp_low), _p(logits), _p(out), B, h, w, scale)
        ctx.save_for_backward(disp_low, logits)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        disp_low, logits = ctx.saved_tensors
        B, _, h, w = disp_low.shape
        gd = torch.empty_like(disp_low) if ctx.needs_input_grad[0] else None
        gl = torch.empty_like(logits) if ctx.needs_input_grad[1] else None
        ws = None
        if gd is not None:
            ws = _WS.get("convex_upsample_bwd", get_lib().raw("stx_convex_upsample_bwd_workspace_floats")(B, 1, h, w), disp_low.device)
        _call("stx_softmax_context_upsample_bwd", _p(_aligned16(g.contiguous())), _p(disp_low), _p(logits), _p(gd), _p(gl), _p(ws), B, h, w,
              ctx.scale)
        return gd, gl, None


@fp32_region
def softmax_context_upsample(disp_low, logits, scale=4.0):
    """disp_low [B, 1, h, w], logits [B, 9, 4h, 4w] -> [B, 4h, 4w] = context_upsample(scale * disp_low, softmax(logits, 1)) without
    the full-resolution soft-max pass or its saved output.  Differentiable in both."""
    who = "softmax_context_upsample"
    if disp_low.dim() != 4 or logits.dim() != 4 or disp_low.shape[1] != 1 or \
            logits.shape != (disp_low.shape[0], 9, 4 * disp_low.shape[2], 4 * disp_low.shape[3]):
        raise StxError(f"{who}: disp_low [B, 1, h, w] wants logits [B, 9, 4h, 4w], got {tuple(disp_low.shape)} / {tuple(logits.shape)}")
    if logits.dtype in _LOW:
        logits = logits.float()
    disp_low, logits = disp_low.contiguous(), _aligned16(logits.contiguous())
    _chk(disp_low, "disp_low", 4)
    _chk(logits, "logits", 4)
    if torch.is_grad_enabled() and (disp_low.requires_grad or logits.requires_grad):
        return SoftmaxContextUpsampleFn.apply(disp_low, logits, float(scale))
    return SoftmaxContextUpsampleFn.forward(_NoCtx(), disp_low, logits, float(scale))


def sequence_loss_max_predictions():
    return int(get_lib().raw("stx_sequence_loss_max_predictions")())


def _pointer_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class SequenceLossFn(torch.autograd.Function):
    """The trainer's loss over a list of predictions (trainer/trainer_torchrun.py:272-284) on stx_sequence_loss_fwd / _bwd."""

    @staticmethod
    def forward(ctx, gt, maxdisp, weights, *preds):
        K, n = len(preds), gt.numel()
        out = torch.empty(2, dtype=torch.float32, device=gt.device)            # the loss and, as an int, the valid count
        count = out[1:].view(torch.int32)
        ws = _WS.get("sequence_loss", get_lib().raw("stx_sequence_loss_workspace_floats")(n), gt.device)
        wts = (ctypes.c_double * K)(*weights)
        _call("stx_sequence_loss_fwd", _pointer_table(preds), wts, K, _p(gt), maxdisp, _p(out), _p(count), _p(ws), n)
        ctx.save_for_backward(gt, count, *preds)
        ctx.cfg = (maxdisp, tuple(weights))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        gt, count, *preds = ctx.saved_tensors
        maxdisp, weights = ctx.cfg
        K, n = len(preds), gt.numel()
        needs = ctx.needs_input_grad[3:]
        slab = torch.empty(sum(needs), n, dtype=torch.float32, device=gt.device)
        rows = iter(slab)
        grads = [next(rows).view(p.shape) if need else None for p, need in zip(preds, needs)]
        wts = (ctypes.c_double * K)(*weights)
        _call("stx_sequence_loss_bwd", _p(g.contiguous()), _pointer_table(preds), wts, K, _p(gt), maxdisp, _p(count),
              _pointer_table(grads), n)
        return (None, None, None, *grads)


def sequence_loss(preds, gt, maxdisp, weights):
    """sum_k weights[k] * mean_valid smooth_l1(preds[k], gt), valid = (gt > 0) & (gt < maxdisp - 1): the value of
    losses.masked_smooth_l1_multi, every prediction in ONE launch forward and one backward, no host sync.  preds: a list of
    [B, H, W] or [B, 1, H, W] fp32 tensors of gt's size; an empty mask gives 0 (and zero gradients); NaN / inf in gt is excluded."""
    who = "sequence_loss"
    preds, weights = list(preds), [float(w) for w in weights]
    if len(preds) != len(weights):
        raise ValueError(f"{who}: {len(preds)} predictions but {len(weights)} weights")
    limit = sequence_loss_max_predictions()
    if not 1 <= len(preds) <= limit:
        raise StxError(f"{who}: {len(preds)} predictions, one launch takes 1..{limit}")
    gt = gt.contiguous()
    _chk(gt, "gt")
    shape = tuple(gt.shape[:1]) + tuple(gt.shape[-2:])
    if gt.dim() not in (3, 4) or gt.numel() != shape[0] * shape[1] * shape[2]:
        raise StxError(f"{who}: gt must be [B, H, W] or [B, 1, H, W], got {tuple(gt.shape)}")
    dense = []
    for k, p in enumerate(preds):
        if p.dim() not in (3, 4) or tuple(p.shape[:1]) + tuple(p.shape[-2:]) != shape or p.numel() != gt.numel():
            raise StxError(f"{who}: prediction {k} is {tuple(p.shape)}, gt {tuple(gt.shape)}")
        p = p.contiguous()
        _chk(p, f"preds[{k}]")
        dense.append(p)
    if torch.is_grad_enabled() and any(p.requires_grad for p in dense):
        return SequenceLossFn.apply(gt, float(maxdisp), weights, *dense)
    return SequenceLossFn.forward(_NoCtx(), gt, float(maxdisp), weights, *dense)


# --------------------------------------------------------------------------------------- self-supervised losses
SSIM_WINDOWS = (3, 5, 7, 9, 11)                                          # csrc/selfsup_loss.hip SL_MAX_PAD
PHOTO_WINDOW = 7                                                         # photometric_loss calls ssim() with its default


def _images_are_data(who, **images):
    """The images of the self-supervised losses carry no gradient (as the positions of corr1d_lookup): one that asks for it raises."""
    for name, t in images.items():
        if t is not None and t.requires_grad and torch.is_grad_enabled():
            raise StxError(f"{who}: {name} requires grad, but the images are data here (no image gradient is built) -- detach() it")


def _image_pair(who, left, right, names=("left_image", "right_image")):
    left, right = left.contiguous(), right.contiguous()
    _chk(left, names[0])
    _chk(right, names[1])
    if left.dim() != 4 or left.shape != right.shape:
        raise StxError(f"{who}: {names[0]} / {names[1]} must be two [B, C, H, W] tensors of one shape, got {tuple(left.shape)} / "
                       f"{tuple(right.shape)}")
    return left, right


def _disp_map(who, disp, like):
    disp = disp.contiguous()
    _chk(disp, "disp")
    B, _, H, W = like.shape
    if disp.shape != (B, 1, H, W):
        raise StxError(f"{who}: disp must be [B, 1, H, W] = {(B, 1, H, W)}, got {tuple(disp.shape)}")
    if H < 2 or W < 2:
        raise StxError(f"{who}: the reference's sampling grid needs H, W >= 2, got {H} x {W}")
    return disp


def _window_fits(who, H, W, window):
    if H <= window // 2 or W <= window // 2:
        raise StxError(f"{who}: reflect padding by {window // 2} needs H, W > {window // 2}, got {H} x {W}")


class PhotoWarpFn(torch.autograd.Function):
    """warp_right_to_left (loss_functions/photometric_loss.py:5-37) on stx_photo_warp_fwd / _bwd; gradient to disp only."""

    @staticmethod
    def forward(ctx, right, disp):
        B, C, H, W = right.shape
        warped = torch.empty_like(right)
        valid = torch.empty(B, 1, H, W, dtype=torch.float32, device=right.device)
        _call("stx_photo_warp_fwd", _p(right), _p(disp), _p(warped), _p(valid), B, C, H, W)
        ctx.save_for_backward(right, disp)
        ctx.mark_non_differentiable(valid)
        return warped, valid

    @staticmethod
    def backward(ctx, g, _gvalid):
        right, disp = ctx.saved_tensors
        B, C, H, W = right.shape
        gdisp = torch.empty_like(disp)
        _call("stx_photo_warp_bwd", _p(g.contiguous()), _p(right), _p(disp), _p(gdisp), B, C, H, W)
        return None, gdisp


@fp32_region
def photo_warp(right_image, disp):
    """right_image [B, C, H, W], disp [B, 1, H, W] -> (warped, valid_mask), both [B, C, H, W] (the mask a broadcast view): the right
    image sampled at x = (w - disp) W / (W - 1) - 1/2, y = h H / (H - 1) - 1/2, bilinear with zeros outside -- the reference's
    linspace grid under align_corners=False, not `warp` above.  valid_mask is the summed weight of the in-image corners and carries
    no gradient; warped is differentiable in disp."""
    who = "photo_warp"
    right = right_image.contiguous()
    _chk(right, "right_image", 4)
    _images_are_data(who, right_image=right)
    disp = _disp_map(who, disp, right)
    if torch.is_grad_enabled() and disp.requires_grad:
        warped, valid = PhotoWarpFn.apply(right, disp)
    else:
        warped, valid = PhotoWarpFn.forward(_NoCtx(), right, disp)
    return warped, valid.expand_as(warped)


class SsimDistanceFn(torch.autograd.Function):
    """ssim (loss_functions/photometric_loss.py:40-77) on stx_ssim_fwd / _bwd."""

    @staticmethod
    def forward(ctx, x, y, window):
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        _call("stx_ssim_fwd", _p(x), _p(y), _p(out), B, C, H, W, window)
        ctx.save_for_backward(x, y)
        ctx.window = window
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        ws = _WS.get("ssim_bwd", get_lib().raw("stx_ssim_bwd_workspace_floats")(B, C, H, W), x.device)
        _call("stx_ssim_bwd", _p(g.contiguous()), _p(x), _p(y), _p(gx), _p(gy), _p(ws), B, C, H, W, ctx.window)
        return gx, gy, None


@fp32_region
def ssim_distance(x, y, window_size=7, pad_mode="reflect"):
    """x, y [B, C, H, W] -> [B, C, H, W] clamp((1 - SSIM) / 2, 0, 1) over window_size x window_size boxes of the reflect-padded
    images; differentiable in both.  Odd windows 3 .. 11 and pad_mode 'reflect' only."""
    who = "ssim_distance"
    if pad_mode != "reflect":
        raise StxError(f"{who}: pad_mode {pad_mode!r} is not built (only 'reflect')")
    if not isinstance(window_size, int) or window_size not in SSIM_WINDOWS:
        raise StxError(f"{who}: window_size {window_size!r} is not one of the odd sizes {SSIM_WINDOWS}")
    x, y = _image_pair(who, x, y, ("x", "y"))
    _window_fits(who, x.shape[2], x.shape[3], window_size)
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return SsimDistanceFn.apply(x, y, window_size)
    return SsimDistanceFn.forward(_NoCtx(), x, y, window_size)


class PhotometricLossFn(torch.autograd.Function):
    """photometric_loss (loss_functions/photometric_loss.py:80-104) on stx_photometric_fwd / _bwd; gradient to disp only."""

    @staticmethod
    def forward(ctx, left, right, disp, ssim_weight, enable_mask):
        B, C, H, W = left.shape
        loss = torch.empty(B, 1, H, W, dtype=torch.float32, device=left.device)
        _call("stx_photometric_fwd", _p(left), _p(right), _p(disp), ssim_weight, int(enable_mask), _p(loss), B, C, H, W)
        ctx.save_for_backward(left, right, disp)
        ctx.cfg = (ssim_weight, int(enable_mask))
        return loss

    @staticmethod
    def backward(ctx, g):
        left, right, disp = ctx.saved_tensors
        B, C, H, W = left.shape
        gdisp = torch.empty_like(disp)
        ws = _WS.get("photometric_bwd", get_lib().raw("stx_photometric_bwd_workspace_floats")(B, C, H, W), left.device)
        _call("stx_photometric_bwd", _p(g.contiguous()), _p(left), _p(right), _p(disp), *ctx.cfg, _p(gdisp), _p(ws), B, C, H, W)
        return None, None, gdisp, None, None


@fp32_region
def photometric_loss(left_image, right_image, disp=None, ssim_weight=0.85, enable_mask=True):
    """[B, 1, H, W] = mean_C((ssim_weight * ssim(left, warped) + (1 - ssim_weight) * |left - warped|) * valid_mask) with warped,
    valid_mask = photo_warp(right_image, disp), in one launch; disp=None compares the images as they are (then there is no mask:
    enable_mask must be False).  Differentiable in disp."""
    who = "photometric_loss"
    if disp is None and enable_mask:
        raise StxError(f"{who}: enable_mask=True needs a disparity -- without a warp there is no valid_mask (pass enable_mask=False)")
    left, right = _image_pair(who, left_image, right_image)
    _images_are_data(who, left_image=left, right_image=right)
    _window_fits(who, left.shape[2], left.shape[3], PHOTO_WINDOW)
    if disp is not None:
        disp = _disp_map(who, disp, left)
    if disp is not None and torch.is_grad_enabled() and disp.requires_grad:
        return PhotometricLossFn.apply(left, right, disp, float(ssim_weight), bool(enable_mask))
    return PhotometricLossFn.forward(_NoCtx(), left, right, disp, float(ssim_weight), bool(enable_mask))


@fp32_region
def auto_mask(left_image, right_image, disp, denorm=False):
    """bool [B, 1, H, W]: photometric_loss(left, right, disp) < photometric_loss(left, right), both with enable_mask=False
    (loss_functions/auto_mask.py:7-17), one launch; denorm=True undoes the ImageNet normalisation of both images first (3
    channels).  No gradient."""
    who = "auto_mask"
    left, right = _image_pair(who, left_image.detach(), right_image.detach())
    if denorm and left.shape[1] != 3:
        raise StxError(f"{who}: denorm=True is defined for 3 channels, got {left.shape[1]}")
    _window_fits(who, left.shape[2], left.shape[3], PHOTO_WINDOW)
    disp = _disp_map(who, disp.detach(), left)
    B, C, H, W = left.shape
    mask = torch.empty(B, 1, H, W, dtype=torch.bool, device=left.device)
    _call("stx_auto_mask_fwd", _p(left), _p(right), _p(disp), int(bool(denorm)), _p(mask), B, C, H, W)
    return mask


class SmoothnessLossFn(torch.autograd.Function):
    """smoothness_loss (loss_functions/smoothness_loss.py:5-44) on stx_smoothness_fwd / _bwd -> (loss, max of img), 0-d both."""

    @staticmethod
    def forward(ctx, disp, img):
        B, C, H, W = img.shape
        out = torch.empty(2, dtype=torch.float32, device=img.device)
        stats = torch.empty(4 * B, dtype=torch.float32, device=img.device)
        ws = _WS.get("smoothness", get_lib().raw("stx_smoothness_workspace_floats")(B, H, W), img.device)
        _call("stx_smoothness_fwd", _p(disp), _p(img), _p(out), _p(stats), _p(ws), B, C, H, W)
        ctx.save_for_backward(disp, img, stats)
        loss, peak = out[0], out[1]
        ctx.mark_non_differentiable(peak)
        return loss, peak

    @staticmethod
    def backward(ctx, g, _gpeak):
        disp, img, stats = ctx.saved_tensors
        B, C, H, W = img.shape
        gdisp = torch.empty_like(disp)
        _call("stx_smoothness_bwd", _p(g.contiguous()), _p(disp), _p(img), _p(stats), _p(gdisp), B, C, H, W)
        return gdisp, None


@fp32_region
def smoothness_loss(disp, img, warn=True):
    """0-d tensor mean(|dx n| exp(-mean_C |dx img|)) + mean(|dy n| exp(-mean_C |dy img|)), n = disp / (per-image mean + 1e-7);
    differentiable in disp (the term through the mean included).  warn=True prints the reference's warning when img.max() > 1 --
    the max comes out of the same pass, but reading it is a device-to-host sync; warn=False never syncs."""
    who = "smoothness_loss"
    img = img.contiguous()
    _chk(img, "img", 4)
    _images_are_data(who, img=img)
    disp = _disp_map(who, disp, img)
    if torch.is_grad_enabled() and disp.requires_grad:
        loss, peak = SmoothnessLossFn.apply(disp, img)
    else:
        loss, peak = SmoothnessLossFn.forward(_NoCtx(), disp, img)
    if warn and float(peak) > 1.0:
        print("Warning: Image may not be normalized. Expected range: [0,1]")
    return loss


# --------------------------------------------------------------------------------------- STTR matching head
STTR_MAX_W = 431                                                         # csrc/sttr_head.hip ST_MAX_W
STTR_MAX_ITERS = 10                                                      # ... ST_MAX_ITERS
_STTR_CONSTANTS = {}


def _sttr_constants(W):
    """(log(1 / 2W), log(W / 2W), log(2W)) as the reference forms them: fp32 tensors on the host (regression_head.py:176-188),
    also in an fp64 run.  Passed to the kernels as arguments, so no device logf of a constant enters the comparison."""
    c = _STTR_CONSTANTS.get(W)
    if c is None:
        log_marginal = (torch.cat([torch.ones(W), torch.tensor([W]).float()]) / (2 * W)).log()
        c = (float(log_marginal[0]), float(log_marginal[W]), float(torch.log(torch.tensor([2.0 * W]))[0]))
        _STTR_CONSTANTS[W] = c
    return c


def _sttr_args(who, attn, phi, ot, iters):
    """Checks of the three STTR entry points -> phi as a dense [1] tensor (a differentiable view; read on the device)."""
    if not isinstance(attn, torch.Tensor) or attn.dim() != 4 or attn.shape[2] != attn.shape[3]:
        raise StxError(f"{who}: attn must be [N, H, W, W], got {tuple(attn.shape) if isinstance(attn, torch.Tensor) else attn!r}")
    if attn.dtype != torch.float32:
        raise StxError(f"{who}: attn must be float32, got {attn.dtype}")
    if not attn.is_contiguous():
        raise StxError(f"{who}: attn must be a dense contiguous tensor, strides {attn.stride()}")
    W = attn.shape[3]
    if not 2 <= W <= STTR_MAX_W:
        raise StxError(f"{who}: W={W} outside the supported 2..{STTR_MAX_W}")
    if ot and not (isinstance(iters, int) and 1 <= iters <= STTR_MAX_ITERS):
        raise StxError(f"{who}: iters={iters!r} outside the supported 1..{STTR_MAX_ITERS}")
    if not isinstance(phi, torch.Tensor) or phi.numel() != 1 or phi.dtype != torch.float32:
        raise StxError(f"{who}: phi must be one float32 value on attn's device")
    phi = phi.reshape(1)
    _chk(attn, "attn", 4)
    _chk(phi, "phi")
    return phi


def _sttr_grad(attn, phi):
    return torch.is_grad_enabled() and (attn.requires_grad or phi.requires_grad)


class SttrTransportFn(torch.autograd.Function):
    """The dense transported (mode 1) or softmax (mode 0) matrix P [N, H, W+1, W+1] on stx_sttr_transport_fwd / _bwd."""

    @staticmethod
    def forward(ctx, attn, phi, mode, iters):
        N, H, W, _ = attn.shape
        M = W + 1
        P = torch.empty(N, H, M, M, dtype=torch.float32, device=attn.device)
        us = vs = None
        if not isinstance(ctx, _NoCtx):
            shape = (N, H, iters, M) if mode else (N, H, M)
            us, vs = (torch.empty(shape, dtype=torch.float64, device=attn.device) for _ in range(2))
        _call("stx_sttr_transport_fwd", _p(attn), _p(phi), mode, iters, *_sttr_constants(W), _p(P), _p(us), _p(vs), N, H, W)
        ctx.save_for_backward(attn, phi, us, vs)
        ctx.cfg = (mode, iters)
        return P

    @staticmethod
    def backward(ctx, G):
        attn, phi, us, vs = ctx.saved_tensors
        mode, iters = ctx.cfg
        N, H, W, _ = attn.shape
        g_attn = torch.empty_like(attn)
        part = torch.empty(N * H, dtype=torch.float64, device=attn.device)
        g_phi = torch.empty(1, dtype=torch.float32, device=attn.device)
        _call("stx_sttr_transport_bwd", _p(G.contiguous()), _p(attn), _p(phi), mode, iters, *_sttr_constants(W), _p(us), _p(vs),
              _p(g_attn), _p(part), _p(g_phi), N, H, W)
        return g_attn, g_phi, None, None


def _sttr_dense(who, attn, phi, mode, iters):
    phi = _sttr_args(who, attn, phi, mode, iters)
    if _sttr_grad(attn, phi):
        return SttrTransportFn.apply(attn, phi, mode, iters)
    return SttrTransportFn.forward(_NoCtx(), attn, phi, mode, iters)


@fp32_region
def sttr_optimal_transport(attn, phi, iters):
    """attn [N, H, W, W] (-inf allowed above the diagonal), phi a device scalar -> the transported matrix [N, H, W+1, W+1] after
    `iters` log-space Sinkhorn iterations with a dustbin row and column (reference `_optimal_transport`); gradients to attn and
    phi.  2 <= W <= 431, 1 <= iters <= 10."""
    return _sttr_dense("sttr_optimal_transport", attn, phi, 1, iters)


@fp32_region
def sttr_softmax(attn, phi):
    """The row softmax of attn with the dustbin row and column, [N, H, W+1, W+1] (reference `_softmax`)."""
    return _sttr_dense("sttr_softmax", attn, phi, 0, 1)


class SttrHeadFn(torch.autograd.Function):
    """The fused head on stx_sttr_head_fwd / _bwd -> (disp, occ, arg, bin_left, bin_right[, gt_response]), [N, H, W] each; the
    transported matrix is never written.  Kept for the backward: the 2 * iters scaling vectors (softmax: row max and sum)."""

    @staticmethod
    def forward(ctx, attn, phi, mode, iters, mask, target):
        N, H, W, _ = attn.shape
        M = W + 1

        def new(*shape, dtype=torch.float32):
            return torch.empty(*shape, dtype=dtype, device=attn.device)
        disp, occ, norm, bin_l, bin_r = (new(N, H, W) for _ in range(5))
        arg = new(N, H, W, dtype=torch.int32)
        gt = new(N, H, W) if target is not None else None
        us = vs = None
        if not isinstance(ctx, _NoCtx):
            shape = (N, H, iters, M) if mode else (N, H, M)
            us, vs = new(*shape, dtype=torch.float64), new(*shape, dtype=torch.float64)
            ctx.set_materialize_grads(False)                             # an output the loss does not use: NULL, not zeros
        _call("stx_sttr_head_fwd", _p(attn), _p(phi), mode, iters, *_sttr_constants(W), _p(mask), _p(target), _p(disp), _p(occ),
              _p(norm), _p(arg), _p(gt), _p(bin_l), _p(bin_r), _p(us), _p(vs), N, H, W)
        ctx.save_for_backward(attn, phi, target, disp, norm, arg, us, vs)
        ctx.cfg = (mode, iters)
        ctx.mark_non_differentiable(arg)
        return (disp, occ, arg, bin_l, bin_r) + (() if gt is None else (gt,))

    @staticmethod
    def backward(ctx, g_disp, g_occ, _g_arg, g_bin_l, g_bin_r, g_gt=None):
        attn, phi, target, disp, norm, arg, us, vs = ctx.saved_tensors
        mode, iters = ctx.cfg
        N, H, W, _ = attn.shape
        grads = [None if g is None else g.contiguous() for g in (g_disp, g_occ, g_gt, g_bin_l, g_bin_r)]
        if all(g is None for g in grads):
            raise StxError("sttr_regress: backward without a gradient for any output")
        g_attn = torch.empty_like(attn)
        part = torch.empty(N * H, dtype=torch.float64, device=attn.device)
        g_phi = torch.empty(1, dtype=torch.float32, device=attn.device)
        _call("stx_sttr_head_bwd", *(_p(g) for g in grads), _p(attn), _p(phi), mode, iters, *_sttr_constants(W), _p(target),
              _p(disp), _p(norm), _p(arg), _p(us), _p(vs), _p(g_attn), _p(part), _p(g_phi), N, H, W)
        return g_attn, g_phi, None, None, None, None


@fp32_region
def sttr_regress(attn, phi, ot=True, iters=10, occ_mask=None, target=None):
    """STTR's regression head fused (reference RegressionHead.forward up to the upsampling): attn [N, H, W, W], phi a device
    scalar -> (disp, occ, gt_response, bin_left, bin_right), [N, H, W] each, and the arg-max index as a sixth tensor.
    ot: optimal transport with `iters` Sinkhorn iterations, else the softmax alternative.  occ_mask (bool [N, H, W]): norm is
    forced to 1 where it is set; None: where norm < 0.1.  target ([N, H, W], the ground-truth location in low-resolution
    columns; no gradient): gt_response is the matrix sampled there, None without it.  bin_left / bin_right are the dustbin
    column and row.  Gradients to attn and phi from any subset of the outputs."""
    who = "sttr_regress"
    mode = 1 if ot else 0
    phi = _sttr_args(who, attn, phi, mode, iters)
    N, H, W, _ = attn.shape
    if occ_mask is not None:
        if tuple(occ_mask.shape) != (N, H, W) or occ_mask.dtype != torch.bool or occ_mask.device != attn.device:
            raise StxError(f"{who}: occ_mask must be a bool tensor [{N}, {H}, {W}] on attn's device, got {tuple(occ_mask.shape)} "
                           f"{occ_mask.dtype}")
        occ_mask = occ_mask.contiguous()
    if target is not None:
        if tuple(target.shape) != (N, H, W):
            raise StxError(f"{who}: target must be [{N}, {H}, {W}], got {tuple(target.shape)}")
        target = target.detach().contiguous()
        _chk(target, "target")
    if _sttr_grad(attn, phi):
        got = SttrHeadFn.apply(attn, phi, mode, iters if mode else 1, occ_mask, target)
    else:
        got = SttrHeadFn.forward(_NoCtx(), attn, phi, mode, iters if mode else 1, occ_mask, target)
    disp, occ, arg, bin_l, bin_r = got[:5]
    return disp, occ, (got[5] if target is not None else None), bin_l, bin_r, arg


# --------------------------------------------------------------------------------------- STTR attention with relative positions
STTR_ATTN_HEAD_DIM = 16                                                  # csrc/sttr_attention.hip SA_HD
STTR_ATTN_MAX_HEADS = 8                                                  # ... SA_MAX_E


def _sttr_attn_chunks(W, B, E):
    """Into how many chunks the table-gradient kernel splits the rows b: about 2048 waves, one per (chunk, head, 16 queries) --
    two per SIMD of an MI355X; measured at 192 x 320: 1024 waves 7.0 ms per backward, 2048 6.0 ms, 4096 and more no faster."""
    per = E * ((W + 15) // 16)
    return max(1, min(B, (2048 + per - 1) // per))


def sttr_attn_scratch_floats(W, B, E, tables=True):
    """Floats of scratch one backward call takes: the row sums dO . o and the partial windows of dQr / dKr."""
    W16 = (W + 15) // 16
    return B * E * W + (_sttr_attn_chunks(W, B, E) * E * W16 * 2 * (W16 + 1) * 256 if tables else 0)


def _sttr_attn_dense(who, name, t):
    if t.dtype != torch.float32:
        raise StxError(f"{who}: {name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise StxError(f"{who}: {name} must be a dense contiguous tensor, strides {t.stride()}")


class SttrRelAttentionFn(torch.autograd.Function):
    """stx_sttr_attn_fwd / _bwd.  Kept for the backward: the inputs, o and the row max / row sum [2, B, E, W]."""

    @staticmethod
    def forward(ctx, q, k, v, q_r, k_r, causal, need_raw, need_avg):
        W, B, E, D = q.shape
        o = torch.empty_like(q)
        raw = torch.empty(B, W, W, dtype=torch.float32, device=q.device) if need_raw else None
        avg = torch.empty(B, W, W, dtype=torch.float32, device=q.device) if need_avg else None
        stats = None
        if not isinstance(ctx, _NoCtx):
            stats = torch.empty(2, B, E, W, dtype=torch.float32, device=q.device)
            ctx.set_materialize_grads(False)
        _call("stx_sttr_attn_fwd", _p(q), _p(k), _p(v), _p(q_r), _p(k_r), int(causal), _p(o), _p(raw), _p(avg), _p(stats), W, B, E, D)
        ctx.save_for_backward(q, k, v, q_r, k_r, o, stats)
        ctx.causal = causal
        if avg is not None:
            ctx.mark_non_differentiable(avg)
        return o, raw, avg

    @staticmethod
    def backward(ctx, g_o, g_raw, _g_avg):
        q, k, v, q_r, k_r, o, stats = ctx.saved_tensors
        W, B, E, D = q.shape
        if g_o is None and g_raw is None:
            raise StxError("sttr_rel_attention: backward without a gradient for o or raw")
        g_o = None if g_o is None else g_o.contiguous()
        g_raw = None if g_raw is None else g_raw.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dqr = dkr = None
        if q_r is not None:
            dqr, dkr = torch.empty_like(q_r), torch.empty_like(k_r)
        n = sttr_attn_scratch_floats(W, B, E, q_r is not None)
        scratch = torch.empty(n, dtype=torch.float32, device=q.device)
        _call("stx_sttr_attn_bwd", _p(g_o), _p(g_raw), _p(q), _p(k), _p(v), _p(q_r), _p(k_r), _p(o), _p(stats), int(ctx.causal),
              _p(dq), _p(dk), _p(dv), _p(dqr), _p(dkr), _p(scratch), n, _sttr_attn_chunks(W, B, E), W, B, E, D)
        return dq, dk, dv, dqr, dkr, None, None, None


@fp32_region
def sttr_rel_attention(q, k, v, q_r=None, k_r=None, causal=False, need_raw=False, need_avg=False):
    """The core of STTR's `MultiheadAttentionRelative` (reference models/STTR/attention.py:98-137) between the projections.
    q (already scaled), k, v: [W, B, E, 16] dense fp32 -- a view of what a linear layer on [W, B, C] leaves; q_r (scaled) and
    k_r: the PROJECTED relative table [2W-1, E, 16], both or neither.  The scores are
        S[b, e, w, v] = q[w].k[v] + q[w].k_r[W-1-w+v] + k[v].q_r[W-1-w+v]
    which is the reference's three einsums for its pos_indexes[w, v] = (W-1-w) + v; `causal` adds its upper-triangular -inf mask.
    -> (o [W, B, E, 16] = softmax_v(S) v, raw [B, W, W] = sum_e S or None, avg [B, W, W] = mean_e softmax(S) or None).
    Gradients reach q, k, v, q_r and k_r through o and raw; avg is a debugging output and is NOT differentiable.
    2 <= W <= 431, at most 8 heads, head dim 16 only."""
    who = "sttr_rel_attention"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise StxError(f"{who}: {name} must be [W, B, E, 16], got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
        _sttr_attn_dense(who, name, t)
        _chk(t, f"{who}: {name}", 4)
    W, B, E, D = q.shape
    if D != STTR_ATTN_HEAD_DIM:
        raise StxError(f"{who}: head dim {D} is not supported, only {STTR_ATTN_HEAD_DIM}")
    if tuple(k.shape) != tuple(q.shape) or tuple(v.shape) != tuple(q.shape):
        raise StxError(f"{who}: q, k and v must have one shape, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    if not 2 <= W <= STTR_MAX_W:
        raise StxError(f"{who}: W={W} outside the supported 2..{STTR_MAX_W}")
    if not 1 <= E <= STTR_ATTN_MAX_HEADS:
        raise StxError(f"{who}: {E} heads outside the supported 1..{STTR_ATTN_MAX_HEADS}")
    if B < 1 or B > 65535:
        raise StxError(f"{who}: B={B} rows outside the supported 1..65535")
    if (q_r is None) != (k_r is None):
        raise StxError(f"{who}: q_r and k_r go together (the projected relative table, or neither)")
    for name, t in (("q_r", q_r), ("k_r", k_r)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (2 * W - 1, E, D):
            raise StxError(f"{who}: {name} must be [2W-1, E, 16] = [{2 * W - 1}, {E}, {D}], got {tuple(t.shape)}")
        _sttr_attn_dense(who, name, t)
        _chk(t, f"{who}: {name}", 3)
    args = (q, k, v, q_r, k_r, bool(causal), bool(need_raw), bool(need_avg))
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in args[:5]):
        return SttrRelAttentionFn.apply(*args)
    return SttrRelAttentionFn.forward(_NoCtx(), *args)


# --------------------------------------------------------------------------------------- FoundationStereo disparity transformer
DISP_ATTN_MAX_L = 32                                                     # csrc/disp_attention.hip DA_MAX_L
DISP_ATTN_MAX_C = 32                                                     # ... DA_MAX_C (channels and feed-forward width)
DISP_ATTN_MAX_HEAD_DIM = 8                                               # ... DA_MAX_HD
DISP_ATTN_MAX_LAYERS = 8                                                 # ... DA_MAX_LAYERS
DISP_ATTN_TENSORS = 16                                                   # tensors of one layer, state-dict order
DISP_ATTN_SITES = 3                                                      # dropout sites of one layer


def disp_attention_served(C, nhead, F, layers=1, L=1):
    """The rule of stx_disp_attention_supported, for checks at construction (no library needed)."""
    ok = lambda n, top: isinstance(n, int) and 4 <= n <= top and n % 4 == 0                     # noqa: E731
    return (ok(C, DISP_ATTN_MAX_C) and ok(F, DISP_ATTN_MAX_C) and isinstance(nhead, int) and nhead >= 1 and C % nhead == 0
            and C // nhead <= DISP_ATTN_MAX_HEAD_DIM and 1 <= layers <= DISP_ATTN_MAX_LAYERS and 1 <= L <= DISP_ATTN_MAX_L)


def _da_view(x):
    """(N, L, C, hw, sb, sp, st) of a dense [B, D, H, W, C] volume or a dense [N, L, C] tensor: include/stx_hip.h."""
    if x.dim() == 5:
        B, D, H, W, C = x.shape
        return B * H * W, D, C, H * W, D * H * W * C, C, H * W * C
    N, L, C = x.shape
    return N, L, C, 1, L * C, 0, C


def _da_layer_shapes(C, F):
    return [(C, C), (C,)] * 4 + [(F, C), (F,), (C, F), (C,)] + [(C,)] * 4


def _da_seed(who, seed, like):
    if seed is None:
        return None
    if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != like.device:
        raise StxError(f"{who}: seed must be a one-element int64 tensor on {like.device}, got {seed!r}")
    return seed.contiguous()


class DispAttentionFn(torch.autograd.Function):
    """stx_disp_attention_fwd / _bwd: all layers as one node.  Saved: the input of every layer [layers, N, L, C], the parameters
    and the seed by reference.  The dropout masks are drawn again in the backward from the same seed tensor."""

    @staticmethod
    def forward(ctx, x, pe, seed, cfg, *params):
        nhead, F, layers, p, eps = cfg
        N, L, C, hw, sb, sp, st = _da_view(x)
        need = not isinstance(ctx, _NoCtx) and any(ctx.needs_input_grad)
        y = torch.empty_like(x)
        saved = torch.empty(layers, N, L, C, dtype=torch.float32, device=x.device) if need else None
        prm = [t.detach() for t in params]
        _call("stx_disp_attention_fwd", _p(x), _p(pe), _pointer_table(prm), _p(y), _p(saved), _p(seed), p, eps, N, L, C, nhead, F,
              layers, hw, sb, sp, st)
        if need:
            ctx.save_for_backward(saved, seed, *params)
            ctx.cfg = cfg
            ctx.form = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        saved, seed, *params = ctx.saved_tensors
        nhead, F, layers, p, eps = ctx.cfg
        gy = gy.contiguous()
        N, L, C, hw, sb, sp, st = _da_view(gy)
        dev = gy.device
        need = ctx.needs_input_grad
        gx = torch.empty(ctx.form, dtype=torch.float32, device=dev) if need[0] else None
        grads = [torch.empty_like(t) if n else None for t, n in zip(params, need[4:])]
        if gx is None and not any(g is not None for g in grads):
            return (None,) * len(need)
        gbuf = torch.empty(N, L, C, dtype=torch.float32, device=dev) if layers > 1 else None
        n = get_lib().raw("stx_disp_attention_bwd_workspace_floats")(N, L, C, F)
        ws = _WS.get("disp_attention", n, dev)
        prm = [t.detach() for t in params]
        _call("stx_disp_attention_bwd", _p(gy), _p(saved), _pointer_table(prm), _pointer_table(grads), _p(gx), _p(gbuf), _p(ws), n,
              _p(seed), p, eps, N, L, C, nhead, F, layers, hw, sb, sp, st)
        return (gx, None, None, None, *grads)


def _disp_attention_args(who, x, pe, params, nhead, p, seed, training):
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 5):
        raise StxError(f"{who}: x must be a dense [B, D, H, W, C] volume or [N, L, C], got "
                       f"{tuple(x.shape) if isinstance(x, torch.Tensor) else x!r}")
    if not on_device(x):
        raise StxError(f"{who}: expected a ROCm device tensor, got {x.device} -- there is no CPU fallback")
    if x.dtype != torch.float32:
        raise StxError(f"{who}: expected float32, got {x.dtype}")
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()                                         # (a slice that starts off a 16-byte boundary: the kernel loads float4)
    params = list(params)
    N, L, C, hw, sb, sp, st = _da_view(x)
    if len(params) % DISP_ATTN_TENSORS or not params:
        raise StxError(f"{who}: {len(params)} parameter tensors; {DISP_ATTN_TENSORS} per layer are expected")
    layers = len(params) // DISP_ATTN_TENSORS
    w1 = params[8]
    F = int(w1.shape[0]) if isinstance(w1, torch.Tensor) and w1.dim() == 2 else -1
    nhead = int(nhead)
    if F < 0 or nhead < 1 or not get_lib().raw("stx_disp_attention_supported")(L, C, nhead, F, layers):
        raise StxError(f"{who}: L={L}, C={C}, {nhead} heads, feed-forward {F}, {layers} layers is not served (L 1..{DISP_ATTN_MAX_L}; C "
                       f"and feed-forward multiples of 4 up to {DISP_ATTN_MAX_C}; head dim <= {DISP_ATTN_MAX_HEAD_DIM}; "
                       f"1..{DISP_ATTN_MAX_LAYERS} layers)")
    if N < 1 or N * L * C >= 2 ** 31:
        raise StxError(f"{who}: {N} sequences of {L} x {C}: N L C must lie in 1 .. 2^31 - 1")
    shapes = _da_layer_shapes(C, F) * layers
    dense = []
    for i, (t, shape) in enumerate(zip(params, shapes)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise StxError(f"{who}: parameter {i % DISP_ATTN_TENSORS} of layer {i // DISP_ATTN_TENSORS} must be {shape}, got "
                           f"{tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
        if t.dtype != torch.float32 or t.device != x.device:
            raise StxError(f"{who}: parameter {i} must be float32 on {x.device}, got {t.dtype} on {t.device}")
        dense.append(t if t.is_contiguous() else t.contiguous())
    if pe is not None:
        if not isinstance(pe, torch.Tensor) or tuple(pe.shape) != (L, C) or pe.dtype != torch.float32 or pe.device != x.device:
            raise StxError(f"{who}: pe must be a float32 [{L}, {C}] table on {x.device}")
        pe = pe.detach().contiguous()
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise StxError(f"{who}: dropout probability {p} outside [0, 1)")
    seed = _da_seed(who, seed, x)
    if not training or p == 0.0:
        p, seed = 0.0, None
    elif seed is None:
        raise StxError(f"{who}: training with p = {p} needs a seed tensor")
    return x, pe, dense, nhead, F, layers, p, seed


@fp32_region
def disp_attention(x, pe, params, nhead, p=0.0, seed=None, training=False, eps=1e-5):
    """FoundationStereo's disparity transformer (reference FoundationStereo/submodule.py `CostVolumeDisparityAttention`) on
    csrc/disp_attention.hip, one autograd node: x + pe, then len(params) / 16 post-norm encoder layers
        a = softmax(Q K^T / sqrt(hd)) V per head;  x1 = LayerNorm(x + drop(out_proj(a)));
        y = LayerNorm(x1 + drop(linear2(drop(gelu(linear1(x1))))))
    over the sequences of x: a dense channels-last volume [B, D, H, W, C] (one sequence of D tokens per pixel, read in place) or
    [N, L, C].  pe: None or a [L, C] table.  params: 16 tensors per layer in state-dict order (q/k/v/out_proj weight and bias,
    linear1, linear2, norm1, norm2).  training with p > 0 draws the three dropout masks of every layer inside the kernel from
    `seed`, a one-element int64 tensor on x's device (never read on the host; counter layout in include/stx_hip.h); the backward
    draws them again.  eval, or p = 0: nothing is drawn and seed may be None.  Returns a tensor of x's shape, fp32.
    Served: L <= 32, C and the feed-forward width multiples of 4 up to 32, head dim <= 8, at most 8 layers; anything else raises
    StxError and launches nothing."""
    who = "disp_attention"
    x, pe, dense, nhead, F, layers, p, seed = _disp_attention_args(who, x, pe, params, nhead, p, seed, training)
    cfg = (nhead, F, layers, p, float(eps))
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in dense)):
        return DispAttentionFn.apply(x, pe, seed, cfg, *dense)
    return DispAttentionFn.forward(_NoCtx(), x, pe, seed, cfg, *dense)


def disp_attention_masks(seed, p, N, L, C, F, layers):
    """The keep decisions (1 / 0) `disp_attention` makes with this seed and p, as uint8 [layers, 3, N, L, max(C, F)]: site 0 behind
    out_proj (C channels), 1 behind the GELU (F channels), 2 behind linear2 (C channels)."""
    who = "disp_attention_masks"
    if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or seed.numel() != 1:
        raise StxError(f"{who}: seed must be a one-element int64 tensor, got {seed!r}")
    if not on_device(seed):
        raise StxError(f"{who}: expected a ROCm device tensor, got {seed.device} -- there is no CPU fallback")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise StxError(f"{who}: dropout probability {p} outside [0, 1)")
    out = torch.empty(layers, DISP_ATTN_SITES, N, L, max(C, F), dtype=torch.uint8, device=seed.device)
    _call("stx_disp_attention_masks", _p(seed.contiguous()), p, _p(out), N, L, C, F, layers)
    return out


# --------------------------------------------------------------------------------------- MonSter mutual refinement
MONSTER_PADDING = ("border", "zeros")                                    # warp.py:58
MONSTER_MAX_N = 1 << 24                                                  # csrc/monster.hip: counts of the radix select
MONSTER_BWD_MAX_W = 2048                                                 # csrc/monster.hip MS_MAX_W (gradient to the sampled map)


def _low_dtype(t):
    return t.dtype if isinstance(t, torch.Tensor) and t.dtype in _LOW else None


def _as_dtype(out, dtype):
    if dtype is None:
        return out
    return tuple(t.to(dtype) for t in out) if isinstance(out, tuple) else out.to(dtype)


def _monster_pair(who, img, disps, padding_mode, left=None):
    """The shape rules of the warp, checked on the shapes alone before anything is copied or launched."""
    if padding_mode not in MONSTER_PADDING:
        raise StxError(f"{who}: padding_mode {padding_mode!r} is not one of {MONSTER_PADDING}")
    if not isinstance(img, torch.Tensor) or img.dim() != 4:
        raise StxError(f"{who}: the sampled map must be [B, C, H, W], got {tuple(getattr(img, 'shape', ()))}")
    B, C, H, W = img.shape
    if left is not None and (not isinstance(left, torch.Tensor) or left.shape != img.shape):
        raise StxError(f"{who}: left {tuple(getattr(left, 'shape', ()))} does not match right {tuple(img.shape)}")
    for name, d in disps:
        if not isinstance(d, torch.Tensor) or tuple(d.shape) != (B, 1, H, W):
            raise StxError(f"{who}: {name} must be [B, 1, H, W] = {(B, 1, H, W)}, got {tuple(getattr(d, 'shape', ()))}")
    if H < 2 or W < 2:
        raise StxError(f"{who}: the reference's sampling grid divides by H - 1 and W - 1: H, W >= 2 needed, got {H} x {W}")
    out = []
    for name, t in (("left", left), ("right", img), *disps):
        if t is not None:
            t = t.contiguous()
            _chk(t, name, 4)
        out.append(t)
    return out


class MonsterFlawFn(torch.autograd.Function):
    """disp_warp(right, d)[0] - left (monster.py:469-473, refinement.py:403-407) for one or two disparities on
    stx_monster_flaw_fwd / _bwd: one forward launch; the backward is a per-pixel kernel and a gather, without float atomics.
    Saves the inputs only (right and the disparities; left is not needed).  left None: the warped map itself."""

    @staticmethod
    def forward(ctx, left, right, da, db, zeros, want_valid):
        B, C, H, W = right.shape
        oa = torch.empty_like(right)
        ob = torch.empty_like(right) if db is not None else None
        valid = torch.empty(B, 1, H, W, dtype=torch.float32, device=right.device) if want_valid else None
        _call("stx_monster_flaw_fwd", _p(left), _p(right), _p(da), _p(db), zeros, _p(oa), _p(ob), _p(valid), B, C, H, W)
        if not isinstance(ctx, _NoCtx):
            ctx.set_materialize_grads(False)
        ctx.save_for_backward(right, da, db)
        ctx.zeros = zeros
        if valid is not None:
            ctx.mark_non_differentiable(valid)
        return oa, ob, valid

    @staticmethod
    def backward(ctx, ga, gb, _gvalid):
        right, da, db = ctx.saved_tensors
        if ga is None and gb is None:
            return None, None, None, None, None, None
        B, C, H, W = right.shape
        ga, gb = (None if g is None else g.contiguous() for g in (ga, gb))
        need = ctx.needs_input_grad
        if need[1] and W > MONSTER_BWD_MAX_W:
            raise StxError(f"monster_flaws: W={W} above the {MONSTER_BWD_MAX_W} the gradient to the sampled map supports")
        g_left = torch.empty_like(right) if need[0] else None
        g_right = torch.empty_like(right) if need[1] else None
        g_da = torch.empty_like(da) if need[2] else None
        g_db = torch.empty_like(db) if db is not None and need[3] else None
        if g_left is None and g_right is None and g_da is None and g_db is None:
            return None, None, None, None, None, None
        _call("stx_monster_flaw_bwd", _p(ga), _p(gb), _p(right), _p(da), _p(db), ctx.zeros, _p(g_left), _p(g_right), _p(g_da),
              _p(g_db), B, C, H, W)
        return g_left, g_right, g_da, g_db, None, None


def _monster_flaw_call(left, right, da, db, padding_mode, want_valid):
    zeros = int(padding_mode == "zeros")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (left, right, da, db)):
        return MonsterFlawFn.apply(left, right, da, db, zeros, want_valid)
    return MonsterFlawFn.forward(_NoCtx(), left, right, da, db, zeros, want_valid)


@fp32_region
def _monster_flaws(left, right, disp_a, disp_b, padding_mode):
    who = "monster_flaws"
    disps = (("disp_a", disp_a),) + ((("disp_b", disp_b),) if disp_b is not None else ())
    if not isinstance(left, torch.Tensor):
        raise StxError(f"{who}: left must be a [B, C, H, W] tensor, got {type(left).__name__}")
    left, right, da, *rest = _monster_pair(who, right, disps, padding_mode, left=left)
    fa, fb, _ = _monster_flaw_call(left, right, da, rest[0] if rest else None, padding_mode, False)
    return fa if disp_b is None else (fa, fb)


def monster_flaws(left, right, disp_a, disp_b=None, padding_mode="border"):
    """left, right [B, C, H, W], disp_a (and disp_b) [B, 1, H, W] -> flaw_a (, flaw_b) = disp_warp(right, d)[0] - left of the
    reference's MonSter (monster.py:469-473): right sampled at ix = (x - d) W / (W - 1) - 1/2, iy = y H / (H - 1) - 1/2, bilinear
    in both directions, padding 'border' (the model's) or 'zeros'.  Both flaws come from one launch and one autograd node,
    differentiable in left, right and the disparities; the backward is bitwise reproducible (no float atomics).  fp16 / bf16
    maps are cast up and the flaws returned in the dtype of `right`, as the reference's `interp` does."""
    low = _low_dtype(right)
    return _as_dtype(_monster_flaws(*_to_fp32((left, right, disp_a, disp_b)), padding_mode), low)


@fp32_region
def _monster_disp_warp(img, disp, padding_mode):
    _, img, disp = _monster_pair("monster_disp_warp", img, (("disp", disp),), padding_mode)
    warped, _, valid = _monster_flaw_call(None, img, disp, None, padding_mode, True)
    return warped, valid


def monster_disp_warp(img, disp, padding_mode="border"):
    """img [B, C, H, W], disp [B, 1, H, W] -> (warped, valid_mask), both [B, C, H, W] (the mask a broadcast view, no gradient):
    the reference's disp_warp (MonSter/warp.py:53-79).  valid_mask is formed from the weights of the corners inside the image:
    1 everywhere under 'border'; under 'zeros' 0 where their sum is below 0.9999, else 1."""
    low = _low_dtype(img)
    warped, valid = _as_dtype(_monster_disp_warp(*_to_fp32((img, disp)), padding_mode), low)
    return warped, valid.expand_as(warped)


def _monster_fit_args(who, mono, gt, mask):
    for name, t in (("mono", mono), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise StxError(f"{who}: {name} must be a [B, ...] tensor, got {tuple(getattr(t, 'shape', ()))}")
    if gt.shape != mono.shape:
        raise StxError(f"{who}: gt {tuple(gt.shape)} does not match mono {tuple(mono.shape)}")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.shape != mono.shape):
        raise StxError(f"{who}: mask must be a bool tensor of mono's shape {tuple(mono.shape)}")
    B = mono.shape[0]
    n = mono.numel() // max(1, B)
    if B < 1 or not 0 < n < MONSTER_MAX_N:
        raise StxError(f"{who}: {n} elements per image outside 1..2^24 - 1")
    mono, gt = mono.detach().contiguous(), gt.detach().contiguous()
    _chk(mono, "mono")
    _chk(gt, "gt")
    if mask is not None:
        if not on_device(mask):
            raise StxError(f"{who}: mask: expected a ROCm device tensor, got {mask.device}")
        mask = mask.contiguous().view(torch.uint8)
    return mono, gt, mask, B, n


@fp32_region
def _monster_fit(mono, gt, mask, who="monster_scale_shift"):
    mono, gt, mask, B, n = _monster_fit_args(who, mono, gt, mask)
    ss = torch.empty(B, 2, dtype=torch.float32, device=mono.device)
    stats = torch.empty(B, 8, dtype=torch.float64, device=mono.device)
    k = int(0.2 * n)                                                     # monster.py:47, the same Python expression
    _call("stx_monster_scale_shift", _p(mono), _p(gt), _p(mask), k, _p(ss), _p(stats), B, n)
    return ss, stats


def monster_scale_shift(mono, gt, mask=None):
    """mono, gt [B, 1, H, W] -> [B, 2] fp32 on the device, per image (scale, shift) of compute_scale_shift (monster.py:31-66): the
    least-squares fit gt ~ scale mono + shift, ridge 1e-6, over mask, by default (gt > 0) & (mono > 1e-2) & (mono > the value of
    rank int(0.2 n) of mono).  An empty mask gives (0, 0).  Constants of the graph; no host synchronisation."""
    return _monster_fit(*_to_fp32((mono, gt)), mask)[0]


def monster_fit_stats(mono, gt, mask=None):
    """What `monster_scale_shift` summed, [B, 8] fp64: S_mm, S_m, N, S_mg, S_g, the rank threshold, the rank, 0."""
    return _monster_fit(*_to_fp32((mono, gt)), mask)[1]


class MonsterApplyFn(torch.autograd.Function):
    """scale_b * mono[b] + shift_b on stx_monster_apply_scale_shift; the gradient goes to mono only (scale and shift are
    constants, as the reference's `.item()` makes them)."""

    @staticmethod
    def forward(ctx, mono, ss):
        B = mono.shape[0]
        out = torch.empty_like(mono)
        _call("stx_monster_apply_scale_shift", _p(mono), _p(ss), 1, _p(out), B, mono.numel() // B)
        ctx.save_for_backward(ss)
        return out

    @staticmethod
    def backward(ctx, g):
        ss, = ctx.saved_tensors
        g = g.contiguous()
        gm = torch.empty_like(g)
        _call("stx_monster_apply_scale_shift", _p(g), _p(ss), 0, _p(gm), g.shape[0], g.numel() // g.shape[0])
        return gm, None


@fp32_region
def _monster_align(mono, gt, mask):
    ss, _ = _monster_fit(mono, gt, mask, who="monster_align")
    mono = mono.contiguous()
    _chk(mono, "mono")
    if torch.is_grad_enabled() and mono.requires_grad:
        return MonsterApplyFn.apply(mono, ss)
    return MonsterApplyFn.forward(_NoCtx(), mono, ss)


def monster_align(mono, gt, mask=None):
    """mono, gt [B, 1, H, W] -> scale_b * mono[b] + shift_b with `monster_scale_shift`'s fit per image (monster.py:463-467, batched:
    no Python loop, no host synchronisation).  Differentiable in mono with the fit held constant; returned in mono's dtype."""
    low = _low_dtype(mono)
    return _as_dtype(_monster_align(*_to_fp32((mono, gt)), mask), low)


# --------------------------------------------------------------------------------------- instance norm + activation (+ residual tail)
INSTNORM_ACTS = {"none": 0, "relu": 1, "lrelu": 3}                       # the codes of stx_act (csrc/stx_common.h)
INSTNORM_MAX_PLANE = 1 << 31                                             # csrc/instnorm.hip: elements per plane, exclusive


def instance_norm_plan(planes, S):
    """(chunks per plane, path) the launchers of csrc/instnorm.hip take for `planes` planes of S elements: path 0 = one workgroup
    per plane and one launch, 1 = per-chunk partial sums and an apply launch."""
    chunks, path = ctypes.c_int(0), ctypes.c_int(0)
    get_lib().call("stx_instnorm_plan", planes, S, 0, ctypes.byref(chunks), ctypes.byref(path))
    return chunks.value, path.value


def _instnorm_ws(planes, S, device):
    nbytes = get_lib().raw("stx_instnorm_ws_bytes")(planes, S, 0)
    if nbytes < 0:
        raise StxError(f"instance_norm: {planes} planes of {S} elements are not served")
    return _WS.get("instnorm", (nbytes + 7) // 8 * 2, device) if nbytes else None     # (an 8-byte aligned start: torch's allocations are)


class InstanceNormFn(torch.autograd.Function):
    """act(instance_norm(x)) or relu(skip + act(instance_norm(x))) on stx_instnorm_fwd / _bwd.  Saves x, skip and the per-plane
    (mean, rstd) -- [B C][2] doubles; the output is not saved, the backward re-forms xhat and the masks."""

    @staticmethod
    def forward(ctx, x, skip, act, eps):
        planes = x.shape[0] * x.shape[1]
        S = x.numel() // planes
        y = torch.empty_like(x)
        grad = not isinstance(ctx, _NoCtx)
        stats = torch.empty(planes, 2, dtype=torch.float64, device=x.device) if grad else None
        _call("stx_instnorm_fwd", _p(x), _p(skip), _p(y), _p(stats), _p(_instnorm_ws(planes, S, x.device)), planes, S, 0, act, eps)
        if grad:
            ctx.save_for_backward(x, skip, stats)
            ctx.act = act
        return y

    @staticmethod
    def backward(ctx, gy):
        x, skip, stats = ctx.saved_tensors
        planes = x.shape[0] * x.shape[1]
        S = x.numel() // planes
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gskip = torch.empty_like(skip) if skip is not None and ctx.needs_input_grad[1] else None
        if gx is None and gskip is None:
            return None, None, None, None
        ws = _instnorm_ws(planes, S, x.device) if gx is not None else None
        gy = _aligned16(gy.contiguous())                                  # (held until the launch is queued)
        _call("stx_instnorm_bwd", _p(gy), _p(x), _p(skip), _p(stats), _p(gx), _p(gskip), _p(ws), planes, S, 0, ctx.act)
        return gx, gskip, None, None


def _instnorm_dense(t, name):
    """Dense NCHW / NCDHW, 16-byte aligned, fp32, on the device -- the one layout the kernels serve."""
    t = _aligned16(t.contiguous())
    _chk(t, name)
    return t


@fp32_region
def _instance_norm(x, skip, act, eps):
    x, skip = _instnorm_dense(x, "x"), (None if skip is None else _instnorm_dense(skip, "skip"))
    if torch.is_grad_enabled() and (x.requires_grad or (skip is not None and skip.requires_grad)):
        return InstanceNormFn.apply(x, skip, act, eps)
    return InstanceNormFn.forward(_NoCtx(), x, skip, act, eps)


def instance_norm(x, act="none", eps=1e-5, skip=None):
    """x [B, C, H, W] or [B, C, D, H, W] -> act(F.instance_norm(x, eps=eps)) with act "none", "relu" or "lrelu" (LeakyReLU(0.01));
    with `skip` (x's shape, dtype and device) relu(skip + act(instance_norm(x))), the tail of the reference's ResidualBlock.  No
    affine parameters, no running statistics, biased variance: nn.InstanceNorm2d / 3d as the reference constructs them, the same
    in train and eval.  One autograd node, differentiable in x and skip; the output is not saved.  The sums, the moments and the
    normalised value are formed in double and rounded once; no float atomics, bitwise reproducible.  A dense channels_last input
    goes through one layout copy each way and the result comes back channels_last; other strides are made contiguous.  fp16 / bf16
    inputs (also under autocast) are cast up and the result is returned in x's dtype."""
    who = "instance_norm"
    if act not in INSTNORM_ACTS:
        raise StxError(f"{who}: act {act!r} is not one of {tuple(INSTNORM_ACTS)}")
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise StxError(f"{who}: x must be [B, C, H, W] or [B, C, D, H, W], got {tuple(getattr(x, 'shape', ()))}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise StxError(f"{who}: empty tensor {tuple(x.shape)}")
    if x.dtype != torch.float32 and x.dtype not in _LOW:
        raise StxError(f"{who}: x must be float32, float16 or bfloat16, got {x.dtype}")
    if not on_device(x):
        raise StxError(f"{who}: expected a ROCm device tensor, got {x.device} -- there is no CPU fallback")
    S = x.numel() // (x.shape[0] * x.shape[1])
    if S < 2:
        raise StxError(f"{who}: more than one value per plane is needed, got {tuple(x.shape)} (torch refuses it in training)")
    if S >= INSTNORM_MAX_PLANE:
        raise StxError(f"{who}: {S} elements per plane are not served (2^31 and above)")
    if skip is not None and (not isinstance(skip, torch.Tensor) or skip.shape != x.shape or skip.dtype != x.dtype
                             or skip.device != x.device):
        raise StxError(f"{who}: skip must match x in shape, dtype and device: {tuple(x.shape)} {x.dtype} {x.device}, got "
                       f"{tuple(getattr(skip, 'shape', ()))} {getattr(skip, 'dtype', None)} {getattr(skip, 'device', None)}")
    low = _low_dtype(x)
    cl = x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    y = _as_dtype(_instance_norm(*_to_fp32((x, skip)), INSTNORM_ACTS[act], float(eps)), low)
    return y.contiguous(memory_format=torch.channels_last) if cl else y
