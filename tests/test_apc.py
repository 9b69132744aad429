"""FoundationStereo's axial-planar convolution block (`Conv3dNormActReduced`, reference FoundationStereo/submodule.py:89-114) on
csrc/conv3d_axial.hip: the (1,3,3) and (kd,1,1) stride-1 convolutions, forward / data gradient / weight gradient.

Every test runs on the host emulator build (CPU, `-m "not gpu"`) and on gfx950 (`-m gpu`):
  * state-dict keys, shapes and order equal the reference's (tests/golden/state_dict_keys_apc.json);
  * the block in train mode and in eval mode against the reference's own fp64 run (tests/golden/apc*.npz, written by
    make_golden_apc.py): `parity.within_fixture`, 2 x d_ref on values and running statistics, 3 x d_ref on gradients;
  * the kernels through the C-ABI against fp64 F.conv3d computed here, under the rounding model of an n-term fp32 sum in any
    order, |err| <= (n + 2) 2^-24 conv(|x|, |w|) elementwise: raw forward, BatchNorm partial rows, the fused scale / bias /
    residual / ReLU epilogue, the data gradient (autograd's x.grad) and the weight gradient (n = B D H W);
  * the custom backward against central differences; bitwise reproducibility; refusals; autocast.
"""
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from stereo_toolbox_amd.utils import synthetic_tensor
from tests.backends import be, ptr  # noqa: F401
from tests.golden.apc_config import AXIAL_SHAPES, CASES, PLANAR_SHAPES, block_args, inputs, load_gold
from tests.parity import EPS, GRAD_FACTOR, VALUE_FACTOR, directional, env, filled, on, sync, within_fixture  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
TILE_VOXELS = 256          # a workgroup of the forward kernels owns 16 M tiles of 16 voxels: the terms of one partial row


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def _block(tag=None, **kw):
    from stereo_toolbox_amd.models.FoundationStereo import Conv3dNormActReduced
    return filled(Conv3dNormActReduced, **(block_args(tag) if tag else kw))[0]


# ------------------------------------------------------------------------------------------ 1. state dict
def test_state_dict_matches_reference():
    want = json.load(open(os.path.join(HERE, "golden", "state_dict_keys_apc.json")))["short"]
    got = [[k, list(v.shape)] for k, v in _block("short").state_dict().items()]
    assert got == want


# ------------------------------------------------------------------------------------------ 2. block vs the fixture
@pytest.mark.parametrize("backend,tag", on(list(CASES)))
def test_block_matches_reference_fp64(backend, tag, gold, parity_log):
    from tests.parity import Env
    env_ = Env(backend)
    dev = env_.device
    sx, sg = (int(s) for s in gold[f"{tag}/seeds"])
    x, g = inputs(tag, sx, sg)
    m = _block(tag).to(dev).train()
    xd = x.to(dev).requires_grad_()
    with env_.ctx():
        y = m(xd)
        assert y.shape == g.shape and y.dtype == torch.float32
        (y * g.to(dev)).sum().backward()
        sync(env_)
        e = _block(tag).to(dev).eval()
        with torch.no_grad():
            y_eval = e(x.to(dev))
        sync(env_)
    name = f"apc {tag}"
    within_fixture(y, gold, f"{tag}/y", VALUE_FACTOR, f"{name} y [{backend}]", parity_log)
    for n, b in m.named_buffers():
        if n.endswith(("running_mean", "running_var")):
            within_fixture(b, gold, f"{tag}/state/{n}", VALUE_FACTOR, f"{name} {n} [{backend}]", parity_log)
    within_fixture(xd.grad, gold, f"{tag}/gx", GRAD_FACTOR, f"{name} gx [{backend}]", parity_log)
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        within_fixture(p.grad, gold, f"{tag}/grad/{n}", GRAD_FACTOR, f"{name} grad {n} [{backend}]", parity_log)
    within_fixture(y_eval, gold, f"{tag}/y_eval", VALUE_FACTOR, f"{name} y_eval [{backend}]", parity_log)


# ------------------------------------------------------------------------------------------ 3. kernels vs fp64 F.conv3d
def _kernel_case(shape):
    if len(shape) == 6:
        B, D, H, W, Cin, Cout = shape
        k = (1, 3, 3)
    else:
        B, D, H, W, Cin, Cout, kd = shape
        k = (kd, 1, 1)
    x = synthetic_tensor((B, Cin, D, H, W), 11)
    w = synthetic_tensor((Cout, Cin, *k), 12, lo=-0.5, hi=0.5)
    g = synthetic_tensor((B, Cout, D, H, W), 13)
    return x, w, g, k


def _nd(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _cd(t):
    return t.permute(0, 4, 1, 2, 3)


def _pack(be, w, k, mode):  # noqa: F811
    A, Bd = w.shape[0], w.shape[1]
    K, N = (Bd, A) if mode == 0 else (A, Bd)
    n = be.raw("stx_conv3d_axial_packed_floats")(K, N, *k)
    assert n > 0
    wp = be.empty(n)
    be.call("stx_conv3d_axial_pack_weight", ptr(be.dev(w)), ptr(wp), A, Bd, *k, mode)
    return wp


def _fwd(be, x_nd, wp, Cout, k, scale=None, bias=None, residual=None, act=0, stats=False):  # noqa: F811
    B, D, H, W, Cin = x_nd.shape
    out = be.empty(B, D, H, W, Cout)
    st = None
    if stats:
        rows = be.raw("stx_conv3d_axial_fwd_stat_rows")(B, D, H, W, Cin, Cout, *k)
        assert rows > 0
        st = be.empty(rows + 1, 2, Cout)                      # one sentinel row behind the slab
    be.call("stx_conv3d_axial_fwd", ptr(x_nd), ptr(wp), ptr(out), ptr(scale), ptr(bias), ptr(residual), ptr(st), B, D, H, W, Cin,
            Cout, *k, act)
    return out, st


def _assert_bound(got, want64, bound, what):
    err = (got.detach().cpu().double() - want64).abs()
    assert err.shape == bound.shape, (what, err.shape, bound.shape)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (what, err.max().item(), worst)


@pytest.mark.parametrize("shape", PLANAR_SHAPES + AXIAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_fp64_conv3d(be, shape):  # noqa: F811
    x, w, g, k = _kernel_case(shape)
    B, Cin, D, H, W = x.shape
    Cout, T = w.shape[0], k[0] * k[1] * k[2]
    pad = tuple(v // 2 for v in k)
    x64, w64, g64 = x.double().requires_grad_(), w.double().requires_grad_(), g.double()
    z64 = F.conv3d(x64, w64, padding=pad)
    z64.backward(g64)
    xa, wa = x64.detach().abs().requires_grad_(), w64.detach().abs().requires_grad_()
    za = F.conv3d(xa, wa, padding=pad)                                   # conv(|x|, |w|)
    za.backward(g64.abs())                                               # xa.grad = conv^T(|g|, |w|), wa.grad = sum |x| |g|
    n_fwd, n_dg, n_wg = T * Cin, T * Cout, B * D * H * W
    bz = (n_fwd + 2) * EPS * za.detach()

    # raw forward + BatchNorm partial rows
    xd = be.dev(_nd(x))
    wp = _pack(be, w, k, 0)
    z, st = _fwd(be, xd, wp, Cout, k, stats=True)
    _assert_bound(_cd(z), z64.detach(), bz, "forward")
    st = st.cpu()
    assert bool(torch.isfinite(st[:-1]).all()), "a partial row was not written"
    assert bool(torch.isnan(st[-1]).all()), "the launch wrote behind its rows"
    zc = _cd(z).cpu().double()
    s1, s2 = st[:-1, 0].double().sum(0), st[:-1, 1].double().sum(0)
    _assert_bound(s1, zc.sum((0, 2, 3, 4)), (TILE_VOXELS + 2) * EPS * zc.abs().sum((0, 2, 3, 4)), "stats sum")
    _assert_bound(s2, (zc * zc).sum((0, 2, 3, 4)), (TILE_VOXELS + 2) * EPS * (zc * zc).sum((0, 2, 3, 4)), "stats sum of squares")

    # fused epilogue: ReLU(z * scale + bias + residual)
    sc = synthetic_tensor((Cout,), 14, lo=0.5, hi=1.5)
    bs = synthetic_tensor((Cout,), 15, lo=-0.5, hi=0.5)
    res = synthetic_tensor((B, Cout, D, H, W), 16)
    y, _ = _fwd(be, xd, wp, Cout, k, be.dev(sc), be.dev(bs), be.dev(_nd(res)), 1)
    v = sc.double().view(1, -1, 1, 1, 1)
    pre = z64.detach() * v + bs.double().view(1, -1, 1, 1, 1) + res.double()
    by = bz * v + 3 * EPS * ((z64.detach() * v).abs() + bs.double().abs().view(1, -1, 1, 1, 1) + res.double().abs())
    _assert_bound(_cd(y), pre.clamp_min(0), by, "fused epilogue")

    # data gradient: the same kernel on flipped / transposed weights
    gd = be.dev(_nd(g))
    gx, _ = _fwd(be, gd, _pack(be, w, k, 1), Cin, k)
    _assert_bound(_cd(gx), x64.grad, (n_dg + 2) * EPS * xa.grad, "data gradient")

    # weight gradient
    nws = be.raw("stx_conv3d_axial_wgrad_workspace_floats")(B, D, H, W, Cin, Cout, *k)
    assert nws > 0
    ws, dw = be.empty(nws), be.empty(Cout, Cin, T)
    be.call("stx_conv3d_axial_wgrad", ptr(xd), ptr(gd), ptr(dw), ptr(ws), B, D, H, W, Cin, Cout, *k)
    _assert_bound(dw.view(Cout, Cin, *k), w64.grad, (n_wg + 2) * EPS * wa.grad, "weight gradient")


# ------------------------------------------------------------------------------------------ 4. custom backward
def _short():
    B, Cin, hidden, Cout, kdisp, D, H, W = CASES["short"]
    return B, Cin, hidden, Cout, kdisp, D, H, W


@pytest.mark.parametrize("which", ["planar", "axial"])
def test_functional_backward_matches_finite_differences(env, which):  # noqa: F811
    from stereo_toolbox_amd import ops
    B, Cin, hidden, Cout, kdisp, D, H, W = _short()
    k = (1, 3, 3) if which == "planar" else (kdisp, 1, 1)
    x = synthetic_tensor((B, D, H, W, Cin), 21)
    w = synthetic_tensor((hidden, Cin, *k), 22, lo=-0.5, hi=0.5)
    b = synthetic_tensor((hidden,), 23, lo=-0.5, hi=0.5)
    dev = env.device

    def fn(x_, w_, b_):
        return ops.conv3d_axial(x_.to(dev), w_.to(dev), b_.to(dev)).cpu()
    with env.ctx():                                          # (the backward pass runs inside `directional`)
        directional(fn, [x, w, b])


def test_block_backward_matches_finite_differences(env):  # noqa: F811
    dev = env.device
    m = _block("short").to(dev).train()
    names = [n for n, _ in m.named_parameters()]
    x, _ = inputs("short")

    def fn(x_, *ps):
        return torch.func.functional_call(m, {n: p.to(dev) for n, p in zip(names, ps)}, (x_.to(dev),)).cpu()
    # eps: the block is piecewise linear, so the central difference is off only by the ReLUs that flip inside +-eps v -- an
    # error proportional to eps (84 voxels: 4 % at 3e-3, 1.4 % at 1e-3) -- while its fp32 rounding noise, about
    # 2^-24 |y| sqrt(#outputs) / eps = 3e-3 at 1e-3 against directional derivatives of 1..40, still is negligible
    with env.ctx():
        directional(fn, [x] + [p.detach().cpu() for p in m.parameters()], eps=1e-3)


# ------------------------------------------------------------------------------------------ 5. reproducibility
@pytest.mark.parametrize("shape", [PLANAR_SHAPES[2], AXIAL_SHAPES[3]], ids=["planar", "axial"])
def test_two_runs_give_equal_bits(env, shape):  # noqa: F811
    from stereo_toolbox_amd import ops
    x, w, g, k = _kernel_case(shape)
    dev = env.device
    runs = []
    for _ in range(2):
        xd, wd = _nd(x).to(dev).requires_grad_(), w.to(dev).requires_grad_()
        with env.ctx():
            z = ops.conv3d_axial(xd, wd)
            z.backward(_nd(g).to(dev))
            sync(env)
        runs.append((z.detach().cpu(), xd.grad.cpu(), wd.grad.cpu()))
    for a, b, what in zip(runs[0], runs[1], ("forward", "data gradient", "weight gradient")):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models.FoundationStereo import Conv3dNormActReduced
    with pytest.raises(ops.StxError):                       # a CPU tensor on the product path
        _block("short").eval()(inputs("short")[0])
    with pytest.raises(ops.StxError):
        ops.conv3d_axial(torch.zeros(1, 3, 4, 4, 8), torch.zeros(8, 8, 1, 3, 3))
    for kw in (dict(stride=2), dict(norm=nn.InstanceNorm3d), dict(kernel_disp=19), dict(kernel_size=5), dict(kernel_disp=4)):
        with pytest.raises(ops.StxError):
            Conv3dNormActReduced(8, 8, **kw)


def test_kernel_shape_and_layout_refusals(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    x = torch.zeros(1, 3, 4, 4, 8, device=dev)
    if env.name == "hip":                                   # (the emulator context replaces the argument check)
        with pytest.raises(ops.StxError):
            ops.conv3d_axial(x.half(), torch.zeros(8, 8, 1, 3, 3, device=dev))
        with pytest.raises(ops.StxError):
            ops.conv3d_axial(x.permute(0, 1, 3, 2, 4), torch.zeros(8, 8, 1, 3, 3, device=dev))
    with env.ctx():
        for k in ((3, 3, 3), (19, 1, 1), (4, 1, 1), (1, 5, 5), (1, 1, 1)):
            with pytest.raises(ops.StxError):
                ops.conv3d_axial(x, torch.zeros(8, 8, *k, device=dev))
        lib = ops.get_lib()
        assert lib.raw("stx_conv3d_axial_supported")(28, 28, 17, 1, 1) == 1
        assert lib.raw("stx_conv3d_axial_supported")(28, 28, 19, 1, 1) == 0
        assert lib.raw("stx_conv3d_axial_supported")(30, 28, 1, 3, 3) == 0
        assert lib.raw("stx_conv3d_axial_supported")(196, 28, 1, 3, 3) == 0
        assert lib.raw("stx_conv3d_axial_fwd_stat_rows")(1, 4, 4, 4, 28, 28, 3, 3, 3) == 0


def test_gradients_of_distinct_parameters_do_not_alias(env):  # noqa: F811
    dev = env.device
    m = _block("short").to(dev).train()
    x, g = inputs("short")
    with env.ctx():
        (m(x.to(dev)) * g.to(dev)).sum().backward()
        sync(env)
    spans = sorted((p.grad.untyped_storage().data_ptr() + p.grad.storage_offset() * 4, p.grad.numel() * 4, n)
                   for n, p in m.named_parameters())
    for (a, na, ka), (b, _, kb) in zip(spans, spans[1:]):
        assert a + na <= b, f"gradients of {ka} and {kb} share memory"


# ------------------------------------------------------------------------------------------ 7. autocast
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_autocast_is_the_fp32_path_on_the_cast_up_input(env, mode):  # noqa: F811
    dev = env.device
    low = torch.float16 if dev.type == "cuda" else torch.bfloat16
    x, _ = inputs("short")
    xl = x.to(dev).to(low)
    m = _block("short").to(dev)
    m.train(mode == "train")
    with env.ctx(), torch.no_grad():
        with torch.amp.autocast(dev.type, dtype=low):
            under = m(xl)
        plain = m(xl.float())
        sync(env)
    assert under.dtype == torch.float32
    assert torch.equal(under, plain)
