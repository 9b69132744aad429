"""The ConvGRU cell of the iterative families (reference IGEVStereo/update.py:25-40) on csrc/convgru.hip: fused gates, forward
and backward, `ops.convgru` and the drop-in module `models.IGEVStereo.ConvGRU`.

Every product test runs on the host emulator build (CPU, `-m "not gpu"`) and on gfx950 (`-m gpu`):
  * state-dict keys, shapes and order equal the reference's (tests/golden/state_dict_keys_convgru.json); the plain-torch
    restatement of the cell is pinned to the fixture (`parity.pin_fixture`: fp64 to 1e-11, fp32 to 2 x d_ref);
  * the module against the reference's own fp64 run (tests/golden/convgru*.npz, written by make_golden_convgru.py):
    `parity.within_fixture`, 2 x d_ref on h', 3 x d_ref on every gradient;
  * at the real width (hidden 128): the raw epilogue through the C-ABI against fp64 F.conv2d computed here, under the rounding
    model of an n-term fp32 sum in any order, |err| <= (n + 2) 2^-24 conv(|x|, |w|) elementwise -- forward (n = 9 K), the
    two-source data gradient with an addend on mode-1 weights (n = 9 x summed channels, one more term for the addend) and the
    weight gradient (n = B H W); and the gated cell against the pinned restatement in fp64, d_ref = the restatement's own
    fp32 CPU run;
  * strides (channel-split c*, NCHW and channels-last h, a missing c*), finite differences, skipped gradients,
    reproducibility, the pack cache, refusals and autocast.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from stereo_toolbox_amd.utils import synthetic_tensor
from tests.backends import Backend, ptr
from tests.golden.convgru_config import CASES, PARAMS, WIDE_SHAPES, cell, cell_inputs, inputs, load_gold, module_args, run_case
from tests.parity import (EPS, GRAD_FACTOR, VALUE_FACTOR, Env, directional, env, filled, on, pin_fixture, sync, within,  # noqa: F401
                          within_fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
WIDE_IDS = ["x".join(map(str, s[:4])) + "+" + "_".join(map(str, s[4])) for s in WIDE_SHAPES]
WIDE = dict(zip(WIDE_IDS, WIDE_SHAPES))
# 4 x 8 x 9 = 288 pixel tiles: the launcher takes 8-row tiles once they fill the chip, 4-row tiles below (every other shape here)
TILE8 = "tile8_4x57x129x16+8"
WIDE[TILE8] = (4, 57, 129, 16, (8,))


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def _module(tag=None, **kw):
    from stereo_toolbox_amd.models.IGEVStereo import ConvGRU
    return filled(ConvGRU, **(module_args(tag) if tag else kw))[0]


def _params(m):
    return [dict(m.named_parameters())[n] for n in PARAMS]


# ------------------------------------------------------------------------------------------ 1. state dict, restatement
def test_state_dict_matches_reference():
    want = json.load(open(os.path.join(HERE, "golden", "state_dict_keys_convgru.json")))["two_src"]
    got = [[k, list(v.shape)] for k, v in _module("two_src").state_dict().items()]
    assert got == want


def test_one_class_serves_the_five_families():
    from stereo_toolbox_amd import models
    import importlib
    classes = {importlib.import_module(f"{models.__name__}.{n}").ConvGRU
               for n in ("IGEVStereo", "RAFTStereo", "DEFOMStereo", "StereoAnywhere", "FoundationStereo")}
    assert len(classes) == 1


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_is_pinned_to_the_fixture(tag, gold):
    for dtype in (torch.float64, torch.float32):
        m = _module(tag).to(dtype)
        out = run_case(lambda h, cz, cr, cq, xs: cell(h, cz, cr, cq, xs, *_params(m)), dict(m.named_parameters()), tag, dtype)
        for k, v in out.items():
            is64 = dtype == torch.float64
            pin_fixture(v if is64 else None, None if is64 else v, gold, f"{tag}/{k}")


# ------------------------------------------------------------------------------------------ 2. module vs the fixture
@pytest.mark.parametrize("backend,tag", on(list(CASES)))
def test_module_matches_reference_fp64(backend, tag, gold, parity_log):
    env_ = Env(backend)
    dev = env_.device
    m = _module(tag).to(dev)
    with env_.ctx():
        out = run_case(lambda h, cz, cr, cq, xs: m(h.to(dev), cz.to(dev), cr.to(dev), cq.to(dev), *[x.to(dev) for x in xs]).cpu(),
                       dict(m.named_parameters()), tag, torch.float32)
        sync(env_)
    assert out["h"].dtype == torch.float32
    for k, v in out.items():
        assert v is not None, k
        within_fixture(v, gold, f"{tag}/{k}", VALUE_FACTOR if k == "h" else GRAD_FACTOR, f"convgru {tag} {k} [{backend}]", parity_log)


# ------------------------------------------------------------------------------------------ 3. the real width
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _assert_bound(got, want64, bound, what):
    err = (got.detach().cpu().double() - want64).abs()
    assert err.shape == bound.shape, (what, err.shape, bound.shape)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (what, err.max().item(), worst)


def _slices(t, widths):
    """Channel slices of a dense channels-last tensor [B][H][W][C] as the flat source arguments (pointer, channels, pitch) x 4."""
    out, off = [], 0
    for c in widths:
        out += [ptr(t[..., off:off + c]), c, t.shape[-1]]
        off += c
    return out + [None, 0, 0] * (4 - len(widths))


@pytest.mark.parametrize("backend,wid", on(WIDE_IDS, gpu_only=WIDE_IDS[2:]))
def test_raw_kernels_match_fp64_conv2d(backend, wid):
    be = Backend(backend)
    B, H, W, hidden, cx = WIDE[wid]
    K, N = hidden + sum(cx), 2 * hidden
    x = synthetic_tensor((B, K, H, W), 41)
    w = synthetic_tensor((N, K, 3, 3), 42, lo=-0.5, hi=0.5)
    g = synthetic_tensor((B, N, H, W), 43)
    addend = synthetic_tensor((B, K, H, W), 44)
    x64, w64, g64 = x.double().requires_grad_(), w.double().requires_grad_(), g.double()
    y64 = F.conv2d(x64, w64, padding=1)
    y64.backward(g64)
    xa, wa = x64.detach().abs().requires_grad_(), w64.detach().abs().requires_grad_()
    ya = F.conv2d(xa, wa, padding=1)                                     # conv(|x|, |w|)
    ya.backward(g64.abs())                                               # xa.grad = conv^T(|g|, |w|), wa.grad = sum |x| |g|

    def packed(mode, Kp, Np):
        n = be.raw("stx_convgru_packed_floats")(Kp, Np)
        assert n > 0
        wp = be.empty(n)
        be.call("stx_convgru_pack_weight", ptr(be.dev(w[:hidden])), ptr(be.dev(w[hidden:])), ptr(wp), hidden, K, mode)
        return wp

    def gemm(srcs, wp, Nout, add, out):
        be.call("stx_convgru_gemm", *srcs, ptr(wp), Nout, 0, 0, None, None, ptr(add), Nout if add is not None else 0, None, 0,
                None, 0, None, ptr(out), None, None, Nout, B, H, W)

    # forward: the sources are the channel slices [hidden | x..] of one map (pitch K)
    xd = be.dev(_nhwc(x))
    y = be.empty(B, H, W, N)
    gemm(_slices(xd, (hidden,) + tuple(cx)), packed(0, K, N), N, None, y)
    _assert_bound(y.permute(0, 3, 1, 2), y64.detach(), (9 * K + 2) * EPS * ya.detach(), "forward")

    # data gradient: mode-1 weights, the two sources [gz, gr] (pitch 2 hidden), the running gradient as addend, in place
    gd = be.dev(_nhwc(g))
    buf = be.dev(_nhwc(addend)).clone()
    gemm(_slices(gd, (hidden, hidden)), packed(1, N, K), K, buf, buf)
    _assert_bound(buf.permute(0, 3, 1, 2), x64.grad + addend.double(), (9 * N + 3) * EPS * (xa.grad + addend.double().abs()),
                  "data gradient + addend")

    # weight gradient of both maps at once
    nws = be.raw("stx_convgru_wgrad_workspace_floats")(B, H, W, K, N)
    assert nws > 0
    ws, dw = be.empty(nws), be.empty(N, K, 9)
    g0, g1 = gd[..., :hidden].contiguous(), gd[..., hidden:].contiguous()
    be.call("stx_convgru_wgrad", *_slices(xd, (hidden,) + tuple(cx)), ptr(g0), ptr(g1), hidden, ptr(dw), ptr(ws), B, H, W)
    _assert_bound(dw.view(N, K, 3, 3), w64.grad, (B * H * W + 2) * EPS * wa.grad, "weight gradient")


@pytest.fixture(scope="module")
def wide_reference():
    """fp64 and fp32 CPU runs of the pinned restatement at the real width, computed once per shape."""
    cache = {}

    def get(wid):
        if wid not in cache:
            B, H, W, hidden, cx = WIDE[wid]
            h, cz, cr, cq, xs, (g,) = cell_inputs(B, hidden, cx, H, W, seed=51)
            runs = []
            for dtype in (torch.float64, torch.float32):
                md = _module(hidden_dim=hidden, input_dim=sum(cx)).to(dtype)
                leaves = [t.clone().to(dtype).requires_grad_() for t in [h, cz, cr, cq] + xs]
                y = cell(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4:], *_params(md))
                (y * g.to(dtype)).sum().backward()
                runs.append([y.detach()] + [t.grad for t in leaves] + [p.grad for p in _params(md)])
            cache[wid] = ((h, cz, cr, cq, xs, g), runs)
        return cache[wid]
    return get


@pytest.mark.parametrize("backend,wid", on(WIDE_IDS + [TILE8], gpu_only=WIDE_IDS[2:]))
def test_gated_cell_at_real_width(backend, wid, wide_reference, parity_log):
    env_ = Env(backend)
    dev = env_.device
    (h, cz, cr, cq, xs, g), (r64, r32) = wide_reference(wid)
    hidden, cx = WIDE[wid][3:]
    m = _module(hidden_dim=hidden, input_dim=sum(cx)).to(dev)
    leaves = [t.clone().to(dev).requires_grad_() for t in [h, cz, cr, cq] + xs]    # (clone: .to() of a CPU tensor is the tensor)
    with env_.ctx():
        y = m(*leaves)
        (y * g.to(dev)).sum().backward()
        sync(env_)
    got = [y] + [t.grad for t in leaves] + [p.grad for p in _params(m)]
    names = ["h'", "g_h", "g_cz", "g_cr", "g_cq"] + [f"g_x{i}" for i in range(len(xs))] + ["grad/" + n for n in PARAMS]
    for name, a, w64, w32 in zip(names, got, r64, r32):
        dref = (w32.double() - w64).abs().max().item()
        within(a, w64, dref, VALUE_FACTOR if name == "h'" else GRAD_FACTOR, f"convgru {wid} {name} [{backend}]", parity_log)


# ------------------------------------------------------------------------------------------ 4. strides
def test_strided_inputs_are_consumed_in_place(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    B, hidden, cx, H, W, _ = CASES["two_src"]
    h, cz, cr, cq, xs, _ = inputs("two_src")
    m = _module("two_src").to(dev)
    ps = [p.detach() for p in _params(m)]
    dense = [t.to(dev) for t in (h, cz, cr, cq)]
    xd = [x.to(dev) for x in xs]
    c3 = torch.cat([cz, cr, cq], 1).to(dev).contiguous(memory_format=torch.channels_last)
    split = list(c3.split(hidden, 1))
    assert ops._cl_pitch(split[1]) == 3 * hidden and ops._cl_pitch(dense[0]) is None
    h_cl = dense[0].contiguous(memory_format=torch.channels_last)
    with env.ctx():
        want = ops.convgru(*dense, xd, *ps)
        for hh in (dense[0], h_cl):
            got = ops.convgru(hh, *split, xd, *ps)
            assert torch.equal(got, want)
            assert got.shape == h.shape and got.permute(0, 2, 3, 1).is_contiguous()
        none = ops.convgru(dense[0], dense[1], None, dense[3], xd, *ps)
        zeros = ops.convgru(dense[0], dense[1], torch.zeros_like(dense[2]), dense[3], xd, *ps)
        sync(env)
    assert torch.equal(none, zeros) and not torch.equal(none, want)


def test_loop_converts_only_in_its_first_iteration(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    h, cz, cr, cq, xs, _ = inputs("loop3")
    m = _module("loop3").to(dev)
    with env.ctx(), torch.no_grad():
        net = m(h.to(dev), cz.to(dev), cr.to(dev), cq.to(dev), *[x.to(dev) for x in xs])
    assert ops._cl_pitch(net) == net.shape[1]


# ------------------------------------------------------------------------------------------ 5. custom backward
def _fd_inputs():
    B, H, W, hidden, cx = 1, 3, 5, 16, (8, 4)
    h, cz, cr, cq, xs, _ = cell_inputs(B, hidden, cx, H, W, seed=61)
    m = _module(hidden_dim=hidden, input_dim=sum(cx))
    return [h, cz, cr, cq] + xs + [p.detach().clone() for p in _params(m)]


def _apply(dev, ts):
    from stereo_toolbox_amd import ops
    h, cz, cr, cq, x0, x1, *ps = [t.to(dev) if t.device != dev else t for t in ts]
    return ops.convgru(h, cz, cr, cq, [x0, x1], *ps)


def test_backward_matches_finite_differences(env):  # noqa: F811
    dev = env.device
    with env.ctx():                                          # (the backward pass runs inside `directional`)
        directional(lambda *ts: _apply(dev, ts).cpu(), _fd_inputs())


def test_skipped_gradients_leave_the_others_unchanged(env):  # noqa: F811
    dev = env.device
    base = _fd_inputs()
    g = synthetic_tensor(tuple(base[0].shape), 62).to(dev)

    def run(wanted):
        ts = [t.clone().to(dev).requires_grad_(i in wanted) for i, t in enumerate(base)]
        with env.ctx():
            (_apply(dev, ts) * g).sum().backward()
            sync(env)
        return [None if t.grad is None else t.grad.cpu() for t in ts]
    full = run(set(range(12)))
    assert all(t is not None for t in full)
    for wanted in ({0, 1, 6, 7}, {0, 3, 5, 10, 11}, {2, 4}, {8, 9}):           # no x source; one x source; no weight; wr alone
        part = run(wanted)
        for i, (a, b) in enumerate(zip(part, full)):
            assert (a is not None) == (i in wanted), i
            if a is not None:
                assert torch.equal(a, b), (sorted(wanted), i)


# ------------------------------------------------------------------------------------------ 6. reproducibility
def _two_runs(env_, m, h, cz, cr, cq, xs, g):
    dev = env_.device
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        leaves = [t.clone().to(dev).requires_grad_() for t in [h, cz, cr, cq] + xs]    # (clone: .to() of a CPU tensor is the tensor)
        with env_.ctx():
            y = m(*leaves)
            (y * g.to(dev)).sum().backward()
            sync(env_)
        runs.append([y.detach().cpu()] + [t.grad.cpu().clone() for t in leaves] + [p.grad.cpu().clone() for p in _params(m)])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i


def test_two_runs_give_equal_bits(env):  # noqa: F811
    h, cz, cr, cq, xs, (g,) = inputs("ragged")
    _two_runs(env, _module("ragged").to(env.device), h, cz, cr, cq, xs, g)


@pytest.mark.gpu
def test_two_runs_give_equal_bits_at_real_width():
    env_ = Env("hip")
    B, H, W, hidden, cx = WIDE_SHAPES[2]
    h, cz, cr, cq, xs, (g,) = cell_inputs(B, hidden, cx, H, W, seed=51)
    _two_runs(env_, _module(hidden_dim=hidden, input_dim=sum(cx)).to(env_.device), h, cz, cr, cq, xs, g)


# ------------------------------------------------------------------------------------------ 7. pack cache
def test_pack_cache_follows_the_weight_version(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    h, cz, cr, cq, xs, _ = inputs("one_src")
    args = [t.to(dev) for t in (h, cz, cr, cq)] + [x.to(dev) for x in xs]
    m = _module("one_src").to(dev)
    with env.ctx(), torch.no_grad():
        before = m(*args).clone()
        m.convq.weight.mul_(0.5)                             # an in-place update: the version counter moves
        m.convz.weight.add_(0.01)
        after = m(*args)
        fresh = _module("one_src").to(dev)
        fresh.load_state_dict(m.state_dict())
        want = fresh(*args)
        sync(env)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_training_loop_packs_once(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    m = _module("loop3").to(dev)
    n0 = ops.CONVGRU_PACKS
    with env.ctx():
        run_case(lambda h, cz, cr, cq, xs: m(h.to(dev), cz.to(dev), cr.to(dev), cq.to(dev), *[x.to(dev) for x in xs]).cpu(),
                 dict(m.named_parameters()), "loop3", torch.float32)
        sync(env)
    assert ops.CONVGRU_PACKS - n0 == 4                       # zr and q, forward and data gradient: not 3 x 4
    assert len(m.convz.weight.__dict__["_stx_packed"]) == 2 and len(m.convq.weight.__dict__["_stx_packed"]) == 2


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_without_a_device():
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models.IGEVStereo import ConvGRU
    h, cz, cr, cq, xs, _ = inputs("one_src")
    with pytest.raises(ops.StxError):                       # CPU tensors on the product path
        _module("one_src")(h, cz, cr, cq, *xs)
    with pytest.raises(ops.StxError):
        ConvGRU(16, 16, kernel_size=5)


def test_shape_refusals(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device

    def call(hidden, cx, H=4, W=6, dtype=torch.float32, hw=None):
        z = lambda c, s=None: torch.zeros(1, c, *(s or (H, W)), device=dev, dtype=dtype)          # noqa: E731
        K = hidden + sum(cx)
        w, b = torch.zeros(hidden, K, 3, 3, device=dev, dtype=dtype), torch.zeros(hidden, device=dev, dtype=dtype)
        xs = [z(c) for c in cx]
        if hw:
            xs[-1] = z(cx[-1], hw)
        return ops.convgru(z(hidden), z(hidden), z(hidden), z(hidden), xs, w, b, w, b, w, b)
    with env.ctx():
        assert call(16, (8,)).shape == (1, 16, 4, 6)         # the edge that is served
        for kw in (dict(hidden=24, cx=(8,)), dict(hidden=16, cx=(6,)), dict(hidden=16, cx=(4, 4, 4, 4)), dict(hidden=16, cx=()),
                   dict(hidden=128, cx=(256, 132)), dict(hidden=144, cx=(16,)), dict(hidden=16, cx=(8,), dtype=torch.float16),
                   dict(hidden=16, cx=(8, 8), hw=(4, 7))):
            with pytest.raises(ops.StxError):
                call(**kw)
        with pytest.raises(ops.StxError):                   # a 5x5 weight
            ops.convgru(torch.zeros(1, 16, 4, 6, device=dev), None, None, None, [torch.zeros(1, 8, 4, 6, device=dev)],
                        *[torch.zeros(16, 24, 5, 5, device=dev), None] * 3)
        sup = ops.get_lib().raw("stx_convgru_supported")
        assert sup(128, 2, 128, 128, 0, 3) == 1 and sup(128, 2, 256, 128, 0, 3) == 1 and sup(128, 3, 256, 124, 4, 3) == 1
        assert sup(128, 2, 256, 132, 0, 3) == 0              # K above 512
        assert sup(16, 1, 4, 0, 0, 3) == 1 and sup(16, 1, 6, 0, 0, 3) == 0
        assert sup(24, 1, 8, 0, 0, 3) == 0 and sup(144, 1, 16, 0, 0, 3) == 0
        assert sup(16, 0, 0, 0, 0, 3) == 0 and sup(16, 4, 4, 4, 4, 3) == 0 and sup(16, 1, 8, 4, 0, 3) == 0
        assert sup(16, 1, 8, 0, 0, 5) == 0
        assert ops.get_lib().raw("stx_convgru_packed_floats")(516, 16) == 0
        assert ops.get_lib().raw("stx_convgru_wgrad_workspace_floats")(1, 4, 4, 24, 24) == 0


# ------------------------------------------------------------------------------------------ 9. autocast
def test_autocast_is_the_fp32_path_on_the_cast_up_inputs(env):  # noqa: F811
    dev = env.device
    low = torch.float16 if dev.type == "cuda" else torch.bfloat16
    h, cz, cr, cq, xs, _ = inputs("one_src")
    args = [t.to(dev).to(low) for t in [h, cz, cr, cq] + xs]
    m = _module("one_src").to(dev)
    with env.ctx(), torch.no_grad():
        with torch.amp.autocast(dev.type, dtype=low):
            under = m(*args)
        plain = m(*[t.float() for t in args])
        sync(env)
    assert under.dtype == torch.float32
    assert torch.equal(under, plain)
