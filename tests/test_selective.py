"""SelectiveStereo on csrc/selgru.hip and csrc/csa.hip: the selective recurrent unit (`ops.raft_convgru`, `ops.selective_convgru`,
`models.SelectiveStereo.RaftConvGRU / SelectiveConvGRU`) and the contextual spatial attention (`ops.csa_gate`, `ops.csa_spatial`,
`ops.csa`, `ChannelAttentionEnhancement`, `SpatialAttentionExtractor`, `contextual_spatial_attention`), forward and backward.

Every product test runs on the host emulator build (CPU, `-m "not gpu"`) and on gfx950 (`-m gpu`):
  * state-dict keys, shapes and order equal the reference's (tests/golden/state_dict_keys_selective.json); the plain-torch
    restatements are pinned to the fixture (`parity.pin_fixture`: fp64 to 1e-11, fp32 to 2 x d_ref);
  * the modules against the reference's own fp64 run (tests/golden/selective*.npz, written by make_golden_selective.py):
    `parity.within_fixture`, 2 x d_ref on outputs, 3 x d_ref on every gradient (h, att, every x source, the twelve cell
    parameters; x and the three attention weights);
  * at the real width (hidden 128): the raw 1x1 kernels through the C-ABI against fp64 F.conv2d computed here, under the rounding
    model of an n-term fp32 sum in any order, |err| <= (n + 2) 2^-24 conv(|x|, |w|) elementwise -- forward (n = K), the
    two-source data gradient with its addends on mode-1 weights (n = N + 1 in place, N + 2 with both addends) and the weight
    gradient (n = B H W); the selective cell and the attention against the pinned restatement in fp64, d_ref = the restatement's
    own fp32 CPU run on one thread, RECORDED in tests/golden/selective_parity_dref.json (tests/parity.py::RecordedDref;
    STX_SELECTIVE_DREF_RECORD=<path> runs the module with the live values and writes them to <path>);
  * identities to the bit, strides, finite differences, skipped gradients, reproducibility, the pack cache, refusals, autocast.
"""
import contextlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from stereo_toolbox_amd.utils import synthetic_tensor
from tests.backends import Backend, ptr
from tests.golden.selective_config import (CELL_CASES, CELL_PARAMS, CSA_CASES, CSA_GPU_CASE, CSA_KERNEL, CSA_PARAMS, WIDE_SHAPES, cell,
                                           cell_inputs, csa, csa_inputs, csa_shape, inputs, load_gold, module_args, run_cell_case,
                                           run_csa_case)
from tests.parity import (EPS, GRAD_FACTOR, VALUE_FACTOR, Env, RecordedDref, directional, env, filled, on, pin_fixture, sync,  # noqa: F401
                          within, within_fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
_dref = RecordedDref(os.path.join(HERE, "golden", "selective_parity_dref.json"), "STX_SELECTIVE_DREF_RECORD")
WIDE_IDS = ["x".join(map(str, s[:4])) + "+" + "_".join(map(str, s[4])) for s in WIDE_SHAPES]
WIDE = dict(zip(WIDE_IDS, WIDE_SHAPES))
WIDE_GPU_ONLY = WIDE_IDS[2:3]
CSA_BIG = CSA_GPU_CASE[0]


@pytest.fixture(scope="module")
def gold():
    return load_gold()


@contextlib.contextmanager
def _one_thread():
    """The references run on ONE thread: d_ref must not depend on the core count (tests/parity.py::RecordedDref)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _cell_module(tag=None, **kw):
    from stereo_toolbox_amd.models.SelectiveStereo import SelectiveConvGRU
    return filled(SelectiveConvGRU, **(module_args(tag) if tag else kw))[0]


def _cell_params(m):
    return [dict(m.named_parameters())[n] for n in CELL_PARAMS]


def _csa_modules(C):
    from stereo_toolbox_amd.models.SelectiveStereo import ChannelAttentionEnhancement, SpatialAttentionExtractor
    return filled(ChannelAttentionEnhancement, C)[0], filled(SpatialAttentionExtractor, CSA_KERNEL)[0]


def _csa_named(cam, sam):
    params = {"cam/" + k: v for k, v in cam.named_parameters()}
    params.update({"sam/" + k: v for k, v in sam.named_parameters()})
    assert tuple(params) == CSA_PARAMS
    return params


# ------------------------------------------------------------------------------------------ 1. state dict, package, restatement
def test_state_dict_matches_reference():
    from stereo_toolbox_amd.models.SelectiveStereo import ChannelAttentionEnhancement, SelectiveConvGRU, SpatialAttentionExtractor
    want = json.load(open(os.path.join(HERE, "golden", "state_dict_keys_selective.json")))
    for name, m in (("SelectiveConvGRU", SelectiveConvGRU(**module_args("two_src"))),
                    ("ChannelAttentionEnhancement", ChannelAttentionEnhancement(32)),
                    ("SpatialAttentionExtractor", SpatialAttentionExtractor(CSA_KERNEL))):
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want[name], name


def test_sub_packages_export_the_same_objects():
    from stereo_toolbox_amd.models import IGEVStereo, RAFTStereo, SelectiveStereo
    from stereo_toolbox_amd.models.SelectiveStereo import SelectiveIGEV, SelectiveRAFT
    for name in ("RaftConvGRU", "SelectiveConvGRU", "ChannelAttentionEnhancement", "SpatialAttentionExtractor",
                 "contextual_spatial_attention"):
        assert getattr(SelectiveIGEV, name) is getattr(SelectiveRAFT, name) is getattr(SelectiveStereo, name), name
    for name in ("ConvGRU", "Combined_Geo_Encoding_Volume", "context_upsample", "upsample_disp_from_logits", "build_gwc_volume"):
        assert getattr(SelectiveIGEV, name) is getattr(IGEVStereo, name), name
    for name in ("CorrBlock1D", "CorrBlockFast1D", "PytorchAlternateCorrBlock1D", "upsample_flow"):
        assert getattr(SelectiveRAFT, name) is getattr(RAFTStereo, name), name
    assert SelectiveRAFT.ConvGRU is IGEVStereo.ConvGRU and SelectiveRAFT.context_upsample is IGEVStereo.context_upsample


@pytest.mark.parametrize("tag", list(CELL_CASES) + list(CSA_CASES))
def test_restatement_is_pinned_to_the_fixture(tag, gold):
    for dtype in (torch.float64, torch.float32):
        if tag in CELL_CASES:
            m = _cell_module(tag).to(dtype)
            out = run_cell_case(lambda att, h, xs: cell(att, h, xs, _cell_params(m)), dict(m.named_parameters()), tag, dtype)
        else:
            cam, sam = (t.to(dtype) for t in _csa_modules(CSA_CASES[tag][1]))
            out = run_csa_case(lambda x: csa(x, cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight), _csa_named(cam, sam), tag, dtype)
        for k, v in out.items():
            is64 = dtype == torch.float64
            pin_fixture(v if is64 else None, None if is64 else v, gold, f"{tag}/{k}")


# ------------------------------------------------------------------------------------------ 2. modules vs the fixture
@pytest.mark.parametrize("backend,tag", on(list(CELL_CASES)))
def test_cell_matches_reference_fp64(backend, tag, gold, parity_log):
    env_ = Env(backend)
    dev = env_.device
    m = _cell_module(tag).to(dev)
    with env_.ctx():
        out = run_cell_case(lambda att, h, xs: m(att.to(dev), h.to(dev), *[x.to(dev) for x in xs]).cpu(), dict(m.named_parameters()),
                            tag, torch.float32)
        sync(env_)
    assert out["h"].dtype == torch.float32 and len(out) == 3 + len(CELL_CASES[tag][2]) + 12
    for k, v in out.items():
        assert v is not None, k
        within_fixture(v, gold, f"{tag}/{k}", VALUE_FACTOR if k == "h" else GRAD_FACTOR, f"selective {tag} {k} [{backend}]", parity_log)


@pytest.mark.parametrize("backend,tag", on(list(CSA_CASES)))
def test_attention_matches_reference_fp64(backend, tag, gold, parity_log):
    from stereo_toolbox_amd.models.SelectiveStereo import contextual_spatial_attention
    env_ = Env(backend)
    dev = env_.device
    cam, sam = (t.to(dev) for t in _csa_modules(CSA_CASES[tag][1]))

    def step(x):
        (xp,), (att,) = contextual_spatial_attention(cam, sam, [x.to(dev)])
        return xp.cpu(), att.cpu()
    with env_.ctx():
        out = run_csa_case(step, _csa_named(cam, sam), tag, torch.float32)
        sync(env_)
    assert len(out) == 6
    for k, v in out.items():
        assert v is not None, k
        within_fixture(v, gold, f"{tag}/{k}", VALUE_FACTOR if k in ("xp", "att") else GRAD_FACTOR, f"csa {tag} {k} [{backend}]", parity_log)


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


@pytest.mark.parametrize("backend,wid", on(WIDE_IDS, gpu_only=WIDE_GPU_ONLY))
def test_raw_1x1_kernels_match_fp64_conv2d(backend, wid):
    be = Backend(backend)
    B, H, W, hidden, cx = WIDE[wid]
    K, N, P = hidden + sum(cx), 2 * hidden, B * H * W
    x = synthetic_tensor((B, K, H, W), 41)
    w = synthetic_tensor((N, K, 1, 1), 42, lo=-0.5, hi=0.5)
    g = synthetic_tensor((B, N, H, W), 43)
    add_a, add_b = synthetic_tensor((B, K, H, W), 44), synthetic_tensor((B, K, H, W), 45)
    x64, w64, g64 = x.double().requires_grad_(), w.double().requires_grad_(), g.double()
    y64 = F.conv2d(x64, w64)
    y64.backward(g64)
    xa, wa = x64.detach().abs().requires_grad_(), w64.detach().abs().requires_grad_()
    ya = F.conv2d(xa, wa)                                                # conv(|x|, |w|)
    ya.backward(g64.abs())                                               # xa.grad = conv^T(|g|, |w|), wa.grad = sum |x| |g|

    def packed(mode, Kp, Np):
        n = be.raw("stx_selgru_packed_floats")(Kp, Np)
        assert n > 0
        wp = be.empty(n)
        be.call("stx_selgru_pack_weight", ptr(be.dev(w[:hidden])), ptr(be.dev(w[hidden:])), ptr(wp), hidden, K, mode)
        return wp

    def gemm(srcs, wp, Nout, add0, add1, out):
        be.call("stx_selgru_gemm", *srcs, ptr(wp), Nout, 0, 0, None, None, ptr(add0), Nout if add0 is not None else 0, ptr(add1),
                Nout if add1 is not None else 0, None, 0, None, None, None, 0, ptr(out), None, None, Nout, P)

    # forward: the sources are the channel slices [hidden | x..] of one map (pitch K)
    xd = be.dev(_nhwc(x))
    y = be.empty(B, H, W, N)
    gemm(_slices(xd, (hidden,) + tuple(cx)), packed(0, K, N), N, None, None, y)
    _assert_bound(y.permute(0, 3, 1, 2), y64.detach(), (K + 2) * EPS * ya.detach(), "forward")

    # data gradient: mode-1 weights, the two sources [gz, gr] (pitch 2 hidden), the running gradient as addend, in place
    gd = be.dev(_nhwc(g))
    wp1 = packed(1, N, K)
    buf = be.dev(_nhwc(add_a)).clone()
    gemm(_slices(gd, (hidden, hidden)), wp1, K, buf, None, buf)
    _assert_bound(buf.permute(0, 3, 1, 2), x64.grad + add_a.double(), (N + 3) * EPS * (xa.grad + add_a.double().abs()),
                  "data gradient + addend")
    # ... and with the other cell's buffer as the second addend: (acc + a) + b
    buf2, other = be.dev(_nhwc(add_a)).clone(), be.dev(_nhwc(add_b))
    gemm(_slices(gd, (hidden, hidden)), wp1, K, buf2, other, buf2)
    _assert_bound(buf2.permute(0, 3, 1, 2), x64.grad + add_a.double() + add_b.double(),
                  (N + 4) * EPS * (xa.grad + add_a.double().abs() + add_b.double().abs()), "data gradient + two addends")

    # weight gradient of both maps at once
    nws = be.raw("stx_selgru_wgrad_workspace_floats")(P, K, N)
    assert nws > 0
    ws, dw = be.empty(nws), be.empty(N, K)
    g0, g1 = gd[..., :hidden].contiguous(), gd[..., hidden:].contiguous()
    be.call("stx_selgru_wgrad", *_slices(xd, (hidden,) + tuple(cx)), ptr(g0), ptr(g1), hidden, ptr(dw), ptr(ws), P)
    _assert_bound(dw.view(N, K, 1, 1), w64.grad, (P + 2) * EPS * wa.grad, "weight gradient")


CELL_NAMES = ["h'", "g_att", "g_h"]


@pytest.fixture(scope="module")
def wide_reference():
    """fp64 and fp32 CPU runs (one thread) of the pinned restatement at the real width, computed once per shape."""
    cache = {}

    def get(wid):
        if wid not in cache:
            B, H, W, hidden, cx = WIDE[wid]
            att, h, xs, (g,) = cell_inputs(B, hidden, cx, H, W, seed=51)
            runs = []
            with _one_thread():
                for dtype in (torch.float64, torch.float32):
                    md = _cell_module(hidden_dim=hidden, input_dim=sum(cx)).to(dtype)
                    leaves = [t.clone().to(dtype).requires_grad_() for t in [att, h] + xs]
                    y = cell(leaves[0], leaves[1], leaves[2:], _cell_params(md))
                    (y * g.to(dtype)).sum().backward()
                    runs.append([y.detach()] + [t.grad for t in leaves] + [p.grad for p in _cell_params(md)])
            names = CELL_NAMES + [f"g_x{i}" for i in range(len(xs))] + ["grad/" + n for n in CELL_PARAMS]
            cache[wid] = ((att, h, xs, g), names, runs)
        return cache[wid]
    return get


@pytest.fixture(scope="module")
def csa_big_reference():
    """The same for the GPU-only attention case."""
    cache = []

    def get():
        if not cache:
            runs = []
            with _one_thread():
                for dtype in (torch.float64, torch.float32):
                    cam, sam = (t.to(dtype) for t in _csa_modules(csa_shape(CSA_BIG)[1]))
                    out = run_csa_case(lambda x: csa(x, cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight), _csa_named(cam, sam),
                                       CSA_BIG, dtype)
                    runs.append(out)
            cache.append(runs)
        return cache[0]
    return get


def _live(w32, w64):
    return (w32.double() - w64).abs().max().item()


@pytest.mark.parametrize("backend,wid", on(WIDE_IDS, gpu_only=WIDE_GPU_ONLY))
def test_selective_cell_at_real_width(backend, wid, wide_reference, parity_log):
    env_ = Env(backend)
    dev = env_.device
    (att, h, xs, g), names, (r64, r32) = wide_reference(wid)
    hidden, cx = WIDE[wid][3:]
    m = _cell_module(hidden_dim=hidden, input_dim=sum(cx)).to(dev)
    leaves = [t.clone().to(dev).requires_grad_() for t in [att, h] + xs]      # (clone: .to() of a CPU tensor is the tensor)
    with env_.ctx():
        y = m(leaves[0], leaves[1], *leaves[2:])
        (y * g.to(dev)).sum().backward()
        sync(env_)
    got = [y] + [t.grad for t in leaves] + [p.grad for p in _cell_params(m)]
    for name, a, w64, w32 in zip(names, got, r64, r32):
        what = f"selective[{backend}:{wid}]:{name}"
        within(a, w64, _dref(what, _live(w32, w64)), VALUE_FACTOR if name == "h'" else GRAD_FACTOR, what, parity_log)


@pytest.mark.gpu
def test_attention_at_the_gpu_only_shape(csa_big_reference, parity_log):
    from stereo_toolbox_amd.models.SelectiveStereo import contextual_spatial_attention
    env_ = Env("hip")
    dev = env_.device
    r64, r32 = csa_big_reference()
    cam, sam = (t.to(dev) for t in _csa_modules(csa_shape(CSA_BIG)[1]))

    def step(x):
        (xp,), (att,) = contextual_spatial_attention(cam, sam, [x.to(dev)])
        return xp.cpu(), att.cpu()
    out = run_csa_case(step, _csa_named(cam, sam), CSA_BIG, torch.float32)
    sync(env_)
    for k, v in out.items():
        what = f"csa[hip:{CSA_BIG}]:{k}"
        within(v, r64[k], _dref(what, _live(r32[k], r64[k])), VALUE_FACTOR if k in ("xp", "att") else GRAD_FACTOR, what, parity_log)


def test_the_gpu_only_cases_have_their_recorded_dref(wide_reference, csa_big_reference):
    """The GPU-only cases never run on the host that records the table: their d_ref is looked up (and, recording, written) here."""
    for wid in WIDE_GPU_ONLY:
        _, names, (r64, r32) = wide_reference(wid)
        for name, w64, w32 in zip(names, r64, r32):
            assert _dref(f"selective[hip:{wid}]:{name}", _live(w32, w64)) > 0
    r64, r32 = csa_big_reference()
    for k in r64:
        assert _dref(f"csa[hip:{CSA_BIG}]:{k}", _live(r32[k], r64[k])) > 0


# ------------------------------------------------------------------------------------------ 4. identities, to the bit
def _cell_args(tag, dev):
    att, h, xs, gs = inputs(tag)
    return att.to(dev), h.to(dev), [x.to(dev) for x in xs]


def test_blend_identities(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    att, h, xs = _cell_args("ragged", dev)
    m = _cell_module("ragged").to(dev)
    with env.ctx(), torch.no_grad():
        large = ops.raft_convgru(h, xs, *m.large_gru.weights())
        small = ops.raft_convgru(h, xs, *m.small_gru.weights())
        at0 = m(torch.zeros_like(att), h, *xs)
        at1 = m(torch.ones_like(att), h, *xs)
        mixed = m(att, h, *xs)
        as_convgru = ops.convgru(h, None, None, None, xs, *m.large_gru.weights())
        sync(env)
    assert torch.equal(at0, large) and torch.equal(at1, small)
    assert torch.equal(large, as_convgru)
    assert not torch.equal(mixed, large) and not torch.equal(mixed, small) and not torch.equal(small, large)
    assert mixed.shape == h.shape and mixed.permute(0, 2, 3, 1).is_contiguous()


def test_either_cell_may_be_the_1x1_one(env):  # noqa: F811
    """small 3x3 / large 1x1: the same two cells with att and 1 - att exchanged, formed by the other blend of the 1x1 epilogue."""
    from stereo_toolbox_amd import ops
    dev = env.device
    att, h, xs = _cell_args("two_src", dev)
    m = _cell_module("two_src").to(dev)
    with env.ctx(), torch.no_grad():
        want = ops.selective_convgru(att, h, xs, m.small_gru.weights(), m.large_gru.weights())
        got = ops.selective_convgru(1 - att, h, xs, m.large_gru.weights(), m.small_gru.weights())
        sync(env)
    assert (got - want).abs().max().item() <= 4 * EPS            # (1 - (1 - att) is not att to the bit)


def test_fused_attention_equals_its_two_halves(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    for tag in ("c16", "c48"):
        cam, sam = (t.to(dev) for t in _csa_modules(CSA_CASES[tag][1]))
        x = csa_inputs(tag)[0].to(dev)
        with env.ctx(), torch.no_grad():
            xp, att = ops.csa(x, cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight)
            gate = cam(x)
            halves = gate * x
            att2 = sam(halves)
            sync(env)
        assert gate.shape == (x.shape[0], x.shape[1], 1, 1) and att.shape == (x.shape[0], 1) + tuple(x.shape[2:])
        assert torch.equal(xp, halves) and torch.equal(att, att2)


# ------------------------------------------------------------------------------------------ 5. strides
def test_strided_inputs_are_consumed_in_place(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    att, h, xs = _cell_args("two_src", dev)
    m = _cell_module("two_src").to(dev)
    both = torch.cat(xs, 1).contiguous(memory_format=torch.channels_last)
    split = list(both.split([x.shape[1] for x in xs], 1))
    assert ops._cl_pitch(split[1]) == both.shape[1] and ops._cl_pitch(h) is None
    h_cl = h.contiguous(memory_format=torch.channels_last)
    with env.ctx(), torch.no_grad():
        want = m(att, h, *xs)
        for hh in (h, h_cl):
            assert torch.equal(m(att, hh, *split), want)
        C = CSA_CASES["c16"][1]
        cam, sam = (t.to(dev) for t in _csa_modules(C))
        x = csa_inputs("c16")[0].to(dev)
        wide = torch.cat([x, x.flip(1)], 1).contiguous(memory_format=torch.channels_last)
        half = wide[:, :C]
        assert ops._cl_pitch(half) == 2 * C
        w = (cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight)
        for a, b in zip(ops.csa(half, *w), ops.csa(x, *w)):
            assert torch.equal(a, b)
        sync(env)


# ------------------------------------------------------------------------------------------ 6. custom backward
def _fd_cell_inputs():
    B, H, W, hidden, cx = 1, 3, 5, 16, (8, 4)
    att, h, xs, _ = cell_inputs(B, hidden, cx, H, W, seed=61)
    m = _cell_module(hidden_dim=hidden, input_dim=sum(cx))
    # `directional` steps relative to an input's magnitude: biases of fill_state_dict's size (0.1) would be stepped by 1e-4, and
    # the difference quotient of the fp32 outputs would be rounding noise; they are drawn in (-0.5, 0.5) instead
    ps = [p.detach().clone() if p.dim() > 1 else synthetic_tensor(tuple(p.shape), 69, stream=i, lo=-0.5, hi=0.5)
          for i, p in enumerate(_cell_params(m))]
    return [att, h] + xs + ps


def _apply_cell(dev, ts):
    from stereo_toolbox_amd import ops
    att, h, x0, x1, *ps = [t.to(dev) if t.device != dev else t for t in ts]
    return ops.selective_convgru(att, h, [x0, x1], ps[:6], ps[6:])


def _fd_csa_inputs():
    """x with every maximum far ahead of its runner-up and every MLP pre-activation far from 0 (far: against the step of
    `directional`): channel c peaks at pixel c, every other pixel p has its channel p % C raised, the hidden units of w1 have one
    sign each."""
    B, C, H, W = 1, 16, 4, 5
    x = synthetic_tensor((B, C, H * W), 63, lo=-0.2, hi=0.2)
    for p in range(H * W):
        x[0, p % C, p] = 3.0 if p < C else 1.5
    sign = torch.tensor([1.0, -1.0]).repeat(C // 16 * 8)[:C // 16].view(-1, 1, 1, 1)
    w1 = sign * synthetic_tensor((C // 16, C, 1, 1), 64, lo=0.1, hi=0.15)
    w2 = synthetic_tensor((C, C // 16, 1, 1), 65, lo=-0.5, hi=0.5)
    w_sam = synthetic_tensor((1, 2, CSA_KERNEL, CSA_KERNEL), 66, lo=-0.3, hi=0.3)
    return [x.view(B, C, H, W), w1, w2, w_sam]


def test_backward_matches_finite_differences(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    to = lambda ts: [t.to(dev) if t.device != dev else t for t in ts]   # noqa: E731
    with env.ctx():                                          # (the backward pass runs inside `directional`)
        directional(lambda *ts: _apply_cell(dev, ts).cpu(), _fd_cell_inputs())
        x, w1, w2, w_sam = _fd_csa_inputs()
        directional(lambda *ts: [t.cpu() for t in ops.csa(*to(ts))], [x, w1, w2, w_sam])
        directional(lambda *ts: ops.csa_gate(*to(ts)).cpu(), [x, w1, w2])
        directional(lambda *ts: ops.csa_spatial(*to(ts)).cpu(), [x, w_sam])


def test_skipped_gradients_leave_the_others_unchanged(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    base = _fd_cell_inputs()
    g = synthetic_tensor(tuple(base[1].shape), 62).to(dev)

    def run(wanted, apply, base, g):
        ts = [t.clone().to(dev).requires_grad_(i in wanted) for i, t in enumerate(base)]
        with env.ctx():
            y = apply(ts)
            sum((a * b).sum() for a, b in zip(y if isinstance(y, tuple) else (y,), g)).backward()
            sync(env)
        return [None if t.grad is None else t.grad.cpu() for t in ts]

    def check(apply, base, g, subsets):
        full = run(set(range(len(base))), apply, base, g)
        assert all(t is not None for t in full)
        for wanted in subsets:
            part = run(wanted, apply, base, g)
            for i, (a, b) in enumerate(zip(part, full)):
                assert (a is not None) == (i in wanted), i
                if a is not None:
                    assert torch.equal(a, b), (sorted(wanted), i)
    # no att; att alone; no x source; one x source and the small cell; the large cell's wr alone; no weight
    check(lambda ts: _apply_cell(dev, ts), base, (g,),
          ({1, 2, 3} | set(range(4, 16)), {0}, {0, 1, 4, 5, 10, 11}, {1, 3} | set(range(4, 10)), {12, 13}, {0, 1, 2, 3}))
    xb = _fd_csa_inputs()
    gs = (synthetic_tensor(tuple(xb[0].shape), 67).to(dev), synthetic_tensor((1, 1) + tuple(xb[0].shape[2:]), 68).to(dev))
    check(lambda ts: ops.csa(*ts), xb, gs, ({0}, {1, 2}, {3}, {0, 3}, {2}))


# ------------------------------------------------------------------------------------------ 7. reproducibility
def _two_cell_runs(env_, m, att, h, xs, g):
    dev = env_.device
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        leaves = [t.clone().to(dev).requires_grad_() for t in [att, h] + xs]      # (clone: .to() of a CPU tensor is the tensor)
        with env_.ctx():
            y = m(leaves[0], leaves[1], *leaves[2:])
            (y * g.to(dev)).sum().backward()
            sync(env_)
        runs.append([y.detach().cpu()] + [t.grad.cpu().clone() for t in leaves] + [p.grad.cpu().clone() for p in _cell_params(m)])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i


def _two_csa_runs(env_, tag):
    dev = env_.device
    cam, sam = (t.to(dev) for t in _csa_modules(csa_shape(tag)[1]))
    runs = []
    for _ in range(2):
        cam.zero_grad(set_to_none=True)
        sam.zero_grad(set_to_none=True)
        with env_.ctx():
            out = run_csa_case(lambda x: tuple(t.cpu() for t in _ops().csa(x.to(dev), cam.fc[0].weight, cam.fc[2].weight,
                                                                          sam.samconv.weight)), _csa_named(cam, sam), tag, torch.float32)
            sync(env_)
        runs.append({k: v.clone() for k, v in out.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def _ops():
    from stereo_toolbox_amd import ops
    return ops


def test_two_runs_give_equal_bits(env):  # noqa: F811
    att, h, xs, (g,) = inputs("ragged")
    _two_cell_runs(env, _cell_module("ragged").to(env.device), att, h, xs, g)
    _two_csa_runs(env, "c48")


@pytest.mark.gpu
def test_two_runs_give_equal_bits_at_real_width():
    env_ = Env("hip")
    B, H, W, hidden, cx = WIDE_SHAPES[2]
    att, h, xs, (g,) = cell_inputs(B, hidden, cx, H, W, seed=51)
    _two_cell_runs(env_, _cell_module(hidden_dim=hidden, input_dim=sum(cx)).to(env_.device), att, h, xs, g)
    _two_csa_runs(env_, CSA_BIG)


# ------------------------------------------------------------------------------------------ 8. pack cache, no_grad
def test_training_loop_packs_once(env):  # noqa: F811
    ops = _ops()
    dev = env.device
    m = _cell_module("loop3").to(dev)
    n3, n1 = ops.CONVGRU_PACKS, ops.SELGRU_PACKS
    with env.ctx():
        run_cell_case(lambda att, h, xs: m(att.to(dev), h.to(dev), *[x.to(dev) for x in xs]).cpu(), dict(m.named_parameters()), "loop3",
                      torch.float32)
        sync(env)
    # per cell: zr and q, forward and data gradient -- not 3 x 4
    assert ops.CONVGRU_PACKS - n3 == 4 and ops.SELGRU_PACKS - n1 == 4
    for gru in (m.small_gru, m.large_gru):
        assert len(gru.convz.weight.__dict__["_stx_packed"]) == 2 and len(gru.convq.weight.__dict__["_stx_packed"]) == 2


def test_pack_cache_follows_the_weight_version(env):  # noqa: F811
    dev = env.device
    att, h, xs = _cell_args("one_src", dev)
    m = _cell_module("one_src").to(dev)
    with env.ctx(), torch.no_grad():
        before = m(att, h, *xs).clone()
        m.small_gru.convq.weight.mul_(0.5)                   # an in-place update: the version counter moves
        m.small_gru.convz.weight.add_(0.01)
        after = m(att, h, *xs)
        fresh = _cell_module("one_src").to(dev)
        fresh.load_state_dict(m.state_dict())
        want = fresh(att, h, *xs)
        sync(env)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_no_grad_keeps_neither_cell_state(env):  # noqa: F811
    """Under no_grad the call allocates the gates and ONE state buffer: the large cell's state is blended in place."""
    ops = _ops()
    dev = env.device
    att, h, xs = _cell_args("one_src", dev)
    m = _cell_module("one_src").to(dev)
    made = []
    real = torch.empty

    def counting(*shape, **kw):
        t = real(*shape, **kw)
        made.append(tuple(t.shape))
        return t
    with env.ctx(), torch.no_grad():
        m(att, h, *xs)                                       # (packs the weights)
        sync(env)
        torch.empty = counting
        try:
            out = m(att, h, *xs)
        finally:
            torch.empty = real
        sync(env)
    B, hidden, H, W = h.shape
    assert made.count((B, H, W, hidden)) == 5, made          # z and r h of each cell, one state
    assert out.requires_grad is False and ops._cl_pitch(out) == hidden


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_without_a_device():
    ops = _ops()
    from stereo_toolbox_amd.models.IGEVStereo import ConvGRU
    from stereo_toolbox_amd.models.SelectiveStereo import RaftConvGRU, SelectiveConvGRU
    att, h, xs, _ = inputs("one_src")
    with pytest.raises(ops.StxError):                       # CPU tensors on the product path
        _cell_module("one_src")(att, h, *xs)
    cam, sam = _csa_modules(16)
    x = csa_inputs("c16")[0]
    for call in (lambda: cam(x), lambda: sam(x), lambda: ops.csa(x, cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight)):
        with pytest.raises(ops.StxError):
            call()
    with pytest.raises(ops.StxError):
        RaftConvGRU(16, 16, 3, dilation=2)
    with pytest.raises(ops.StxError):
        RaftConvGRU(16, 16, 5)
    with pytest.raises(ops.StxError):
        SelectiveConvGRU(16, 16, 3, 3)
    with pytest.raises(ops.StxError):                       # the 3x3 cell's own refusal stands
        ConvGRU(16, 16, kernel_size=5)


def test_shape_refusals(env):  # noqa: F811
    ops = _ops()
    dev = env.device

    def cell_call(hidden, cx, H=4, W=6, dtype=torch.float32, ks=(1, 3), att_c=1):
        z = lambda c: torch.zeros(1, c, H, W, device=dev, dtype=dtype)          # noqa: E731
        K = hidden + sum(cx)
        cells = [[torch.zeros(hidden, K, k, k, device=dev, dtype=dtype), torch.zeros(hidden, device=dev, dtype=dtype)] * 3 for k in ks]
        return ops.selective_convgru(z(att_c), z(hidden), [z(c) for c in cx], *cells)

    def csa_call(C, k=7, dtype=torch.float32):
        z = lambda *s: torch.zeros(*s, device=dev, dtype=dtype)          # noqa: E731
        return ops.csa(z(1, C, 4, 6), z(C // 16, C, 1, 1), z(C, C // 16, 1, 1), z(1, 2, k, k))
    with env.ctx():
        assert cell_call(16, (8,)).shape == (1, 16, 4, 6)    # the edges that are served
        assert cell_call(16, (8,), ks=(3, 1)).shape == (1, 16, 4, 6) and cell_call(16, (8,), ks=(1, 1)).shape == (1, 16, 4, 6)
        for kw in (dict(hidden=24, cx=(8,)), dict(hidden=16, cx=(6,)), dict(hidden=16, cx=(4, 4, 4, 4)), dict(hidden=16, cx=()),
                   dict(hidden=128, cx=(256, 132)), dict(hidden=144, cx=(16,)), dict(hidden=16, cx=(8,), dtype=torch.float16),
                   dict(hidden=16, cx=(8,), ks=(3, 3)), dict(hidden=16, cx=(8,), ks=(1, 5)), dict(hidden=16, cx=(8,), att_c=16)):
            with pytest.raises(ops.StxError):
                cell_call(**kw)
        xp, att = csa_call(16)
        assert xp.shape == (1, 16, 4, 6) and att.shape == (1, 1, 4, 6) and csa_call(256, k=1)[1].shape == (1, 1, 4, 6)
        for kw in (dict(C=24), dict(C=272), dict(C=16, k=8), dict(C=16, k=9), dict(C=16, dtype=torch.float16)):
            with pytest.raises(ops.StxError):
                csa_call(**kw)
        with pytest.raises(ops.StxError):                   # the MLP's hidden width is C / 16
            ops.csa_gate(torch.zeros(1, 32, 4, 6, device=dev), torch.zeros(4, 32, 1, 1, device=dev), torch.zeros(32, 4, 1, 1, device=dev))
        lib = ops.get_lib()
        sup = lib.raw("stx_selgru_supported")
        assert sup(128, 2, 256, 128, 0) == 1 and sup(128, 2, 256, 132, 0) == 0 and sup(24, 1, 8, 0, 0) == 0 and sup(16, 1, 6, 0, 0) == 0
        assert lib.raw("stx_convgru_supported")(16, 1, 8, 0, 0, 5) == 0 and lib.raw("stx_convgru_supported")(16, 1, 8, 0, 0, 1) == 0
        assert lib.raw("stx_selgru_packed_floats")(516, 16) == 0 and lib.raw("stx_selgru_wgrad_workspace_floats")(16, 24, 24) == 0
        csup = lib.raw("stx_csa_supported")
        assert csup(16, 7) == 1 and csup(256, 1) == 1 and csup(24, 7) == 0 and csup(16, 8) == 0 and csup(16, 9) == 0 and csup(272, 3) == 0


# ------------------------------------------------------------------------------------------ 10. autocast
def test_autocast_is_the_fp32_path_on_the_cast_up_inputs(env):  # noqa: F811
    dev = env.device
    low = torch.float16 if dev.type == "cuda" else torch.bfloat16
    att, h, xs = _cell_args("one_src", dev)
    args = [t.to(low) for t in [att, h] + xs]
    m = _cell_module("one_src").to(dev)
    cam, sam = (t.to(dev) for t in _csa_modules(16))
    x = csa_inputs("c16")[0].to(dev).to(low)
    w = (cam.fc[0].weight, cam.fc[2].weight, sam.samconv.weight)
    with env.ctx(), torch.no_grad():
        with torch.amp.autocast(dev.type, dtype=low):
            under = [m(*args)] + list(_ops().csa(x, *w))
        plain = [m(*[t.float() for t in args])] + list(_ops().csa(x.float(), *w))
        sync(env)
    for a, b in zip(under, plain):
        assert a.dtype == torch.float32 and torch.equal(a, b)
