"""Instance norm + activation (+ residual tail) on csrc/instnorm.hip: `ops.instance_norm`, and the blocks built on it --
`models.IGEVStereo.BasicConv_IN / Conv2x_IN`, `models.RAFTStereo.ResidualBlock` -- forward and backward.

Every product test runs on the host emulator build (CPU, `-m "not gpu"`) and on gfx950 (`-m gpu`):
  * the op against F.instance_norm + activation (+ add + relu) in fp64 computed here: `parity.within`, 2 x d_ref on the output,
    3 x d_ref on the gradients, d_ref = the same sequence in fp32 on the CPU on one thread, RECORDED in
    tests/golden/instnorm_parity_dref.json (tests/parity.py::RecordedDref; STX_INSTNORM_DREF_RECORD=<path> runs the module with the
    live values and writes them to <path>).  Inputs: x = randn sigma_plane + mu_plane with sigma_plane in [0.5, 2] and mu_plane 0
    ("centred") or 4 randn ("offset": sum x^2 - (sum x)^2 / S cancels).  The fp64 run must keep every element 1e-6 away from the
    kinks (xhat = 0; with a tail skip + act(xhat) = 0): a branch flip would move a gradient by O(1) and say nothing of the kernel;
  * the shapes are the smallest at which the kernel can go wrong, and together they reach every path stx_instnorm_plan returns;
  * the modules against the reference's own fp64 run (tests/golden/instnorm*.npz, written by make_golden_instnorm.py):
    `parity.within_fixture`, 2 x d_ref on outputs, 3 x d_ref on every gradient; state-dict keys, shapes and order equal the
    reference's (tests/golden/state_dict_keys_instnorm.json); the packages that share the class text share the class object;
  * finite differences, skipped gradients, nothing saved under no_grad, reproducibility to the bit, independence of the samples
    of a batch, refusals, fp16 / bf16 inputs and autocast.
"""
import contextlib
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from stereo_toolbox_amd import ops
from stereo_toolbox_amd._capi import StxError
from tests.golden.instnorm_config import KEY_CASES, KEYS, MODULE_CASES, build, load_gold, run_module_case, state_keys
from tests.parity import (GRAD_FACTOR, VALUE_FACTOR, Env, RecordedDref, directional, env, near, on, sync, within,  # noqa: F401
                          within_fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
_dref = RecordedDref(os.path.join(HERE, "golden", "instnorm_parity_dref.json"), "STX_INSTNORM_DREF_RECORD")
KINK_MARGIN = 1e-6
ACTS = ("none", "relu", "lrelu")
# tag: (shape, channels_last, seed).  The seed is one for which the fp64 run keeps KINK_MARGIN in all twelve variants of the case
# (the GPU-only case: _move_off_the_kinks).
OP_CASES = {
    "2x3x5x7": ((2, 3, 5, 7), False, 0),               # S = 35: odd (plane bases off the 16-byte grid), smaller than a wave
    "2x1x1x2": ((2, 1, 1, 2), False, 0),               # S = 2, C = 1
    "2x48x37x53": ((2, 48, 37, 53), False, 10),        # S = 1961: two chunks, the second shorter; C = 48
    "1x2x96x160": ((1, 2, 96, 160), False, 1),         # few planes, large S: many chunks per plane
    "2x5x4x5x6": ((2, 5, 4, 5, 6), False, 0),          # 3-D
    "2x48x37x53_cl": ((2, 48, 37, 53), True, 10),      # channels_last
    "2x3x5x7_cl": ((2, 3, 5, 7), True, 0),
    "1x32x288x480": ((1, 32, 288, 480), False, 0),     # GPU only: IGEV's first stem at 576 x 960
}
OP_GPU_ONLY = ("1x32x288x480",)
OP_VARIANTS = [(act, skip, mu) for act in ACTS for skip in (False, True) for mu in ("centred", "offset")]
PATHS = {0: "one launch", 1: "two launches"}           # what stx_instnorm_plan can return


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


def _classes():
    from stereo_toolbox_amd.models.IGEVStereo import BasicConv_IN, Conv2x_IN
    from stereo_toolbox_amd.models.RAFTStereo import ResidualBlock
    return {"BasicConv_IN": BasicConv_IN, "Conv2x_IN": Conv2x_IN, "ResidualBlock": ResidualBlock}


def _act(t, act):
    return {"none": lambda v: v, "relu": F.relu, "lrelu": F.leaky_relu}[act](t)


def _margin(x, s, act):
    """Distance of the run from the kinks: min |xhat|, and with a tail min |skip + act(xhat)|."""
    xhat = F.instance_norm(x, eps=1e-5)
    return xhat.abs().min().item() if s is None else min(xhat.abs().min().item(), (s + _act(xhat, act)).abs().min().item())


def _move_off_the_kinks(x, s):
    """At 4.4 M elements no seed keeps KINK_MARGIN (about three elements of a draw lie within 1e-6 of xhat = 0): the few
    elements of x, and of skip for any of the activations, that lie within 4 x KINK_MARGIN of a kink are moved by 1 % of a
    standard deviation, until none is left.  The caller still asserts the margin on its own fp64 run."""
    for _ in range(8):
        xhat = F.instance_norm(x.double(), eps=1e-5)
        near_x = xhat.abs() < 4 * KINK_MARGIN
        x[near_x] += 0.01 * x.std()
        if s is None:
            if not near_x.any():
                return
            continue
        near_s = torch.zeros_like(near_x)
        for act in ACTS:
            near_s |= (s.double() + _act(xhat, act)).abs() < 4 * KINK_MARGIN
        s[near_s] += 0.01
        if not near_x.any() and not near_s.any():
            return


@functools.lru_cache(maxsize=4)
def _op_inputs(tag, skip, mu):
    """x, skip, gy of a case (shared by the variants that differ in the activation alone; never written to)."""
    shape, cl, seed = OP_CASES[tag]
    g = torch.Generator().manual_seed(seed * 1000 + 7 * OP_VARIANTS.index(("none", skip, mu)) + len(shape))
    plane = shape[:2] + (1,) * (len(shape) - 2)
    sigma = 0.5 + 1.5 * torch.rand(plane, generator=g)
    offset = 4.0 * torch.randn(plane, generator=g) if mu == "offset" else torch.zeros(plane)
    x = torch.randn(shape, generator=g) * sigma + offset
    s = torch.randn(shape, generator=g) if skip else None
    gy = torch.randn(shape, generator=g)
    if tag in OP_GPU_ONLY:
        _move_off_the_kinks(x, s)
    if cl:
        x, gy = (t.contiguous(memory_format=torch.channels_last) for t in (x, gy))
        s = None if s is None else s.contiguous(memory_format=torch.channels_last)
    return x, s, gy


def _stock(x, s, act):
    """The op sequence of the reference's blocks: F.instance_norm, the activation, and with a skip the add and the ReLU."""
    y = _act(F.instance_norm(x, eps=1e-5), act)
    return y if s is None else F.relu(s + y)


def _stock_run(x, s, gy, act, dtype):
    """(y, gx, gskip) of the stock sequence on the CPU in `dtype`, and the distance of the run from the kinks."""
    x = x.detach().to(dtype).requires_grad_()
    s = None if s is None else s.detach().to(dtype).requires_grad_()
    y = _stock(x, s, act)
    grads = torch.autograd.grad((y * gy.to(dtype)).sum(), [x] + ([] if s is None else [s]))
    with torch.no_grad():
        margin = _margin(x, s, act)
    return (y.detach(), grads[0], grads[1] if s is not None else None), margin


def _product_run(env_, x, s, gy, act):
    dev = env_.device
    xd = x.to(dev).detach().clone().requires_grad_()
    sd = None if s is None else s.to(dev).detach().clone().requires_grad_()
    with env_.ctx():
        y = ops.instance_norm(xd, act, skip=sd)
        grads = torch.autograd.grad(y, [xd] + ([] if sd is None else [sd]), gy.to(dev))
        sync(env_)
    return y.detach(), grads[0], grads[1] if sd is not None else None


def _plan(env_, shape):
    with env_.ctx():
        return ops.instance_norm_plan(shape[0] * shape[1], int(torch.Size(shape[2:]).numel()))


# ------------------------------------------------------------------------------------------ 1. the op vs fp64
@pytest.mark.parametrize("backend,tag", on(list(OP_CASES), gpu_only=OP_GPU_ONLY))
def test_op_matches_fp64(backend, tag, parity_log):
    env_ = Env(backend)
    shape, cl, _ = OP_CASES[tag]
    for act, skip, mu in OP_VARIANTS:
        x, s, gy = _op_inputs(tag, skip, mu)
        want, margin = _stock_run(x, s, gy, act, torch.float64)
        assert margin >= KINK_MARGIN, f"{tag} {act} skip={skip} {mu}: an element {margin:.1e} from a kink in fp64: another seed"
        with _one_thread():
            ref32, _ = _stock_run(x, s, gy, act, torch.float32)
        got = _product_run(env_, x, s, gy, act)
        assert got[0].dtype == torch.float32 and got[0].shape == x.shape
        if cl:
            assert all(t is None or t.is_contiguous(memory_format=torch.channels_last) for t in got[:1]), "layout of the output"
        for name, factor, g, w, r in zip(("y", "gx", "gskip"), (VALUE_FACTOR, GRAD_FACTOR, GRAD_FACTOR), got, want, ref32):
            if w is None:
                assert g is None
                continue
            what = f"instnorm {tag} {act}{'+skip' if skip else ''} {mu} [{backend}:{name}]"
            live = (r.double() - w).abs().max().item()
            within(g, w, _dref(what, live), factor, what, parity_log)


def test_listed_shapes_reach_every_path(env):
    seen = {}
    for tag, (shape, _, _) in OP_CASES.items():
        if tag in OP_GPU_ONLY and env.name != "hip":
            continue
        chunks, path = _plan(env, shape)
        assert path in PATHS and chunks >= 1 and (chunks == 1) == (path == 0), (tag, chunks, path)
        seen.setdefault(path, []).append(tag)
    assert sorted(seen) == sorted(PATHS), seen
    assert _plan(env, (1, 2, 96, 160))[0] > 1, "few planes of a large S must be split over workgroups"
    assert _plan(env, (2, 48, 37, 53)) == (2, 1), "S = 1961 is two chunks, the second shorter"


# ------------------------------------------------------------------------------------------ 2. modules
def test_state_dict_matches_reference():
    want = json.load(open(KEYS))
    classes = _classes()
    assert sorted(want) == sorted(KEY_CASES)
    for name in KEY_CASES:
        assert state_keys(build(classes, name, KEY_CASES)) == want[name], name
    block = build(classes, "res_s2")
    assert [n for n, _ in block.named_children()] == ["conv1", "conv2", "relu", "norm1", "norm2", "norm3", "downsample"]
    assert block.downsample[1] is block.norm3 and build(classes, "res_s1").downsample is None
    assert [n for n, _ in build(classes, "basic2d").named_children()] == ["conv", "IN"]


def test_sub_packages_export_the_same_objects():
    from stereo_toolbox_amd.models import DEFOMStereo, FoundationStereo, IGEVStereo, MonSter, RAFTStereo, StereoAnywhere
    from stereo_toolbox_amd.models.SelectiveStereo import SelectiveIGEV, SelectiveRAFT
    for pkg in (DEFOMStereo, IGEVStereo, MonSter, StereoAnywhere, SelectiveIGEV, SelectiveRAFT):
        assert pkg.ResidualBlock is RAFTStereo.ResidualBlock, pkg.__name__
    for pkg in (FoundationStereo, MonSter, SelectiveIGEV, SelectiveRAFT):
        assert pkg.BasicConv_IN is IGEVStereo.BasicConv_IN, pkg.__name__
    for pkg in (MonSter, SelectiveIGEV, SelectiveRAFT):
        assert pkg.Conv2x_IN is IGEVStereo.Conv2x_IN, pkg.__name__
    # FoundationStereo's Conv2x_IN and ResidualBlock are other classes in the reference: not served by these
    assert not hasattr(FoundationStereo, "Conv2x_IN") and not hasattr(FoundationStereo, "ResidualBlock")


@pytest.mark.parametrize("backend,tag", on(list(MODULE_CASES)))
def test_module_matches_reference_fp64(backend, tag, gold, parity_log):
    env_ = Env(backend)
    m = build(_classes(), tag)
    with env_.ctx():
        out = run_module_case(m, tag, torch.float32, env_.device)
        sync(env_)
    assert sorted(f"{tag}/{k}:f64" for k in out) == sorted(k for k in gold if k.startswith(tag + "/") and k.endswith(":f64"))
    for k, v in out.items():
        within_fixture(v, gold, f"{tag}/{k}", VALUE_FACTOR if k == "out" else GRAD_FACTOR, f"instnorm module {tag} {k} [{backend}]",
                       parity_log)


@pytest.mark.parametrize("norm_fn", ["group", "batch", "none"])
def test_residual_block_other_norms_follow_the_stock_modules(norm_fn):
    """Without instance norm the block is the reference's sequence on stock modules: restated here from its parts."""
    m = build(_classes(), "res", {"res": ("ResidualBlock", (8, 16), dict(norm_fn=norm_fn, stride=2))}).train()
    x = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(3))
    y = F.relu(m.norm1(m.conv1(x)))
    y = F.relu(m.norm2(m.conv2(y)))
    want = F.relu(m.norm3(m.downsample[0](x)) + y)
    assert torch.equal(m(x), want)


# ------------------------------------------------------------------------------------------ 3. derivative, bookkeeping
@pytest.mark.parametrize("act", ACTS)
def test_finite_differences(env, act):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 3, 6, 5, generator=g) * 1.5 + 2.0
    s = torch.randn(1, 3, 6, 5, generator=g)
    dev = env.device
    with env.ctx():
        directional(lambda a: ops.instance_norm(a.to(dev), act).cpu(), [x])
        directional(lambda a, b: ops.instance_norm(a.to(dev), act, skip=b.to(dev)).cpu(), [x, s])


def test_skipped_gradients_and_no_grad(env):
    x, s, gy = (t.to(env.device) for t in _op_inputs("2x3x5x7", True, "offset"))
    with env.ctx():
        full = _product_run(env, x, s, gy, "lrelu")
        xr = x.clone().requires_grad_()
        y = ops.instance_norm(xr, "lrelu", skip=s)                        # x only
        assert torch.equal(torch.autograd.grad(y, xr, gy)[0], full[1])
        sr = s.clone().requires_grad_()
        y = ops.instance_norm(x, "lrelu", skip=sr)                        # skip only
        assert torch.equal(torch.autograd.grad(y, sr, gy)[0], full[2])
        assert torch.equal(y.detach(), full[0])
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
            with torch.no_grad():
                y = ops.instance_norm(xr, "lrelu", skip=sr)
            assert not saved and not y.requires_grad and y.grad_fn is None
            y = ops.instance_norm(xr, "lrelu", skip=sr)
        # x, skip and the per-plane statistics; never the output
        assert len(saved) == 3 and sorted(tuple(t.shape) for t in saved) == sorted([tuple(x.shape), tuple(s.shape), (6, 2)])
        assert all(t.data_ptr() != y.data_ptr() for t in saved)
        sync(env)


@pytest.mark.parametrize("tag", ["2x3x5x7", "2x48x37x53"])
def test_bitwise_reproducible_and_samples_independent(env, tag):
    x, s, gy = _op_inputs(tag, True, "offset")
    a = _product_run(env, x, s, gy, "relu")
    b = _product_run(env, x, s, gy, "relu")
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    x2, s2, gy2 = x.clone(), s.clone(), gy.clone()
    x2[1], s2[1], gy2[1] = x[1] * 1.5 + 0.25, s[1] - 1.0, gy[1] * 2.0
    c = _product_run(env, x2, s2, gy2, "relu")
    assert all(torch.equal(p[0], q[0]) for p, q in zip(a, c)), "sample 0 must not see sample 1"
    assert not torch.equal(a[0][1], c[0][1])


def test_refusals(env):
    dev = env.device
    x = torch.randn(2, 3, 4, 5).to(dev)
    with env.ctx():
        for bad, kw in ((torch.randn(2, 3, 1, 1), {}), (torch.randn(2, 3, 1, 1, 1), {}),          # S = 1
                        (torch.randn(2, 3, 8), {}), (torch.randn(1, 2, 2, 2, 2, 2), {}),          # dimension
                        (x, dict(skip=torch.randn(2, 3, 4, 4).to(dev))),                           # skip: shape
                        (x, dict(skip=torch.randn(2, 3, 4, 5).to(dev).double())),                  # skip: dtype
                        (x, dict(act="mish")), (x.double(), {}), (x.long(), {})):
            with pytest.raises(StxError):
                ops.instance_norm(bad.to(dev) if isinstance(bad, torch.Tensor) else bad, **kw)
        if env.name == "hip":
            with pytest.raises(StxError):
                ops.instance_norm(x, skip=torch.randn(2, 3, 4, 5))                                 # skip: device
            with pytest.raises(StxError):
                ops.instance_norm(x.cpu())                                                         # no CPU fallback
        big = torch.zeros(1).to(dev).expand(1, 1, 1 << 16, 1 << 15)                                # 2^31 elements per plane, no memory
        with pytest.raises(StxError):
            ops.instance_norm(big)


@pytest.mark.parametrize("dtype,rel", [(torch.float16, 2.0 ** -10), (torch.bfloat16, 2.0 ** -7)])
def test_low_precision_inputs(env, dtype, rel):
    """One rounding in the input's dtype (half an ulp: 2^-11 / 2^-8 relative), doubled."""
    dev = env.device
    x, s, _ = _op_inputs("2x3x5x7", True, "centred")
    x, s = x.to(dtype), s.to(dtype)
    want = _stock(x.double(), s.double(), "lrelu")
    with env.ctx():
        y = ops.instance_norm(x.to(dev), "lrelu", skip=s.to(dev))
        assert y.dtype == dtype
        near(y, want, rel, f"instance_norm {dtype}")
        xr = x.to(dev).requires_grad_()
        ops.instance_norm(xr, "relu").sum().backward()
        assert xr.grad.dtype == dtype
        m = build(_classes(), "basic2d").to(dev)
        xin = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(5)).to(dev)
        with torch.autocast(dev.type, dtype=dtype):
            conv = m.conv(xin)
            out = m(xin)
        assert conv.dtype == dtype and out.dtype == dtype
        near(out, _stock(conv.double().cpu(), None, "lrelu"), rel, f"BasicConv_IN under autocast {dtype}")
        sync(env)
