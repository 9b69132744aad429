"""What the product tests share: the two backends of a product-path test (`Env`, `env`, `on`, `sync`), the acceptance rule
against a reference (`within`, `near`), the rule that pins a plain-torch restatement to a reference fixture (`pin`,
`pin_subsample`) and the finite-difference check of a custom backward (`directional`).  Each is stated here once.

This is neither a test module nor a conftest.py, so pytest does not rewrite its assertions: every assert carries its numbers.
"""
import contextlib

import pytest
import torch

from stereo_toolbox_amd.utils import fill_state_dict

VALUE_FACTOR = 2.0
GRAD_FACTOR = 3.0     # product-vs-fp64 may be at most this many times the fp32 reference's own distance from fp64
EPS = 2.0 ** -24
LOSS_W = (0.5, 0.5, 0.7, 1.0)


# ------------------------------------------------------------------------------------------ backends
class Env:
    def __init__(self, name):
        self.name = name
        if name == "hip":
            if not torch.cuda.is_available():
                pytest.skip("no ROCm device")
            self.device = torch.device("cuda:0")
        else:
            self.device = torch.device("cpu")

    def ctx(self):
        if self.name == "emu":
            from tests.emu_util import emu_product_path
            return emu_product_path()
        return contextlib.nullcontext()


@pytest.fixture(params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def env(request):
    return Env(request.param)


def on(tags, gpu_only=()):
    """(backend, tag): every case on the GPU, on the emulator all but the gpu-only ones."""
    return [("emu", t) for t in tags if t not in gpu_only] + [pytest.param("hip", t, marks=pytest.mark.gpu) for t in tags]


def sync(env):
    if env.name == "hip":
        torch.cuda.synchronize()


def filled(ctor, *a, **k):
    m = ctor(*a, **k)
    sd = m.state_dict()
    fill_state_dict(sd)
    m.load_state_dict(sd)
    return m, {k_: v.clone() for k_, v in sd.items()}


# ------------------------------------------------------------------------------------------ product vs reference
def _floor(want64):
    """The tolerance where the reference's fp32 and fp64 runs agree to the bit (d_ref = 0)."""
    return 2e-7 * max(1.0, want64.abs().max().item())


def within(got, want64, dref, factor, what, log=None):
    """|got - want64| <= factor * d_ref over the whole tensor, d_ref = max|fp32 - fp64| of the REFERENCE (floor
    2e-7 * max(1, max|want|) where d_ref is zero).  The achieved ratio is printed and, with `log`, goes to the parity report."""
    got, want = got.detach().cpu().double(), want64.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    tol = factor * dref if dref > 0 else _floor(want)
    ratio = err / dref if dref else float("nan")
    print(f"{what}: err {err:.3e}  d_ref {dref:.3e}  ratio {ratio:.2f}")
    if log is not None:
        log(what, err=err, d_ref=dref, ratio=ratio, allowed=factor)
    assert err <= tol, (what, err, dref)


def within_fixture(got, gold, key, factor, what, log=None):
    """`within` against the tensor a fixture stores as `key:f64` / `key:dref`."""
    within(got, torch.from_numpy(gold[key + ":f64"]), float(gold[key + ":dref"]), factor, what, log)


def near(got, want, rel, what):
    """|got - want| <= rel * max(1, max|want|): a rounding-model bound where no reference run exists."""
    want = want.detach().cpu().double()
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    assert err <= rel * max(1.0, want.abs().max().item()), (what, err)


# ------------------------------------------------------------------------------------------ restatement vs fixture
def pin(r64, r32, want64, want32, dref, what, peak=None, zero_dref=None):
    """The restatement in fp64 within 1e-11 * max(1, max|want64|) of the reference's fp64 tensor, in fp32 within 2 x d_ref of its
    fp32 tensor (two fp32 evaluations of one quantity).  Either pair may be None (a test parametrised over the dtype).
    `peak`: the max|fp64| a fixture stores next to the tensor; it then sets the fp64 tolerance and max|r64| must meet it.
    `zero_dref`: None -- d_ref > 0 is asserted; "exact" -- 2 x 0: the fp32 tensors must be equal; "floor" -- the floor of `within`."""
    assert zero_dref in (None, "exact", "floor"), zero_dref
    assert dref > 0 or zero_dref is not None, (what, dref)
    if r64 is not None:
        r64 = r64.detach()
        assert r64.dtype == want64.dtype == torch.float64 and r64.shape == want64.shape, (what, r64.dtype, r64.shape, want64.shape)
        tol = 1e-11 * max(1.0, want64.abs().max().item() if peak is None else peak)
        if peak is not None:
            top = r64.abs().max().item()
            assert abs(top - peak) <= tol, (what, "max|fp64|", top, peak)
        err = (r64 - want64).abs().max().item()
        assert err <= tol, (what, "fp64", err, tol)
    if r32 is not None:
        r32 = r32.detach()
        assert r32.dtype == want32.dtype == torch.float32 and r32.shape == want32.shape, (what, r32.dtype, r32.shape, want32.shape)
        tol = 2 * dref if dref > 0 or zero_dref == "exact" else _floor(want64)
        err = (r32 - want32).abs().max().item()
        assert err <= tol, (what, "fp32", err, dref)


def pin_fixture(r64, r32, gold, key, **kw):
    """`pin` against the tensors a fixture stores as `key:f64` / `key:f32` / `key:dref`."""
    pin(r64, r32, torch.from_numpy(gold[key + ":f64"]), torch.from_numpy(gold[key + ":f32"]), float(gold[key + ":dref"]), key, **kw)


def pin_subsample(r64, want_sub, peak, subsample, min_count, what):
    """Where a fixture keeps max|fp64| and a strided subsample of the fp64 tensor: both within 1e-11 * max(1, peak), and the
    subsample holds at least `min_count` elements."""
    r64 = r64.detach()
    got = subsample(r64)
    assert got.shape == want_sub.shape and want_sub.numel() >= min_count, (what, got.shape, want_sub.shape, min_count)
    tol = 1e-11 * max(1.0, peak)
    top = r64.abs().max().item()
    assert abs(top - peak) <= tol, (what, "max|fp64|", top, peak)
    err = (got - want_sub).abs().max().item()
    assert err <= tol, (what, "subsample", err, tol)


# ------------------------------------------------------------------------------------------ finite differences
def directional(fn, inputs, eps=3e-3, tol=3e-2, seed=0):
    """fn(*inputs) -> tensor (or list of tensors).  Checks <grad_i, v_i> against the central difference for every input."""
    g = torch.Generator().manual_seed(seed)

    def flat(y):
        return torch.cat([t.reshape(-1) for t in y]) if isinstance(y, (list, tuple)) else y.reshape(-1)

    xs = [t.clone().requires_grad_() for t in inputs]
    y = flat(fn(*xs))
    gy = torch.randn(y.shape, generator=g)
    (y * gy).sum().backward()
    for i, x in enumerate(xs):
        v = torch.randn(x.shape, generator=g)
        v *= float(x.detach().abs().mean()) / (v.norm() / (x.numel() ** 0.5))     # step relative to the input's magnitude
        with torch.no_grad():
            args_p = [t.detach() + (eps * v if j == i else 0) for j, t in enumerate(inputs)]
            args_m = [t.detach() - (eps * v if j == i else 0) for j, t in enumerate(inputs)]
            fd = ((flat(fn(*args_p)).double() - flat(fn(*args_m)).double()) * gy.double()).sum().item() / (2 * eps)
        an = (x.grad.double() * v.double()).sum().item()
        scale = max(abs(an), abs(fd), 1e-3 * (x.grad.norm().item() * v.norm().item()))
        assert abs(an - fd) <= tol * scale, f"input {i}: analytic {an:.6e} vs finite difference {fd:.6e}"
