"""What the product tests share: the two backends of a product-path test (`Env`, `env`, `on`, `sync`), the acceptance rule
against a reference (`within`, `near`), the rule that pins a plain-torch restatement to a reference fixture (`pin`,
`pin_subsample`), the finite-difference check of a custom backward (`directional`) and, for the kernel-level parity modules, the
recorded d_ref (`RecordedDref`) and the tensor-by-tensor verdict of a test (`Verdict`, `PastTheFactor`).  Each is stated here once.

This is neither a test module nor a conftest.py, so pytest does not rewrite its assertions: every assert carries its numbers.
"""
import atexit
import contextlib
import functools
import json
import os
import re

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


def within_inf(got, want64, dref, factor, what, log=None, rule=None):
    """`within` over the finite entries; the -inf entries of want64 compared by equality.  `rule`: another form of the rule with
    the arguments (got, want64, dref, factor, what), such as Verdict.within."""
    inf = torch.isinf(want64)
    assert torch.equal(got.detach().cpu() == float("-inf"), inf), what
    got, want64 = got.detach().cpu().masked_fill(inf, 0.0), want64.masked_fill(inf, 0.0)
    if rule is None:
        within(got, want64, dref, factor, what, log)
    else:
        rule(got, want64, dref, factor, what)


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


# ------------------------------------------------------------------------------------------ recorded d_ref, verdict of a test
# d_ref of a kernel-level parity module is RECORDED from the fp32 CPU torch run on one thread (a json under tests/golden, keyed by
# the parity-report name without the backend).  Recomputed on the spot it is not one number: the CPU convolution picks its blocking
# by instruction set and thread count, and the same d_ref came out 0.42-3.4 x as large on another host (2 x between 4 and 16 threads
# of one host) -- with a factor of 2 or 3 the verdict would follow the host CPU, not the kernel.  want64 is always computed live.
# The live value still guards the record: it must lie within DREF_DRIFT of the entry, a bound that judges the fixture, never a
# kernel -- over twice the widest drift seen between hosts, while a slipped exponent, an entry of another tensor (values against
# gradients, sums against outputs) or a table left over from other shapes is off by an order of magnitude.
DREF_DRIFT = 8.0
RATIO_STEP = 0.005 * (1 + 1e-6)                       # the ratios of a table of listed tensors are written to two decimals


class RecordedDref:
    """`lookup(what, live)` -> the recorded d_ref of `what` from the table at `path`, the live value held within DREF_DRIFT of
    it.  With the environment variable `record_var` set to a path, the module runs with the live values and writes them there
    when the interpreter exits (a new or changed case)."""

    def __init__(self, path, record_var):
        self.path, self.record, self.recorded = path, os.environ.get(record_var), {}
        if self.record:
            atexit.register(lambda: json.dump(self.recorded, open(self.record, "w"), indent=0, sort_keys=True))

    @functools.lru_cache(maxsize=None)
    def table(self):
        with open(self.path) as f:
            return json.load(f)

    def __call__(self, what, live):
        key = re.sub(r"\[(emu|hip):", "[", what)
        if self.record:
            assert self.recorded.setdefault(key, live) == live, key
            return live
        rec = self.table()[key]
        assert rec / DREF_DRIFT <= live <= rec * DREF_DRIFT, f"{key}: d_ref recorded {rec:.3e}, on this host {live:.3e}: a stale entry?"
        return rec


class PastTheFactor(AssertionError):
    """Exactly the tensors the module's table lists for the test are past the factor, each at its recorded ratio -- and nothing
    else: a NaN, a touched guard band, any other tensor past the factor or a listed one elsewhere is a plain AssertionError."""


class Verdict:
    """`within` for every tensor of a test; each goes to the parity report.  `listed` = {tensor: ratio}: the tensors of this test
    the rule is known to refuse (the module's table, `table` names it in the messages).  A tensor is named by the suffix of `what`
    behind the last colon when that is one of `tensors`, else it is "out".  Every other tensor goes through `within` as it is, and
    a failure there fails the test.  A listed tensor must be finite, must be refused by `within`, and must sit at its recorded
    ratio to the two decimals written down (the kernels are deterministic, d_ref is recorded): a kernel that starts to pass has
    to leave the table, one that moves -- a lower-precision product path sits at 7-25 x -- fails the test."""

    def __init__(self, log, listed, dref=None, tensors=("sum", "sumsq", "dz", "dw"), table="SUMMATION_ORDER",
                 why="for the order of the additions alone"):
        self.log, self.listed, self.seen, self.dref, self.tensors, self.table, self.why = log, listed, [], dref, tensors, table, why

    def within(self, got, want64, dref, factor, what):
        dref = self.dref(what, dref)
        tensor = what.rsplit(":", 1)[-1]
        tensor = tensor if tensor in self.tensors else "out"
        # (a recorded d_ref of zero -- the reference's fp32 and fp64 runs agree to the bit -- leaves `within` its floor; no listing there)
        assert got.shape == want64.shape and (dref > 0 or dref == 0 and tensor not in self.listed), (what, got.shape, want64.shape, dref)
        bad = int((~torch.isfinite(got)).sum())
        assert bad == 0, f"{what}: {bad} of {got.numel()} values are not finite (a read past a NaN band, or an unwritten value)"
        if tensor not in self.listed:
            within(got, want64, dref, factor, what, self.log)
            return
        try:
            within(got, want64, dref, factor, what, self.log)
        except AssertionError as e:
            ratio = e.args[0][1] / dref
        else:
            raise AssertionError(f"{what}: inside {factor} x d_ref now; take `{tensor}` out of {self.table}")
        assert abs(ratio - self.listed[tensor]) <= RATIO_STEP, \
            f"{what}: {ratio:.3f} x d_ref, {self.table} records {self.listed[tensor]:.2f} {self.why}"
        self.seen.append(tensor)

    def done(self):
        assert sorted(self.seen) == sorted(self.listed), (self.seen, self.listed)
        if self.listed:
            raise PastTheFactor(", ".join(f"{t} {r:.2f}" for t, r in self.listed.items()))


def listed_verdict(request, log, reason, prefix, **kw):
    """The Verdict of a test whose row in the module's table is `reason` = "tensor ratio, tensor ratio" (None: nothing listed);
    a listed test is marked as a strict expected failure that only PastTheFactor satisfies."""
    if reason is None:
        return Verdict(log, {}, **kw)
    request.applymarker(pytest.mark.xfail(strict=True, raises=PastTheFactor, reason=prefix + reason))
    return Verdict(log, {t: float(r) for t, r in (tr.split() for tr in reason.split(", "))}, **kw)


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
