"""The rules of tests/parity.py on literal tensors: each accepts at its bound and refuses just past it."""
import pytest
import torch

from tests.parity import directional, pin, pin_subsample, within

WANT = torch.tensor([1.0, -4.0, 2.0], dtype=torch.float64)
DREF = 2.0 ** -20                              # errors below are multiples of it at a power-of-two entry: exact in fp64


def _off(by, dtype=torch.float64):
    return (WANT + torch.tensor([0.0, by, 0.0], dtype=torch.float64)).to(dtype)


def test_within_holds_factor_times_dref():
    within(_off(3 * DREF), WANT, DREF, 3.0, "at the bound")
    with pytest.raises(AssertionError, match="past the bound"):
        within(_off(3.5 * DREF), WANT, DREF, 3.0, "past the bound")
    with pytest.raises(AssertionError, match="shape"):
        within(WANT[:2], WANT, DREF, 3.0, "shape")


def test_within_falls_back_on_the_floor_where_dref_is_zero():
    within(_off(1.9e-7 * 4.0), WANT, 0.0, 2.0, "under the floor")        # max|want| = 4
    with pytest.raises(AssertionError, match="past the floor"):
        within(_off(2.5e-7 * 4.0), WANT, 0.0, 2.0, "past the floor")


def test_within_reports_to_the_log():
    seen = []
    within(_off(DREF), WANT, DREF, 2.0, "logged", lambda what, **fields: seen.append((what, fields)))
    assert seen == [("logged", {"err": DREF, "d_ref": DREF, "ratio": 1.0, "allowed": 2.0})]


def test_pin_holds_1e11_in_fp64_and_two_dref_in_fp32():
    w32 = WANT.float()
    pin(_off(3e-11), _off(2 * DREF, torch.float32), WANT, w32, DREF, "inside the bounds")          # 1e-11 * max|want| = 4e-11
    with pytest.raises(AssertionError, match="fp64"):
        pin(WANT * (1 + 1e-10), w32, WANT, w32, DREF, "relative 1e-10")
    with pytest.raises(AssertionError, match="fp32"):
        pin(WANT, _off(3 * DREF, torch.float32), WANT, w32, DREF, "3 x d_ref")
    with pytest.raises(AssertionError, match="no distance"):
        pin(WANT, w32, WANT, w32, 0.0, "no distance")
    pin(WANT, w32, WANT, w32, 0.0, "equal bits", zero_dref="exact")
    with pytest.raises(AssertionError, match="fp32"):
        pin(WANT, _off(2.0 ** -21, torch.float32), WANT, w32, 0.0, "one bit", zero_dref="exact")


def test_pin_subsample_holds_count_and_peak():
    every_other = lambda t: t.reshape(-1)[::2]  # noqa: E731
    sub = every_other(WANT)
    pin_subsample(WANT, sub, 4.0, every_other, 2, "as stored")
    with pytest.raises(AssertionError, match="short"):
        pin_subsample(WANT, sub, 4.0, every_other, 3, "short")
    with pytest.raises(AssertionError, match="peak"):
        pin_subsample(WANT, sub, 4.0 + 1e-9, every_other, 2, "peak")
    with pytest.raises(AssertionError, match="subsample"):
        pin_subsample(WANT, sub * (1 + 1e-10), 4.0, every_other, 2, "values")


class _Twice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return (x * x).sum().reshape(1)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return 2 * (2 * x * g)


def test_directional_tells_a_doubled_gradient():
    x = torch.linspace(-1.0, 2.0, 7)
    directional(lambda t: (t * t).sum().reshape(1), [x])
    with pytest.raises(AssertionError, match="input 0"):
        directional(_Twice.apply, [x])
