"""Convex upsampling from logits (RAFT layout: `upsample_flow` / `convex_upflow` / `upsample_disp`; pixel layout: IGEV's
`F.softmax(spx_pred, 1)` + `context_upsample`) and the trainer's sequence loss on the kernels of csrc/convex_upsample.hip.

* tests/golden/convex_upsample.npz, convex_upsample_pixel.npz and sequence_loss.npz hold what the reference's OWN code gives on the
  seeded cases of tests/golden/convex_upsample_config.py, in fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64|
  (tests/golden/make_golden_convex_upsample.py says which functions were run).
* A plain-torch restatement in gather form (no unfold) lives in this file and is pinned to the fixture on the CPU first -- in fp64 to
  1e-11 * max(1, max|want|), in fp32 to 2 x d_ref (two fp32 evaluations of one quantity) -- so the fixture and the restatement check
  each other.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture, every element of every tensor: values
  within VALUE_FACTOR (2) x d_ref, gradients within GRAD_FACTOR (3) x d_ref; where d_ref is zero the floor 2e-7 * max(1, max|want|)
  applies (tests/parity.within, which prints the achieved ratio).
* Where no fixture exists (sequence loss at K = 1, 2, 33; the all-invalid map) the reference is losses.masked_smooth_l1_multi on the
  CPU in fp64, d_ref its own fp32 run's distance from that, the same factors.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.backends import be, ptr  # noqa: F401
from tests.golden.convex_upsample_config import (CASES, LOSS_GAMMA, LOSS_KS, LOSS_MAXDISP, LOSS_PREDICTIONS, LOSS_SHAPE, PIXEL_CASES,
                                                 PIXEL_SCALE, inputs, loss_inputs, pixel_inputs, trainer_weights)
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, env, pin, sync, within, within_fixture  # noqa: F401
from tests.restated import convex, upsample

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    store = {}
    for name in ("convex_upsample.npz", "convex_upsample_pixel.npz", "sequence_loss.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as z:
            store.update({k: z[k] for k in z.files})
    return store


# ------------------------------------------------------------------------------------------ the restatement (plain torch)
def trainer_loss(init_disp, disp_preds, gt, maxdisp, loss_gamma=LOSS_GAMMA):
    """trainer/trainer_torchrun.py:272-284 (the test of losses.sequence_loss compares with the fixture of the trainer's own run)"""
    mask = (gt > 0) * (gt < maxdisp - 1)
    n = len(disp_preds)
    loss = torch.nn.functional.smooth_l1_loss(init_disp.squeeze(1)[mask], gt[mask], reduction="mean")
    adjusted = loss_gamma ** (15 / (n - 1))
    for i in range(n):
        loss = loss + adjusted ** (n - i - 1) * torch.nn.functional.smooth_l1_loss(disp_preds[i].squeeze(1)[mask], gt[mask], reduction="mean")
    return loss


def _pinned(gold, tag, res, dtype):
    """One dtype per test; a d_ref of zero (an output both reference runs give to the bit) falls back on the floor of `within`."""
    for k, v in res.items():
        want64, want32 = torch.from_numpy(gold[f"{tag}:{k}:f64"]), torch.from_numpy(gold[f"{tag}:{k}:f32"])
        r64, r32 = (v, None) if dtype == torch.float64 else (None, v)
        pin(r64, r32, want64, want32, float(gold[f"{tag}:{k}:dref"]), f"{tag}:{k}", zero_dref="floor")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_matches_reference_fixture(gold, tag, dtype):
    N, D, H, W, n, use_scale, _ = CASES[tag]
    flow, mask, gw = inputs(tag)
    flow, mask = flow.to(dtype).requires_grad_(), mask.to(dtype).requires_grad_()
    out = convex(flow, mask, 2 ** n, float(2 ** n) if use_scale else 1.0)
    (out * gw.to(dtype)).sum().backward()
    _pinned(gold, tag, {"out": out, "g_flow": flow.grad, "g_mask": mask.grad}, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tag", list(PIXEL_CASES))
def test_pixel_restatement_matches_reference_fixture(gold, tag, dtype):
    disp, logits, gw = pixel_inputs(tag)
    disp, logits = disp.to(dtype).requires_grad_(), logits.to(dtype).requires_grad_()
    out = upsample(disp * PIXEL_SCALE, torch.softmax(logits, 1))
    (out * gw.to(dtype)).sum().backward()
    _pinned(gold, tag, {"out": out, "g_disp": disp.grad, "g_logits": logits.grad}, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_loss_restatement_matches_trainer_fixture(gold, dtype):
    gt, preds = loss_inputs()
    leaves = [p.to(dtype).clone().requires_grad_() for p in preds]
    loss = trainer_loss(leaves[0], leaves[1:], gt.to(dtype), LOSS_MAXDISP)
    loss.backward()
    _pinned(gold, "trainer", {"loss": loss, "grads": torch.stack([p.grad for p in leaves])}, dtype)


def test_case_table_covers_the_shapes_the_kernel_branches_on():
    fs = {2 ** c[4] for c in CASES.values()}
    assert fs == {2, 4, 8} and {c[1] for c in CASES.values()} >= {1, 2, 3} and any(c[0] == 2 for c in CASES.values())
    assert any(c[2] == 1 for c in CASES.values()) and any(c[3] == 1 for c in CASES.values()) and any(not c[5] for c in CASES.values())
    assert sum(1 for c in CASES.values() if c[2] * c[3] > 64 and (c[2] * c[3]) % 64) >= 3
    _, mask, _ = inputs("large_2x35_n2")
    assert mask.abs().max().item() > 89 and not torch.isfinite(torch.exp(mask)).all()           # a naive exp overflows
    _, mask, _ = inputs("const_3x5_n2")
    assert torch.equal(mask.view(1, 9, -1)[:, 0], mask.view(1, 9, -1)[:, 8])
    assert set(PIXEL_CASES.values()) >= {(1, 1, 1), (1, 5, 67)} and PIXEL_CASES["b2_3x17"][1:] == (3, 17)


# ------------------------------------------------------------------------------------------ the product vs the fp64 fixture
def _product(env, tag, needs=(True, True), flow_channels=None):  # noqa: F811
    from stereo_toolbox_amd import ops
    N, D, H, W, n, use_scale, _ = CASES[tag]
    flow, mask, gw = inputs(tag)
    if flow_channels is not None:
        flow, gw = flow[:, flow_channels].contiguous(), gw[:, flow_channels].contiguous()
    dev = env.device
    flow, mask = flow.to(dev).requires_grad_(needs[0]), mask.to(dev).requires_grad_(needs[1])
    with env.ctx():
        out = ops.convex_upsample(flow, mask, n_downsample=n, use_scale_factor=use_scale)
        (out * gw.to(dev)).sum().backward()
        sync(env)
    return out.detach(), flow.grad, mask.grad


@pytest.mark.parametrize("tag", list(CASES))
def test_convex_upsample_matches_reference_fp64(env, gold, tag):  # noqa: F811
    N, D, H, W, n, _, _ = CASES[tag]
    out, g_flow, g_mask = _product(env, tag)
    assert out.shape == (N, D, H << n, W << n) and out.dtype == torch.float32 and out.is_contiguous()
    within_fixture(out, gold, f"{tag}:out", VALUE_FACTOR, f"{tag} out")
    within_fixture(g_flow, gold, f"{tag}:g_flow", GRAD_FACTOR, f"{tag} g_flow")
    within_fixture(g_mask, gold, f"{tag}:g_mask", GRAD_FACTOR, f"{tag} g_mask")
    assert g_mask.abs().max().item() > 0


def test_constant_mask_gives_the_neighbourhood_mean(env):  # noqa: F811
    tag = "const_3x5_n2"
    flow, _, _ = inputs(tag)
    out, _, _ = _product(env, tag)
    mean = 4.0 * torch.nn.functional.avg_pool2d(flow.double(), 3, 1, 1, count_include_pad=True)
    want = mean.repeat_interleave(4, 2).repeat_interleave(4, 3)
    assert (out.cpu().double() - want).abs().max().item() <= 4 * 2.0 ** -24 * want.abs().max().item()   # the mean's own rounding


@pytest.mark.parametrize("tag", list(PIXEL_CASES))
def test_softmax_context_upsample_matches_reference_fp64(env, gold, tag):  # noqa: F811
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models.IGEVStereo import upsample_disp_from_logits
    B, h, w = PIXEL_CASES[tag]
    disp, logits, gw = pixel_inputs(tag)
    dev = env.device

    def run(fn):
        d, z = disp.to(dev).requires_grad_(), logits.to(dev).requires_grad_()
        with env.ctx():
            out = fn(d, z)
            (out * gw.to(dev)).sum().backward()
            sync(env)
        return out.detach(), d.grad, z.grad
    got = run(upsample_disp_from_logits)
    assert got[0].shape == (B, 4 * h, 4 * w) and got[0].dtype == torch.float32 and got[0].is_contiguous()
    for g, k, factor in zip(got, ("out", "g_disp", "g_logits"), (VALUE_FACTOR, GRAD_FACTOR, GRAD_FACTOR)):
        within_fixture(g, gold, f"{tag}:{k}", factor, f"{tag} {k}")
    # the unfused pair the models run today: the existing kernel on stock soft-max weights
    old = run(lambda d, z: ops.context_upsample(PIXEL_SCALE * d, torch.softmax(z, 1)))
    for a, b, k, factor in zip(got, old, ("out", "g_disp", "g_logits"), (VALUE_FACTOR, GRAD_FACTOR, GRAD_FACTOR)):
        err, dref = (a.double() - b.double()).abs().max().item(), float(gold[f"{tag}:{k}:dref"])
        print(f"{tag} {k} fused vs softmax + context_upsample: err {err:.3e}  d_ref {dref:.3e}  ratio {err / dref:.2f}")
        assert err <= factor * dref, (k, err, dref)
    again = run(lambda d, z: ops.softmax_context_upsample(d, z, PIXEL_SCALE))
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------------------------------ equivalences, reproducibility
def test_two_channel_flow_equals_two_one_channel_calls(env):  # noqa: F811
    tag = "b2_d2_5x7_n2"
    out, g_flow, _ = _product(env, tag)
    for d in (0, 1):
        o1, g1, _ = _product(env, tag, flow_channels=[d])
        assert torch.equal(o1, out[:, d:d + 1]) and torch.equal(g1, g_flow[:, d:d + 1]), d


@pytest.mark.parametrize("tag", ["b2_d2_5x7_n2", "d1_2x33_n3", "d3_5x14_n1"])
def test_two_runs_give_the_same_bits(env, tag):  # noqa: F811
    a, b = _product(env, tag), _product(env, tag)
    assert all(torch.equal(x, y) and x.abs().max().item() > 0 for x, y in zip(a, b))


@pytest.mark.parametrize("tag", ["b2_d2_5x7_n2", "d1_5x67_n1_noscale", "d3_5x14_n1"])
def test_a_skipped_gradient_leaves_the_other_unchanged(env, tag):  # noqa: F811
    _, g_flow, g_mask = _product(env, tag)
    _, only_flow, none_mask = _product(env, tag, needs=(True, False))
    _, none_flow, only_mask = _product(env, tag, needs=(False, True))
    assert none_mask is None and none_flow is None
    assert torch.equal(only_flow, g_flow) and torch.equal(only_mask, g_mask)


def test_fp16_mask_under_autocast_is_its_fp32_cast(env):  # noqa: F811
    from stereo_toolbox_amd.models.RAFTStereo import upsample_flow
    from stereo_toolbox_amd.models.StereoAnywhere import convex_upflow
    tag = "b2_d2_5x7_n2"
    flow, mask, gw = inputs(tag)
    dev = env.device
    device_type = "cuda" if env.name == "hip" else "cpu"
    res = []
    for low in (False, True):
        f = flow.to(dev).requires_grad_()
        m = (mask.half() if low else mask.half().float()).to(dev).requires_grad_()
        with env.ctx(), torch.autocast(device_type, dtype=torch.float16, enabled=low):
            out = upsample_flow(f, m, 2)
            assert torch.equal(out, convex_upflow(f, m, n_downsample=2, use_scale_factor=True))
            (out * gw.to(dev)).sum().backward()
            sync(env)
        res.append((out.detach(), f.grad, m.grad))
    assert res[1][0].dtype == torch.float32 and res[1][2].dtype == torch.float16
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2].half(), res[1][2])                       # the cast's backward rounds the fp32 gradient to fp16


# ------------------------------------------------------------------------------------------ kernel level (C-ABI)
def test_kernel_level_convex_upsample(be, gold):  # noqa: F811
    """stx_convex_upsample_fwd / _bwd through the C-ABI at f = 8 across a workgroup border; a NULL gradient leaves the other
    bitwise unchanged; refused calls launch nothing (the output keeps its NaN fill)."""
    from stereo_toolbox_amd import ops
    tag = "d1_2x33_n3"
    N, D, H, W, n, _, _ = CASES[tag]
    f = 2 ** n
    flow, mask, gw = (be.dev(t) for t in inputs(tag))
    out, gf, gm = be.empty(N, D, f * H, f * W), be.empty(N, D, H, W), be.empty(N, 9 * f * f, H, W)
    nws = be.raw("stx_convex_upsample_bwd_workspace_floats")(N, D, H, W)
    assert nws == 2 * N * D * 9 * H * W
    ws = be.empty(nws)
    be.call("stx_convex_upsample_fwd", ptr(flow), ptr(mask), ptr(out), N, D, H, W, 9 * f * f, f, float(f))
    be.call("stx_convex_upsample_bwd", ptr(gw), ptr(flow), ptr(mask), ptr(gf), ptr(gm), ptr(ws), N, D, H, W, 9 * f * f, f, float(f))
    within_fixture(out, gold, f"{tag}:out", VALUE_FACTOR, "kernel out")
    within_fixture(gf, gold, f"{tag}:g_flow", GRAD_FACTOR, "kernel g_flow")
    within_fixture(gm, gold, f"{tag}:g_mask", GRAD_FACTOR, "kernel g_mask")
    only_f, only_m = be.empty(N, D, H, W), be.empty(N, 9 * f * f, H, W)
    be.call("stx_convex_upsample_bwd", ptr(gw), ptr(flow), ptr(mask), ptr(only_f), None, ptr(ws), N, D, H, W, 9 * f * f, f, float(f))
    be.call("stx_convex_upsample_bwd", ptr(gw), ptr(flow), ptr(mask), None, ptr(only_m), None, N, D, H, W, 9 * f * f, f, float(f))
    assert torch.equal(only_f, gf) and torch.equal(only_m, gm)
    untouched, untouched_g = be.empty(N, D, f * H, f * W), be.empty(N, 9 * f * f, H, W)
    for bad in ((ptr(flow), ptr(mask), ptr(untouched), N, D, H, W, 9 * 9, 3, 3.0),             # f = 3
                (ptr(flow), ptr(mask), ptr(untouched), N, D, H, W, 9 * 16 * 16, 16, 16.0),      # f = 16
                (ptr(flow), ptr(mask), ptr(untouched), N, D, H, W, 9 * f * f - 1, f, float(f)),  # channel count
                (ptr(flow), ptr(mask), ptr(untouched), N, D, H, W, 9 * 16, f, float(f)),         # another factor's channel count
                (None, ptr(mask), ptr(untouched), N, D, H, W, 9 * f * f, f, float(f)),
                (ptr(flow), None, ptr(untouched), N, D, H, W, 9 * f * f, f, float(f)),
                (ptr(flow), ptr(mask), ptr(untouched), N, 0, H, W, 9 * f * f, f, float(f))):
        with pytest.raises(ops.StxError):
            be.call("stx_convex_upsample_fwd", *bad)
    with pytest.raises(ops.StxError):
        be.call("stx_convex_upsample_fwd", ptr(flow), ptr(mask), None, N, D, H, W, 9 * f * f, f, float(f))
    for bad in ((ptr(gw), ptr(flow), ptr(mask), None, ptr(untouched_g), None, N, D, H, W, 9 * f * f, 5, 5.0),
                (ptr(gw), ptr(flow), ptr(mask), None, ptr(untouched_g), None, N, D, H, W, 9 * f * f + 9, f, float(f)),
                (None, ptr(flow), ptr(mask), None, ptr(untouched_g), None, N, D, H, W, 9 * f * f, f, float(f)),
                (ptr(gw), ptr(flow), ptr(mask), None, None, ptr(ws), N, D, H, W, 9 * f * f, f, float(f)),
                (ptr(gw), ptr(flow), ptr(mask), ptr(untouched_g), None, None, N, D, H, W, 9 * f * f, f, float(f))):   # g_flow without workspace
        with pytest.raises(ops.StxError):
            be.call("stx_convex_upsample_bwd", *bad)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(untouched).all() and torch.isnan(untouched_g).all()


def test_kernel_level_softmax_context_upsample(be, gold):  # noqa: F811
    from stereo_toolbox_amd import ops
    tag = "b2_3x17"
    B, h, w = PIXEL_CASES[tag]
    disp, logits, gw = (be.dev(t) for t in pixel_inputs(tag))
    out, gd, gl = be.empty(B, 4 * h, 4 * w), be.empty(B, 1, h, w), be.empty(B, 9, 4 * h, 4 * w)
    ws = be.empty(be.raw("stx_convex_upsample_bwd_workspace_floats")(B, 1, h, w))
    be.call("stx_softmax_context_upsample_fwd", ptr(disp), ptr(logits), ptr(out), B, h, w, PIXEL_SCALE)
    be.call("stx_softmax_context_upsample_bwd", ptr(gw), ptr(disp), ptr(logits), ptr(gd), ptr(gl), ptr(ws), B, h, w, PIXEL_SCALE)
    within_fixture(out, gold, f"{tag}:out", VALUE_FACTOR, "kernel out")
    within_fixture(gd, gold, f"{tag}:g_disp", GRAD_FACTOR, "kernel g_disp")
    within_fixture(gl, gold, f"{tag}:g_logits", GRAD_FACTOR, "kernel g_logits")
    only_d, only_l = be.empty(B, 1, h, w), be.empty(B, 9, 4 * h, 4 * w)
    be.call("stx_softmax_context_upsample_bwd", ptr(gw), ptr(disp), ptr(logits), ptr(only_d), None, ptr(ws), B, h, w, PIXEL_SCALE)
    be.call("stx_softmax_context_upsample_bwd", ptr(gw), ptr(disp), ptr(logits), None, ptr(only_l), None, B, h, w, PIXEL_SCALE)
    assert torch.equal(only_d, gd) and torch.equal(only_l, gl)
    untouched = be.empty(B, 4 * h, 4 * w)
    for bad in ((None, ptr(logits), ptr(untouched), B, h, w, PIXEL_SCALE), (ptr(disp), None, ptr(untouched), B, h, w, PIXEL_SCALE),
                (ptr(disp), ptr(logits), ptr(untouched), B, 0, w, PIXEL_SCALE)):
        with pytest.raises(ops.StxError):
            be.call("stx_softmax_context_upsample_fwd", *bad)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(untouched).all()


# ------------------------------------------------------------------------------------------ sequence loss
def _weights(K):
    return trainer_weights(K - 1) if K >= 3 else [1.0, 0.7][:K]


def _loss_product(env, gt, preds, weights, fn=None):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    leaves = [p.to(dev).clone().requires_grad_() for p in preds]
    with env.ctx():
        loss = fn(leaves, gt.to(dev)) if fn else ops.sequence_loss(leaves, gt.to(dev), LOSS_MAXDISP, weights)
        loss.backward()
        sync(env)
    return loss.detach(), torch.stack([p.grad for p in leaves])


def _multi(gt, preds, weights, dtype):
    from stereo_toolbox_amd.losses import masked_smooth_l1_multi
    leaves = [p.to(dtype).clone().requires_grad_() for p in preds]
    loss = masked_smooth_l1_multi(leaves, gt.to(dtype), LOSS_MAXDISP, weights)
    loss.backward()
    return loss.detach(), torch.stack([p.grad for p in leaves])


def test_loss_inputs_hold_the_planted_pixels():
    gt, preds = loss_inputs(2)
    valid = (gt > 0) & (gt < LOSS_MAXDISP - 1)
    assert gt.shape == LOSS_SHAPE and preds[0].shape == (LOSS_SHAPE[0], 1) + LOSS_SHAPE[1:]
    assert (gt == 0).sum() >= 2 and (gt >= LOSS_MAXDISP - 1).sum() >= 3 and torch.isnan(gt).sum() == 1 and torch.isinf(gt).sum() == 2
    d = (preds[1][:, 0] - gt)[valid]
    assert (d == 1).any() and (d == -1).any() and (d.abs() < 1).any() and (d > 1).any() and (d < -1).any()
    assert 0 < valid.sum() < gt.numel()


@pytest.mark.parametrize("K", LOSS_KS)
def test_sequence_loss_equals_masked_smooth_l1_multi(env, K):  # noqa: F811
    gt, preds = loss_inputs(K)
    w = _weights(K)
    (want_l, want_g), (l32, g32) = _multi(gt, preds, w, torch.float64), _multi(gt, preds, w, torch.float32)
    loss, grads = _loss_product(env, gt, preds, w)
    assert loss.shape == () and loss.dtype == torch.float32 and grads.shape == (K, LOSS_SHAPE[0], 1) + LOSS_SHAPE[1:]
    # (no fixture: d_ref is the distance of the reference's fp32 run from its fp64 run, formed here)
    within(loss, want_l, (l32.double() - want_l).abs().max().item(), VALUE_FACTOR, f"K={K} loss")
    within(grads, want_g, (g32.double() - want_g).abs().max().item(), GRAD_FACTOR, f"K={K} gradients")
    excluded = ~((gt > 0) & (gt < LOSS_MAXDISP - 1))
    assert excluded.sum() > 8 and (grads.cpu()[:, excluded.unsqueeze(1)] == 0).all() and torch.isfinite(grads).all()
    again = _loss_product(env, gt, preds, w)
    assert torch.equal(again[0], loss) and torch.equal(again[1], grads)
    flat = _loss_product(env, gt, [p.squeeze(1) for p in preds], w)                 # [B, H, W] predictions
    assert torch.equal(flat[0], loss) and torch.equal(flat[1].unsqueeze(2), grads)


def test_sequence_loss_matches_the_trainer_fixture(env, gold):  # noqa: F811
    from stereo_toolbox_amd.losses import sequence_loss, sequence_loss_weights
    gt, preds = loss_inputs()
    assert sequence_loss_weights(LOSS_PREDICTIONS, LOSS_GAMMA) == trainer_weights(LOSS_PREDICTIONS)
    loss, grads = _loss_product(env, gt, preds, None, fn=lambda p, g: sequence_loss(p[0], p[1:], g, LOSS_MAXDISP, LOSS_GAMMA))
    within_fixture(loss, gold, "trainer:loss", VALUE_FACTOR, "trainer loss")
    within_fixture(grads, gold, "trainer:grads", GRAD_FACTOR, "trainer gradients")
    with pytest.raises(ValueError):
        sequence_loss_weights(1)
    with pytest.raises(ValueError), env.ctx():
        sequence_loss(preds[0].to(env.device), [preds[1].to(env.device)], gt.to(env.device), LOSS_MAXDISP)


def test_all_invalid_gt_gives_zero_loss_and_zero_gradients(env):  # noqa: F811
    gt, preds = loss_inputs(3)
    for bad in (torch.zeros_like(gt), torch.full_like(gt, float("nan")), torch.full_like(gt, LOSS_MAXDISP + 1.0)):
        loss, grads = _loss_product(env, bad, preds, _weights(3))
        assert loss.item() == 0.0 and (grads == 0).all()


def test_only_some_predictions_require_grad(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    gt, preds = loss_inputs(3)
    _, full = _loss_product(env, gt, preds, _weights(3))
    dev = env.device
    leaves = [p.to(dev).clone().requires_grad_(k != 1) for k, p in enumerate(preds)]
    with env.ctx():
        ops.sequence_loss(leaves, gt.to(dev), LOSS_MAXDISP, _weights(3)).backward()
        sync(env)
    assert leaves[1].grad is None and torch.equal(leaves[0].grad, full[0]) and torch.equal(leaves[2].grad, full[2])


def test_kernel_level_sequence_loss_refuses_too_many_predictions(be):  # noqa: F811
    from stereo_toolbox_amd import ops
    limit = be.raw("stx_sequence_loss_max_predictions")()
    assert limit >= 33
    gt, preds = loss_inputs(1)
    n = gt.numel()
    g, p = be.dev(gt), be.dev(preds[0])
    out, cnt = be.empty(1), be.empty(1, dtype=torch.int32)
    ws = be.empty(be.raw("stx_sequence_loss_workspace_floats")(n))
    gp = be.empty(n)

    def table(K, t):
        return (ctypes.c_void_p * K)(*[t.data_ptr()] * K), (ctypes.c_double * K)(*[1.0] * K)
    for K in (0, limit + 1):
        tab, w = table(max(K, 1), p)
        with pytest.raises(ops.StxError):
            be.call("stx_sequence_loss_fwd", tab, w, K, ptr(g), float(LOSS_MAXDISP), ptr(out), ptr(cnt), ptr(ws), n)
        with pytest.raises(ops.StxError):
            be.call("stx_sequence_loss_bwd", ptr(out), tab, w, K, ptr(g), float(LOSS_MAXDISP), ptr(cnt), table(max(K, 1), gp)[0], n)
    tab, w = table(1, p)
    with pytest.raises(ops.StxError):
        be.call("stx_sequence_loss_fwd", tab, w, 1, None, float(LOSS_MAXDISP), ptr(out), ptr(cnt), ptr(ws), n)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(gp).all() and int(cnt.item()) == 0
    # the limit itself runs: `limit` copies of one prediction with weight 1 give `limit` times its loss
    tab, w = table(limit, p)
    be.call("stx_sequence_loss_fwd", tab, w, limit, ptr(g), float(LOSS_MAXDISP), ptr(out), ptr(cnt), ptr(ws), n)
    valid = (gt > 0) & (gt < LOSS_MAXDISP - 1)
    one = torch.nn.functional.smooth_l1_loss(preds[0].double()[:, 0][valid], gt.double()[valid])
    assert int(cnt.item()) == int(valid.sum()) and abs(out.item() - limit * one.item()) <= 2.0 ** -23 * limit * one.item()


# ------------------------------------------------------------------------------------------ argument errors
def test_unsupported_arguments_are_refused(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    flow, mask, _ = inputs("b2_d2_5x7_n2")
    disp, logits, _ = pixel_inputs("b2_3x17")
    gt, preds = loss_inputs(2)
    dev = env.device
    flow, mask, disp, logits, gt = (t.to(dev) for t in (flow, mask, disp, logits, gt))
    preds = [p.to(dev) for p in preds]
    with env.ctx():
        limit = ops.sequence_loss_max_predictions()
        for f, m, kw in ((flow[0], mask, {}), (flow, mask[0], {}),                                # ranks
                         (flow, mask[:, :143], {}), (flow, mask, {"n_downsample": 1}),            # channel count != 9 * 4^n
                         (flow, mask[:, :, :4], {}), (flow, mask[..., :6], {}), (flow[:1], mask, {}),      # H, W, N
                         (flow, mask, {"n_downsample": 0}), (flow, mask, {"n_downsample": 4}), (flow, mask, {"n_downsample": 2.0})):
            with pytest.raises(ops.StxError, match=r"\(2, 2, 5, 7\)|\(2, 5, 7\)|\(2, 144, 5, 7\)"):
                ops.convex_upsample(f, m, **kw)
        for d, z in ((disp[:, 0], logits), (disp, logits[:, :8]), (disp, logits[..., :67]), (disp.repeat(1, 2, 1, 1), logits)):
            with pytest.raises(ops.StxError, match=r"\(2, "):
                ops.softmax_context_upsample(d, z)
        with pytest.raises(ValueError, match="2 predictions but 3 weights"):
            ops.sequence_loss(preds, gt, LOSS_MAXDISP, [1.0, 1.0, 1.0])
        with pytest.raises(ops.StxError, match="predictions"):
            ops.sequence_loss(preds[:1] * (limit + 1), gt, LOSS_MAXDISP, [1.0] * (limit + 1))
        with pytest.raises(ops.StxError, match="predictions"):
            ops.sequence_loss([], gt, LOSS_MAXDISP, [])
        with pytest.raises(ops.StxError, match="prediction 1"):
            ops.sequence_loss([preds[0], preds[1][..., :66]], gt, LOSS_MAXDISP, [1.0, 1.0])
