"""StereoAnywhere's mono-stereo alignment stage (reference models/StereoAnywhere/utils/utils.py:48-54, 172-198, 240-269, 345-384,
stereoanywhere.py:167-235) on the kernels of csrc/mono_align.hip: the masks and the masked N-channel volume, softlrc,
weighted_lsq, the mirror detector and their composition `align_mono`.

* tests/golden/mono_align.npz holds what the reference's OWN functions give on the seeded cases of
  tests/golden/mono_align_config.py, in fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| > 0
  (tests/golden/make_golden_mono_align.py).  The masks, the masked volume and its gradient are exact: fp32 only, compared with ==.
* A plain-torch restatement lives in this file and is pinned to the fixture on the CPU first -- in fp64 to 1e-11, in fp32 to
  2 x d_ref -- so the fixture and the restatement check each other.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture: values within VALUE_FACTOR (2) x
  d_ref, gradients within GRAD_FACTOR (3) x d_ref, floor 2e-7 * max(1, max|want|) where d_ref is zero.  Every element of every
  tensor is compared and the achieved ratios go to the parity report.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.backends import be, ptr  # noqa: F401
from tests.golden.mono_align_config import (ALIGN_ARGS, ALIGN_FIELDS, ALIGN_INPUTS, LRC_CASES, LRC_THRESHOLDS, LSQ_CASES, MASK_CASES,
                                            MIRROR_THRESHOLDS, QUANTILES, align_inputs, lrc_inputs, lsq_inputs, mask_inputs,
                                            mirror_inputs)
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, Env, env, on, pin_fixture, sync, within_fixture  # noqa: F401
from tests.restated import truncation_mask
from stereo_toolbox_amd.utils import synthetic_tensor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mono_align.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------------------------------ the restatement (plain torch)
def masks_of(mde, N, threshold_dtype=torch.float32):
    """[B,1,H,W] -> one-hot fp16 [B,N,H,W]; the thresholds i/N rounded to `threshold_dtype` and compared in it"""
    m = mde.to(threshold_dtype)
    th = [torch.tensor(i / N, dtype=torch.float64).to(threshold_dtype) for i in range(N + 1)]
    return torch.cat([(m >= th[i]) & (m < th[i + 1]) for i in range(N)], dim=1).to(torch.float16)


def masked(volume, left, right, N):
    return volume * masks_of(left, N).unsqueeze(4) * masks_of(right, N).unsqueeze(3)


def warp(img, disp, sign):
    """disp_warping (utils.py:172-187): the grid 2 (x -+ d) / W - 1, 2 y / H - 1 under align_corners=True, zeros outside"""
    B, _, H, W = img.shape
    x = torch.arange(W, dtype=img.dtype, device=img.device).view(1, 1, W).expand(B, H, W)
    y = torch.arange(H, dtype=img.dtype, device=img.device).view(1, H, 1).expand(B, H, W)
    grid = 2 * torch.stack([(x + sign * disp[:, 0]) / W, y / H], dim=-1) - 1
    return F.grid_sample(img, grid, align_corners=True)


def soft_lrc(d2, d3, th):
    import math
    w2, w3 = warp(d2, torch.relu(d3), 1.0), warp(d3, torch.relu(d2), -1.0)
    div = math.log(1 + math.exp(th))
    return F.softplus(th - (d2 - w3).abs()) / div, F.softplus(th - (d3 - w2).abs()) / div


def lsq(mde, disp, conf, qmin, qmax):
    """utils.py:345-384 in the tensors' own dtype (a loop over the batch, boolean indexing, quantile and lstsq as there)"""
    B = mde.shape[0]
    rows = []
    for b in range(B):
        m, s, c = mde[b].flatten().abs(), torch.relu(disp[b].flatten()), conf[b].flatten().abs()
        keep = (torch.quantile(s, qmin) <= s) & (s <= torch.quantile(s, qmax))
        w = torch.sqrt(c[keep] * (1 - 0.1) + 0.1)
        A = torch.stack([m[keep] * w, w], dim=-1).unsqueeze(0)          # a batch of one, as there: the same LAPACK path in fp32
        rows.append(torch.linalg.lstsq(A, (s[keep] * w).unsqueeze(-1).unsqueeze(0))[0].reshape(2))
    ss = torch.stack(rows)
    return ss[:, 0].reshape(B, 1, 1, 1), ss[:, 1].reshape(B, 1, 1, 1)


def mirror(sd, md, sc, mc, th, gain=20):
    near = torch.sigmoid(gain * (md - sd))
    a, b = sc * mc * near, (1 - sc) * mc
    return torch.sigmoid(gain * (a + b - a * b - th))


def align(x):
    th = ALIGN_ARGS["lrc_th"]
    lrc2, lrc3 = soft_lrc(x["dispmono2"], x["dispmono3"], th)
    conf2, conf3 = x["lconf2"] * lrc2, x["lconf3"] * lrc3
    scale, shift = lsq(torch.cat([x["mde2"], x["mde3"]], 1), torch.cat([x["dispmono2"], x["dispmono3"]], 1),
                       torch.cat([conf2, conf3], 1), *QUANTILES)
    scaled2, scaled3 = scale * x["mde2"] + shift, scale * x["mde3"] + shift
    lrcs2, _ = soft_lrc(scaled2, scaled3, th)
    mir = mirror(x["dispmono2"], scaled2, conf2, lrcs2, ALIGN_ARGS["mirror_conf_th"])
    mask = truncation_mask(scaled2, mir, None, ALIGN_ARGS["mirror_attenuation"]).detach()
    return dict(zip(ALIGN_FIELDS, (lrc2, lrc3, conf2, conf3, scale, shift, scaled2, scaled3, lrcs2, mir, mask)))


def _restated_lrc(tag, dtype):
    d2, d3, gws = lrc_inputs(tag)
    a, b = d2.to(dtype).requires_grad_(), d3.to(dtype).requires_grad_()
    o2, o3 = soft_lrc(a, b, LRC_THRESHOLDS[tag])
    ((o2 * gws[0].to(dtype)).sum() + (o3 * gws[1].to(dtype)).sum()).backward()
    return {"out2": o2.detach(), "out3": o3.detach(), "g_disp2": a.grad, "g_disp3": b.grad}


def _restated_lsq(tag, dtype):
    mde, disp, conf, gws = lsq_inputs(tag)
    m, d, c = (t.to(dtype).requires_grad_() for t in (mde, disp, conf))
    scale, shift = lsq(m, d, c, *QUANTILES)
    ((scale * gws[0].to(dtype)).sum() + (shift * gws[1].to(dtype)).sum()).backward()
    return {"scale": scale.detach(), "shift": shift.detach(), "g_mde": m.grad, "g_disp": d.grad, "g_conf": c.grad}


def _restated_mirror(name, dtype):
    sd, md, sc, mc, gw = mirror_inputs()
    xs = [t.to(dtype).requires_grad_() for t in (sd, md, sc, mc)]
    out = mirror(*xs, MIRROR_THRESHOLDS[name])
    (out * gw.to(dtype)).sum().backward()
    return {"out": out.detach(), "g_sd": xs[0].grad, "g_md": xs[1].grad, "g_sc": xs[2].grad, "g_mc": xs[3].grad}


def _restated_align(dtype):
    x, gws = align_inputs()
    x = {k: v.to(dtype).requires_grad_() for k, v in x.items()}
    fields = align(x)
    sum((fields[f] * g.to(dtype)).sum() for f, g in gws.items()).backward()
    res = {k: v.detach() for k, v in fields.items()}
    res.update({"g_" + k: x[k].grad for k in ALIGN_INPUTS})
    return res


@pytest.mark.parametrize("tag", list(MASK_CASES))
def test_mask_restatement_equals_reference_fixture(gold, tag):
    B, N, H, W2, W3 = MASK_CASES[tag]
    vol, left, right, gw = mask_inputs(tag)
    assert torch.equal(masks_of(left, N), torch.from_numpy(gold[f"mask:{tag}:left:f32"]))
    assert torch.equal(masks_of(right, N), torch.from_numpy(gold[f"mask:{tag}:right:f32"]))
    v = vol.clone().requires_grad_()
    out = masked(v, left, right, N)
    (out * gw).sum().backward()
    assert torch.equal(out.detach(), torch.from_numpy(gold[f"mask:{tag}:out:f32"]))
    assert torch.equal(v.grad, torch.from_numpy(gold[f"mask:{tag}:g_volume:f32"]))


def test_fixture_tells_fp32_thresholds_from_double_thresholds(gold):
    """N = 6: a bin rule that compares in double disagrees with the reference on the planted f32(i/6); N = 8 and 3 cannot tell."""
    differs = {}
    for tag, (B, N, H, W2, W3) in MASK_CASES.items():
        _, left, right, _ = mask_inputs(tag)
        differs[N] = any(not torch.equal(masks_of(m, N, torch.float64), torch.from_numpy(gold[f"mask:{tag}:{k}:f32"]))
                         for m, k in ((left, "left"), (right, "right")))
    assert differs == {8: False, 6: True, 3: False}


@pytest.mark.parametrize("tag", list(LRC_CASES))
def test_softlrc_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated_lrc(tag, torch.float64), _restated_lrc(tag, torch.float32)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"lrc:{tag}:{k}")


@pytest.mark.parametrize("tag", list(LSQ_CASES))
def test_weighted_lsq_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated_lsq(tag, torch.float64), _restated_lsq(tag, torch.float32)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"lsq:{tag}:{k}")


@pytest.mark.parametrize("name", list(MIRROR_THRESHOLDS))
def test_mirror_restatement_matches_reference_fixture(gold, name):
    r64, r32 = _restated_mirror(name, torch.float64), _restated_mirror(name, torch.float32)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"mirror:{name}:{k}")


def test_align_restatement_matches_reference_fixture(gold):
    r64, r32 = _restated_align(torch.float64), _restated_align(torch.float32)
    assert len(r64) == len(ALIGN_FIELDS) + len(ALIGN_INPUTS)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"align:{k}")


# ------------------------------------------------------------------------------------------ masks and the masked volume: exact
def _masked_volume(env, tag):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    B, N, H, W2, W3 = MASK_CASES[tag]
    vol, left, right, gw = (t.to(env.device) for t in mask_inputs(tag))
    v = vol.clone().requires_grad_()
    with env.ctx():
        ml, mr = SA.generate_masks(left, N=N), SA.generate_masks(right, N=N)
        out = SA.masked_volume(v, left, right, N)
        loss = (out * gw).sum()
        loss.backward(retain_graph=True)
        sync(env)
    return ml, mr, out, v, loss


@pytest.mark.parametrize("backend,tag", on(MASK_CASES))
def test_masks_and_masked_volume_equal_reference(backend, tag, gold):
    env_ = Env(backend)
    B, N, H, W2, W3 = MASK_CASES[tag]
    ml, mr, out, v, _ = _masked_volume(env_, tag)
    assert ml.dtype == mr.dtype == torch.float16 and ml.shape == (B, N, H, W2) and mr.shape == (B, N, H, W3)
    assert torch.equal(ml.cpu(), torch.from_numpy(gold[f"mask:{tag}:left:f32"]))
    assert torch.equal(mr.cpu(), torch.from_numpy(gold[f"mask:{tag}:right:f32"]))
    assert out.dtype == torch.float32 and out.shape == (B, N, H, W2, W3) and out.is_contiguous()
    assert torch.equal(out.detach().cpu(), torch.from_numpy(gold[f"mask:{tag}:out:f32"]))
    assert v.grad.shape == v.shape and torch.equal(v.grad.cpu(), torch.from_numpy(gold[f"mask:{tag}:g_volume:f32"]))
    stock = v.detach() * ml.unsqueeze(4) * mr.unsqueeze(3)               # stock ops on the product's own masks
    assert torch.equal(out.detach(), stock) and (out != 0).sum().item() > 0


def test_masked_volume_gives_zero_for_a_non_finite_entry_under_a_zero_mask(env):  # noqa: F811
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    vol, left, right, _ = mask_inputs("b2_13")
    vol[0, 0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.5])
    left[0, 0, 0, 0], right[0, 0, 0, :4] = 0.05, 0.95                    # bins 0 and 7: nothing of the row's start survives
    with env.ctx():
        out = SA.masked_volume(vol.to(env.device), left.to(env.device), right.to(env.device), 8)
        sync(env)
    assert (out[0, :, 0, 0, :4] == 0).all() and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------ softlrc vs fp64
def _softlrc(env, tag, which=(0, 1)):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    d2, d3, gws = lrc_inputs(tag)
    a, b = d2.to(env.device).requires_grad_(), d3.to(env.device).requires_grad_()
    with env.ctx():
        outs = SA.softlrc(a, b, lrc_th=LRC_THRESHOLDS[tag])
        loss = sum((outs[i] * gws[i].to(env.device)).sum() for i in which)
        loss.backward(retain_graph=True)
        sync(env)
    return outs, a, b, loss


@pytest.mark.parametrize("backend,tag", on(LRC_CASES))
def test_softlrc_matches_reference_fp64(backend, tag, gold, parity_log):
    env_ = Env(backend)
    B, H, W, _ = LRC_CASES[tag]
    outs, a, b, _ = _softlrc(env_, tag)
    for k, got, factor in (("out2", outs[0], VALUE_FACTOR), ("out3", outs[1], VALUE_FACTOR), ("g_disp2", a.grad, GRAD_FACTOR),
                           ("g_disp3", b.grad, GRAD_FACTOR)):
        assert got.shape == (B, 1, H, W) and got.dtype == torch.float32
        key = f"lrc:{tag}:{k}"
        within_fixture(got, gold, key, factor, f"mono_align softlrc {tag} {k} [{backend}]", parity_log)


def test_softlrc_gradient_of_one_output_alone(env, gold, parity_log):  # noqa: F811
    """The loss on one output only (the other's gradient is absent, as in the model's second call): the two single-output
    gradients add up to the fixture's."""
    _, a0, b0, _ = _softlrc(env, "px37", which=(0,))
    _, a1, b1, _ = _softlrc(env, "px37", which=(1,))
    for k, got in (("g_disp2", a0.grad.double() + a1.grad.double()), ("g_disp3", b0.grad.double() + b1.grad.double())):
        key = f"lrc:px37:{k}"
        within_fixture(got, gold, key, GRAD_FACTOR, f"mono_align softlrc px37 {k} summed [{env.name}]", parity_log)


# ------------------------------------------------------------------------------------------ weighted_lsq vs fp64
def _weighted_lsq(env, tag):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    mde, disp, conf, gws = lsq_inputs(tag)
    m, d, c = (t.to(env.device).requires_grad_() for t in (mde, disp, conf))
    with env.ctx():
        scale, shift = SA.weighted_lsq(m, d, c, min_quantile=QUANTILES[0], max_quantile=QUANTILES[1])
        loss = (scale * gws[0].to(env.device)).sum() + (shift * gws[1].to(env.device)).sum()
        loss.backward(retain_graph=True)
        sync(env)
    return {"scale": scale, "shift": shift, "g_mde": m.grad, "g_disp": d.grad, "g_conf": c.grad}, (m, d, c), loss


@pytest.mark.parametrize("backend,tag", on(LSQ_CASES))
def test_weighted_lsq_matches_reference_fp64(backend, tag, gold, parity_log):
    from stereo_toolbox_amd import ops
    env_ = Env(backend)
    B, C, H, W = LSQ_CASES[tag][:4]
    got, (m, d, c), _ = _weighted_lsq(env_, tag)
    assert got["scale"].shape == got["shift"].shape == (B, 1, 1, 1) and got["g_mde"].shape == (B, C, H, W)
    for k, t in got.items():
        assert t.dtype == torch.float32
        key = f"lsq:{tag}:{k}"
        within_fixture(t, gold, key, GRAD_FACTOR if k.startswith("g_") else VALUE_FACTOR,
                       f"mono_align weighted_lsq {tag} {k} [{backend}]", parity_log)
    with env_.ctx():
        th = ops.quantile_thresholds(d.detach(), *QUANTILES)
        sync(env_)
    assert torch.equal(th.cpu(), torch.from_numpy(gold[f"lsq:{tag}:thresholds:f32"]))    # torch.quantile, fp32, on the CPU


def test_quantile_thresholds_equal_torch_quantile_bit_for_bit(env):  # noqa: F811
    """The on-device selection against torch.quantile on the same device: seeded vectors of several lengths (a single element,
    integer and fractional ranks, more elements than the workgroup has threads), three images a call, relu ties at 0."""
    from stereo_toolbox_amd import ops
    for n, qs in ((1, (0.2, 0.9)), (2, (0.2, 0.9)), (12, (0.2, 0.9)), (21, (0.2, 0.9)), (64, (0.0, 1.0)), (513, (0.33, 0.5)),
                  (1000, (0.2, 0.9)), (5000, (0.2, 0.9))):
        disp = synthetic_tensor((3, 1, 1, n), 4500 + n, lo=-2.0, hi=12.0).to(env.device)
        disp[2] = torch.round(disp[2])
        with env.ctx():
            got = ops.quantile_thresholds(disp, *qs)
            sync(env)
        want = torch.stack([torch.stack([torch.quantile(torch.relu(disp[b].flatten()), q) for q in qs]) for b in range(3)])
        assert got.dtype == torch.float32 and torch.equal(got, want), (n, got, want)


def test_weighted_lsq_singular_system_gives_the_weighted_mean(env):  # noqa: F811
    """One distinct |mde|: the determinant of the normal equations is exactly 0 (powers of two) -> scale 0, shift sum w s / sum w."""
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    mde = torch.full((1, 1, 2, 8), 0.5)
    disp = torch.arange(16, dtype=torch.float32).view(1, 1, 2, 8)
    conf = torch.ones(1, 1, 2, 8)
    with env.ctx():
        scale, shift = SA.weighted_lsq(mde.to(env.device), disp.to(env.device), conf.to(env.device), 0.0, 1.0)
        sync(env)
    assert scale.item() == 0.0 and shift.item() == 7.5


# ------------------------------------------------------------------------------------------ mirror detector, align_mono
def _mirror(env, name):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    sd, md, sc, mc, gw = mirror_inputs()
    xs = [t.to(env.device).requires_grad_() for t in (sd, md, sc, mc)]
    with env.ctx():
        out = SA.handcrafted_mirror_detector(*xs, conf_th=MIRROR_THRESHOLDS[name])
        loss = (out * gw.to(env.device)).sum()
        loss.backward(retain_graph=True)
        sync(env)
    return {"out": out, "g_sd": xs[0].grad, "g_md": xs[1].grad, "g_sc": xs[2].grad, "g_mc": xs[3].grad}, xs, loss


@pytest.mark.parametrize("backend,name", on(MIRROR_THRESHOLDS))
def test_mirror_detector_matches_reference_fp64(backend, name, gold, parity_log):
    got, _, _ = _mirror(Env(backend), name)
    for k, t in got.items():
        assert t.dtype == torch.float32
        key = f"mirror:{name}:{k}"
        within_fixture(t, gold, key, GRAD_FACTOR if k.startswith("g_") else VALUE_FACTOR,
                       f"mono_align mirror {name} {k} [{backend}]", parity_log)


def _align(env):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    x, gws = align_inputs()
    x = {k: v.to(env.device).requires_grad_() for k, v in x.items()}
    with env.ctx():
        res = SA.align_mono(*(x[k] for k in ALIGN_INPUTS), **ALIGN_ARGS)
        loss = sum((getattr(res, f) * g.to(env.device)).sum() for f, g in gws.items())
        loss.backward(retain_graph=True)
        sync(env)
    return res, x, loss


def test_align_mono_matches_reference_fp64(env, gold, parity_log):  # noqa: F811
    res, x, _ = _align(env)
    assert res._fields == ALIGN_FIELDS and res.truncate_mask.requires_grad is False
    for f in ALIGN_FIELDS:
        key = f"align:{f}"
        within_fixture(getattr(res, f), gold, key, VALUE_FACTOR, f"mono_align align_mono {f} [{env.name}]", parity_log)
    for k in ALIGN_INPUTS:
        key = f"align:g_{k}"
        within_fixture(x[k].grad, gold, key, GRAD_FACTOR, f"mono_align align_mono g_{k} [{env.name}]", parity_log)


def test_drop_in_one_liners(env):  # noqa: F811
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    x, y = synthetic_tensor((2, 1, 3, 13), 4600, lo=0.0, hi=1.0), synthetic_tensor((2, 1, 3, 13), 4601, lo=0.0, hi=1.0)
    assert torch.equal(SA.fuzzy_and(x, y), x * y) and torch.equal(SA.fuzzy_or(x, y), x + y - x * y)
    assert torch.equal(SA.fuzzy_not(x), 1 - x)
    s, t = torch.tensor([2.0, 3.0]).view(2, 1, 1, 1), torch.tensor([0.5, -0.5]).view(2, 1, 1, 1)
    assert torch.equal(SA.apply_scale_shift(x, s, t), s * x + t)
    m = masks_of(x, 4).float()
    assert torch.equal(SA.apply_scale_shift(x, s, t, m), ((s * x + t) * m).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------ reproducibility, host syncs
def _grads(ts):
    return [t.grad.clone() for t in ts]


@pytest.mark.parametrize("what", ["masked_volume", "softlrc", "weighted_lsq", "mirror", "align_mono"])
def test_bitwise_reproducible_and_second_backward_equals_the_first(env, what):  # noqa: F811
    def run():
        if what == "masked_volume":
            _, _, out, v, loss = _masked_volume(env, "w70_66")
            return [out], [v], loss
        if what == "softlrc":
            outs, a, b, loss = _softlrc(env, "w70")
            return list(outs), [a, b], loss
        if what == "weighted_lsq":
            got, leaves, loss = _weighted_lsq(env, "general")
            return [got["scale"], got["shift"]], list(leaves), loss
        if what == "mirror":
            got, xs, loss = _mirror(env, "th_default")
            return [got["out"]], xs, loss
        res, x, loss = _align(env)
        return list(res), [x[k] for k in ALIGN_INPUTS], loss
    a_out, a_leaves, a_loss = run()
    b_out, b_leaves, _ = run()
    first = _grads(a_leaves)
    assert all(torch.equal(p, q) for p, q in zip(a_out, b_out))
    assert all(torch.equal(p, q) for p, q in zip(first, _grads(b_leaves))) and all(g.abs().max().item() > 0 for g in first)
    for t in a_leaves:
        t.grad = None
    with env.ctx():
        a_loss.backward()
        sync(env)
    assert all(torch.equal(p, q) for p, q in zip(first, _grads(a_leaves)))


@pytest.mark.gpu
def test_no_host_synchronisation():
    """align_mono (forward and backward) and a weighted_lsq call with B = 3 under torch's sync debug mode "error"."""
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    env_ = Env("hip")
    x, gws = align_inputs()
    x = {k: v.to(env_.device).requires_grad_() for k, v in x.items()}
    gws = {k: v.to(env_.device) for k, v in gws.items()}
    trio = [synthetic_tensor((3, 2, 5, 37), 4700 + i, lo=lo, hi=hi).to(env_.device).requires_grad_()
            for i, (lo, hi) in enumerate(((0.0, 1.0), (-2.0, 12.0), (0.0, 1.0)))]
    SA.align_mono(*(x[k] for k in ALIGN_INPUTS), **ALIGN_ARGS)            # (first use loads the library)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = SA.align_mono(*(x[k] for k in ALIGN_INPUTS), **ALIGN_ARGS)
        sum((getattr(res, f) * g).sum() for f, g in gws.items()).backward()
        scale, shift = SA.weighted_lsq(*trio)
        (scale.sum() + shift.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert scale.shape == (3, 1, 1, 1) and all(torch.isfinite(t.grad).all() for t in trio)
    assert all(torch.isfinite(v.grad).all() for v in x.values())


# ------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_are_refused():
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    vol, left, right, _ = mask_inputs("b2_13")
    d2, d3, _ = lrc_inputs("b2_13")
    mde, disp, conf, _ = lsq_inputs("dozen")
    x, _ = align_inputs()
    for call in (lambda: SA.generate_masks(left, N=8), lambda: SA.masked_volume(vol, left, right, 8), lambda: SA.softlrc(d2, d3),
                 lambda: SA.weighted_lsq(mde, disp, conf), lambda: ops.quantile_thresholds(disp),
                 lambda: SA.handcrafted_mirror_detector(d2, d3, d2, d3), lambda: SA.align_mono(*(x[k] for k in ALIGN_INPUTS))):
        with pytest.raises(ops.StxError, match="ROCm device"):
            call()


def test_unsupported_arguments_are_refused(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    dev = env.device
    vol, left, right, _ = (t.to(dev) for t in mask_inputs("b2_13"))
    d2, d3, _ = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in lrc_inputs("b2_13"))
    mde, disp, conf, _ = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in lsq_inputs("dozen"))
    with env.ctx():
        for n in (0, 65, 8.0, True):
            with pytest.raises(ops.StxError, match="number of masks"):
                SA.generate_masks(left, N=n)
            with pytest.raises(ops.StxError, match="number of masks"):
                SA.masked_volume(vol, left, right, n)
        with pytest.raises(ops.StxError, match=r"\[B, 1, H, W\]"):
            SA.generate_masks(left[:, 0], N=8)                                                # wrong rank
        with pytest.raises(ops.StxError, match=r"\[B, 1, H, W\]"):
            SA.generate_masks(torch.cat([left, left], 1), N=8)                                # two channels
        with pytest.raises(ops.StxError, match="volume must be"):
            SA.masked_volume(vol[:, 0], left, right, 8)
        with pytest.raises(ops.StxError, match="do not match"):
            SA.masked_volume(vol, left[..., :12].contiguous(), right, 8)
        with pytest.raises(ops.StxError, match="W3="):
            SA.masked_volume(torch.zeros(1, 1, 1, 1, 2049, device=dev), torch.zeros(1, 1, 1, 1, device=dev),
                             torch.zeros(1, 1, 1, 2049, device=dev), 2)
        for th in (20.5, None, True):
            with pytest.raises(ops.StxError, match="lrc_th"):
                SA.softlrc(d2, d3, lrc_th=th)
        assert SA.softlrc(d2, d3, lrc_th=20.0)[0].shape == d2.shape
        with pytest.raises(ops.StxError, match="does not match"):
            SA.softlrc(d2, d3[..., :12].contiguous())
        with pytest.raises(ops.StxError, match=r"\[B, 1, H, W\]"):
            SA.softlrc(torch.cat([d2, d2], 1), torch.cat([d3, d3], 1))
        with pytest.raises(ops.StxError, match="backward supports"):
            SA.softlrc(torch.zeros(1, 1, 1, 1025, device=dev).requires_grad_(), torch.zeros(1, 1, 1, 1025, device=dev))
        assert SA.softlrc(torch.zeros(1, 1, 1, 1025, device=dev), torch.zeros(1, 1, 1, 1025, device=dev))[1].shape == (1, 1, 1, 1025)
        for q in ((-0.1, 0.9), (0.2, 1.5), (None, 0.9)):
            with pytest.raises(ops.StxError, match="quantile"):
                SA.weighted_lsq(mde, disp, conf, *q)
        with pytest.raises(ops.StxError, match="does not match"):
            SA.weighted_lsq(mde, disp[:, :1].contiguous(), conf)
        with pytest.raises(ops.StxError, match=r"\[B, C, H, W\]"):
            SA.weighted_lsq(mde[0], disp[0], conf[0])
        with pytest.raises(ops.StxError, match="does not match"):
            SA.handcrafted_mirror_detector(d2, d3, d2[..., :12].contiguous(), d3)
        with pytest.raises(ops.StxError, match="step_gain"):
            SA.handcrafted_mirror_detector(d2, d3, d2, d3, step_gain=None)


def test_c_entry_points_refuse_without_launching(be):  # noqa: F811
    """The C-ABI returns an error -- and writes nothing -- for N outside 1..64, a right row past the LDS limit, lrc_th above 20,
    no gradient at all, a backward row past its limit, a quantile outside 0..1 and 2^24 elements per image."""
    from stereo_toolbox_amd import ops
    maps = be.dev(torch.zeros(1, 1, 2, 8))
    out, wide, ws = be.empty(16), be.empty(8 * 16 * 8), be.empty(8 * 16)
    bad = [("stx_generate_masks_fwd", (ptr(maps), ptr(wide), 1, 65, 2, 8)),
           ("stx_generate_masks_fwd", (ptr(maps), ptr(wide), 1, 0, 2, 8)),
           ("stx_masked_volume_fwd", (ptr(wide), ptr(maps), ptr(maps), ptr(wide), 1, 65, 2, 8, 8)),
           ("stx_masked_volume_fwd", (ptr(wide), ptr(maps), ptr(maps), ptr(wide), 1, 2, 1, 1, 2049)),
           ("stx_masked_volume_bwd", (ptr(wide), ptr(maps), ptr(maps), ptr(wide), 1, 0, 2, 8, 8)),
           ("stx_softlrc_fwd", (ptr(maps), ptr(maps), 20.5, ptr(out), ptr(out), 1, 2, 8)),
           ("stx_softlrc_bwd", (None, None, ptr(maps), ptr(maps), 1.0, ptr(ws), ptr(out), ptr(out), 1, 2, 8)),
           ("stx_softlrc_bwd", (ptr(maps), None, ptr(maps), ptr(maps), 1.0, ptr(ws), ptr(out), ptr(out), 1, 1, 1025)),
           ("stx_weighted_lsq_fwd", (ptr(maps), ptr(maps), ptr(maps), 0.2, 1.5, ptr(out), ptr(out), ptr(ws), 1, 16)),
           ("stx_weighted_lsq_fwd", (ptr(maps), ptr(maps), ptr(maps), 0.2, 0.9, ptr(out), ptr(out), ptr(ws), 1, 1 << 24)),
           ("stx_weighted_lsq_bwd", (None, None, ptr(maps), ptr(maps), ptr(maps), ptr(ws), ptr(out), ptr(out), ptr(out), 1, 16)),
           ("stx_mirror_detector_fwd", (ptr(maps), ptr(maps), ptr(maps), ptr(maps), 0.5, 20.0, ptr(out), 0)),
           ("stx_mirror_detector_bwd", (ptr(maps), ptr(maps), ptr(maps), ptr(maps), ptr(maps), 0.5, 20.0, ptr(out), ptr(out), ptr(out),
                                        None, 16))]
    for name, args in bad:
        with pytest.raises(ops.StxError):
            be.call(name, *args)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(wide).all() and torch.isnan(ws).all()
    assert be.lib.raw("stx_softlrc_bwd_workspace_floats")(2, 3, 13) == 8 * 2 * 3 * 13
