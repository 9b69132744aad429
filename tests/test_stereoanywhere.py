"""StereoAnywhere's volume stage (reference models/StereoAnywhere/corr.py:75-132, utils/utils.py:112-170, 216-238) on the kernels
of csrc/allpairs.hip: the four estimates regressed from the all-pairs volume, the volume-in `CorrBlock1D` and the truncation mask.

* tests/golden/stereoanywhere.npz holds what the reference's OWN functions give on the seeded cases of
  tests/golden/stereoanywhere_config.py, in fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| > 0
  (tests/golden/make_golden_stereoanywhere.py).  The volume gradients of the larger estimator cases keep d_ref, max|fp64| and a
  strided subsample of the fp64 tensor.
* A plain-torch restatement lives in this file (the truncation mask, shared with tests/test_mono_align.py, in tests/restated.py) and
  is pinned to the fixture on the CPU first -- in fp64 to 1e-11 (whole tensors or the subsample), in fp32 to 2 x d_ref -- so the
  fixture and the restatement check each other.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture -- for the subsampled tensors with the
  restatement evaluated in fp64 at test time: values within VALUE_FACTOR (2) x d_ref, gradients within GRAD_FACTOR (3) x d_ref,
  floor 2e-7 * max(1, max|want|) where d_ref is zero (the rule of tests/parity.within).  Every element of every tensor is
  compared and the achieved ratios go to the parity report.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.backends import be, ptr  # noqa: F401
from tests.golden.stereoanywhere_config import (ATTENUATION, BLOCK_CASES, EST_CASES, EST_GPU_ONLY, EST_WHOLE, MASK_THRESHOLDS, OUTPUTS,
                                                SUBSAMPLE, block_inputs, block_out_width, est_inputs, mask_inputs, subsample)
from tests.parity import EPS, GRAD_FACTOR, VALUE_FACTOR, Env, env, near, on, pin_fixture, pin_subsample, sync, within, within_fixture  # noqa: F401
from tests.restated import _pack, estimates, pool, sample, truncation_mask

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereoanywhere.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------------------------------ the restatement (plain torch)
def block_pyramid(vol, maps, L):
    v = vol.squeeze(3)
    if maps is not None:
        v = truncation_mask(maps[0].to(vol.dtype), maps[1].to(vol.dtype), None, ATTENUATION)[:, 0].detach() * v
    cp = [v]
    for _ in range(L - 1):
        cp.append(pool(cp[-1]))
    return cp


def block_lookup(cp, coords, r, pad):
    B, _, H, W1 = coords.shape
    dx = torch.arange(-r, r + 1, dtype=coords.dtype)
    x = coords[:, 0].reshape(B, H, W1, 1) + pad[0]
    out = torch.cat([sample(c, x / 2 ** i + dx) for i, c in enumerate(cp)], dim=-1)
    return out[:, :, pad[0]:W1 - pad[1]].permute(0, 3, 1, 2).contiguous()


def _restated_est(tag, dtype):
    vol, gws = est_inputs(tag)
    res = {}
    for only in (None, 0, 1, 2, 3):
        v = vol.to(dtype).clone().requires_grad_()
        outs = estimates(v)
        sum((o * g.to(dtype)).sum() for i, (o, g) in enumerate(zip(outs, gws)) if only is None or only == i).backward()
        if only is None:
            res.update({k: o.detach() for k, o in zip(OUTPUTS, outs)})
        res["g_all" if only is None else "g_" + OUTPUTS[only]] = v.grad
    return res


@functools.lru_cache(maxsize=2)
def _restated_est64(tag):
    return _restated_est(tag, torch.float64)


def _restated_block(tag, dtype):
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES[tag]
    vol, maps, coords, gws, wc = block_inputs(tag)
    v = vol.to(dtype).clone().requires_grad_()
    cp = block_pyramid(v, maps, L)
    outs = [block_lookup(cp, c.to(dtype), r, pad) for c in coords]
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws)) + sum((c * w.to(dtype)).sum() for c, w in zip(cp, wc))
    loss.backward()
    return {"outs": torch.stack(outs).detach(), "g_fullcorr": v.grad}


def _pin(gold, key, r64, r32):
    if key + ":f64" in gold:
        pin_fixture(r64, r32, gold, key)
    else:
        assert float(gold[key + ":dref"]) > 0, key
        pin_subsample(r64, torch.from_numpy(gold[key + ":sub"]), float(gold[key + ":max"]), subsample, min(r64.numel(), SUBSAMPLE), key)


@pytest.mark.parametrize("tag", list(EST_CASES))
def test_estimator_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated_est64(tag), _restated_est(tag, torch.float32)
    assert len(r64) == 9
    for k in r64:
        _pin(gold, f"est:{tag}:{k}", r64[k], r32[k])


@pytest.mark.parametrize("tag", list(BLOCK_CASES))
def test_block_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated_block(tag, torch.float64), _restated_block(tag, torch.float32)
    for k in r64:
        _pin(gold, f"block:{tag}:{k}", r64[k], r32[k])


@pytest.mark.parametrize("name", list(MASK_THRESHOLDS))
def test_mask_restatement_matches_reference_fixture(gold, name):
    disp, conf = mask_inputs()
    th = MASK_THRESHOLDS[name]
    _pin(gold, f"mask:{name}", truncation_mask(disp.double(), conf.double(), th, ATTENUATION), truncation_mask(disp, conf, th, ATTENUATION))


# ------------------------------------------------------------------------------------------ the estimates vs fp64
def _want(gold, tag, k):
    key = f"est:{tag}:{k}"
    want = torch.from_numpy(gold[key + ":f64"]) if key + ":f64" in gold else _restated_est64(tag)[k]
    return want, float(gold[key + ":dref"])


def _estimates_together(env, tag, only=None):
    """estimate_all, the loss on all four outputs or on output `only` alone -> (outputs, volume gradient)"""
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    vol, gws = est_inputs(tag)
    v = vol.to(env.device).requires_grad_()
    with env.ctx():
        outs = SA.estimate_all(v)
        sum((o * g.to(env.device)).sum() for i, (o, g) in enumerate(zip(outs, gws)) if only is None or only == i).backward()
        sync(env)
    return outs, v.grad


def _estimate_alone(env, tag, i):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    fn = (SA.estimate_left_disparity, SA.estimate_left_confidence, SA.estimate_right_disparity, SA.estimate_right_confidence)[i]
    vol, gws = est_inputs(tag)
    v = vol.to(env.device).requires_grad_()
    with env.ctx():
        out = fn(v)
        (out * gws[i].to(env.device)).sum().backward()
        sync(env)
    return out, v.grad


@pytest.mark.parametrize("backend,tag", on(EST_CASES, EST_GPU_ONLY))
def test_estimates_match_reference_fp64(backend, tag, gold, parity_log):
    """All four outputs from one call and each asked for alone (bitwise the same), the volume gradient of the summed loss and of
    each output's loss alone -- fed alone to the four-output node and through the single-output call (bitwise the same)."""
    env = Env(backend)
    B, H, W1, W2, s = EST_CASES[tag]
    outs, g_all = _estimates_together(env, tag)
    for i, k in enumerate(OUTPUTS):
        assert outs[i].shape == (B, 1, H, W2 if i >= 2 else W1) and outs[i].dtype == torch.float32
        within(outs[i], *_want(gold, tag, k), VALUE_FACTOR, f"stereoanywhere {tag} {k} [{backend}]", parity_log)
    assert g_all.shape == (B, 1, H, W1, W2)
    within(g_all, *_want(gold, tag, "g_all"), GRAD_FACTOR, f"stereoanywhere {tag} g_all [{backend}]", parity_log)
    for i, k in enumerate(OUTPUTS):
        alone, g_alone = _estimate_alone(env, tag, i)
        assert torch.equal(alone, outs[i]), k
        _, g_fed = _estimates_together(env, tag, only=i)
        assert torch.equal(g_fed, g_alone), k
        within(g_alone, *_want(gold, tag, "g_" + k), GRAD_FACTOR, f"stereoanywhere {tag} g_{k} [{backend}]", parity_log)


def test_vol_pad_crops_the_disparities(env):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    vol, _ = est_inputs("b2_13")
    with env.ctx():
        v = vol.to(env.device)
        full = SA.estimate_all(v)
        assert torch.equal(SA.estimate_left_disparity(v, vol_pad=[2, 1]), full[0][:, :, :, 2:12])
        assert torch.equal(SA.estimate_right_disparity(v, vol_pad=[2, 1]), full[2][:, :, :, 2:12])
        assert torch.equal(SA.estimate_all(v[:, 0])[3], full[3]) and full[0].requires_grad is False


def test_estimates_are_bitwise_reproducible(env):
    a_out, a_g = _estimates_together(env, "px37")
    b_out, b_g = _estimates_together(env, "px37")
    assert all(torch.equal(a, b) for a, b in zip(a_out, b_out))
    assert torch.equal(a_g, b_g) and a_g.abs().max().item() > 0


# ------------------------------------------------------------------------------------------ the block vs fp64
def _block_case(env, tag, fused=True, cls=None, retain=False):
    """Three lookups on one object plus a weighted sum of the public pyramid; `fused`: truncate= instead of mask * volume."""
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES[tag]
    vol, maps, coords, gws, wc = block_inputs(tag)
    dev = env.device
    v = vol.to(dev).requires_grad_()
    with env.ctx():
        full, kw = v, {}
        if trunc and fused:
            kw = {"truncate": (maps[0].to(dev), maps[1].to(dev), ATTENUATION)}
        elif trunc:
            mask = SA.truncate_corr_volume_v2(maps[0].to(dev), maps[1].to(dev), conf_th=None, attenuation_gain=ATTENUATION)
            full = (mask[:, 0] * v.squeeze(3)).unsqueeze(3)
        fn = (cls or SA.CorrBlock1D)(full, num_levels=L, radius=r, pad=list(pad), **kw)
        outs = [fn(c.to(dev)) for c in coords]
        loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, gws)) + (fn.corr_pyramid * _pack(wc).to(dev)).sum()
        loss.backward(retain_graph=retain)
        sync(env)
    return outs, v, loss


def _check_block(env, gold, log, tag, outs, grad, how=""):
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES[tag]
    for o in outs:
        assert o.shape == (B, L * (2 * r + 1), H, block_out_width(tag)) and o.dtype == torch.float32 and o.is_contiguous()
    for k, got, factor in (("outs", torch.stack(outs), VALUE_FACTOR), ("g_fullcorr", grad, GRAD_FACTOR)):
        within_fixture(got, gold, f"block:{tag}:{k}", factor, f"stereoanywhere block {tag}{how} {k} [{env.name}]", log)


@pytest.mark.parametrize("tag", list(BLOCK_CASES))
def test_block_matches_reference_fp64(env, gold, parity_log, tag):
    outs, v, _ = _block_case(env, tag)
    _check_block(env, gold, parity_log, tag, outs, v.grad)


def test_truncate_keyword_equals_mask_times_volume(env, gold, parity_log):
    """`truncate=` against the same reference tensors as the mask volume multiplied in by the caller."""
    outs, v, _ = _block_case(env, "trunc_pad", fused=False)
    _check_block(env, gold, parity_log, "trunc_pad", outs, v.grad, " mask*volume")


def test_fast_block_is_the_same_object_and_static_corr(env):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    a_out, a_v, _ = _block_case(env, "l4_r4")
    b_out, b_v, _ = _block_case(env, "l4_r4", cls=SA.CorrBlockFast1D)
    assert all(torch.equal(a, b) for a, b in zip(a_out, b_out)) and torch.equal(a_v.grad, b_v.grad)
    from stereo_toolbox_amd.utils import synthetic_tensor
    n2, n3 = synthetic_tensor((2, 3, 4, 19), 3501), synthetic_tensor((2, 3, 4, 23), 3502)     # the model's 3-channel normals
    with env.ctx():
        corr = SA.CorrBlock1D.corr(n2.to(env.device), n3.to(env.device))
    assert corr.shape == (2, 4, 19, 1, 23) and corr.dtype == torch.float32
    want = torch.einsum("aijk,aijh->ajkh", n2.double(), n3.double()).unsqueeze(3) / math.sqrt(3.0)
    near(corr, want, 3 * EPS, "static corr")


def test_block_is_bitwise_reproducible_and_second_backward_equals_the_first(env):
    a_out, a_v, loss = _block_case(env, "trunc_pad", retain=True)
    b_out, b_v, _ = _block_case(env, "trunc_pad")
    assert all(torch.equal(a, b) for a, b in zip(a_out, b_out))
    assert torch.equal(a_v.grad, b_v.grad) and a_v.grad.abs().max().item() > 0
    first, a_v.grad = a_v.grad.clone(), None
    with env.ctx():
        loss.backward()
        sync(env)
    assert torch.equal(first, a_v.grad)


@pytest.mark.parametrize("name", list(MASK_THRESHOLDS))
def test_truncation_mask_matches_reference_fp64(env, gold, parity_log, name):
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    disp, conf = mask_inputs()
    with env.ctx():
        mask = SA.truncate_corr_volume_v2(disp.to(env.device), conf.to(env.device), conf_th=MASK_THRESHOLDS[name],
                                          attenuation_gain=ATTENUATION)
    key = f"mask:{name}"
    assert mask.shape == tuple(gold[key + ":f64"].shape) and mask.dtype == torch.float32
    within_fixture(mask, gold, key, VALUE_FACTOR, f"stereoanywhere {name} [{env.name}]", parity_log)


# ------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_are_refused():
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    vol, _ = est_inputs("b2_13")
    disp, conf = mask_inputs()
    for call in (lambda: SA.estimate_all(vol), lambda: SA.estimate_left_confidence(vol), lambda: SA.truncate_corr_volume_v2(disp, conf),
                 lambda: SA.CorrBlock1D(block_inputs("l4_r4")[0]), lambda: ops.corr1d_volume_pyramid(block_inputs("l4_r4")[0], 2)):
        with pytest.raises(ops.StxError, match="ROCm device"):
            call()


def test_unsupported_arguments_are_refused(env):
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models import StereoAnywhere as SA
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES["l4_r4"]
    vol, _, coords, _, _ = block_inputs("l4_r4")
    dev = env.device
    vol, c0 = vol.to(dev), coords[0].to(dev)
    with env.ctx():
        fn = SA.CorrBlock1D(vol.clone().requires_grad_(), num_levels=L, radius=r)
        with pytest.raises(ops.StxError, match="detach"):
            fn(c0.clone().requires_grad_())
        assert fn(c0.clone().requires_grad_().detach()).shape == (B, L * (2 * r + 1), H, W1)
        with pytest.raises(ops.StxError, match="coords"):
            fn(c0[0])
        with pytest.raises(ops.StxError, match="fullcorr"):                                  # wrong rank
            SA.CorrBlock1D(vol.squeeze(3))
        with pytest.raises(ops.StxError):
            SA.CorrBlock1D(vol, num_levels=5)
        with pytest.raises(ops.StxError, match="radius"):
            SA.CorrBlock1D(vol, radius=9)(c0)
        with pytest.raises(ops.StxError, match="shorter than 2"):
            SA.CorrBlock1D(vol[..., :7].contiguous(), num_levels=4)                         # 7 -> 3 -> 1
        with pytest.raises(ops.StxError, match="truncate"):
            SA.CorrBlock1D(vol, truncate=(torch.zeros(B, 1, H, W1 + 1, device=dev), torch.zeros(B, 1, H, W1 + 1, device=dev), 0.1))
        with pytest.raises(ops.StxError, match="volume must be"):                            # wrong rank
            SA.estimate_all(torch.zeros(2, 3, 8, device=dev))
        with pytest.raises(ops.StxError, match="volume must be"):
            SA.estimate_all(torch.zeros(1, 2, 3, 8, 8, device=dev))
        for shape in ((1, 1, 1, 513, 8), (1, 1, 1, 8, 513), (1, 1, 1, 1, 8), (1, 1, 1, 8, 1)):
            with pytest.raises(ops.StxError, match="supported"):
                SA.estimate_all(torch.zeros(shape, device=dev))
        with pytest.raises(ops.StxError, match="which"):
            ops.allpairs_estimates(torch.zeros(1, 1, 1, 8, 8, device=dev), 16)
        with pytest.raises(ops.StxError, match=r"\[B, 1, H, W\]"):
            SA.truncate_corr_volume_v2(torch.zeros(1, 2, 8, device=dev), torch.zeros(1, 2, 8, device=dev))
        assert SA.estimate_all(torch.zeros(1, 1, 1, 512, 3, device=dev))[2].shape == (1, 1, 1, 3)


def test_c_entry_points_refuse_without_launching(be):  # noqa: F811
    """The C-ABI returns an error -- and writes nothing -- for a width past the limit, outputs that do not match `which`, no
    gradient at all, a last level shorter than 2 and a lone truncation map."""
    from stereo_toolbox_amd import ops
    vol = be.dev(torch.zeros(1, 1, 8, 8))
    out, stats, gvol = be.empty(8), be.empty(4 * 16), be.empty(64)
    wide = be.dev(torch.zeros(1, 1, 2, 513))
    bad = [("stx_allpairs_estimates_fwd", (ptr(wide), 1, ptr(out), None, None, None, None, 1, 1, 2, 513)),
           ("stx_allpairs_estimates_fwd", (ptr(vol), 3, ptr(out), None, None, None, None, 1, 1, 8, 8)),
           ("stx_allpairs_estimates_fwd", (ptr(vol), 0, None, None, None, None, None, 1, 1, 8, 8)),
           ("stx_allpairs_estimates_bwd", (None, None, None, None, ptr(vol), ptr(stats), ptr(gvol), 1, 1, 8, 8)),
           ("stx_corr1d_volume_pyramid_fwd", (ptr(vol), None, None, 0.1, ptr(gvol), 1, 1, 8, 8, 4)),
           ("stx_corr1d_volume_pyramid_fwd", (ptr(vol), ptr(out), None, 0.1, ptr(gvol), 1, 1, 8, 8, 1)),
           ("stx_corr1d_volume_pyramid_bwd", (ptr(vol), None, None, 0.1, ptr(gvol), 1, 1, 8, 8, 5))]
    for name, args in bad:
        with pytest.raises(ops.StxError):
            be.call(name, *args)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(stats).all() and torch.isnan(gvol).all()
