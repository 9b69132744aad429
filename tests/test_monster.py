"""MonSter's mono / stereo mutual refinement (reference models/MonSter/monster.py:456-494, warp.py, refinement.py:403-407) on the
kernels of csrc/monster.hip, through `stereo_toolbox_amd.ops` and `stereo_toolbox_amd.models.MonSter`.

* tests/golden/monster.npz holds what the reference's OWN `disp_warp` and `compute_scale_shift` give on the seeded cases of
  tests/golden/monster_config.py, in fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| (tests/golden/make_golden_monster.py);
  of the cases too large to store whole d_ref, max|fp64| and a strided subsample of the fp64 tensor.
* A plain-torch restatement (the warp in gather form, no grid_sample; the fit with kthvalue in place of the sort) lives in this
  file and is pinned to the fixture on the CPU first -- in fp64 to 1e-11 (whole tensors or the subsample), in fp32 to 2 x d_ref.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture -- for the subsampled cases with the
  restatement evaluated in fp64 at test time: values within VALUE_FACTOR (2) x d_ref, gradients within GRAD_FACTOR (3) x d_ref,
  floor 2e-7 * max(1, max|want|) where d_ref is zero (tests/parity.within).  Every element is compared, the ratios go to the
  parity report.  The validity map, the rank threshold and the mask count must be equal.
"""
import functools
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

from tests.backends import Guards, be, ptr  # noqa: F401
from tests.golden.monster_config import (DISP_WARP_SIGNATURE, FD_CASE, FIT_CASES, FIT_SUBSAMPLED, FLAW_CASES, GPU_ONLY, GRAD_KEYS,
                                         ONE_DISPARITY, OWN_EXPORTS, REQUIRED, SHARED_WITH_IGEV, SUBSAMPLE, SUBSAMPLED, VALUE_KEYS,
                                         ZERO_DREF, check_fit_inputs, check_flaw_inputs, fit_inputs, fit_mask, flaw_inputs, subsample)
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, Env, directional, env, on, pin_fixture, pin_subsample, sync, within  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monster.npz")
PKG = "stereo_toolbox_amd.models.MonSter"
VALID_TH = 0.9999


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _ms():
    return importlib.import_module(PKG)


# ------------------------------------------------------------------------------------------ the restatement (plain torch)
def r_warp(right, disp, padding):
    """-> (warped [B,C,H,W], valid [B,1,H,W]): the four corners gathered; ix = (x - disp) W / (W - 1) - 1/2, iy = y H / (H - 1) - 1/2
    in fp64 whatever the dtype (as the kernels form them), clipped to the image under 'border', the interpolation in the dtype"""
    B, C, H, W = right.shape
    dt, f64 = right.dtype, torch.float64
    x = (torch.arange(W, dtype=f64).view(1, 1, W) - disp[:, 0].to(f64)) * (W / (W - 1)) - 0.5
    y = (torch.arange(H, dtype=f64) * (H / (H - 1)) - 0.5).view(1, H, 1).expand(B, H, W)
    if padding == "border":
        x, y = x.clamp(0, W - 1), y.clamp(0, H - 1)
    x0, y0 = torch.floor(x).detach(), torch.floor(y)
    fx, fy = (x - x0).to(dt), (y - y0).to(dt)
    flat = right.reshape(B, C, H * W)
    warped, weight = 0, 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).to(dt)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
            wgt = (wx * wy * ok).unsqueeze(1)
            warped = warped + wgt * flat.gather(2, idx).reshape(B, C, H, W)
            weight = weight + wgt
    valid = torch.ones_like(weight) if padding == "border" else (weight.detach() >= VALID_TH).to(dt)
    return warped, valid.detach()


def r_fit(mono, gt, mask):
    """one image -> (scale, shift) tensors of compute_scale_shift (monster.py:53-62), the threshold, the mask count"""
    keep, thr = fit_mask(mono, gt, mask)
    m, g = mono[keep], gt[keep]
    X = torch.stack([m, torch.ones_like(m)], dim=1)
    A = torch.matmul(X.t(), X) + 1e-6 * torch.eye(2, dtype=mono.dtype)
    p = torch.linalg.solve(A, torch.matmul(X.t(), g))
    return p[0], p[1], thr, int(keep.sum())


def _flaw_restated(tag, dtype):
    t = flaw_inputs(tag)
    padding = t.pop("padding")
    t = {k: None if v is None else v.to(dtype) for k, v in t.items()}
    left, right = t["left"].clone().requires_grad_(), t["right"].clone().requires_grad_()
    da = t["disp_a"].clone().requires_grad_()
    db = None if t["disp_b"] is None else t["disp_b"].clone().requires_grad_()
    warped, valid = r_warp(right, da, padding)
    res = {"warped_a": warped.detach(), "valid_a": valid, "flaw_a": (warped - left).detach()}
    loss = ((warped - left) * t["gw_a"]).sum()
    if db is not None:
        flaw_b = r_warp(right, db, padding)[0] - left
        res["flaw_b"] = flaw_b.detach()
        loss = loss + (flaw_b * t["gw_b"]).sum()
    if FLAW_CASES[tag][3]:
        leaves = [left, right, da] + ([db] if db is not None else [])
        grads = torch.autograd.grad(loss, leaves)
        res.update(zip(("g_left", "g_right", "g_disp_a", "g_disp_b"), (g.detach() for g in grads)))
    return res


@functools.lru_cache(maxsize=None)
def _flaw64(tag):
    return _flaw_restated(tag, torch.float64)


def _fit_restated(tag, dtype):
    mono, gt, mask, gw = fit_inputs(tag)
    mono, gt, gw = mono.to(dtype), gt.to(dtype), gw.to(dtype)
    fits = [r_fit(mono[b], gt[b], None if mask is None else mask[b]) for b in range(mono.shape[0])]
    scale, shift = torch.stack([f[0] for f in fits]), torch.stack([f[1] for f in fits])
    return {"scale": scale, "shift": shift, "aligned": scale.view(-1, 1, 1, 1) * mono + shift.view(-1, 1, 1, 1),
            "g_mono": scale.view(-1, 1, 1, 1) * gw, "thr": [float(f[2]) for f in fits], "count": [f[3] for f in fits]}


@functools.lru_cache(maxsize=None)
def _fit64(tag):
    return _fit_restated(tag, torch.float64)


def _zero_dref(tag, k):
    return "floor" if k in ZERO_DREF.get(tag, ()) else None


@pytest.mark.parametrize("tag", list(FLAW_CASES))
def test_flaw_restatement_matches_reference_fixture(gold, tag):
    check_flaw_inputs(tag)
    r64 = _flaw64(tag)
    r32 = None if tag in SUBSAMPLED else _flaw_restated(tag, torch.float32)
    assert set(VALUE_KEYS) - {"flaw_b"} <= set(r64) and (not FLAW_CASES[tag][3] or "g_right" in r64)
    for k in r64:
        key = f"flaw:{tag}:{k}"
        if k == "valid_a":
            assert torch.equal(r64[k], torch.from_numpy(gold[key]).double()), key
            assert r32 is None or torch.equal(r32[k], torch.from_numpy(gold[key]).float()), key
        elif tag in SUBSAMPLED:
            assert float(gold[key + ":dref"]) > 0, key
            pin_subsample(r64[k], torch.from_numpy(gold[key + ":sub"]), float(gold[key + ":max"]), subsample,
                          min(r64[k].numel(), SUBSAMPLE), key)
        else:
            pin_fixture(r64[k], r32[k], gold, key, zero_dref=_zero_dref(tag, k))


@pytest.mark.parametrize("tag", list(FIT_CASES))
def test_fit_restatement_matches_reference_fixture(gold, tag):
    check_fit_inputs(tag)
    r64, r32 = _fit64(tag), _fit_restated(tag, torch.float32)
    for r in (r64, r32):
        assert r["thr"] == gold[f"fit:{tag}:thr"].tolist() and r["count"] == gold[f"fit:{tag}:count"].tolist(), tag
    for k in ("scale", "shift", "aligned", "g_mono"):
        key = f"fit:{tag}:{k}"
        if tag in FIT_SUBSAMPLED and k in ("aligned", "g_mono"):
            pin_subsample(r64[k], torch.from_numpy(gold[key + ":sub"]), float(gold[key + ":max"]), subsample, SUBSAMPLE, key)
        else:
            pin_fixture(r64[k], r32[k], gold, key, zero_dref="exact" if tag == "empty" else None)


# ------------------------------------------------------------------------------------------ the product vs fp64: flaws
def _flaw_product(env, tag, wanted=("left", "right", "disp_a", "disp_b")):
    """monster_disp_warp and monster_flaws on the case's inputs, forward and backward to the `wanted` inputs -> dict of tensors
    named as in the fixture"""
    from stereo_toolbox_amd import ops
    t = flaw_inputs(tag)
    padding = t.pop("padding")
    t = {k: None if v is None else v.to(env.device) for k, v in t.items()}
    grads = FLAW_CASES[tag][3]
    leaf = {k: (t[k].clone().requires_grad_(grads and k in wanted) if t[k] is not None else None)
            for k in ("left", "right", "disp_a", "disp_b")}
    res = {}
    with env.ctx():
        warped, valid = ops.monster_disp_warp(t["right"], t["disp_a"], padding)
        assert valid.shape == warped.shape and valid.requires_grad is False
        res["warped_a"], res["valid_a"] = warped, valid[:, :1]
        out = ops.monster_flaws(leaf["left"], leaf["right"], leaf["disp_a"], leaf["disp_b"], padding)
        if leaf["disp_b"] is None:
            assert isinstance(out, torch.Tensor)
            res["flaw_a"], loss = out, (out * t["gw_a"]).sum()
        else:
            res["flaw_a"], res["flaw_b"] = out
            assert out[0].grad_fn is out[1].grad_fn or not grads          # one autograd node
            loss = (out[0] * t["gw_a"]).sum() + (out[1] * t["gw_b"]).sum()
        if grads:
            names = [k for k in ("left", "right", "disp_a", "disp_b") if leaf[k] is not None and k in wanted]
            for k, g in zip(names, torch.autograd.grad(loss, [leaf[k] for k in names])):
                res["g_" + k] = g
        sync(env)
    return {k: v.detach().cpu() for k, v in res.items()}


def _flaw_want(gold, tag, k):
    return _flaw64(tag)[k] if tag in SUBSAMPLED else torch.from_numpy(gold[f"flaw:{tag}:{k}:f64"])


def _compare_flaws(got, gold, tag, backend, parity_log, note=""):
    for k, v in got.items():
        if k == "valid_a":
            assert torch.equal(v, torch.from_numpy(gold[f"flaw:{tag}:valid_a"]).float()), (tag, k)
            continue
        factor = GRAD_FACTOR if k in GRAD_KEYS else VALUE_FACTOR
        within(v, _flaw_want(gold, tag, k), float(gold[f"flaw:{tag}:{k}:dref"]), factor, f"monster {tag} {k}{note} [{backend}]", parity_log)


@pytest.mark.parametrize("backend,tag", on(FLAW_CASES, GPU_ONLY))
def test_flaws_match_reference_fp64(backend, tag, gold, parity_log):
    """warped, the validity map, both flaws; the gradients to left, right and both disparities"""
    got = _flaw_product(Env(backend), tag)
    assert set(got) == set(_flaw64(tag)), (sorted(got), sorted(_flaw64(tag)))
    if tag == "zeros":
        share = got["valid_a"].mean().item()
        assert 0.2 < share < 0.8, share                                    # a non-trivial map
    if tag == "clipped":
        assert not got["g_disp_a"].any() and not got["g_disp_b"].any()     # exactly zero where ix is clipped
    _compare_flaws(got, gold, tag, backend, parity_log)


@pytest.mark.parametrize("backend,wanted", on((("right",), ("disp_a", "disp_b"), ("left",))))
def test_a_single_gradient_is_the_same_gradient(backend, wanted, gold, parity_log):
    """only g_right, only the disparity gradients, only g_left: the kernels skip what is not asked for and give the same bits"""
    env_ = Env(backend)
    full, part = _flaw_product(env_, "odd"), _flaw_product(env_, "odd", wanted)
    assert {k for k in part if k.startswith("g_")} == {"g_" + k for k in wanted}
    for k in part:
        assert torch.equal(part[k], full[k]), k
    _compare_flaws(part, gold, "odd", backend, parity_log, note=" alone")


@pytest.mark.parametrize("backend,tag", on(("collide", "wave96")))
def test_backward_is_bitwise_reproducible(backend, tag):
    a, b = _flaw_product(Env(backend), tag), _flaw_product(Env(backend), tag)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(a[k].abs().max().item() > 0 for k in a)


def test_unreached_cells_are_written_as_zeros(be):  # noqa: F811
    """The collision case through the C-ABI into NaN-filled, guarded buffers, twice: equal bits; g_right is non-zero in the two
    columns either disparity samples and an exact zero everywhere else (nothing is left unwritten, nothing is memset)."""
    t = flaw_inputs("collide")
    (B, C, H, W), _, _, _ = FLAW_CASES["collide"]
    g = Guards(be)
    right, da, db, ga, gb = (g.inp(t[k]) for k in ("right", "disp_a", "disp_b", "gw_a", "gw_b"))
    runs = []
    for _ in range(2):
        outs = [g.out(B, C, H, W), g.out(B, C, H, W), g.out(B, 1, H, W), g.out(B, 1, H, W)]
        be.call("stx_monster_flaw_bwd", ptr(ga), ptr(gb), ptr(right), ptr(da), ptr(db), 0, *(ptr(o) for o in outs), B, C, H, W)
        if be.name == "hip":
            torch.cuda.synchronize()
        g.check("monster_flaw_bwd")
        runs.append([o.cpu().clone() for o in outs])
    for x, y in zip(*runs):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    g_right = runs[0][1]
    hit = torch.zeros(W, dtype=torch.bool)
    hit[[6, 7, 20, 21]] = True                                             # ix = 6.987 and 20.628
    assert (g_right[..., ~hit] == 0).all() and (g_right[..., hit] != 0).all()
    only = [g.out(B, C, H, W)]
    be.call("stx_monster_flaw_bwd", ptr(ga), None, ptr(right), ptr(da), ptr(db), 0, None, ptr(only[0]), None, None, B, C, H, W)
    g.check("monster_flaw_bwd, g_right of a alone")
    assert (only[0].cpu()[..., 8:] == 0).all() and torch.isfinite(only[0]).all()


# ------------------------------------------------------------------------------------------ the product vs fp64: the fit
def _fit_product(env, tag):
    from stereo_toolbox_amd import ops
    mono, gt, mask, gw = (None if v is None else v.to(env.device) for v in fit_inputs(tag))
    with env.ctx():
        ss = ops.monster_scale_shift(mono, gt, mask)
        stats = ops.monster_fit_stats(mono, gt, mask)
        assert ss.shape == (mono.shape[0], 2) and ss.dtype == torch.float32 and ss.requires_grad is False
        x = mono.clone().requires_grad_()
        aligned = ops.monster_align(x, gt, mask)
        g_mono, = torch.autograd.grad((aligned * gw).sum(), x)
        sync(env)
    return {"scale": ss[:, 0].cpu(), "shift": ss[:, 1].cpu(), "aligned": aligned.detach().cpu(), "g_mono": g_mono.cpu(),
            "thr": stats[:, 5].cpu().tolist(), "count": [int(c) for c in stats[:, 2].cpu().tolist()]}


@pytest.mark.parametrize("backend,tag", on(FIT_CASES))
def test_fit_matches_reference_fp64(backend, tag, gold, parity_log):
    """scale, shift, the aligned map and its gradient; the rank threshold and the mask count equal to the reference's"""
    got = _fit_product(Env(backend), tag)
    assert got["thr"] == gold[f"fit:{tag}:thr"].tolist() and got["count"] == gold[f"fit:{tag}:count"].tolist(), (got["thr"], got["count"])
    if tag == "empty":
        assert got["count"] == [0] and not got["scale"].any() and not got["shift"].any()       # exactly (0, 0)
    for k in ("scale", "shift", "aligned", "g_mono"):
        key = f"fit:{tag}:{k}"
        want = _fit64(tag)[k] if tag in FIT_SUBSAMPLED and k in ("aligned", "g_mono") else torch.from_numpy(gold[key + ":f64"])
        within(got[k], want, float(gold[key + ":dref"]), GRAD_FACTOR if k == "g_mono" else VALUE_FACTOR,
               f"monster fit {tag} {k} [{backend}]", parity_log)


@pytest.mark.parametrize("backend,tag", on(("n222", "mask")))
def test_compute_scale_shift_returns_the_references_floats(backend, tag, gold, parity_log):
    MS, env_ = _ms(), Env(backend)
    mono, gt, mask, _ = (None if v is None else v.to(env_.device) for v in fit_inputs(tag))
    with env_.ctx():
        got = [MS.compute_scale_shift(mono[b].squeeze(1), gt[b].squeeze(1), None if mask is None else mask[b].squeeze(1))
               for b in range(mono.shape[0])]
    assert all(isinstance(v, float) for pair in got for v in pair)
    for i, k in enumerate(("scale", "shift")):
        within(torch.tensor([pair[i] for pair in got]), torch.from_numpy(gold[f"fit:{tag}:{k}:f64"]), float(gold[f"fit:{tag}:{k}:dref"]),
               VALUE_FACTOR, f"monster compute_scale_shift {tag} {k} [{backend}]", parity_log)


def test_model_entry_points_are_the_ops(env):  # noqa: F811
    """align_mono_disp, mutual_flaws, refinement_flaws and disp_warp give the bits of the ops they wrap"""
    from stereo_toolbox_amd import ops
    MS = _ms()
    t = {k: v.to(env.device) if isinstance(v, torch.Tensor) else v for k, v in flaw_inputs("odd").items()}
    mono, gt, _, _ = (None if v is None else v.to(env.device) for v in fit_inputs("b3"))
    with env.ctx():
        fa, fb = ops.monster_flaws(t["left"], t["right"], t["disp_a"], t["disp_b"])
        stereo, mono_flaw = MS.mutual_flaws(t["left"], t["right"], t["disp_a"], t["disp_b"])
        assert torch.equal(stereo, fa) and torch.equal(mono_flaw, fb)
        rm, rs = MS.refinement_flaws(t["left"], t["right"], t["disp_b"], t["disp_a"])
        assert torch.equal(rm, fb) and torch.equal(rs, fa)
        for mode in ("border", "zeros"):
            for a, b in zip(MS.disp_warp(t["right"], t["disp_a"], mode), ops.monster_disp_warp(t["right"], t["disp_a"], mode)):
                assert torch.equal(a, b)
        assert torch.equal(MS.align_mono_disp(mono, gt), ops.monster_align(mono, gt))
        half = ops.monster_flaws(t["left"].half(), t["right"].half(), t["disp_a"].half())
        assert half.dtype == torch.float16                                 # cast up, returned in the map's dtype


# ------------------------------------------------------------------------------------------ finite differences (emulator)
def test_finite_difference_gradients():
    """Directional derivatives through the product host code on the emulator.  The disparity steps (1e-3 of the mean |disp|, a few
    thousandths of a pixel) stay inside the 0.05 px the inputs keep from the bilinear kinks."""
    from stereo_toolbox_amd import ops
    from tests.emu_util import emu_product_path
    t = flaw_inputs(FD_CASE)
    mono, gt, _, _ = fit_inputs("b3")
    with emu_product_path():
        directional(lambda l, r: list(ops.monster_flaws(l, r, t["disp_a"], t["disp_b"])), [t["left"], t["right"]], seed=31)
        directional(lambda a, b: list(ops.monster_flaws(t["left"], t["right"], a, b)), [t["disp_a"], t["disp_b"]], eps=1e-3, seed=32)
        directional(lambda r, a: ops.monster_flaws(t["left"], r, a), [t["right"], t["disp_a"]], eps=1e-3, seed=33)
        z = flaw_inputs("zeros")
        directional(lambda r, a: ops.monster_flaws(z["left"], r, a, None, "zeros"), [z["right"], z["disp_a"]], eps=1e-3, seed=34)
        # monster_align for mono: the fit is a constant of the graph (the reference reads it with .item()), so the derivative is
        # taken with the fit of the unperturbed mono held fixed -- the node monster_align builds, and its gradient must be that one
        ss = ops.monster_scale_shift(mono, gt)
        directional(lambda m: ops.MonsterApplyFn.apply(m, ss), [mono], seed=35)
        x, gy = mono.clone().requires_grad_(), torch.randn(mono.shape, generator=torch.Generator().manual_seed(36))
        g_align, = torch.autograd.grad((ops.monster_align(x, gt) * gy).sum(), x)
        g_fixed, = torch.autograd.grad((ops.MonsterApplyFn.apply(x, ss) * gy).sum(), x)
        assert torch.equal(g_align, g_fixed) and g_align.abs().max() > 0


# ------------------------------------------------------------------------------------------ no host synchronisation (GPU)
@pytest.mark.gpu
def test_no_host_synchronisation():
    """align_mono_disp, mutual_flaws (forward and backward) and monster_scale_shift with B = 3 under torch's sync debug mode
    "error"."""
    from stereo_toolbox_amd import ops
    MS, env_ = _ms(), Env("hip")
    mono, gt, _, _ = (None if v is None else v.to(env_.device) for v in fit_inputs("b3"))
    t = {k: v.to(env_.device) for k, v in flaw_inputs("odd").items() if isinstance(v, torch.Tensor)}
    leaves = [t[k].clone().requires_grad_() for k in ("left", "right", "disp_a", "disp_b")]
    x = mono.clone().requires_grad_()
    MS.align_mono_disp(x, gt)                                              # (first use loads the library)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        aligned = MS.align_mono_disp(x, gt)
        aligned.sum().backward()
        stereo, mono_flaw = MS.mutual_flaws(*leaves)
        ((stereo * t["gw_a"]).sum() + (mono_flaw * t["gw_b"]).sum()).backward()
        ss = ops.monster_scale_shift(mono, gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert ss.shape == (3, 2) and torch.isfinite(x.grad).all() and all(torch.isfinite(v.grad).all() for v in leaves)


# ------------------------------------------------------------------------------------------ surface, refusals
def test_public_surface():
    MS = _ms()
    igev = importlib.import_module("stereo_toolbox_amd.models.IGEVStereo")
    assert importlib.import_module("stereo_toolbox_amd.models").MonSter is MS
    for name in OWN_EXPORTS:
        assert callable(getattr(MS, name)), name
    for name in SHARED_WITH_IGEV:
        assert getattr(MS, name) is getattr(igev, name), name
    sig = inspect.signature(MS.disp_warp)
    got = tuple((p.name, REQUIRED if p.default is inspect.Parameter.empty else p.default) for p in sig.parameters.values())
    assert got == DISP_WARP_SIGNATURE, got
    assert tuple(inspect.signature(MS.compute_scale_shift).parameters) == ("monocular_depth", "gt_depth", "mask")


def test_cpu_tensors_are_refused():
    from stereo_toolbox_amd import ops
    MS = _ms()
    t = flaw_inputs("single")
    mono, gt, _, _ = fit_inputs("n222")
    for call in (lambda: ops.monster_flaws(t["left"], t["right"], t["disp_a"]), lambda: MS.disp_warp(t["right"], t["disp_a"]),
                 lambda: ops.monster_scale_shift(mono, gt), lambda: MS.align_mono_disp(mono, gt),
                 lambda: MS.compute_scale_shift(mono[0], gt[0])):
        with pytest.raises(ops.StxError, match="ROCm device"):
            call()


def test_unsupported_arguments_are_refused(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    t = {k: v.to(env.device) if isinstance(v, torch.Tensor) else v for k, v in flaw_inputs("odd").items()}
    left, right, da, db = t["left"], t["right"], t["disp_a"], t["disp_b"]
    mono, gt, _, _ = (None if v is None else v.to(env.device) for v in fit_inputs("n222"))
    with env.ctx():
        for img, d in ((right[:, :, :1], da[:, :, :1]), (right[..., :1], da[..., :1])):                # H or W of 1
            with pytest.raises(ops.StxError, match="H, W >= 2"):
                ops.monster_flaws(img, img, d)
            with pytest.raises(ops.StxError, match="H, W >= 2"):
                ops.monster_disp_warp(img, d)
        with pytest.raises(ops.StxError, match="does not match"):
            ops.monster_flaws(left[:, :3], right, da)
        with pytest.raises(ops.StxError, match="disp_b must be"):
            ops.monster_flaws(left, right, da, db[:, :, :5])
        with pytest.raises(ops.StxError, match="disp must be"):
            ops.monster_disp_warp(right, da[:, 0])
        with pytest.raises(ops.StxError, match="padding_mode"):
            ops.monster_flaws(left, right, da, db, "reflection")
        with pytest.raises(ops.StxError, match="does not match"):
            ops.monster_scale_shift(mono, gt[..., :30])
        with pytest.raises(ops.StxError, match="bool"):
            ops.monster_scale_shift(mono, gt, torch.ones_like(mono))
        huge = torch.zeros(1, device=env.device).expand(1, 1, 4096, 4096)                                # 2^24, nothing allocated
        for call in (lambda: ops.monster_scale_shift(huge, huge), lambda: ops.monster_align(huge, huge)):
            with pytest.raises(ops.StxError, match="2\\^24"):
                call()


def test_c_entry_points_refuse_without_launching(be):  # noqa: F811
    """The C-ABI returns an error -- and writes nothing -- for H or W of 1, disp_b without its output, a gradient to the sampled
    map past its width limit, no gradient at all, 2^24 elements per image and a rank outside the image."""
    from stereo_toolbox_amd import ops
    img = be.dev(torch.zeros(1, 1, 2, 8))
    out, st = be.empty(64), be.empty(8, dtype=torch.float64)
    bad = [("stx_monster_flaw_fwd", (ptr(img), ptr(img), ptr(img), None, 0, ptr(out), None, None, 1, 1, 1, 16)),
           ("stx_monster_flaw_fwd", (ptr(img), ptr(img), ptr(img), None, 0, ptr(out), None, None, 1, 1, 16, 1)),
           ("stx_monster_flaw_fwd", (ptr(img), ptr(img), ptr(img), ptr(img), 0, ptr(out), None, None, 1, 1, 2, 8)),
           ("stx_monster_flaw_bwd", (ptr(img), None, ptr(img), ptr(img), None, 0, None, ptr(out), None, None, 1, 1, 2, 2049)),
           ("stx_monster_flaw_bwd", (ptr(img), None, ptr(img), ptr(img), None, 0, None, None, None, None, 1, 1, 2, 8)),
           ("stx_monster_flaw_bwd", (None, None, ptr(img), ptr(img), None, 0, ptr(out), None, None, None, 1, 1, 2, 8)),
           ("stx_monster_scale_shift", (ptr(img), ptr(img), None, 3, ptr(out), ptr(st), 1, 1 << 24)),
           ("stx_monster_scale_shift", (ptr(img), ptr(img), None, 16, ptr(out), ptr(st), 1, 16)),
           ("stx_monster_scale_shift", (ptr(img), ptr(img), None, -1, ptr(out), ptr(st), 1, 16)),
           ("stx_monster_apply_scale_shift", (ptr(img), ptr(img), 1, ptr(out), 1, 1 << 24))]
    for name, args in bad:
        with pytest.raises(ops.StxError):
            be.call(name, *args)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(out).all()
