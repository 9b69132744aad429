"""The self-supervised losses (reference loss_functions/photometric_loss.py, auto_mask.py, smoothness_loss.py) on the kernels of
csrc/selfsup_loss.hip, through `stereo_toolbox_amd.loss_functions`.

* tests/golden/selfsup_loss.npz holds what the reference's OWN functions give on the seeded cases of
  tests/golden/selfsup_config.py, in fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| > 0
  (tests/golden/make_golden_selfsup.py); of the GPU-only case d_ref, max|fp64| and a strided subsample of the fp64 tensor.
* A plain-torch restatement (gather form, no grid_sample) lives in this file and is pinned to the fixture on the CPU first -- in
  fp64 to 1e-11 (whole tensors or the subsample), in fp32 to 2 x d_ref -- so the fixture and the restatement check each other.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture -- for the GPU-only case with the
  restatement evaluated in fp64 at test time: values within VALUE_FACTOR (2) x d_ref, gradients within GRAD_FACTOR (3) x d_ref,
  floor 2e-7 * max(1, max|want|) where d_ref is zero (the rule of tests/parity.within).  Every element of every tensor
  is compared and the achieved ratios go to the parity report.
* auto_mask: the product's bool map against the fp64 one; a pixel may be skipped only where the fp64 errors are within 1e-5 of
  each other, at most 1 % of a case; both outcomes must hold at least 5 % of the fp64 map.
"""
import functools
import importlib
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.backends import be, ptr  # noqa: F401
from tests.golden.selfsup_config import (AUTO_MASK_CASES, AUTO_MASK_DENORM, AUTO_MASK_MARGIN, AUTO_MASK_MAX_SKIPPED,
                                         AUTO_MASK_MIN_SHARE, CASES, FD_SHAPE, GPU_ONLY, PACKAGE_EXPORTS, REQUIRED, SSIM_WEIGHT,
                                         SSIM_WINDOW_CASES, SUBSAMPLE, SURFACE, fd_inputs, inputs, normalised, subsample)
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, Env, directional, env, on, pin_fixture, pin_subsample, sync, within  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selfsup_loss.npz")
PKG = "stereo_toolbox_amd.loss_functions"
C1, C2 = 0.01 ** 2, 0.03 ** 2


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _mods():
    return (importlib.import_module(PKG + ".photometric_loss"), importlib.import_module(PKG + ".auto_mask"),
            importlib.import_module(PKG + ".smoothness_loss"))


# ------------------------------------------------------------------------------------------ the restatement (plain torch)
def r_warp(right, disp):
    """-> (warped [B,C,H,W], valid [B,1,H,W]): the four corners gathered, zero outside; x = (w - disp) W / (W - 1) - 1/2,
    y = h H / (H - 1) - 1/2 -- what a linspace(0, 1) grid means to grid_sample(align_corners=False)"""
    B, C, H, W = right.shape
    dt = right.dtype
    f64 = torch.float64                  # the coordinate in fp64 whatever the dtype (as the kernels form it), the interpolation in dt
    x = (torch.arange(W, dtype=f64).view(1, 1, W) - disp[:, 0].to(f64)) * (W / (W - 1)) - 0.5
    y = (torch.arange(H, dtype=f64) * (H / (H - 1)) - 0.5).view(1, H, 1).expand(B, H, W)
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = (x - x0).to(dt), (y - y0).to(dt)
    flat = right.reshape(B, C, H * W)
    warped, valid = 0, 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).to(dt)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
            wgt = (wx * wy * ok).unsqueeze(1)
            warped = warped + wgt * flat.gather(2, idx).reshape(B, C, H, W)
            valid = valid + wgt
    return warped, valid.detach()


def r_box(t, ws):
    p = ws // 2
    return F.avg_pool2d(F.pad(t, (p, p, p, p), mode="reflect"), ws, stride=1)


def r_ssim(x, y, ws=7):
    mx, my = r_box(x, ws), r_box(y, ws)
    vx, vy, cxy = r_box(x * x, ws) - mx * mx, r_box(y * y, ws) - my * my, r_box(x * y, ws) - mx * my
    s = (2 * mx * my + C1) * (2 * cxy + C2) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return ((1 - s) / 2).clamp(0, 1)


def r_photo(left, right, disp=None, weight=SSIM_WEIGHT, mask=True):
    warped, valid = (right, None) if disp is None else r_warp(right, disp)
    loss = weight * r_ssim(left, warped) + (1 - weight) * (left - warped).abs()
    if mask:
        loss = loss * valid
    return loss.mean(1, keepdim=True)


def r_smooth(disp, img):
    n = disp / (disp.mean((2, 3), keepdim=True) + 1e-7)
    wx = torch.exp(-(img[..., :-1] - img[..., 1:]).abs().mean(1, keepdim=True))
    wy = torch.exp(-(img[..., :-1, :] - img[..., 1:, :]).abs().mean(1, keepdim=True))
    return ((n[..., :-1] - n[..., 1:]).abs() * wx).mean() + ((n[..., :-1, :] - n[..., 1:, :]).abs() * wy).mean()


def _grad(out, weight, *leaves):
    grads = torch.autograd.grad((out * weight).sum(), leaves)
    return [g.detach() for g in grads]


def _windows(tag):
    return (7,) + SSIM_WINDOW_CASES.get(tag, ())


def _restated(tag, dtype):
    t = {k: v.to(dtype) for k, v in inputs(tag).items()}
    left, right = t["left"], t["right"]
    res = {}
    disp = t["disp"].clone().requires_grad_()
    warped, valid = r_warp(right, disp)
    res["warped"], res["valid"] = warped.detach(), valid
    res["g_warp"], = _grad(warped, t["gw_c"], disp)
    for ws in _windows(tag):
        x, y = left.clone().requires_grad_(), right.clone().requires_grad_()
        s = r_ssim(x, y, ws)
        res[f"ssim{ws}"] = s.detach()
        res[f"g_ssim{ws}_x"], res[f"g_ssim{ws}_y"] = _grad(s, t["gw_c"], x, y)
    for name, on in (("photo_mask", True), ("photo_nomask", False)):
        out = r_photo(left, right, disp, mask=on)
        res[name] = out.detach()
        res["g_" + name], = _grad(out, t["gw_1"], disp)
    res["photo_none"] = r_photo(left, right, mask=False)
    sdisp = t["sdisp"].clone().requires_grad_()
    loss = r_smooth(sdisp, left)
    res["smooth"] = loss.detach()
    res["g_smooth"], = torch.autograd.grad(loss, sdisp)
    if tag in AUTO_MASK_DENORM:
        mean = torch.tensor([0.485, 0.456, 0.406], dtype=dtype).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225], dtype=dtype).view(1, 3, 1, 1)
        ln, rn = normalised(inputs(tag)["left"]).to(dtype) * std + mean, normalised(inputs(tag)["right"]).to(dtype) * std + mean
        res["dn_reproj"], res["dn_ident"] = r_photo(ln, rn, t["disp"], mask=False), r_photo(ln, rn, mask=False)
    return res


@functools.lru_cache(maxsize=None)
def _restated64(tag):
    return _restated(tag, torch.float64)


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated64(tag), _restated(tag, torch.float32)
    assert len(r64) >= 13
    for k in r64:
        key = f"{tag}:{k}"
        if tag in GPU_ONLY:
            assert float(gold[key + ":dref"]) > 0, key
            pin_subsample(r64[k], torch.from_numpy(gold[key + ":sub"]), float(gold[key + ":max"]), subsample,
                          min(r64[k].numel(), SUBSAMPLE), key)
        else:
            pin_fixture(r64[k], r32[k], gold, key)


# ------------------------------------------------------------------------------------------ the product vs fp64
def _product(env, tag):
    """Every function of the package on the case's inputs, forward and backward -> dict of tensors named as in the fixture."""
    P, _, S = _mods()
    dev = env.device
    t = {k: v.to(dev) for k, v in inputs(tag).items()}
    left, right = t["left"], t["right"]
    res = {}
    with env.ctx():
        disp = t["disp"].clone().requires_grad_()
        warped, valid = P.warp_right_to_left(right, disp)
        assert valid.shape == warped.shape == right.shape and valid.requires_grad is False
        assert all(torch.equal(valid[:, :1], valid[:, c:c + 1]) for c in range(valid.shape[1]))
        res["warped"], res["valid"] = warped.detach(), valid[:, :1]
        res["g_warp"], = _grad(warped, t["gw_c"], disp)
        for ws in _windows(tag):
            x, y = left.clone().requires_grad_(), right.clone().requires_grad_()
            s = P.ssim(x, y, window_size=ws)
            res[f"ssim{ws}"] = s.detach()
            res[f"g_ssim{ws}_x"], res[f"g_ssim{ws}_y"] = _grad(s, t["gw_c"], x, y)
            if ws == 7:                                                    # one side alone: the same bits
                gx_alone, = _grad(P.ssim(x, right), t["gw_c"], x)
                assert torch.equal(gx_alone, res["g_ssim7_x"])
        for name, on in (("photo_mask", True), ("photo_nomask", False)):
            out = P.photometric_loss(left, right, disp, enable_mask=on)
            assert out.shape == t["gw_1"].shape
            res[name] = out.detach()
            res["g_" + name], = _grad(out, t["gw_1"], disp)
        res["photo_none"] = P.photometric_loss(left, right, enable_mask=False)
        sdisp = t["sdisp"].clone().requires_grad_()
        loss = S.smoothness_loss(sdisp, left, warn=False)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        res["smooth"] = loss.detach()
        res["g_smooth"], = torch.autograd.grad(loss, sdisp)
        sync(env)
    return {k: v.detach().cpu() for k, v in res.items()}


def _factor(k):
    return GRAD_FACTOR if k.startswith("g_") else VALUE_FACTOR


@pytest.mark.parametrize("backend,tag", on(CASES, GPU_ONLY))
def test_product_matches_reference_fp64(backend, tag, gold, parity_log):
    """warped, valid_mask, the ssim map (windows 7 / 3 / 11), photometric_loss with the mask on and off and without a disparity,
    the smoothness scalar; the gradients to disp of warp, photometric and smoothness and to x and y of ssim."""
    got = _product(Env(backend), tag)
    names = [k for k in _restated64(tag) if not k.startswith("dn_")]
    assert set(got) == set(names)
    for k in names:
        want = _restated64(tag)[k] if tag in GPU_ONLY else torch.from_numpy(gold[f"{tag}:{k}:f64"])
        within(got[k], want, float(gold[f"{tag}:{k}:dref"]), _factor(k), f"selfsup {tag} {k} [{backend}]", parity_log)


def _check_mask(log, got, want64, reproj64, ident64, what):
    want = torch.from_numpy(want64).bool()
    share = want.double().mean().item()
    assert AUTO_MASK_MIN_SHARE <= share <= 1 - AUTO_MASK_MIN_SHARE, (what, share)
    assert got.dtype == torch.bool and got.shape == want.shape, (what, got.dtype, got.shape)
    close = (torch.from_numpy(reproj64) - torch.from_numpy(ident64)).abs() <= AUTO_MASK_MARGIN
    skipped = close.double().mean().item()
    wrong = ((got.cpu() != want) & ~close).sum().item()
    print(f"{what}: true share {share:.3f}  skipped {skipped:.4f}  mismatches {wrong}")
    log(what, true_share=share, skipped=skipped, mismatches=wrong)
    assert skipped <= AUTO_MASK_MAX_SKIPPED and wrong == 0, (what, skipped, wrong)


@pytest.mark.parametrize("backend,tag", on(AUTO_MASK_CASES))
def test_auto_mask_matches_reference_fp64(backend, tag, gold, parity_log):
    _, A, _ = _mods()
    env = Env(backend)
    t = {k: v.to(env.device) for k, v in inputs(tag).items()}
    with env.ctx():
        mask = A.auto_mask(t["left"], t["right"], t["disp"].clone().requires_grad_())
        again = A.auto_mask(t["left"], t["right"], t["disp"])
        assert mask.requires_grad is False and torch.equal(mask, again)
        _check_mask(parity_log, mask, gold[f"{tag}:am:f64"], gold[f"{tag}:photo_nomask:f64"], gold[f"{tag}:photo_none:f64"],
                    f"selfsup {tag} auto_mask [{backend}]")
        if tag in AUTO_MASK_DENORM:
            ln, rn = normalised(inputs(tag)["left"]).to(env.device), normalised(inputs(tag)["right"]).to(env.device)
            mask = A.auto_mask(ln, rn, t["disp"], denorm=True)
            _check_mask(parity_log, mask, gold[f"{tag}:am_dn:f64"], gold[f"{tag}:dn_reproj:f64"], gold[f"{tag}:dn_ident:f64"],
                        f"selfsup {tag} auto_mask denorm [{backend}]")


@pytest.mark.parametrize("backend,tag", on(("r37x70",)))
def test_every_kernel_is_bitwise_reproducible(backend, tag):
    a, b = _product(Env(backend), tag), _product(Env(backend), tag)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert all(a[k].abs().max().item() > 0 for k in a)


# ------------------------------------------------------------------------------------------ finite differences (emulator)
def test_finite_difference_gradients():
    """Directional derivatives through the product host code on the emulator at (1, 3, 9, 13).  The disparity steps (1e-3 of the
    mean |disp|, a few thousandths of a pixel) stay inside the 0.05 px the inputs keep from the bilinear kinks."""
    from tests.emu_util import emu_product_path
    P, _, S = _mods()
    left, right, disp = fd_inputs()
    assert left.shape == FD_SHAPE
    with emu_product_path():
        # (enable_mask=False: the reference detaches valid_mask, so with the mask on the gradient is NOT the derivative of the
        #  forward; the masked gradient is compared with the reference's in test_product_matches_reference_fp64)
        directional(lambda d: P.photometric_loss(left, right, d, enable_mask=False), [disp], eps=1e-3, seed=21)
        directional(lambda d: P.photometric_loss(left, right, d, ssim_weight=0.4, enable_mask=False), [disp], eps=1e-3, seed=22)
        directional(lambda d: P.warp_right_to_left(right, d)[0], [disp], eps=1e-3, seed=23)
        directional(lambda x, y: P.ssim(x, y), [left, right], seed=24)
        directional(lambda x, y: P.ssim(x, y, window_size=3), [left, right], seed=25)
        directional(lambda d: S.smoothness_loss(d, left, warn=False).reshape(1), [disp.abs() + 1], eps=1e-3, seed=26)


# ------------------------------------------------------------------------------------------ warning, refusals, surface
def test_smoothness_warning_is_the_references_and_optional(env, capsys):
    _, _, S = _mods()
    t = inputs("b2_9x13")
    img, sdisp = (t["left"] * 1.5).to(env.device), t["sdisp"].to(env.device)
    with env.ctx():
        quiet = S.smoothness_loss(sdisp, img, warn=False)
        assert capsys.readouterr().out == ""
        loud = S.smoothness_loss(sdisp, img)
        assert capsys.readouterr().out == "Warning: Image may not be normalized. Expected range: [0,1]\n"
        assert torch.equal(quiet, loud)
        S.smoothness_loss(sdisp, t["left"].to(env.device))
        assert capsys.readouterr().out == ""


def test_cpu_tensors_are_refused():
    from stereo_toolbox_amd import ops
    P, A, S = _mods()
    t = inputs("s4")
    left, right, disp = t["left"], t["right"], t["disp"]
    for call in (lambda: P.warp_right_to_left(right, disp), lambda: P.ssim(left, right), lambda: P.photometric_loss(left, right, disp),
                 lambda: P.photometric_loss(left, right, enable_mask=False), lambda: A.auto_mask(left, right, disp),
                 lambda: S.smoothness_loss(t["sdisp"], left)):
        with pytest.raises(ops.StxError, match="ROCm device"):
            call()


def test_unsupported_arguments_are_refused(env):
    from stereo_toolbox_amd import ops
    P, A, S = _mods()
    t = {k: v.to(env.device) for k, v in inputs("b2_9x13").items()}
    left, right, disp = t["left"], t["right"], t["disp"]
    with env.ctx():
        for call in (lambda: P.photometric_loss(left.clone().requires_grad_(), right, disp),
                     lambda: P.photometric_loss(left, right.clone().requires_grad_(), disp),
                     lambda: P.warp_right_to_left(right.clone().requires_grad_(), disp),
                     lambda: S.smoothness_loss(t["sdisp"], left.clone().requires_grad_())):
            with pytest.raises(ops.StxError, match="detach"):
                call()
        assert P.photometric_loss(left.clone().requires_grad_().detach(), right, disp).shape == disp.shape
        with pytest.raises(ops.StxError, match="enable_mask"):
            P.photometric_loss(left, right)                                # the reference dies on an unbound valid_mask here
        with pytest.raises(ops.StxError, match="enable_mask"):
            P.photometric_loss(left, right, None, 0.85, True)
        for ws in (4, 1, 13, 7.0):
            with pytest.raises(ops.StxError, match="window_size"):
                P.ssim(left, right, window_size=ws)
        for mode in ("replicate", "constant", "circular"):
            with pytest.raises(ops.StxError, match="pad_mode"):
                P.ssim(left, right, pad_mode=mode)
        small, narrow = left[:, :, :3].contiguous(), left[:, :, :, :3].contiguous()
        for img in (small, narrow):
            B, _, H, W = img.shape
            with pytest.raises(ops.StxError, match="reflect padding"):
                P.ssim(img, img)
            with pytest.raises(ops.StxError, match="reflect padding"):
                P.photometric_loss(img, img, enable_mask=False)
            with pytest.raises(ops.StxError, match="reflect padding"):
                A.auto_mask(img, img, torch.zeros(B, 1, H, W, device=env.device))
            assert P.ssim(img, img, window_size=5).shape == img.shape      # 3 > 5 // 2
        with pytest.raises(ops.StxError, match="reflect padding"):
            P.ssim(left[:, :, :5].contiguous(), right[:, :, :5].contiguous(), window_size=11)
        with pytest.raises(ops.StxError, match="one shape"):
            P.ssim(left, right[:, :, :5].contiguous())
        with pytest.raises(ops.StxError, match="disp must be"):
            P.photometric_loss(left, right, disp[:, 0])
        with pytest.raises(ops.StxError, match="3 channels"):
            A.auto_mask(left[:, :2].contiguous(), right[:, :2].contiguous(), disp, denorm=True)


def test_c_entry_points_refuse_without_launching(be):  # noqa: F811
    """The C-ABI returns an error -- and writes nothing -- for an even or too large window, an image too small for the window, a
    mask without a disparity and a missing output."""
    from stereo_toolbox_amd import ops
    img = be.dev(torch.zeros(1, 1, 8, 8))
    out, ws = be.empty(64), be.empty(4 * 64)
    bad = [("stx_ssim_fwd", (ptr(img), ptr(img), ptr(out), 1, 1, 8, 8, 4)),
           ("stx_ssim_fwd", (ptr(img), ptr(img), ptr(out), 1, 1, 8, 8, 13)),
           ("stx_ssim_fwd", (ptr(img), ptr(img), ptr(out), 1, 1, 3, 8, 7)),
           ("stx_ssim_bwd", (ptr(img), ptr(img), ptr(img), None, None, ptr(ws), 1, 1, 8, 8, 7)),
           ("stx_photometric_fwd", (ptr(img), ptr(img), None, 0.85, 1, ptr(out), 1, 1, 8, 8)),
           ("stx_photo_warp_fwd", (ptr(img), ptr(img), ptr(out), ptr(out), 1, 1, 1, 64)),
           ("stx_smoothness_fwd", (ptr(img), ptr(img), ptr(out), ptr(out), ptr(ws), 1, 1, 1, 64)),
           ("stx_auto_mask_fwd", (ptr(img), ptr(img), ptr(img), 1, ptr(out), 1, 1, 8, 8))]
    for name, args in bad:
        with pytest.raises(ops.StxError):
            be.call(name, *args)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()


def test_public_surface_is_the_references():
    """Names, parameter names and defaults of the reference's loss_functions package (the list lives in selfsup_config.SURFACE),
    importable from the package and from the three modules."""
    pkg = importlib.import_module(PKG)
    assert set(PACKAGE_EXPORTS) <= set(pkg.__all__)
    for name in PACKAGE_EXPORTS:
        assert callable(getattr(pkg, name)), name
    assert "out of scope" not in pkg.__doc__
    for mod, fns in SURFACE.items():
        m = importlib.import_module(f"{PKG}.{mod}")
        for name, params in fns.items():
            fn = getattr(m, name)
            if name in PACKAGE_EXPORTS:
                assert getattr(pkg, name) is fn, name
            sig = inspect.signature(fn)
            got = tuple((p.name, REQUIRED if p.default is inspect.Parameter.empty else p.default) for p in sig.parameters.values())
            assert got == params, (mod, name, got)
