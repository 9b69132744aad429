"""Golden fixture for the self-supervised losses (tests/test_selfsup_loss.py).

  python tests/golden/make_golden_selfsup.py        (build container only: needs /root/reference)

The reference's OWN loss_functions/photometric_loss.py, auto_mask.py and smoothness_loss.py (pure torch) are executed in fp32 and
in fp64 on the seeded inputs of tests/golden/selfsup_config.py.  The fp64 run is under torch.set_default_dtype(torch.float64):
the reference builds its linspace grid (and auto_mask its mean / std) in the default dtype.  Loss weights are drawn in fp32 and cast.
Stored per tensor: the fp32 result (`:f32`), the fp64 result (`:f64`) and d_ref = max|fp32 - fp64| (`:dref`); of the GPU-only case
d_ref, max|fp64| (`:max`) and selfsup_config.subsample of the fp64 tensor (`:sub`).  valid_mask is the same in every channel
(asserted here) and stored as its first channel.  auto_mask's bool maps are stored as bytes (`am:f32`, `am:f64`).  Every d_ref
must be > 0.  -> tests/golden/selfsup_loss.npz
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.selfsup_config import (AUTO_MASK_CASES, AUTO_MASK_DENORM, AUTO_MASK_MARGIN, AUTO_MASK_MIN_SHARE, CASES,  # noqa: E402
                                         GPU_ONLY, SSIM_WINDOW_CASES, inputs, normalised, subsample)


@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _grad(out, weight, *leaves):
    (out * weight).sum().backward()
    grads = [leaf.grad for leaf in leaves]
    for leaf in leaves:
        leaf.grad = None
    return grads


def run_case(L, tag, dtype):
    P = L.photometric_loss
    t = {k: v.to(dtype) for k, v in inputs(tag).items()}
    left, right = t["left"], t["right"]
    res = {}
    with default_dtype(dtype):
        disp = t["disp"].clone().requires_grad_()
        warped, valid = P.warp_right_to_left(right, disp)
        assert valid.requires_grad is False and all(torch.equal(valid[:, :1], valid[:, c:c + 1]) for c in range(valid.shape[1]))
        res["warped"], res["valid"] = warped.detach(), valid[:, :1].contiguous()
        res["g_warp"], = _grad(warped, t["gw_c"], disp)
        for ws in (7,) + SSIM_WINDOW_CASES.get(tag, ()):
            x, y = left.clone().requires_grad_(), right.clone().requires_grad_()
            s = P.ssim(x, y, window_size=ws)
            res[f"ssim{ws}"] = s.detach()
            res[f"g_ssim{ws}_x"], res[f"g_ssim{ws}_y"] = _grad(s, t["gw_c"], x, y)
        for name, on in (("photo_mask", True), ("photo_nomask", False)):
            out = P.photometric_loss(left, right, disp, enable_mask=on)
            res[name] = out.detach()
            res["g_" + name], = _grad(out, t["gw_1"], disp)
        res["photo_none"] = P.photometric_loss(left, right, enable_mask=False)
        sdisp = t["sdisp"].clone().requires_grad_()
        loss = L.smoothness_loss.smoothness_loss(sdisp, left)
        assert loss.dim() == 0
        res["smooth"] = loss.detach()
        res["g_smooth"], = torch.autograd.grad(loss, sdisp)
        masks = {}
        if tag in AUTO_MASK_CASES:
            masks["am"] = L.auto_mask.auto_mask(left, right, t["disp"])
        if tag in AUTO_MASK_DENORM:
            mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
            std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
            ln, rn = normalised(inputs(tag)["left"]).to(dtype), normalised(inputs(tag)["right"]).to(dtype)
            res["dn_reproj"] = P.photometric_loss(ln * std + mean, rn * std + mean, t["disp"], enable_mask=False)
            res["dn_ident"] = P.photometric_loss(ln * std + mean, rn * std + mean, enable_mask=False)
            masks["am_dn"] = L.auto_mask.auto_mask(ln, rn, t["disp"], denorm=True)
    assert all(v.dtype == dtype for v in res.values()), {k: v.dtype for k, v in res.items()}
    return res, masks


def main():
    sys.path.insert(0, "/root/reference/stereo_toolbox")
    import loss_functions                            # noqa: F401  the reference's own package (imports only torch); its __init__
    #                                                  shadows the modules with the functions, so take them from sys.modules
    L = type("Ref", (), {k: sys.modules["loss_functions." + k] for k in ("photometric_loss", "auto_mask", "smoothness_loss")})
    store = {}
    for tag in CASES:
        (r32, m32), (r64, m64) = run_case(L, tag, torch.float32), run_case(L, tag, torch.float64)
        for k in r32:
            a, b = r32[k].detach(), r64[k].detach()
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
            dref = (a.double() - b).abs().max().item()
            assert dref > 0, (tag, k)
            store[f"{tag}:{k}:dref"] = np.float64(dref)
            if tag in GPU_ONLY:
                store[f"{tag}:{k}:max"] = np.float64(b.abs().max().item())
                store[f"{tag}:{k}:sub"] = subsample(b).numpy().copy()
            else:
                store[f"{tag}:{k}:f32"] = a.numpy()
                store[f"{tag}:{k}:f64"] = b.numpy()
            print(f"{tag:10s} {k:14s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {dref:.3e}", flush=True)
        for k in m32:
            a, b = m32[k], m64[k]
            assert a.dtype == b.dtype == torch.bool
            pre = "dn_" if k == "am_dn" else ""
            gap = (r64[pre + "reproj" if pre else "photo_nomask"] - r64[pre + "ident" if pre else "photo_none"]).abs()
            share = b.double().mean().item()
            close = (gap <= AUTO_MASK_MARGIN).double().mean().item()
            wrong = ((a != b) & (gap > AUTO_MASK_MARGIN)).sum().item()
            print(f"{tag:10s} {k:14s} true share {share:.3f}  inside the margin {close:.4f}  fp32 mismatches outside it {wrong}")
            assert AUTO_MASK_MIN_SHARE <= share <= 1 - AUTO_MASK_MIN_SHARE and wrong == 0, (tag, k)
            if tag not in GPU_ONLY:
                store[f"{tag}:{k}:f32"] = a.numpy().astype(np.uint8)
                store[f"{tag}:{k}:f64"] = b.numpy().astype(np.uint8)
    path = os.path.join(HERE, "selfsup_loss.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
