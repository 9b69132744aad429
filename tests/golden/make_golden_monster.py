"""Golden fixture for MonSter's mutual-refinement stage (tests/test_monster.py).

  python tests/golden/make_golden_monster.py        (build container only: needs /root/reference)

The reference's OWN models/MonSter/warp.py (`disp_warp`) and monster.py (`compute_scale_shift`) are executed, in fp32 and in fp64,
on the seeded inputs of tests/golden/monster_config.py.  The files are loaded by path under a stand-in package with stubs for
what this machine lacks or what they do not need here (opt_einsum, timm, the DepthAnything package, matplotlib / scipy / PIL where
missing); none of the functions used touches a stub.  fp64: `interp` calls `.float()`; around the calls `Tensor.float` is a cast
to float64 (`keep_fp64` of make_golden_stereoanywhere.py) and the default dtype is float64 (the ridge `1e-6 * torch.eye(2)`).
Flaws are formed as the model forms them: disp_warp(right, d)[0] - left, with the loss sum(flaw_a gw_a) + sum(flaw_b gw_b).
Stored per tensor: the fp32 result (`:f32`), the fp64 result (`:f64`) and d_ref = max|fp32 - fp64| (`:dref`); of the cases in
SUBSAMPLED / FIT_SUBSAMPLED d_ref, max|fp64| (`:max`) and monster_config.subsample of the fp64 tensor (`:sub`).  d_ref must be > 0
except for the tensors monster_config.ZERO_DREF lists, where it must be 0.  The validity map must agree between fp32 and fp64.
The fit also stores the rank threshold and the mask count, read off the reference's own expressions (monster.py:45-51), which
must agree between fp32 and fp64.  -> tests/golden/monster.npz
"""
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_stereoanywhere import keep_fp64  # noqa: E402
from tests.golden.monster_config import (FIT_CASES, FIT_SUBSAMPLED, FLAW_CASES, GRAD_KEYS, SUBSAMPLED, ZERO_DREF,  # noqa: E402
                                         check_fit_inputs, check_flaw_inputs, subsample)

REF = "/root/reference/stereo_toolbox/models/MonSter"


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
    except ImportError:
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        if "." in name:
            setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)


def reference():
    """-> (warp module, monster module) of the reference, under the stand-in package `ms_ref.MonSter`"""
    _stub("opt_einsum", contract=None)
    _stub("timm_0_5_4")
    _stub("matplotlib")
    _stub("matplotlib.pyplot")
    _stub("scipy", interpolate=None)
    _stub("PIL", Image=None)
    for name, path in (("ms_ref", None), ("ms_ref.MonSter", REF), ("ms_ref.MonSter.utils", os.path.join(REF, "utils")),
                       ("ms_ref.depth_anything_v2", None)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path] if path else []
        sys.modules[name] = pkg
    dpt = types.ModuleType("ms_ref.depth_anything_v2.dpt")
    dpt.DepthAnythingV2 = dpt.DepthAnythingV2_decoder = None
    sys.modules["ms_ref.depth_anything_v2.dpt"] = dpt
    return importlib.import_module("ms_ref.MonSter.warp"), importlib.import_module("ms_ref.MonSter.monster")


@contextlib.contextmanager
def precision(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with (keep_fp64() if dtype == torch.float64 else contextlib.nullcontext()):
            yield
    finally:
        torch.set_default_dtype(old)


def run_flaw(Wp, tag, dtype):
    t = check_flaw_inputs(tag)
    padding = t.pop("padding")
    t = {k: None if v is None else v.to(dtype) for k, v in t.items()}
    left, right = t["left"].clone().requires_grad_(), t["right"].clone().requires_grad_()
    da = t["disp_a"].clone().requires_grad_()
    db = None if t["disp_b"] is None else t["disp_b"].clone().requires_grad_()
    res = {}
    with precision(dtype):
        warped, valid = Wp.disp_warp(right, da, padding)
        assert all(torch.equal(valid[:, :1], valid[:, c:c + 1]) for c in range(valid.shape[1]))
        res["warped_a"], res["valid_a"] = warped.detach(), valid[:, :1].detach().contiguous()
        flaw_a = Wp.disp_warp(right, da, padding)[0] - left
        loss = (flaw_a * t["gw_a"]).sum()
        res["flaw_a"] = flaw_a.detach()
        if db is not None:
            flaw_b = Wp.disp_warp(right, db, padding)[0] - left
            loss = loss + (flaw_b * t["gw_b"]).sum()
            res["flaw_b"] = flaw_b.detach()
        loss.backward()
    res["g_left"], res["g_right"], res["g_disp_a"] = left.grad, right.grad, da.grad
    if db is not None:
        res["g_disp_b"] = db.grad
    assert all(v.dtype == dtype for v in res.values()), {k: v.dtype for k, v in res.items()}
    return res


def run_fit(M, tag, dtype):
    mono, gt, mask, gw = check_fit_inputs(tag)
    mono, gt, gw = mono.to(dtype), gt.to(dtype), gw.to(dtype)
    B = mono.shape[0]
    scale, shift, thr, count = [], [], [], []
    with precision(dtype):
        for b in range(B):
            m, g = mono[b].clone().squeeze(1), gt[b].clone().squeeze(1)       # as monster.py:466 passes them
            k = None if mask is None else mask[b].squeeze(1)
            s, h = M.compute_scale_shift(m, g, k)
            scale.append(s)
            shift.append(h)
            srt, _ = torch.sort(m.clone().view(-1).contiguous())              # monster.py:45-51
            th = srt[int(0.2 * len(srt))]
            thr.append(th.item())
            count.append(int(((g > 0) & (m > 1e-2) & (m > th)).sum()) if k is None else int(k.sum()))
        x = mono.clone().requires_grad_()
        aligned = torch.stack([scale[b] * x[b] + shift[b] for b in range(B)])  # monster.py:467
        (aligned * gw).sum().backward()
    assert aligned.dtype == dtype
    res = {"scale": torch.tensor(scale, dtype=dtype), "shift": torch.tensor(shift, dtype=dtype), "aligned": aligned.detach(),
           "g_mono": x.grad}
    return res, thr, count


def _store(store, key, a, b, whole, zero=False):
    a, b = a.detach(), b.detach()
    assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, key
    dref = (a.double() - b).abs().max().item()
    assert (dref == 0) if zero else (dref > 0), (key, dref)
    store[key + ":dref"] = np.float64(dref)
    if whole:
        store[key + ":f32"] = a.numpy()
        store[key + ":f64"] = b.numpy()
    else:
        store[key + ":max"] = np.float64(b.abs().max().item())
        store[key + ":sub"] = subsample(b).numpy().copy()
    print(f"{key:28s} {str(tuple(a.shape)):20s} max|ref| {b.abs().max().item():.4g}  d_ref {dref:.3e}", flush=True)


def main():
    Wp, M = reference()
    store = {}
    for tag, (_, _, _, grads) in FLAW_CASES.items():
        r32, r64 = run_flaw(Wp, tag, torch.float32), run_flaw(Wp, tag, torch.float64)
        assert torch.equal(r32["valid_a"].double(), r64["valid_a"]), tag
        for k in r32:
            if k in GRAD_KEYS and not grads:
                continue
            if k == "valid_a":
                store[f"flaw:{tag}:valid_a"] = r64[k].numpy().astype(np.uint8)
                print(f"flaw:{tag}:valid_a share {r64[k].mean().item():.3f}")
                continue
            _store(store, f"flaw:{tag}:{k}", r32[k], r64[k], tag not in SUBSAMPLED, zero=k in ZERO_DREF.get(tag, ()))
    for tag in FIT_CASES:
        (r32, thr32, n32), (r64, thr64, n64) = run_fit(M, tag, torch.float32), run_fit(M, tag, torch.float64)
        assert thr32 == thr64 and n32 == n64, (tag, thr32, thr64, n32, n64)
        store[f"fit:{tag}:thr"] = np.array(thr32, dtype=np.float64)
        store[f"fit:{tag}:count"] = np.array(n32, dtype=np.int64)
        print(f"fit:{tag} thresholds {thr32} counts {n32} scale {r64['scale'].tolist()} shift {r64['shift'].tolist()}")
        for k in r32:
            whole = tag not in FIT_SUBSAMPLED or k in ("scale", "shift")
            _store(store, f"fit:{tag}:{k}", r32[k], r64[k], whole, zero=tag == "empty")
    path = os.path.join(HERE, "monster.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
