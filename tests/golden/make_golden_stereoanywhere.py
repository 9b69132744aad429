"""Golden fixture for StereoAnywhere's volume stage (tests/test_stereoanywhere.py).

  python tests/golden/make_golden_stereoanywhere.py        (build container only: needs /root/reference)

The reference's OWN models/StereoAnywhere/corr.py (`CorrBlock1D`) and utils/utils.py (`estimate_*`, `truncate_corr_volume_v2`,
`bilinear_sampler`) are executed, in fp32 and in fp64, on the seeded inputs of tests/golden/stereoanywhere_config.py.  The two
files are loaded by path under a stand-in package (the real package `__init__` pulls in cv2) with a stub `kornia.filters` (none
of the functions used here touches it).  fp64: `bilinear_sampler` ends in `.float()`; for the fp64 run the generator makes
`Tensor.float` a cast to float64 around the calls, as make_golden_corr1d.py does -- the reference files are untouched.
Stored per tensor: the fp32 result (`:f32`), the fp64 result (`:f64`) and d_ref = max|fp32 - fp64| (`:dref`); of the volume
gradients of the larger estimator cases d_ref, max|fp64| (`:max`) and stereoanywhere_config.subsample of the fp64 tensor
(`:sub`).  Every d_ref must be > 0.  -> tests/golden/stereoanywhere.npz
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

from tests.golden.stereoanywhere_config import (ATTENUATION, BLOCK_CASES, EST_CASES, EST_WHOLE, MASK_THRESHOLDS, OUTPUTS,  # noqa: E402
                                                block_inputs, est_inputs, mask_inputs, subsample)

REF = "/root/reference/stereo_toolbox/models/StereoAnywhere"


def reference():
    kornia, filters = types.ModuleType("kornia"), types.ModuleType("kornia.filters")
    filters.spatial_gradient = None
    kornia.filters = filters
    sys.modules.setdefault("kornia", kornia)
    sys.modules.setdefault("kornia.filters", filters)
    for name, path in (("sa_ref", REF), ("sa_ref.utils", os.path.join(REF, "utils"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    return importlib.import_module("sa_ref.corr"), importlib.import_module("sa_ref.utils.utils")


@contextlib.contextmanager
def keep_fp64():
    """`.float()` as a cast to float64 (see the module docstring)."""
    to_float = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = to_float


def fp64_if(dtype):
    return keep_fp64() if dtype == torch.float64 else contextlib.nullcontext()


def run_estimates(U, tag, dtype):
    """All four outputs with the summed loss, then each output's loss alone: the outputs and five volume gradients."""
    vol, gws = est_inputs(tag)
    fns = (U.estimate_left_disparity, U.estimate_left_confidence, U.estimate_right_disparity, U.estimate_right_confidence)
    res = {}
    for only in (None, 0, 1, 2, 3):
        v = vol.to(dtype).clone().requires_grad_()
        outs = [fn(v) for fn in fns]
        assert all(o.dtype == dtype for o in outs)
        sum((o * g.to(dtype)).sum() for i, (o, g) in enumerate(zip(outs, gws)) if only is None or only == i).backward()
        if only is None:
            res.update({k: o for k, o in zip(OUTPUTS, outs)})
            res["g_all"] = v.grad
        else:
            res["g_" + OUTPUTS[only]] = v.grad
    return res


def run_block(C, U, tag, dtype):
    B, H, W1, W2, L, r, pad, trunc = BLOCK_CASES[tag]
    vol, maps, coords, gws, wc = block_inputs(tag)
    v = vol.to(dtype).clone().requires_grad_()
    full = v
    if trunc:
        mask = U.truncate_corr_volume_v2(maps[0].to(dtype), maps[1].to(dtype), conf_th=None, attenuation_gain=ATTENUATION)
        full = (mask[:, 0].detach() * v.squeeze(3)).unsqueeze(3)         # [B,H,W,W] x [B,H,W1,W2]
    with fp64_if(dtype):
        fn = C.CorrBlock1D(full, num_levels=L, radius=r, pad=list(pad))
        outs = [fn(c.to(dtype)) for c in coords]
    assert all(o.dtype == dtype and o.shape == g.shape for o, g in zip(outs, gws)), [o.shape for o in outs]
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws))
    for i in range(L):                                                   # (the reference's extra level L has no consumer)
        loss = loss + (fn.corr_pyramid[i].reshape(B, H, W1, W2 >> i) * wc[i].to(dtype)).sum()
    loss.backward()
    return {"outs": torch.stack(outs), "g_fullcorr": v.grad}


def run_masks(U, dtype):
    disp, conf = (t.to(dtype) for t in mask_inputs())
    return {k: U.truncate_corr_volume_v2(disp, conf, conf_th=th, attenuation_gain=ATTENUATION) for k, th in MASK_THRESHOLDS.items()}


def main():
    C, U = reference()
    store = {}
    jobs = [(f"est:{t}", lambda dt, t=t: run_estimates(U, t, dt), lambda k, t=t: t in EST_WHOLE or not k.startswith("g_"))
            for t in EST_CASES]
    jobs += [(f"block:{t}", lambda dt, t=t: run_block(C, U, t, dt), lambda k: True) for t in BLOCK_CASES]
    jobs.append(("mask", lambda dt: run_masks(U, dt), lambda k: True))
    for tag, fn, whole in jobs:
        r32, r64 = fn(torch.float32), fn(torch.float64)
        for k in r32:
            a, b = r32[k].detach(), r64[k].detach()
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
            dref = (a.double() - b).abs().max().item()
            assert dref > 0, (tag, k)
            store[f"{tag}:{k}:dref"] = np.float64(dref)
            if whole(k):
                store[f"{tag}:{k}:f32"] = a.numpy()
                store[f"{tag}:{k}:f64"] = b.numpy()
            else:
                store[f"{tag}:{k}:max"] = np.float64(b.abs().max().item())
                store[f"{tag}:{k}:sub"] = subsample(b).numpy().copy()
            print(f"{tag:18s} {k:10s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {dref:.3e}", flush=True)
    path = os.path.join(HERE, "stereoanywhere.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
