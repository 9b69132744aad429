"""Golden fixture for the IGEV geometry-encoding lookup and the convex upsampling (tests/test_geo_lookup.py).

  python tests/golden/make_golden_geo.py        (build container only: needs /root/reference)

The reference's OWN `Combined_Geo_Encoding_Volume` (models/IGEVStereo/geometry.py) and `context_upsample`
(models/IGEVStereo/submodule.py) are executed, in fp32 and in fp64, on the seeded inputs of tests/golden/geo_config.py.  The
package's `__init__` pulls in the 2-D backbone (`import timm_0_5_4`, absent from this image and never touched here) and
utils/utils.py imports scipy for an unrelated helper: empty module objects of those names are put into sys.modules where the
real ones are missing (the device tests/golden/make_golden_igev_agg.py uses).
fp64: geometry.py:41 builds `dx` with torch.linspace's default dtype and :59 ends in `.float()`; for the fp64 run the
generator makes both keep the dtype of their surroundings (a float64 linspace, an identity `Tensor.float`) around the calls --
the reference file itself is untouched.
Stored per tensor: the fp32 result, the fp64 result and d_ref = max|fp32 - fp64|: tests/golden/geo_lookup.npz.

The second table of geo_config.py (SHAPE_CASES, the 22-call iteration pattern, the extra-consumer case, the larger upsampling
cases; tests/test_geo_lookup_shapes.py) goes through the same reference classes, but whole tensors at those sizes do not belong
in git: tests/golden/geo_lookup_shapes.npz keeps per tensor d_ref (`:dref`), max|fp64| (`:max`) and geo_config.subsample of the
fp64 result (`:sub`).  Half a minute on eight cores, the 144x240 case included.
"""
import contextlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.geo_config import (CASES, EXTRA_CALLS, ITER_CASE, SHAPE_CASES, SHAPE_UPSAMPLE_CASES, UPSAMPLE_CASES,  # noqa: E402
                                     inputs, iter_inputs, shape_inputs, shape_upsample_inputs, subsample, upsample_inputs)


def reference():
    sys.modules.setdefault("timm_0_5_4", types.ModuleType("timm_0_5_4"))
    if importlib.util.find_spec("scipy") is None:
        sp = types.ModuleType("scipy")
        sp.interpolate = types.ModuleType("scipy.interpolate")
        sys.modules.setdefault("scipy", sp)
        sys.modules.setdefault("scipy.interpolate", sp.interpolate)
    sys.path.insert(0, "/root/reference/stereo_toolbox/models")
    from IGEVStereo.geometry import Combined_Geo_Encoding_Volume
    from IGEVStereo.submodule import context_upsample
    return Combined_Geo_Encoding_Volume, context_upsample


@contextlib.contextmanager
def keep_fp64():
    """geometry.py:41 and :59 in the dtype of their surroundings (see the module docstring)."""
    linspace, to_float = torch.linspace, torch.Tensor.float
    torch.linspace = lambda *a, **k: linspace(*a, **{"dtype": torch.float64, **k})
    torch.Tensor.float = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.linspace, torch.Tensor.float = linspace, to_float


def run_lookup(Ref, tag, dtype, shapes=False):
    B, C, D, H, W, W2, Cf, L, r = (SHAPE_CASES if shapes else CASES)[tag]
    geo, f1, f2, coords, disps, gws = (shape_inputs if shapes else inputs)(tag)
    geo, f1, f2 = (t.to(dtype).requires_grad_() for t in (geo, f1, f2))
    ctx = keep_fp64() if dtype == torch.float64 else contextlib.nullcontext()
    with ctx:
        fn = Ref(f1, f2, geo, num_levels=L, radius=r)
        outs = [fn(d.to(dtype), coords.to(dtype)) for d in disps]
        corr = Ref.corr(f1, f2)
    assert all(o.dtype == dtype for o in outs), [o.dtype for o in outs]
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws))
    loss.backward()
    return {"out_a": outs[0], "out_b": outs[1], "corr": corr, "g_geo": geo.grad, "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def run_iterations(Ref, dtype, calls, extra):
    """`calls` lookups on one object, losses summed; extra: plus a weighted sum of every level of both pyramids (the object's
    public attributes, [b*h*w, C, 1, D_i] and [b*h*w, 1, 1, W2_i] in the reference)."""
    B, C, D, H, W, W2, Cf, L, r = ITER_CASE
    geo, f1, f2, coords, disps, gws, wg, wc = iter_inputs()
    geo, f1, f2 = (t.to(dtype).requires_grad_() for t in (geo, f1, f2))
    with keep_fp64() if dtype == torch.float64 else contextlib.nullcontext():
        fn = Ref(f1, f2, geo, num_levels=L, radius=r)
        outs = [fn(d.to(dtype), coords.to(dtype)) for d in disps[:calls]]
    assert all(o.dtype == dtype for o in outs)
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws))
    if extra:
        for i in range(L):
            loss = loss + (fn.geo_volume_pyramid[i].reshape(B, H, W, C, D >> i) * wg[i].to(dtype)).sum()
            loss = loss + (fn.init_corr_pyramid[i].reshape(B, H, W, W2 >> i) * wc[i].to(dtype)).sum()
    loss.backward()
    return {"outs": torch.stack(outs), "g_geo": geo.grad, "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def run_upsample(ref_up, tag, dtype, shapes=False):
    disp, wts, gw = (shape_upsample_inputs if shapes else upsample_inputs)(tag)
    disp, wts = disp.to(dtype).requires_grad_(), wts.to(dtype).requires_grad_()
    out = ref_up(disp, wts)
    assert out.dtype == dtype
    (out * gw.to(dtype)).sum().backward()
    return {"out": out, "g_disp_low": disp.grad, "g_up_weights": wts.grad}


def main():
    Ref, ref_up = reference()
    store = {}
    jobs = [(tag, lambda dt, t=tag: run_lookup(Ref, t, dt)) for tag in CASES]
    jobs += [("up_" + tag, lambda dt, t=tag: run_upsample(ref_up, t, dt)) for tag in UPSAMPLE_CASES]
    for tag, fn in jobs:
        r32, r64 = fn(torch.float32), fn(torch.float64)
        for k in r32:
            a, b = r32[k].detach(), r64[k].detach()
            store[f"{tag}:{k}:f32"] = a.numpy()
            store[f"{tag}:{k}:f64"] = b.numpy()
            store[f"{tag}:{k}:dref"] = np.float64((a.double() - b).abs().max().item())
            print(f"{tag:12s} {k:13s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {store[f'{tag}:{k}:dref']:.3e}")
    path = os.path.join(HERE, "geo_lookup.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")
    main_shapes(Ref, ref_up)


def main_shapes(Ref, ref_up):
    store = {}
    jobs = [(tag, lambda dt, t=tag: run_lookup(Ref, t, dt, shapes=True)) for tag in SHAPE_CASES]
    jobs += [("iter22", lambda dt: run_iterations(Ref, dt, None, False)), ("extra", lambda dt: run_iterations(Ref, dt, EXTRA_CALLS, True))]
    jobs += [("up_" + tag, lambda dt, t=tag: run_upsample(ref_up, t, dt, shapes=True)) for tag in SHAPE_UPSAMPLE_CASES]
    for tag, fn in jobs:
        r32, r64 = fn(torch.float32), fn(torch.float64)
        for k in r32:
            a, b = r32[k].detach(), r64[k].detach()
            assert a.dtype == torch.float32 and b.dtype == torch.float64
            store[f"{tag}:{k}:dref"] = np.float64((a.double() - b).abs().max().item())
            store[f"{tag}:{k}:max"] = np.float64(b.abs().max().item())
            store[f"{tag}:{k}:sub"] = subsample(b).numpy().copy()
            print(f"{tag:16s} {k:13s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {store[f'{tag}:{k}:dref']:.3e}", flush=True)
    path = os.path.join(HERE, "geo_lookup_shapes.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
