"""Golden fixture for the RAFT-family 1-D correlation pyramid and lookup (tests/test_corr1d.py).

  python tests/golden/make_golden_corr1d.py        (build container only: needs /root/reference)

The reference's OWN `CorrBlock1D` classes (models/RAFTStereo/corr.py, models/DEFOMStereo/corr.py, with their
utils/utils.py `bilinear_sampler`) are executed, in fp32 and in fp64, on the seeded inputs of tests/golden/corr1d_config.py.
fp64: both files end in `.float()` and divide by `torch.sqrt(torch.tensor(D).float())`; for the fp64 run the generator makes
`Tensor.float` a cast to float64 around the calls (the `dx` of torch.linspace holds integers and is promoted by the fp64
coordinates it is added to) -- the reference files themselves are untouched.
Stored per tensor of the small cases: the fp32 result, the fp64 result and d_ref = max|fp32 - fp64|; of the larger cases
(SHAPE_CASES, the 32-call iteration pattern with an extra consumer of the pyramid): d_ref (`:dref`), max|fp64| (`:max`) and
corr1d_config.subsample of the fp64 result (`:sub`): tests/golden/corr1d.npz.  About a minute on eight cores.
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.corr1d_config import (ALL_CASES, CASES, DEFOM_SCALE_RADIUS, DEFOM_SCALES, ITER_CALLS, ITER_CASE,  # noqa: E402
                                        SHAPE_CASES, columns, inputs, iter_inputs, subsample)


def reference():
    sys.path.insert(0, "/root/reference/stereo_toolbox/models")
    from DEFOMStereo.corr import CorrBlock1D as Defom
    from RAFTStereo.corr import CorrBlock1D as Raft
    return Raft, Defom


@contextlib.contextmanager
def keep_fp64():
    """`.float()` as a cast to float64 (see the module docstring)."""
    to_float = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = to_float


def run_case(Raft, Defom, tag, dtype):
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    f1, f2, pos, gws = inputs(tag)
    f1, f2 = (t.to(dtype).requires_grad_() for t in (f1, f2))
    with keep_fp64() if dtype == torch.float64 else contextlib.nullcontext():
        if kind == "raft":
            fn = Raft(f1, f2, num_levels=L, radius=r)
            outs = [fn(p.to(dtype)) for p in pos]
            corr = Raft.corr(f1, f2)
        else:
            fn = Defom(f1, f2, columns(tag).to(dtype), num_levels=L, radius=r, scale_list=list(DEFOM_SCALES),
                       scale_corr_radius=DEFOM_SCALE_RADIUS)
            outs = [fn(pos[0].to(dtype)), fn(pos[1].to(dtype), scaling=True)]
            corr = Defom.corr(f1, f2)
    assert all(o.dtype == dtype for o in outs) and corr.dtype == dtype, [o.dtype for o in outs]
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws)).backward()
    return {"out_a": outs[0], "out_b": outs[1], "corr": corr, "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def run_iterations(Raft, dtype):
    """ITER_CALLS lookups on one object, losses summed, plus a weighted sum of every level of the public pyramid
    ([b*h*w, 1, 1, W2_i] in the reference)."""
    kind, B, Cf, H, W1, W2, L, r = CASES[ITER_CASE]
    f1, f2, coords, gws, wc = iter_inputs()
    f1, f2 = (t.to(dtype).requires_grad_() for t in (f1, f2))
    with keep_fp64() if dtype == torch.float64 else contextlib.nullcontext():
        fn = Raft(f1, f2, num_levels=L, radius=r)
        outs = [fn(c.to(dtype)) for c in coords]
    loss = sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws))
    for i in range(L):
        loss = loss + (fn.corr_pyramid[i].reshape(B, H, W1, W2 >> i) * wc[i].to(dtype)).sum()
    loss.backward()
    return {"outs": torch.stack(outs), "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def main():
    Raft, Defom = reference()
    store = {}
    jobs = [(tag, tag in CASES, lambda dt, t=tag: run_case(Raft, Defom, t, dt)) for tag in list(CASES) + list(SHAPE_CASES)]
    jobs.append((f"iter{ITER_CALLS}", False, lambda dt: run_iterations(Raft, dt)))
    for tag, whole, fn in jobs:
        r32, r64 = fn(torch.float32), fn(torch.float64)
        for k in r32:
            a, b = r32[k].detach(), r64[k].detach()
            assert a.dtype == torch.float32 and b.dtype == torch.float64
            store[f"{tag}:{k}:dref"] = np.float64((a.double() - b).abs().max().item())
            if whole:
                store[f"{tag}:{k}:f32"] = a.numpy()
                store[f"{tag}:{k}:f64"] = b.numpy()
            else:
                store[f"{tag}:{k}:max"] = np.float64(b.abs().max().item())
                store[f"{tag}:{k}:sub"] = subsample(b).numpy().copy()
            print(f"{tag:16s} {k:8s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {store[f'{tag}:{k}:dref']:.3e}",
                  flush=True)
    path = os.path.join(HERE, "corr1d.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
