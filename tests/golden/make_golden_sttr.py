"""Golden fixture for STTR's matching head (tests/test_sttr_head.py).

  python tests/golden/make_golden_sttr.py        (build container only: needs /root/reference)

The reference's OWN models/STTR/regression_head.py (`RegressionHead`) and utilities/misc.py are executed, in fp32 and in fp64, on
the seeded inputs of tests/golden/sttr_config.py.  The two files are loaded by path under a stand-in package (the real package
`__init__` pulls in the whole model zoo) with a stub `context_adjustment_layer` (only `build_regression_head` names it).
Per (case, variant) the head's own steps are run -- `_optimal_transport` / `_softmax`, `_compute_gt_location`,
`_compute_low_res_disp`, `_compute_low_res_occ`, the dustbin slices -- with the summed loss and with each output's loss alone.
Asserted on the fp64 run at EVERY pixel: (top1 - top2) / top1 >= 1e-3, |norm - 0.1| >= 1e-4, and that the fp32 run finds the same
arg-max and the same forced norms: the comparisons downstream then leave no pixel out.
Stored per record, in the order of sttr_config.layout: `:f64` (whole tensors up to WHOLE elements, sttr_config.subsample of the
larger ones), `:f32` (the whole tensors only), `:dref` = max|fp32 - fp64| (> 0 but for the softmax's constant dustbin row) and
`:max` = max|fp64| per tensor; the forward
dictionaries of FORWARD_CASES whole.  -> tests/golden/sttr_head.npz
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.sttr_config import (CASE_VARIANTS, CASES, FORWARD_CASES, FORWARD_KEYS, SCALE, VARIANTS, StandInCal,  # noqa: E402
                                      forward_inputs, inputs, is_whole, layout, losses, outputs_of, subsample)

REF = "/root/reference/stereo_toolbox/models/STTR"
MIN_GAP, MIN_DIST = 1e-3, 1e-4


def reference():
    for name, path in (("sttr_ref", REF), ("sttr_ref.utilities", os.path.join(REF, "utilities"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    cal = types.ModuleType("sttr_ref.context_adjustment_layer")
    cal.build_context_adjustment_layer = None
    sys.modules["sttr_ref.context_adjustment_layer"] = cal
    return importlib.import_module("sttr_ref.regression_head"), importlib.import_module("sttr_ref.utilities.misc")


def run_steps(R, U, tag, var, dtype, which, stats=None):
    """The head's steps on one (case, variant) with the loss on output `which` ('all': summed) -> outputs, P, gradients"""
    ot, use_mask, use_target = VARIANTS[var]
    N, H, W, iters = CASES[tag]
    x = inputs(tag)
    head = R.RegressionHead(None, ot).to(dtype)
    with torch.no_grad():
        head.phi.copy_(x["phi"])
    attn = x["attn"].to(dtype).clone().requires_grad_()
    cols, rows = x["sampled_cols"], x["sampled_rows"]
    P = head._optimal_transport(attn, iters) if ot else head._softmax(attn)
    assert P.dtype == dtype and P.shape == (N, H, W + 1, W + 1)
    inner = P[..., :-1, :-1]
    mask = None
    if use_mask:
        mask = U.batched_index_select(U.batched_index_select(x["occ_mask"], 2, cols), 1, rows)
    out = {}
    if use_target:
        out["gt"], _ = head._compute_gt_location(float(SCALE), cols, rows, inner, x["disp_gt"].to(dtype))
    out["disp"], norm = head._compute_low_res_disp(head._compute_unscaled_pos_shift(W, attn.device), inner, mask)
    out["occ"] = head._compute_low_res_occ(norm)
    out["bin_l"], out["bin_r"] = P[..., :-1, -1], P[..., -1, :-1]
    outs = outputs_of(var)
    assert set(outs) == set(out) and all(out[k].shape == (N, H, W) and out[k].dtype == dtype for k in outs), var
    gws = dict(zip(("disp", "occ", "gt", "bin_l", "bin_r"), x["gws"]))
    sum((out[k] * gws[k].to(dtype)).sum() for k in outs if which in ("all", k)).backward()
    res = {"g_attn:" + which: attn.grad, "g_phi:" + which: head.phi.grad}
    assert torch.isfinite(attn.grad).all() and (attn.grad[torch.isinf(x["attn"])] == 0).all()
    if which == "all":
        res.update({k: out[k].detach() for k in outs})
        res["P"] = P.detach()
        if stats is not None:
            top = inner.detach().topk(2, dim=-1)
            raw = torch.gather(torch.nn.functional.pad(inner.detach(), [1, 1]), -1,
                               top.indices[..., :1] + torch.arange(3)).sum(-1)
            stats.update(gap=((top.values[..., 0] - top.values[..., 1]) / top.values[..., 0]).min().item(),
                         dist=(raw - 0.1).abs().min().item(), arg=top.indices[..., 0], forced=mask if use_mask else raw < 0.1,
                         low=(raw < 0.1).float().mean().item())
    return res


def run_record(R, U, tag, var, dtype, stats):
    res = {}
    for which in losses(var):
        res.update(run_steps(R, U, tag, var, dtype, which, stats))
    res["g_phi"] = torch.stack([res.pop("g_phi:" + which) for which in losses(var)])
    return res


def run_forward(R, U, name, dtype):
    tag, ot, mask, gt, down, cal = FORWARD_CASES[name]
    f = forward_inputs(name)
    head = R.RegressionHead(StandInCal() if cal else None, ot).to(dtype)
    with torch.no_grad():
        head.phi.copy_(inputs(tag)["phi"])
    x = U.NestedTensor(f["left"].to(dtype), f["right"].to(dtype), disp=None if f["disp"] is None else f["disp"].to(dtype),
                       sampled_cols=f["sampled_cols"], sampled_rows=f["sampled_rows"], occ_mask=f["occ_mask"],
                       occ_mask_right=f["occ_mask_right"])
    with torch.no_grad():
        return head(f["attn"].to(dtype), x)


def main():
    R, U = reference()
    store = {}
    for tag in CASES:
        for var in CASE_VARIANTS[tag]:
            s32, s64 = {}, {}
            r32, r64 = run_record(R, U, tag, var, torch.float32, s32), run_record(R, U, tag, var, torch.float64, s64)
            assert s64["gap"] >= MIN_GAP, (tag, var, s64["gap"])
            assert s64["dist"] >= MIN_DIST, (tag, var, s64["dist"])
            assert torch.equal(s32["arg"], s64["arg"]) and torch.equal(s32["forced"], s64["forced"]), (tag, var)
            f64, f32, dref, peak = [], [], [], []
            for k, shape in layout(tag, var):
                a, b = r32[k].detach(), r64[k].detach()
                assert a.dtype == torch.float32 and b.dtype == torch.float64 and tuple(a.shape) == tuple(b.shape) == shape, (tag, var, k)
                d = (a.double() - b).abs().max().item()
                dref.append(d)
                peak.append(b.abs().max().item())
                # (softmax: the dustbin row is the constant 1 / M -- exact in fp32 at M = 64 -- and gives attn no gradient)
                assert d > 0 or (not VARIANTS[var][0] and k.endswith("bin_r")), (tag, var, k)
                if is_whole(shape):
                    f64.append(b.reshape(-1))
                    f32.append(a.reshape(-1))
                else:
                    f64.append(subsample(b))
            key = f"{tag}:{var}"
            store[key + ":f64"] = torch.cat(f64).numpy().copy()
            if f32:
                store[key + ":f32"] = torch.cat(f32).numpy().copy()
            store[key + ":dref"] = np.array(dref)
            store[key + ":max"] = np.array(peak)
            print(f"{key:18s} gap {s64['gap']:.2e}  |norm - 0.1| {s64['dist']:.2e}  below 0.1: {100 * s64['low']:.0f} %  "
                  f"d_ref {min(dref):.2e} .. {max(dref):.2e}", flush=True)
    for name in FORWARD_CASES:
        o32, o64 = run_forward(R, U, name, torch.float32), run_forward(R, U, name, torch.float64)
        for k in FORWARD_KEYS:
            assert (k in o32) == (k in o64)
            if o64.get(k) is None:
                continue
            a, b = o32[k].detach(), o64[k].detach()
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape and b.numel() > 0, (name, k)
            d = (a.double() - b).abs().max().item()
            assert d > 0, (name, k)
            store[f"fwd:{name}:{k}:f64"], store[f"fwd:{name}:{k}:f32"] = b.numpy(), a.numpy()
            store[f"fwd:{name}:{k}:dref"] = np.float64(d)
            print(f"fwd {name:16s} {k:22s} {tuple(b.shape)}  d_ref {d:.2e}", flush=True)
    path = os.path.join(HERE, "sttr_head.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
