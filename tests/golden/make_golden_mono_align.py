"""Golden fixture for StereoAnywhere's mono-stereo alignment stage (tests/test_mono_align.py).

  python tests/golden/make_golden_mono_align.py        (build container only: needs the reference tree)

The reference's OWN models/StereoAnywhere/utils/utils.py (`generate_masks`, `softlrc`, `weighted_lsq`,
`handcrafted_mirror_detector`, `fuzzy_and`, `truncate_corr_volume_v2`) is executed on the seeded inputs of
tests/golden/mono_align_config.py, loaded by path with the `kornia.filters` stub exactly as make_golden_stereoanywhere.py does.
fp64: `weighted_lsq` casts with `.float()` and collects its result in a default-dtype `torch.zeros`; for the fp64 run the generator
makes `Tensor.float` a cast to float64 and float64 the default dtype around the calls -- the reference files are untouched.
Stored per tensor: the fp32 result (`:f32`), the fp64 result (`:f64`) and d_ref = max|fp32 - fp64| (`:dref`, must be > 0).
The fp32 run is made twice, before and after the fp64 run, and d_ref is the larger of the two errors: LAPACK's fp32 `gelsy`
behind `torch.linalg.lstsq` does not return the same bits in both (its code path follows the alignment of its buffers), so a
single run understates the reference's own fp32 error by several ulp.
The masks, the masked volume and its gradient are exact quantities: only the fp32 run is stored (in fp64 the reference's bin
comparison is a different function of the fp32 maps), and the test compares with `==`.

The generator asserts what makes the fp32 and the fp64 run differentiate the same branch:
  softlrc       no |disp - warped| and no non-planted relu argument within 1e-4 of its kink; both runs floor every sample column
                to the same tap, and no column that the two runs do not compute identically lies within 1e-4 of an integer;
  weighted_lsq  both runs select the same mask; no element other than the order statistics themselves lies within 1e-5
                (relative) of a threshold.
-> tests/golden/mono_align.npz
"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden_stereoanywhere import keep_fp64, reference  # noqa: E402
from tests.golden.mono_align_config import (ALIGN_ARGS, ALIGN_FIELDS, ALIGN_INPUTS, LRC_CASES, LRC_THRESHOLDS, LSQ_CASES,  # noqa: E402
                                            MASK_CASES, MIRROR_THRESHOLDS, QUANTILES, align_inputs, lrc_inputs, lsq_inputs,
                                            mask_inputs, mirror_inputs)


@contextlib.contextmanager
def all_fp64():
    """`.float()` as a cast to float64 and float64 as the default dtype (see the module docstring)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with keep_fp64():
            yield
    finally:
        torch.set_default_dtype(old)


def fp64_if(dtype):
    return all_fp64() if dtype == torch.float64 else contextlib.nullcontext()


def run_masks(U, tag):
    B, N, H, W2, W3 = MASK_CASES[tag]
    vol, left, right, gw = mask_inputs(tag)
    ml, mr = U.generate_masks(left, N=N), U.generate_masks(right, N=N)
    assert ml.dtype == torch.float16 and ml.shape == (B, N, H, W2)
    v = vol.clone().requires_grad_()
    out = v * ml.unsqueeze(4) * mr.unsqueeze(3)                          # stereoanywhere.py:180,193
    assert out.dtype == torch.float32 and out.shape == gw.shape
    (out * gw).sum().backward()
    assert ml.sum(1).max().item() == 1 and ml.sum(1).min().item() == 0 and out.abs().sum().item() > 0
    return {"left": ml, "right": mr, "out": out.detach(), "g_volume": v.grad}


def check_lrc_branches(U, tag):
    B, H, W, _ = LRC_CASES[tag]
    d2, d3, _ = lrc_inputs(tag)
    cols = {}
    for dt in (torch.float32, torch.float64):
        a, b = d2.to(dt), d3.to(dt)
        u2 = a - U.disp_warping(F.relu(a), b, right_disp=False)
        u3 = b - U.disp_warping(F.relu(b), a, right_disp=True)
        assert min(u2.abs().min().item(), u3.abs().min().item()) > 1e-4, (tag, "abs kink")
        x = torch.arange(W, dtype=dt).view(1, 1, 1, W)
        for name, d, sign in (("2", a, -1.0), ("3", b, 1.0)):
            gx = 2 * ((x + sign * F.relu(d)) / W) - 1
            cols[name, dt] = ((gx + 1) / 2) * (W - 1)                    # grid_sample, align_corners=True
    for d in (d2, d3):
        assert ((d.abs() > 1e-4) | (d == 0)).all(), (tag, "relu kink")
    for name in ("2", "3"):
        c32, c64 = cols[name, torch.float32].double(), cols[name, torch.float64]
        assert torch.equal(c32.floor(), c64.floor()), (tag, "tap")
        away = (c64 - c64.round()).abs() > 1e-4
        assert (away | (c32 == c64)).all(), (tag, "column kink")


def run_lrc(U, tag, dtype):
    d2, d3, gws = lrc_inputs(tag)
    a, b = d2.to(dtype).requires_grad_(), d3.to(dtype).requires_grad_()
    o2, o3 = U.softlrc(a, b, lrc_th=LRC_THRESHOLDS[tag])
    assert o2.dtype == dtype
    ((o2 * gws[0].to(dtype)).sum() + (o3 * gws[1].to(dtype)).sum()).backward()
    return {"out2": o2, "out3": o3, "g_disp2": a.grad, "g_disp3": b.grad}


def check_lsq_mask(tag):
    mde, disp, conf, _ = lsq_inputs(tag)
    B = disp.shape[0]
    thresholds = []
    for b in range(B):
        s32 = F.relu(disp[b]).flatten()
        s64 = s32.double()
        n = s32.numel()
        per = []
        for q in QUANTILES:
            t32, t64 = torch.quantile(s32, q), torch.quantile(s64, q)
            per.append(t32)
            r64, r32 = q * (n - 1), float(np.float32(q) * np.float32(n - 1))       # torch.quantile's rank in either dtype
            stats = torch.sort(s64).values[sorted({int(np.floor(r64)), int(np.ceil(r64)), int(np.floor(r32)), int(np.ceil(r32))})]
            tied = (s64.view(-1, 1) == stats.view(1, -1)).any(1)
            for t in (t32.double(), t64):
                assert (tied | ((s64 - t).abs() > 1e-5 * max(1.0, abs(t.item())))).all(), (tag, q, "near a threshold")
        lo32, hi32 = torch.quantile(s32, QUANTILES[0]), torch.quantile(s32, QUANTILES[1])
        lo64, hi64 = torch.quantile(s64, QUANTILES[0]), torch.quantile(s64, QUANTILES[1])
        assert torch.equal((lo32 <= s32) & (s32 <= hi32), (lo64 <= s64) & (s64 <= hi64)), (tag, "mask")
        if LSQ_CASES[tag][5]:
            srt = torch.sort(s32).values
            for q in QUANTILES:
                r = np.float32(q) * np.float32(n - 1)
                for k in (int(np.floor(r)), int(np.ceil(r))):
                    assert (s32 == srt[k]).sum().item() >= 2, (tag, q, "no tie at the order statistic")
        thresholds.append(torch.stack(per))
    return torch.stack(thresholds)


def run_lsq(U, tag, dtype):
    mde, disp, conf, gws = lsq_inputs(tag)
    m, d, c = (t.to(dtype).requires_grad_() for t in (mde, disp, conf))
    with fp64_if(dtype):
        scale, shift = U.weighted_lsq(m, d, c, min_quantile=QUANTILES[0], max_quantile=QUANTILES[1])
    assert scale.dtype == dtype and scale.shape == gws[0].shape
    ((scale * gws[0].to(dtype)).sum() + (shift * gws[1].to(dtype)).sum()).backward()
    return {"scale": scale, "shift": shift, "g_mde": m.grad, "g_disp": d.grad, "g_conf": c.grad}


def run_mirror(U, name, dtype):
    sd, md, sc, mc, gw = mirror_inputs()
    xs = [t.to(dtype).requires_grad_() for t in (sd, md, sc, mc)]
    out = U.handcrafted_mirror_detector(*xs, conf_th=MIRROR_THRESHOLDS[name])
    (out * gw.to(dtype)).sum().backward()
    return {"out": out, "g_sd": xs[0].grad, "g_md": xs[1].grad, "g_sc": xs[2].grad, "g_mc": xs[3].grad}


def run_align(U, dtype):
    """stereoanywhere.py:218-235 with the reference's functions, in its order"""
    x, gws = align_inputs()
    x = {k: v.to(dtype).requires_grad_() for k, v in x.items()}
    th = ALIGN_ARGS["lrc_th"]
    with fp64_if(dtype):
        lrc2, lrc3 = U.softlrc(x["dispmono2"], x["dispmono3"], lrc_th=th)
        conf2, conf3 = U.fuzzy_and(x["lconf2"], lrc2), U.fuzzy_and(x["lconf3"], lrc3)
        scale, shift = U.weighted_lsq(torch.cat([x["mde2"], x["mde3"]], 1), torch.cat([x["dispmono2"], x["dispmono3"]], 1),
                                      torch.cat([conf2, conf3], 1))
        scaled2 = torch.sum(scale * x["mde2"] + shift, dim=1, keepdim=True)
        scaled3 = torch.sum(scale * x["mde3"] + shift, dim=1, keepdim=True)
        lrcs2, _ = U.softlrc(scaled2, scaled3, lrc_th=th)
        mirror = U.handcrafted_mirror_detector(x["dispmono2"], scaled2, conf2, lrcs2, conf_th=ALIGN_ARGS["mirror_conf_th"])
        mask = U.truncate_corr_volume_v2(scaled2, mirror, conf_th=None, attenuation_gain=ALIGN_ARGS["mirror_attenuation"]).detach()
    fields = dict(zip(ALIGN_FIELDS, (lrc2, lrc3, conf2, conf3, scale, shift, scaled2, scaled3, lrcs2, mirror, mask)))
    assert all(v.dtype == dtype for v in fields.values())
    sum((fields[f] * g.to(dtype)).sum() for f, g in gws.items()).backward()
    res = dict(fields)
    res.update({"g_" + k: x[k].grad for k in ALIGN_INPUTS})
    return res


def main():
    _, U = reference()
    store = {}
    for tag in MASK_CASES:
        for k, v in run_masks(U, tag).items():
            store[f"mask:{tag}:{k}:f32"] = v.numpy()
            print(f"mask:{tag:10s} {k:10s} {tuple(v.shape)} {v.dtype}", flush=True)
    jobs = []
    for t in LRC_CASES:
        check_lrc_branches(U, t)
        jobs.append((f"lrc:{t}", lambda dt, t=t: run_lrc(U, t, dt)))
    for t in LSQ_CASES:
        store[f"lsq:{t}:thresholds:f32"] = check_lsq_mask(t).numpy()
        jobs.append((f"lsq:{t}", lambda dt, t=t: run_lsq(U, t, dt)))
    jobs += [(f"mirror:{n}", lambda dt, n=n: run_mirror(U, n, dt)) for n in MIRROR_THRESHOLDS]
    jobs.append(("align", lambda dt: run_align(U, dt)))
    for tag, fn in jobs:
        r32, r64, again = fn(torch.float32), fn(torch.float64), fn(torch.float32)
        for k in r32:
            a, b = r32[k].detach(), r64[k].detach()
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, (tag, k)
            dref = max((a.double() - b).abs().max().item(), (again[k].detach().double() - b).abs().max().item())
            assert dref > 0, (tag, k)
            store[f"{tag}:{k}:dref"] = np.float64(dref)
            store[f"{tag}:{k}:f32"] = a.numpy()
            store[f"{tag}:{k}:f64"] = b.numpy()
            print(f"{tag:18s} {k:20s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {dref:.3e}", flush=True)
    path = os.path.join(HERE, "mono_align.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
