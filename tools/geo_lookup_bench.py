"""Times the IGEV geometry-encoding lookup and the convex upsampling (csrc/geo_lookup.hip) against the stock-PyTorch op sequence
they replace, on one GPU, at IGEV's shape for a 576x960 input (1/4 resolution 144x240, D/4 = 48, 8 volume channels, 96-channel
matching features, radius 4, 2 levels):

  (a) pyramid construction            Combined_Geo_Encoding_Volume(...)                       (no autograd)
  (b) one lookup forward              geo_fn(disp, coords)                                    (no autograd)
  (c) 22 lookups forward + backward   the GRU-iteration pattern, gradients to geo_volume / init_fmap1 / init_fmap2
  (d) context_upsample forward + backward at 576x960, gradients to disp_low and up_weights

The baseline is the op sequence of the reference written with stock ATen operators (einsum, avg_pool2d, linspace, cat,
grid_sample, unfold, nearest interpolate) on the same device -- `Baseline*` below; it never calls the code under test.
(c) is also run for the alternative the product does NOT ship: a lookup backward that returns its own zero-filled pyramid-sized
gradient tensors for autograd to add (`DenseGradLookupFn`, here only), which is what DESIGN.md's choice between the two rests on.

Method: every variant is warmed up, then the variants of an item are timed alternately (round-robin) in one process, each
sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported, with min / max.
One JSON line per item goes to --out.  `bytes` is the algorithmic traffic computed from the shapes (windows read + output
written for (b); operands and results once for (d)); `frac_of_8TBps` = bytes / time / 8e12.  Both pyramids (about 130 MB) fit
the 256 MiB Infinity Cache and the timed calls repeat on the same buffers, so (b) is a WARM figure: its reads come from the
Infinity Cache, not from HBM.  `fill_ms` is a plain device fill of (b)'s output tensor on the same box.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd import ops  # noqa: E402
from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume, context_upsample  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402


# ------------------------------------------------------------------------------------------------ stock-op baseline
def _sample_rows(img, x):
    """img [N, C, 1, L], x [N, 1, K, 1] pixel positions -> grid_sample along the row (align_corners=True, zero padding)."""
    L = img.shape[-1]
    grid = torch.cat([2 * x / (L - 1) - 1, torch.zeros_like(x)], dim=-1)
    return F.grid_sample(img, grid, align_corners=True)


class BaselineGeo:
    def __init__(self, fmap1, fmap2, geo, num_levels=2, radius=4):
        self.num_levels, self.radius = num_levels, radius
        corr = torch.einsum("aijk,aijh->ajkh", fmap1, fmap2)
        b, c, d, h, w = geo.shape
        g = geo.permute(0, 3, 4, 1, 2).reshape(b * h * w, c, 1, d)
        r = corr.reshape(b * h * w, 1, 1, corr.shape[-1])
        self.geo, self.corr = [g], [r]
        for _ in range(num_levels - 1):
            g, r = F.avg_pool2d(g, [1, 2], stride=[1, 2]), F.avg_pool2d(r, [1, 2], stride=[1, 2])
            self.geo.append(g)
            self.corr.append(r)

    def __call__(self, disp, coords):
        b, _, h, w = disp.shape
        r = self.radius
        dx = torch.linspace(-r, r, 2 * r + 1).view(1, 1, 2 * r + 1, 1).to(disp.device)
        d, c = disp.reshape(b * h * w, 1, 1, 1), coords.reshape(b * h * w, 1, 1, 1)
        out = []
        for i in range(self.num_levels):
            out.append(_sample_rows(self.geo[i], dx + d / 2 ** i).view(b, h, w, -1))
            out.append(_sample_rows(self.corr[i], c / 2 ** i - d / 2 ** i + dx).view(b, h, w, -1))
        return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous().float()


def baseline_upsample(disp_low, up_weights):
    b, c, h, w = disp_low.shape
    u = F.unfold(disp_low, 3, 1, 1).reshape(b, -1, h, w)
    u = F.interpolate(u, (h * 4, w * 4), mode="nearest").reshape(b, 9, h * 4, w * 4)
    return (u * up_weights).sum(1)


# ------------------------------------------------------------------------------------------------ the variant not shipped
class DenseGradLookupFn(torch.autograd.Function):
    """The same kernels with the straightforward gradient flow: every call's backward fills its OWN zeroed pyramid-sized
    tensors and autograd adds the 22 of them."""

    @staticmethod
    def forward(ctx, gpyr, cpyr, disp, coords, cfg):
        ctx.save_for_backward(disp, coords)
        ctx.cfg, ctx.sizes = cfg, (gpyr.numel(), cpyr.numel())
        return ops.GeoLookupFn.forward(ops._NoCtx(), gpyr, cpyr, disp, coords, cfg, None)

    @staticmethod
    def backward(ctx, gout):
        disp, coords = ctx.saved_tensors
        ggp = torch.zeros(ctx.sizes[0], dtype=torch.float32, device=disp.device)
        gcp = torch.zeros(ctx.sizes[1], dtype=torch.float32, device=disp.device)
        ops._call("stx_geo_lookup_bwd", ops._p(gout.contiguous()), ops._p(disp), ops._p(coords), ops._p(ggp), ops._p(gcp), *ctx.cfg)
        return ggp, gcp, None, None, None


# ------------------------------------------------------------------------------------------------ timing
def sample_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(variants, reps, rounds, warmup):
    """variants: {name: callable}; -> {name: (median, min, max)} in ms, the variants timed round-robin."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(sample_ms(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "geo_lookup_bench.jsonl"))
    ap.add_argument("--H", type=int, default=576)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--maxdisp", type=int, default=192)
    ap.add_argument("--iters", type=int, default=22, help="lookups per step in (c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geo_lookup_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    B, C, Cf, L, r = 1, 8, 96, 2, 4
    h, w, D = a.H // 4, a.W // 4, a.maxdisp // 4
    K = 2 * r + 1
    geo = synthetic_tensor((B, D, h, w, C), 1).to(dev).permute(0, 4, 1, 2, 3)          # the view the aggregation returns
    f1, f2 = synthetic_tensor((B, Cf, h, w), 2).to(dev), synthetic_tensor((B, Cf, h, w), 3).to(dev)
    coords = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w).repeat(B, 1, h, 1)
    disps = [synthetic_tensor((B, 1, h, w), 10 + i, lo=0.0, hi=float(D - 1)).to(dev) for i in range(a.iters)]
    npix = B * h * w
    shape = dict(B=B, h=h, w=w, D=D, C=C, fmap_channels=Cf, levels=L, radius=r, device=torch.cuda.get_device_name(0))
    lines = []

    def emit(item, what, t, **extra):
        rec = dict(item=item, what=what, **shape, reps=a.reps, rounds=a.rounds)
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    with torch.no_grad():
        # (a)
        t = alternate({"product": lambda: Combined_Geo_Encoding_Volume(f1, f2, geo, num_levels=L, radius=r),
                       "baseline": lambda: BaselineGeo(f1, f2, geo, L, r)}, a.reps, a.rounds, a.warmup)
        emit("a", "pyramid construction", t)
        # (b)
        prod, base = Combined_Geo_Encoding_Volume(f1, f2, geo, num_levels=L, radius=r), BaselineGeo(f1, f2, geo, L, r)
        out = prod(disps[0], coords)
        err = (out - base(disps[0], coords)).abs().max().item()
        t = alternate({"product": lambda: prod(disps[0], coords), "baseline": lambda: base(disps[0], coords),
                       "fill": lambda: out.fill_(1.0)}, 4 * a.reps, a.rounds, a.warmup)
        wr = out.numel() * 4
        rd = npix * (L * (K + 1) * (C + 1) * 4 + 8)
        emit("b", "one lookup forward (warm: pyramids resident in the Infinity Cache)", t, bytes_written=wr, bytes_read=rd,
             bytes=wr + rd, frac_of_8TBps=round((wr + rd) / (t["product"][0] * 1e-3) / 8e12, 4),
             fill_frac_of_8TBps=round(wr / (t["fill"][0] * 1e-3) / 8e12, 4),
             product_write_rate_over_fill_rate=round(t["fill"][0] / t["product"][0], 3), max_abs_diff_vs_baseline=err)
        del prod, base, out

    # (c)
    gws = [synthetic_tensor((B, L * (C + 1) * K, h, w), 40 + (i % 3)).to(dev) for i in range(a.iters)]
    leaves = [t_.detach().clone().requires_grad_() for t_ in (geo, f1, f2)]

    def step(kind):
        for t_ in leaves:
            t_.grad = None
        g, a1, a2 = leaves
        if kind == "baseline":
            fn = BaselineGeo(a1, a2, g, L, r)
            outs = [fn(d, coords) for d in disps]
        else:
            fn = Combined_Geo_Encoding_Volume(a1, a2, g, num_levels=L, radius=r)
            if kind == "product":
                outs = [fn(d, coords) for d in disps]
            else:
                outs = [DenseGradLookupFn.apply(fn.geo_volume_pyramid, fn.init_corr_pyramid, d, coords, fn._cfg) for d in disps]
        torch.autograd.backward(outs, gws)
        return [t_.grad for t_ in leaves]

    ref = [g.clone() for g in step("product_dense_grads")]
    same = [(x - y).abs().max().item() for x, y in zip(step("product"), ref)]
    vs_base = [(x - y).abs().max().item() for x, y in zip(step("baseline"), ref)]
    t = alternate({"product": lambda: step("product"), "product_dense_grads": lambda: step("product_dense_grads"),
                   "baseline": lambda: step("baseline")}, max(1, a.reps // 2), a.rounds, 2)
    emit("c", f"pyramid construction + {a.iters} lookups forward + backward to geo_volume / fmaps", t,
         accumulated_over_dense_speedup=round(t["product_dense_grads"][0] / t["product"][0], 3),
         max_abs_diff_accumulated_vs_dense=same, max_abs_diff_baseline_vs_dense=vs_base)
    del leaves, ref

    # (d)
    dl = synthetic_tensor((B, 1, h, w), 60, lo=0.0, hi=float(D - 1)).to(dev).requires_grad_()
    wt = torch.softmax(synthetic_tensor((B, 9, 4 * h, 4 * w), 61).to(dev), dim=1).requires_grad_()
    gu = synthetic_tensor((B, 4 * h, 4 * w), 62).to(dev)

    def up(fn):
        dl.grad = wt.grad = None
        fn(dl, wt).backward(gu)

    t = alternate({"product": lambda: up(context_upsample), "baseline": lambda: up(baseline_upsample)}, 2 * a.reps, a.rounds,
                  a.warmup)
    full, low = B * 16 * h * w * 4, B * h * w * 4
    nbytes = (9 * full + low + full) + (full + low + 9 * full) + (full + 9 * full + low)     # fwd | g weights | g disp
    emit("d", "context_upsample forward + backward", t, bytes=nbytes,
         frac_of_8TBps=round(nbytes / (t["product"][0] * 1e-3) / 8e12, 4))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
