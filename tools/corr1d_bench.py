"""Times the RAFT-family 1-D correlation pyramid and lookup (csrc/corr1d.hip) against the stock-PyTorch op sequence they replace,
on one GPU, at RAFT-Stereo's shape for a 576x960 input (1/4 resolution 144x240, 256-channel features, 4 levels, radius 4):

  (a) pyramid construction                  CorrBlock1D(fmap1, fmap2)                          (no autograd)
  (b) one lookup forward                    corr_fn(coords)                                    (no autograd)
  (c) construction + 32 lookups, forward and backward (gradients to fmap1 / fmap2)

The baseline is the op sequence of the reference's `corr_implementation="reg"` written with stock ATen operators (einsum,
avg_pool2d, linspace, cat, grid_sample) on the same device -- `BaselineCorr` below; it never calls the code under test and
reads nothing outside this repository.

Method (tools/geo_lookup_bench.py): every variant is warmed up, then the variants of an item are timed alternately
(round-robin) in one process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds`
samples is reported, with min / max.  One JSON line per item goes to --out.  `bytes` of (b) is the algorithmic traffic
computed from the shapes (windows read + positions read + output written); `frac_of_8TBps` = bytes / time / 8e12.  The pyramid
(about 62 MB) fits the 256 MiB Infinity Cache and the timed calls repeat on the same buffer, so (b) is a WARM figure.
`fill_ms` is a plain device fill of (b)'s output tensor on the same box.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd.models.RAFTStereo import CorrBlock1D  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402


class BaselineCorr:
    """models/RAFTStereo/corr.py:110-156 with utils/utils.py:59-74, operator for operator."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels, self.radius = num_levels, radius
        B, D, H, W1 = fmap1.shape
        corr = torch.einsum("aijk,aijh->ajkh", fmap1, fmap2).reshape(B, H, W1, 1, -1).contiguous()
        corr = corr / torch.sqrt(torch.tensor(D).float())
        corr = corr.reshape(B * H * W1, 1, 1, -1)
        self.corr_pyramid = [corr]
        for _ in range(num_levels):
            corr = F.avg_pool2d(corr, [1, 2], stride=[1, 2])
            self.corr_pyramid.append(corr)

    def __call__(self, coords):
        r = self.radius
        coords = coords[:, :1].permute(0, 2, 3, 1)
        b, h, w, _ = coords.shape
        out = []
        for i in range(self.num_levels):
            corr = self.corr_pyramid[i]
            dx = torch.linspace(-r, r, 2 * r + 1).view(2 * r + 1, 1).to(coords.device)
            x0 = dx + coords.reshape(b * h * w, 1, 1, 1) / 2 ** i
            grid = torch.cat([2 * x0 / (corr.shape[-1] - 1) - 1, torch.zeros_like(x0)], dim=-1)
            out.append(F.grid_sample(corr, grid, align_corners=True).view(b, h, w, -1))
        return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous().float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "corr1d_bench.jsonl"))
    ap.add_argument("--H", type=int, default=576)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--iters", type=int, default=32, help="lookups per step in (c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corr1d_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    B, Cf, L, r = 1, a.channels, 4, 4
    h, w = a.H // 4, a.W // 4
    K = 2 * r + 1
    f1, f2 = synthetic_tensor((B, Cf, h, w), 2).to(dev), synthetic_tensor((B, Cf, h, w), 3).to(dev)
    cols = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w).repeat(B, 1, h, 1)
    rows = torch.arange(h, dtype=torch.float32, device=dev).view(1, 1, h, 1).repeat(B, 1, 1, w)
    coords = [torch.cat([cols - synthetic_tensor((B, 1, h, w), 10 + i, lo=0.0, hi=47.0).to(dev), rows], dim=1) for i in range(a.iters)]
    npix = B * h * w
    shape = dict(B=B, h=h, w=w, fmap_channels=Cf, levels=L, radius=r, device=torch.cuda.get_device_name(0))
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
        t = alternate({"product": lambda: CorrBlock1D(f1, f2, num_levels=L, radius=r),
                       "baseline": lambda: BaselineCorr(f1, f2, L, r)}, a.reps, a.rounds, a.warmup)
        emit("a", "pyramid construction", t)
        # (b)
        prod, base = CorrBlock1D(f1, f2, num_levels=L, radius=r), BaselineCorr(f1, f2, L, r)
        out = prod(coords[0])
        err = (out - base(coords[0])).abs().max().item()
        t = alternate({"product": lambda: prod(coords[0]), "baseline": lambda: base(coords[0]),
                       "fill": lambda: out.fill_(1.0)}, 4 * a.reps, a.rounds, a.warmup)
        wr = out.numel() * 4
        rd = npix * (L * (K + 1) * 4 + 4)
        emit("b", "one lookup forward (warm: pyramid resident in the Infinity Cache)", t, bytes_written=wr, bytes_read=rd,
             bytes=wr + rd, frac_of_8TBps=round((wr + rd) / (t["product"][0] * 1e-3) / 8e12, 4),
             fill_frac_of_8TBps=round(wr / (t["fill"][0] * 1e-3) / 8e12, 4),
             product_write_rate_over_fill_rate=round(t["fill"][0] / t["product"][0], 3), max_abs_diff_vs_baseline=err)
        del prod, base, out

    # (c)
    gws = [synthetic_tensor((B, L * K, h, w), 40 + (i % 3)).to(dev) for i in range(a.iters)]
    leaves = [t_.detach().clone().requires_grad_() for t_ in (f1, f2)]

    def step(kind):
        for t_ in leaves:
            t_.grad = None
        fn = (BaselineCorr if kind == "baseline" else CorrBlock1D)(leaves[0], leaves[1], num_levels=L, radius=r)
        torch.autograd.backward([fn(c) for c in coords], gws)
        return [t_.grad for t_ in leaves]

    ref = [g.clone() for g in step("product")]
    vs_base = [(x - y).abs().max().item() for x, y in zip(step("baseline"), ref)]
    t = alternate({"product": lambda: step("product"), "baseline": lambda: step("baseline")}, max(1, a.reps // 2), a.rounds, 2)
    emit("c", f"pyramid construction + {a.iters} lookups forward + backward to fmap1 / fmap2", t, max_abs_diff_vs_baseline=vs_base)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
