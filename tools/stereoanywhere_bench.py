"""Times StereoAnywhere's volume stage (csrc/allpairs.hip) against the stock-PyTorch op sequence it replaces, on one GPU, at the
model's shape for a 576x960 input (1/4 resolution: B = 1, H = 144, W1 = W2 = 240; the volume is 33 MB):

  (a) the four-output estimator set, forward                 estimate_all(volume)                       (no autograd)
  (b) the set forward + backward to the volume
  (c) pyramid from the volume                                 CorrBlock1D(fullcorr)                      (no autograd)
  (d) pyramid from the volume with the truncation mask        CorrBlock1D(fullcorr, truncate=...)  vs  mask * volume -> block
  (e) one lookup forward                                      corr_fn(coords)

The baseline is the op sequence of the reference's functions written with stock ATen operators (softmax, arange broadcasts,
log2, sum, sigmoid, avg_pool2d, grid_sample) on the same device; it never calls the code under test and reads nothing outside
this repository.  Method (tools/geo_lookup_bench.py): every variant is warmed up, then the variants of an item are timed
alternately in one process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds`
samples is reported with min / max.  `volume_bytes_per_s` of (a) / (b) is the volume's size over the product's time: the
algorithmic traffic is the volume read once per direction (forward) plus read and written once (backward); the timed calls repeat
on one 33 MB buffer, which fits the 256 MiB Infinity Cache, so these are WARM figures.  No time is fixed in advance: the baseline
is the stock sequence on the same box in the same run.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd.models import StereoAnywhere as SA  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402


def baseline_estimates(volume):
    """utils/utils.py:112-170 as the model calls it: four functions, each with its own softmax of the volume."""
    v = volume.squeeze(1)
    B, H, W2, W3 = v.shape
    a2 = torch.arange(W2, dtype=v.dtype, device=v.device)
    a3 = torch.arange(W3, dtype=v.dtype, device=v.device)
    disp_l = a2.view(1, 1, W2) - torch.sum(F.softmax(v, dim=3) * a3.view(1, 1, 1, W3), 3)
    disp_r = torch.sum(F.softmax(v, dim=2) * a2.view(1, 1, W2, 1), 2) - a3.view(1, 1, W3)
    pl = F.softmax(v, dim=3)
    conf_l = 1 - (-torch.sum(pl * torch.log2(pl + 1e-6), dim=3) / math.log2(W3))
    pr = F.softmax(v, dim=2)
    conf_r = 1 - (-torch.sum(pr * torch.log2(pr + 1e-6), dim=2) / math.log2(W2))
    return tuple(t.unsqueeze(1) for t in (disp_l, conf_l, disp_r, conf_r))


def baseline_mask(disp, conf, atten):
    """utils/utils.py:216-238 with conf_th=None"""
    W = disp.shape[3]
    a = torch.arange(W, dtype=disp.dtype, device=disp.device)
    c = conf.unsqueeze(4)
    x = (a.view(1, 1, 1, W) - disp).unsqueeze(4) - a.view(1, 1, 1, 1, W)
    return 1 * (1 - c) + c * (torch.sigmoid(x) * (1 - atten) + atten)


class BaselineBlock:
    """corr.py:75-115 with utils/utils.py:19-35, operator for operator."""

    def __init__(self, fullcorr, num_levels=4, radius=4, pad=(0, 0)):
        self.num_levels, self.radius, self.pad = num_levels, radius, pad
        b, h, w1, dim, w2 = fullcorr.shape
        corr = fullcorr.reshape(b * h * w1, dim, 1, w2)
        self.corr_pyramid = [corr]
        for _ in range(num_levels):
            corr = F.avg_pool2d(corr, [1, 2], stride=[1, 2])
            self.corr_pyramid.append(corr)

    def __call__(self, coords):
        r = self.radius
        coords = coords[:, :1].permute(0, 2, 3, 1) + self.pad[0]
        b, h, w, _ = coords.shape
        out = []
        for i in range(self.num_levels):
            corr = self.corr_pyramid[i]
            dx = torch.linspace(-r, r, 2 * r + 1).view(1, 1, 2 * r + 1, 1).to(coords.device)
            x0 = dx + coords.reshape(b * h * w, 1, 1, 1) / 2 ** i
            grid = torch.cat([2 * x0 / (corr.shape[-1] - 1) - 1, torch.zeros_like(x0)], dim=-1)
            out.append(F.grid_sample(corr.float(), grid, align_corners=True).view(b, h, w, -1)[:, :, self.pad[0]:w - self.pad[1], :])
        return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "stereoanywhere_bench.jsonl"))
    ap.add_argument("--H", type=int, default=576)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stereoanywhere_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    B, L, r, atten = 1, 4, 4, 0.1
    h, w = a.H // 4, a.W // 4
    vol = (sum(synthetic_tensor((B, 1, h, w, w), 7, stream=k) for k in range(3)) * (4.0 / 3.0 ** 0.5)).to(dev)
    vol_bytes = vol.numel() * 4
    gws = [synthetic_tensor((B, 1, h, w), 20 + i).to(dev) for i in range(4)]
    disp = synthetic_tensor((B, 1, h, w), 30, lo=0.0, hi=47.0).to(dev)
    conf = synthetic_tensor((B, 1, h, w), 31, lo=0.0, hi=1.0).to(dev)
    cols = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w).repeat(B, 1, h, 1)
    rows = torch.arange(h, dtype=torch.float32, device=dev).view(1, 1, h, 1).repeat(B, 1, 1, w)
    coords = torch.cat([cols - disp, rows], dim=1)
    fullcorr = vol[:, 0].unsqueeze(3).contiguous()
    shape = dict(B=B, h=h, w1=w, w2=w, levels=L, radius=r, volume_bytes=vol_bytes, device=torch.cuda.get_device_name(0))
    lines = []

    def emit(item, what, t, **extra):
        rec = dict(item=item, what=what, **shape, reps=a.reps, rounds=a.rounds)
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def rate(t):
        return round(vol_bytes / (t["product"][0] * 1e-3), 1)

    with torch.no_grad():
        err = [(x - y).abs().max().item() for x, y in zip(SA.estimate_all(vol), baseline_estimates(vol))]
        t = alternate({"product": lambda: SA.estimate_all(vol), "baseline": lambda: baseline_estimates(vol)}, a.reps, a.rounds, a.warmup)
        emit("a", "four-output estimator set, forward", t, volume_bytes_per_s=rate(t), max_abs_diff_vs_baseline=err)

    leaf = vol.detach().clone().requires_grad_()

    def step(fn):
        leaf.grad = None
        torch.autograd.backward(list(fn(leaf)), gws)
        return leaf.grad

    ref = step(SA.estimate_all).clone()
    err = (step(baseline_estimates) - ref).abs().max().item()
    t = alternate({"product": lambda: step(SA.estimate_all), "baseline": lambda: step(baseline_estimates)}, a.reps, a.rounds, a.warmup)
    emit("b", "four-output estimator set, forward + backward to the volume", t, volume_bytes_per_s=rate(t), max_abs_diff_vs_baseline=err)

    with torch.no_grad():
        t = alternate({"product": lambda: SA.CorrBlock1D(fullcorr, num_levels=L, radius=r),
                       "baseline": lambda: BaselineBlock(fullcorr, L, r)}, a.reps, a.rounds, a.warmup)
        emit("c", "pyramid from the volume", t)
        t = alternate({"product": lambda: SA.CorrBlock1D(fullcorr, num_levels=L, radius=r, truncate=(disp, conf, atten)),
                       "baseline": lambda: BaselineBlock((baseline_mask(disp, conf, atten)[:, 0] * fullcorr.squeeze(3)).unsqueeze(3), L, r)},
                      a.reps, a.rounds, a.warmup)
        emit("d", "pyramid from the volume times the truncation mask (baseline: mask volume, product, pyramid)", t)
        prod, base = SA.CorrBlock1D(fullcorr, num_levels=L, radius=r), BaselineBlock(fullcorr, L, r)
        err = (prod(coords) - base(coords)).abs().max().item()
        t = alternate({"product": lambda: prod(coords), "baseline": lambda: base(coords)}, 4 * a.reps, a.rounds, a.warmup)
        emit("e", "one lookup forward (warm)", t, max_abs_diff_vs_baseline=err)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
