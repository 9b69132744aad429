"""Times the self-supervised losses (csrc/selfsup_loss.hip, stereo_toolbox_amd.loss_functions) against the stock-PyTorch op sequence
they replace, on one GPU, at 576 x 960 with B = 1 and B = 4, forward alone and forward + backward to the disparity:

  (a) photometric_loss(left, right, disp)                       stock: 2 grid_samples, 2 reflect pads, 5 avg_pool2ds, ~20 elementwise
  (b) auto_mask(left, right, disp)                              stock: the above twice, forward only
  (c) smoothness_loss(disp, left, warn=False)                   stock: with the img.max() > 1 host sync of the reference
  (d) 4 predictions x (photometric with auto-mask + smoothness) the objective of one self-supervised training step

The baseline is the op sequence of the reference's functions written with stock ATen operators on the same device; it never calls
the code under test and reads nothing outside this repository.  Method (tools/geo_lookup_bench.py): every variant is warmed up,
then the variants of an item are timed alternately in one process, each sample = device events around `--reps` back-to-back
executions; the median over `--rounds` samples is reported with min / max.  The images (6.6 MB each at B = 1) stay in the 256 MiB
Infinity Cache between repetitions, so these are WARM figures.  No time is fixed in advance.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd import loss_functions as LF  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402


def stock_warp(right, disp):
    B, _, H, W = right.shape
    xs = torch.linspace(0, 1, W, device=disp.device).view(1, 1, W).expand(B, H, W)
    ys = torch.linspace(0, 1, H, device=disp.device).view(1, H, 1).expand(B, H, W)
    grid = torch.stack((xs - disp[:, 0] / (W - 1), ys), dim=3) * 2 - 1
    warped = F.grid_sample(right, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    valid = F.grid_sample(torch.ones_like(right), grid, mode="bilinear", padding_mode="zeros", align_corners=False).detach()
    return warped, valid


def stock_ssim(x, y, ws=7):
    p = ws // 2
    xp, yp = F.pad(x, (p, p, p, p), mode="reflect"), F.pad(y, (p, p, p, p), mode="reflect")
    mx, my = F.avg_pool2d(xp, ws, stride=1), F.avg_pool2d(yp, ws, stride=1)
    vx = F.avg_pool2d(xp * xp, ws, stride=1) - mx.pow(2)
    vy = F.avg_pool2d(yp * yp, ws, stride=1) - my.pow(2)
    cxy = F.avg_pool2d(xp * yp, ws, stride=1) - mx * my
    n = (2 * mx * my + 0.01 ** 2) * (2 * cxy + 0.03 ** 2)
    d = (mx.pow(2) + my.pow(2) + 0.01 ** 2) * (vx + vy + 0.03 ** 2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def stock_photometric(left, right, disp=None, w=0.85, mask=True):
    warped, valid = (right, None) if disp is None else stock_warp(right, disp)
    loss = w * stock_ssim(left, warped) + (1 - w) * torch.abs(left - warped)
    if mask:
        loss = loss * valid
    return loss.mean(1, True)


def stock_auto_mask(left, right, disp):
    return stock_photometric(left, right, disp.detach(), mask=False) < stock_photometric(left, right, mask=False)


def stock_smoothness(disp, img):
    if img.max() > 1.0:
        print("Warning: Image may not be normalized. Expected range: [0,1]")
    n = disp / (disp.mean(2, True).mean(3, True) + 1e-7)
    dx, dy = torch.abs(n[:, :, :, :-1] - n[:, :, :, 1:]), torch.abs(n[:, :, :-1, :] - n[:, :, 1:, :])
    wx = torch.exp(-torch.mean(torch.abs(img[:, :, :, :-1] - img[:, :, :, 1:]), 1, keepdim=True))
    wy = torch.exp(-torch.mean(torch.abs(img[:, :, :-1, :] - img[:, :, 1:, :]), 1, keepdim=True))
    return torch.mean(dx * wx) + torch.mean(dy * wy)


def objective(photometric, auto_mask, smoothness, left, right, disps):
    """4 predictions x (auto-masked photometric + 0.1 smoothness), a scalar"""
    total = 0
    for d in disps:
        m = auto_mask(left, right, d)
        total = total + (photometric(left, right, d) * m).mean() + 0.1 * smoothness(d, left)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "selfsup_loss_bench.jsonl"))
    ap.add_argument("--H", type=int, default=576)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("selfsup_loss_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    lines = []
    quiet = lambda d, img: LF.smoothness_loss(d, img, warn=False)  # noqa: E731

    for B in a.batches:
        shape = dict(B=B, C=3, H=a.H, W=a.W, device=torch.cuda.get_device_name(0))
        left = F.avg_pool2d(synthetic_tensor((B, 3, a.H + 4, a.W + 4), 50, lo=0.0, hi=1.0), 5, stride=1).contiguous().to(dev)
        right = F.avg_pool2d(synthetic_tensor((B, 3, a.H + 4, a.W + 4), 51, lo=0.0, hi=1.0), 5, stride=1).contiguous().to(dev)
        disps = [synthetic_tensor((B, 1, a.H, a.W), 60 + i, lo=1.0, hi=64.0).to(dev) for i in range(4)]
        gw = synthetic_tensor((B, 1, a.H, a.W), 70).to(dev)

        def emit(item, what, t, **extra):
            rec = dict(item=item, what=what, **shape, reps=a.reps, rounds=a.rounds)
            for k, (med, lo, hi) in t.items():
                rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
            rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
            rec.update(extra)
            lines.append(rec)
            print(json.dumps(rec), flush=True)

        def both(item, what, product, baseline, **extra):
            emit(item, what, alternate({"product": product, "baseline": baseline}, a.reps, a.rounds, a.warmup), **extra)

        leaves = [d.clone().requires_grad_() for d in disps]

        def step(fn, weight=None):
            for leaf in leaves:
                leaf.grad = None
            out = fn()
            out.backward(weight) if weight is not None else out.backward()
            return leaves[0].grad

        with torch.no_grad():
            err = (LF.photometric_loss(left, right, disps[0]) - stock_photometric(left, right, disps[0])).abs().max().item()
            both("a", "photometric_loss, forward", lambda: LF.photometric_loss(left, right, disps[0]),
                 lambda: stock_photometric(left, right, disps[0]), max_abs_diff_vs_baseline=err)
            same = (LF.auto_mask(left, right, disps[0]) == stock_auto_mask(left, right, disps[0])).float().mean().item()
            both("b", "auto_mask, forward", lambda: LF.auto_mask(left, right, disps[0]), lambda: stock_auto_mask(left, right, disps[0]),
                 agreement_with_baseline=same)
            err = abs(quiet(disps[0], left).item() - stock_smoothness(disps[0], left).item())
            both("c", "smoothness_loss, forward (baseline with the reference's host sync)", lambda: quiet(disps[0], left),
                 lambda: stock_smoothness(disps[0], left), max_abs_diff_vs_baseline=err)
            both("d", "4 predictions x (photometric with auto-mask + smoothness), forward",
                 lambda: objective(LF.photometric_loss, LF.auto_mask, quiet, left, right, disps),
                 lambda: objective(stock_photometric, stock_auto_mask, stock_smoothness, left, right, disps))
        ref = step(lambda: LF.photometric_loss(left, right, leaves[0]), gw).clone()
        err = (step(lambda: stock_photometric(left, right, leaves[0]), gw) - ref).abs().max().item()
        both("a", "photometric_loss, forward + backward", lambda: step(lambda: LF.photometric_loss(left, right, leaves[0]), gw),
             lambda: step(lambda: stock_photometric(left, right, leaves[0]), gw), max_abs_diff_vs_baseline=err)
        ref = step(lambda: quiet(leaves[0], left)).clone()
        err = (step(lambda: stock_smoothness(leaves[0], left)) - ref).abs().max().item()
        both("c", "smoothness_loss, forward + backward", lambda: step(lambda: quiet(leaves[0], left)),
             lambda: step(lambda: stock_smoothness(leaves[0], left)), max_abs_diff_vs_baseline=err)
        both("d", "4 predictions x (photometric with auto-mask + smoothness), forward + backward",
             lambda: step(lambda: objective(LF.photometric_loss, LF.auto_mask, quiet, left, right, leaves)),
             lambda: step(lambda: objective(stock_photometric, stock_auto_mask, stock_smoothness, left, right, leaves)))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
