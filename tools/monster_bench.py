"""Times MonSter's mutual-refinement stage (csrc/monster.hip, stereo_toolbox_amd.models.MonSter) against the stock-PyTorch op
sequence it replaces, on one GPU, at the model's two maps -- 96 x 144 x 240 (features at 1/4 of 576 x 960) and 3 x 576 x 960
(REMP's front) -- with B = 1 and B = 4:

  (a) one flaw: disp_warp(right, d)[0] - left                    stock: meshgrid, cat, normalise, 2 grid_samples (the second on a
                                                                 tensor of ones), 2 thresholds, 1 subtraction
  (b) the stereo + mono pair of one iteration                    stock: (a) twice; product: one launch, left read once
  (c) the alignment alone (1/4-resolution disparity maps)        stock: per sample a full sort, a boolean-mask gather, a 2 x 2
                                                                 solve and two .item() -- the reference's loop over the batch
  (d) the last eight iterations: 16 flaws + one alignment        forward, and forward + backward to both feature maps and both
                                                                 disparities (the alignment carries no gradient)
(a), (b): forward and forward + backward, with the peak memory of one forward + backward above what is resident before it.

The baseline is the op sequence of the reference's functions written with stock ATen operators on the same device; it never calls
the code under test and reads nothing outside this repository.  Method (tools/geo_lookup_bench.py): every variant is warmed up,
then the variants of an item are timed alternately in one process, each sample = device events around `--reps` back-to-back
executions; the median over `--rounds` samples is reported with min / max.  The maps of B = 1 (13.3 MB each at 96 channels) stay
in the 256 MiB Infinity Cache between repetitions, so these are WARM figures.  `fwd_fraction_of_8TBps` is the forward's compulsory
traffic (left, right and the disparities read once, the flaws written once) per second over 8 TB/s.  No time is fixed in advance.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd import ops  # noqa: E402
from stereo_toolbox_amd.models import MonSter as MS  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def stock_disp_warp(img, disp, padding_mode="border"):
    b, _, h, w = img.shape
    x_range = torch.arange(0, w, device=img.device).view(1, 1, w).expand(1, h, w).type_as(img)
    y_range = torch.arange(0, h, device=img.device).view(1, h, 1).expand(1, h, w).type_as(img)
    grid = torch.cat((x_range, y_range), dim=0).unsqueeze(0).expand(b, 2, h, w)
    grid = grid + torch.cat((-disp, torch.zeros_like(disp)), dim=1)
    grid = torch.stack((2 * (grid[:, 0] / (w - 1)) - 1, 2 * (grid[:, 1] / (h - 1)) - 1), dim=3)
    warped = F.grid_sample(img, grid, mode="bilinear", padding_mode=padding_mode)
    valid = F.grid_sample(torch.ones_like(img), grid, mode="bilinear", padding_mode=padding_mode)
    valid[valid < 0.9999] = 0
    valid[valid > 0] = 1
    return warped, valid


def stock_flaw(left, right, disp):
    return stock_disp_warp(right, disp)[0] - left


def stock_scale_shift(mono, gt):
    srt, _ = torch.sort(mono.clone().view(-1).contiguous())
    thr = srt[int(0.2 * len(srt))]
    mask = (gt > 0) & (mono > 1e-2) & (mono > thr)
    m, g = mono[mask], gt[mask]
    X = torch.stack([m, torch.ones_like(m)], dim=1)
    A = torch.matmul(X.t(), X) + 1e-6 * torch.eye(2, device=X.device)
    p = torch.linalg.solve(A, torch.matmul(X.t(), g))
    return p[0].item(), p[1].item()


def stock_align(mono, gt):
    out = mono.clone()
    for i in range(mono.shape[0]):
        scale, shift = stock_scale_shift(mono[i].clone().squeeze(1), gt[i].clone().squeeze(1))
        out[i] = scale * out[i] + shift
    return out


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "monster_bench.jsonl"))
    ap.add_argument("--shapes", type=int, nargs=3, action="append", metavar=("C", "H", "W"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--iters", type=int, default=8, help="iterations of (d)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("monster_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    lines = []

    for C, H, W in a.shapes or [(96, 144, 240), (3, 576, 960)]:
        for B in a.batches:
            shape = dict(B=B, C=C, H=H, W=W, device=torch.cuda.get_device_name(0))
            left, right = (synthetic_tensor((B, C, H, W), 80 + i).to(dev) for i in range(2))
            ds = synthetic_tensor((B, 1, H, W), 82, lo=1.0, hi=W / 5.0).to(dev)
            dm = (0.6 * ds + synthetic_tensor((B, 1, H, W), 83, lo=-1.0, hi=1.0).to(dev)).contiguous()
            gw = [synthetic_tensor((B, C, H, W), 84 + i).to(dev) for i in range(2)]
            leaves = [t.clone().requires_grad_() for t in (left, right, ds, dm)]

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

            def step(fn):
                """forward + backward of fn(left, right, ds, dm) -> list of flaws, to all four inputs"""
                for leaf in leaves:
                    leaf.grad = None
                outs = fn(*leaves)
                torch.autograd.backward(outs, [gw[i % 2] for i in range(len(outs))])
                return [leaf.grad for leaf in leaves]

            def fraction(ms, flaws):
                moved = 4.0 * B * H * W * (C * (2 + flaws) + flaws)
                return round(moved / (ms * 1e-3) / PEAK_BYTES_PER_S, 4)

            one_p = lambda l, r, s, m: [ops.monster_flaws(l, r, s)]  # noqa: E731
            one_b = lambda l, r, s, m: [stock_flaw(l, r, s)]  # noqa: E731
            pair_p = lambda l, r, s, m: list(MS.mutual_flaws(l, r, s, m))  # noqa: E731
            pair_b = lambda l, r, s, m: [stock_flaw(l, r, s), stock_flaw(l, r, m)]  # noqa: E731

            def seq(flaws, align):
                def run(l, r, s, m):
                    m = align(m, s.detach())
                    outs = []
                    for _ in range(a.iters):
                        outs += flaws(l, r, s, m)
                    return outs
                return run

            seq_p, seq_b = seq(pair_p, MS.align_mono_disp), seq(pair_b, stock_align)

            with torch.no_grad():
                for item, what, p, b, n in (("a", "one flaw", one_p, one_b, 1), ("b", "stereo + mono flaws", pair_p, pair_b, 2)):
                    err = max((x - y).abs().max().item() for x, y in zip(p(left, right, ds, dm), b(left, right, ds, dm)))
                    t = alternate({"product": lambda: p(left, right, ds, dm), "baseline": lambda: b(left, right, ds, dm)},
                                  a.reps, a.rounds, a.warmup)
                    emit(item, what + ", forward", t, max_abs_diff_vs_baseline=err, fwd_fraction_of_8TBps=fraction(t["product"][0], n),
                         baseline_fraction_of_8TBps=fraction(t["baseline"][0], n))
                err = (MS.align_mono_disp(dm, ds) - stock_align(dm, ds)).abs().max().item()
                both("c", "alignment of the mono disparity (baseline: sort, mask gather, solve, 2 x .item() per sample)",
                     lambda: MS.align_mono_disp(dm, ds), lambda: stock_align(dm, ds), max_abs_diff_vs_baseline=err)
                both("d", f"{a.iters} iterations: {2 * a.iters} flaws + one alignment, forward",
                     lambda: seq_p(left, right, ds, dm), lambda: seq_b(left, right, ds, dm))
            for item, what, p, b in (("a", "one flaw", one_p, one_b), ("b", "stereo + mono flaws", pair_p, pair_b)):
                ref = [g.clone() for g in step(p) if g is not None]
                err = max((x - y).abs().max().item() for x, y in zip(ref, [g for g in step(b) if g is not None]))
                both(item, what + ", forward + backward", lambda: step(p), lambda: step(b), max_abs_grad_diff_vs_baseline=err,
                     product_peak_mb=peak_mb(lambda: step(p)), baseline_peak_mb=peak_mb(lambda: step(b)))
            both("d", f"{a.iters} iterations: {2 * a.iters} flaws + one alignment, forward + backward",
                 lambda: step(seq_p), lambda: step(seq_b), product_peak_mb=peak_mb(lambda: step(seq_p)),
                 baseline_peak_mb=peak_mb(lambda: step(seq_b)))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
