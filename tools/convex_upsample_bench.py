"""Times convex upsampling from logits and the sequence loss (csrc/convex_upsample.hip) against the stock-PyTorch op sequences they
replace, on one GPU, at 576x960 and 384x1248, N = 1 and N = 4:

  (a) one RAFT-layout call (upsample_flow / convex_upflow), forward, and forward + backward, n_downsample 2 and 3, D = 2
  (b) 22 such calls forward + backward (train_iters = 22) at n_downsample 2, with the peak device memory of both sides
  (c) the pixel-layout call (IGEV family) forward + backward against softmax + the existing ops.context_upsample, and against the
      stock sequence softmax + unfold + nearest interpolate
  (d) sequence_loss with 23 predictions against losses.masked_smooth_l1_multi, forward + backward

The baseline of (a), (b) is the reference's sequence written with stock ATen operators (view, softmax, unfold, product, sum,
permute, reshape) in this file; it never calls the code under test, and nothing outside the repository is read.

Method (tools/geo_lookup_bench.py, `alternate`): every variant is warmed up, then the variants of an item are timed alternately in
one process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported
with min / max.  `mask_bytes` is one read of the mask (the floor of a forward: 20 MB at 576x960, N = 1); `product_GBps` =
(mask read + output written) / forward time, i.e. the achieved rate next to that floor.  One JSON line per item goes to --out.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from geo_lookup_bench import alternate  # noqa: E402
from stereo_toolbox_amd import losses, ops  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402


def baseline_convex(flow, mask, n_downsample):
    N, D, H, W = flow.shape
    f = 2 ** n_downsample
    mask = torch.softmax(mask.view(N, 1, 9, f, f, H, W), dim=2)
    up = F.unfold(f * flow, [3, 3], padding=1).view(N, D, 9, 1, 1, H, W)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(N, D, f * H, f * W)


def baseline_pixel(disp, logits):
    b, c, h, w = disp.shape
    u = F.unfold(disp * 4.0, 3, 1, 1).reshape(b, -1, h, w)
    u = F.interpolate(u, (h * 4, w * 4), mode="nearest").reshape(b, 9, h * 4, w * 4)
    return (u * F.softmax(logits, 1)).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convex_upsample_bench.jsonl"))
    ap.add_argument("--shapes", default="576x960,384x1248")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convex_upsample_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    lines = []

    def emit(item, what, t, **extra):
        rec = dict(item=item, what=what, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, **extra)
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    for shape in a.shapes.split(","):
        Hf, Wf = (int(v) for v in shape.split("x"))
        for N in (int(v) for v in a.batches.split(",")):
            D = 2
            for n in (2, 3):
                f = 2 ** n
                H, W = Hf // f, Wf // f
                flow = synthetic_tensor((N, D, H, W), 1, lo=-20.0, hi=20.0).to(dev).requires_grad_()
                mask = (2.0 * synthetic_tensor((N, 9 * f * f, H, W), 2)).to(dev).requires_grad_()
                gw = synthetic_tensor((N, D, Hf, Wf), 3).to(dev)
                info = dict(N=N, D=D, H=Hf, W=Wf, n_downsample=n, mask_bytes=mask.numel() * 4, out_bytes=gw.numel() * 4)
                with torch.no_grad():
                    diff = (ops.convex_upsample(flow, mask, n) - baseline_convex(flow, mask, n)).abs().max().item()
                    t = alternate({"product": lambda: ops.convex_upsample(flow, mask, n),
                                   "baseline": lambda: baseline_convex(flow, mask, n)}, 2 * a.reps, a.rounds, a.warmup)
                emit("a", "one RAFT-layout call, forward", t, **info, max_abs_diff_vs_baseline=diff,
                     product_GBps=round((info["mask_bytes"] + info["out_bytes"]) / (t["product"][0] * 1e-3) / 1e9, 1))

                def step(fn, calls=1):
                    flow.grad = mask.grad = None
                    torch.autograd.backward([fn(flow, mask, n) for _ in range(calls)], [gw] * calls)

                t = alternate({"product": lambda: step(ops.convex_upsample), "baseline": lambda: step(baseline_convex)},
                              a.reps, a.rounds, a.warmup)
                emit("a", "one RAFT-layout call, forward + backward to flow and mask", t, **info)
                if n == 2:
                    mem = {k: peak(lambda fn=fn: step(fn, a.iters)) for k, fn in (("product", ops.convex_upsample), ("baseline", baseline_convex))}
                    t = alternate({"product": lambda: step(ops.convex_upsample, a.iters), "baseline": lambda: step(baseline_convex, a.iters)},
                                  1, a.rounds, 1)
                    emit("b", f"{a.iters} RAFT-layout calls forward + backward", t, **info, product_peak_bytes=mem["product"],
                         baseline_peak_bytes=mem["baseline"])
                del flow, mask, gw
            # (c)
            h, w = Hf // 4, Wf // 4
            disp = synthetic_tensor((N, 1, h, w), 4, lo=0.0, hi=48.0).to(dev).requires_grad_()
            logits = (2.0 * synthetic_tensor((N, 9, Hf, Wf), 5)).to(dev).requires_grad_()
            gu = synthetic_tensor((N, Hf, Wf), 6).to(dev)

            def up(fn):
                disp.grad = logits.grad = None
                fn(disp, logits).backward(gu)

            t = alternate({"product": lambda: up(lambda d, z: ops.softmax_context_upsample(d, z, 4.0)),
                           "baseline": lambda: up(lambda d, z: ops.context_upsample(d * 4.0, F.softmax(z, 1))),
                           "stock": lambda: up(baseline_pixel)}, a.reps, a.rounds, a.warmup)
            emit("c", "pixel-layout call forward + backward; baseline = softmax + ops.context_upsample, stock = ATen only", t, N=N, H=Hf,
                 W=Wf, mask_bytes=logits.numel() * 4, speedup_vs_stock=round(t["stock"][0] / t["product"][0], 3))
            del disp, logits, gu
            # (d)
            K = a.iters + 1
            gt = synthetic_tensor((N, Hf, Wf), 7, lo=-5.0, hi=200.0).to(dev)
            preds = [(gt + synthetic_tensor((N, 1, Hf, Wf), 10 + k, lo=-3.0, hi=3.0).to(dev)[:, 0]).unsqueeze(1).requires_grad_()
                     for k in range(K)]
            wts = losses.sequence_loss_weights(a.iters)

            def loss(fn):
                for p in preds:
                    p.grad = None
                fn(preds, gt, 192, wts).backward()

            t = alternate({"product": lambda: loss(ops.sequence_loss), "baseline": lambda: loss(losses.masked_smooth_l1_multi)},
                          a.reps, a.rounds, a.warmup)
            emit("d", f"sequence loss of {K} predictions forward + backward; baseline = masked_smooth_l1_multi", t, N=N, H=Hf, W=Wf,
                 bytes=(2 * K + 1) * gt.numel() * 4 + K * gt.numel() * 4)
            del gt, preds

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
