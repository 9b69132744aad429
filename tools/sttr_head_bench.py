"""Times STTR's matching head (csrc/sttr_head.hip) against the stock-PyTorch op sequence it replaces, on one GPU, at the
head's shapes for a 576x960 input (downsample 3: N = 1, H = 192, W = 320) and a 384x1248 input (N = 1, H = 128, W = 416):

  (a) the fused head, forward                       ops.sttr_regress(attn, phi, ...)                    (no autograd)
  (b) the fused head, forward + backward to attn and phi
  (c) the dense pair, forward + backward            ops.sttr_optimal_transport(attn, phi, 10) with a dense gradient

The baseline is the op sequence of the reference's head written with stock ATen operators (cat, logsumexp, exp, pad, argmax,
gather, floor / ceil) on the same device; it never calls the code under test and reads nothing outside this repository.
Method (tools/geo_lookup_bench.py): every variant is warmed up, then the variants of an item are timed alternately in one
process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported
with min / max.  Peak memory is torch.cuda.max_memory_allocated over one execution of each side minus what was allocated
before it.  `passes` / `bytes_per_pass` state what the product reads: the (W+1)^2 fp32 matrix of every (n, h) once per pass
-- 2 * iters + 1 in the forward and as many in the fused backward; the dense pair also writes P once and reads G three times --
from L2 / Infinity Cache (the inputs of the timed calls stay resident: these are WARM figures).  No time is fixed in advance.
One shape per invocation (`--shape 192x320`), so that each runs under its own time limit; records are appended to --out.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd import ops  # noqa: E402
from stereo_toolbox_amd.utils import synthetic_tensor  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402

ITERS = 10


def baseline_transport(attn, phi, iters=ITERS):
    """regression_head.py:143-190, operator for operator"""
    N, H, W, _ = attn.shape
    marginal = torch.cat([torch.ones([W]), torch.tensor([W]).float()]) / (2 * W)
    log_mu = marginal.log().to(attn.device).expand(N, H, W + 1)
    S = torch.cat([attn, phi.expand(N, H, W, 1)], -1)
    S = torch.cat([S, phi.expand(N, H, 1, W + 1)], -2)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_mu)
    for _ in range(iters):
        v = log_mu - torch.logsumexp(S + u.unsqueeze(3), dim=2)
        u = log_mu - torch.logsumexp(S + v.unsqueeze(2), dim=3)
    return (S + u.unsqueeze(3) + v.unsqueeze(2) + torch.log(torch.tensor([2.0 * W]).to(attn.device))).exp()


def baseline_head(attn, phi, target):
    """regression_head.py:39-101, 219-280 without the upsampling: (disp, occ, gt_response, bin_left, bin_right)"""
    P = baseline_transport(attn, phi)
    inner = P[..., :-1, :-1]
    W = inner.shape[-1]
    t = target.unsqueeze(-1)
    il, ir = torch.floor(t).long().clamp(0, W - 1), torch.ceil(t).long().clamp(0, W - 1)
    wr = t - il
    gt = (torch.gather(inner, -1, il) * (1 - wr) + torch.gather(inner, -1, ir) * wr).squeeze(-1)
    pos = torch.arange(W, dtype=torch.float32, device=attn.device)
    shift = (pos[:, None] - pos[None, :]).clamp_min(0)[None, None]
    high = torch.argmax(inner, dim=-1)
    window = torch.stack([high - 1, high, high + 1], dim=-1)
    padded = F.pad(inner, [1, 1], value=0.0)
    taps = torch.gather(padded, -1, window + 1)
    norm = taps.sum(-1, keepdim=True)
    norm[norm < 0.1] = 1.0
    disp = (taps / norm * torch.gather(F.pad(shift, [1, 1]).expand_as(padded), -1, window + 1)).sum(-1)
    return disp, (1.0 - norm).squeeze(-1), gt, P[..., :-1, -1], P[..., -1, :-1]


def inputs(N, H, W, dev):
    i = torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
    j = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    d = synthetic_tensor((N, H, W, 1), 8, lo=0.0, hi=W / 3.0)
    noise = sum(synthetic_tensor((N, H, W, W), 7, stream=k) for k in range(3)) * (2.0 / 3.0 ** 0.5)
    attn = (noise + 8.0 * torch.exp(-0.5 * ((j - (i - d)) / 1.2) ** 2)).masked_fill(j > i, float("-inf"))
    target = torch.arange(W, dtype=torch.float32).view(1, 1, W) - d.squeeze(-1)
    return attn.to(dev), torch.tensor(0.3, device=dev), target.to(dev)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "sttr_head_bench.jsonl"))
    ap.add_argument("--shape", default="192x320", help="HxW of the low-resolution image (N = 1)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sttr_head_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    N = 1
    H, W = (int(s) for s in a.shape.split("x"))
    attn, phi, target = inputs(N, H, W, dev)
    gws = [synthetic_tensor((N, H, W), 20 + k).to(dev) for k in range(5)]
    G = synthetic_tensor((N, H, W + 1, W + 1), 40).to(dev)
    matrix_bytes = N * H * (W + 1) * (W + 1) * 4
    shape = dict(N=N, H=H, W=W, iters=ITERS, bytes_per_pass=matrix_bytes, device=torch.cuda.get_device_name(0))
    lines = []

    def emit(item, what, t, **extra):
        rec = dict(item=item, what=what, **shape, reps=a.reps, rounds=a.rounds)
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
        rec["bytes_per_s"] = round(extra["passes"] * matrix_bytes / (t["product"][0] * 1e-3), 1)
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def product_fwd():
        return ops.sttr_regress(attn, phi, True, ITERS, None, target)[:5]

    with torch.no_grad():
        err = [(x - y).abs().max().item() for x, y in zip(product_fwd(), baseline_head(attn, phi, target))]
        mem = dict(product_peak_bytes=peak_bytes(product_fwd), baseline_peak_bytes=peak_bytes(lambda: baseline_head(attn, phi, target)))
        t = alternate({"product": product_fwd, "baseline": lambda: baseline_head(attn, phi, target)}, a.reps, a.rounds, a.warmup)
        emit("a", "fused head, forward", t, passes=2 * ITERS + 1, max_abs_diff_vs_baseline=err, **mem)

    leaf_a, leaf_p = attn.clone().requires_grad_(), phi.clone().requires_grad_()

    def step(fn):
        leaf_a.grad = leaf_p.grad = None
        torch.autograd.backward(list(fn()), gws)
        return leaf_a.grad, leaf_p.grad

    def product_step():
        return step(lambda: ops.sttr_regress(leaf_a, leaf_p, True, ITERS, None, target)[:5])

    def baseline_step():
        return step(lambda: baseline_head(leaf_a, leaf_p, target))

    ref = [g.clone() for g in product_step()]
    err = [(x - y).abs().max().item() for x, y in zip(baseline_step(), ref)]
    mem = dict(product_peak_bytes=peak_bytes(product_step), baseline_peak_bytes=peak_bytes(baseline_step))
    t = alternate({"product": product_step, "baseline": baseline_step}, a.reps, a.rounds, a.warmup)
    emit("b", "fused head, forward + backward to attn and phi", t, passes=4 * ITERS + 2, max_abs_diff_vs_baseline=err, **mem)

    def dense(fn):
        leaf_a.grad = leaf_p.grad = None
        fn(leaf_a, leaf_p).backward(G)
        return leaf_a.grad, leaf_p.grad

    def product_dense():
        return dense(lambda x, p: ops.sttr_optimal_transport(x, p, ITERS))

    def baseline_dense():
        return dense(baseline_transport)

    ref = [g.clone() for g in product_dense()]
    err = [(x - y).abs().max().item() for x, y in zip(baseline_dense(), ref)]
    mem = dict(product_peak_bytes=peak_bytes(product_dense), baseline_peak_bytes=peak_bytes(baseline_dense))
    t = alternate({"product": product_dense, "baseline": baseline_dense}, a.reps, a.rounds, a.warmup)
    emit("c", "dense pair, forward + backward with a dense gradient", t, passes=4 * ITERS + 8, max_abs_diff_vs_baseline=err, **mem)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("appended to", a.out)


if __name__ == "__main__":
    main()
