"""Times StereoAnywhere's mono-stereo alignment stage (csrc/mono_align.hip) against the stock-PyTorch op sequence it replaces, on
one GPU, at the model's shape for a 576x960 input (1/4 resolution: maps 144 x 240, volume 144 x 240 x 240 = 33 MB, N = 8 masks,
so the masked volume is 265 MB), for B = 1 and B = 4:

  (a) masked_volume forward            volume * generate_masks(l).unsqueeze(4) * generate_masks(r).unsqueeze(3)   (no autograd)
  (b) masked_volume forward + backward to the volume
  (c) weighted_lsq forward             (d) forward + backward
  (e) softlrc forward                  (f) forward + backward
  (g) align_mono forward + backward    stereoanywhere.py:218-235 end to end

The baseline is the op sequence of the reference's functions written with stock ATen operators on the same device (the mask loop
and broadcast multiplies; meshgrid, grid_sample and softplus; the loop over the batch with boolean indexing, torch.quantile and
torch.linalg.lstsq); it never calls the code under test and reads nothing outside this repository.  Method
(tools/geo_lookup_bench.py): every variant is warmed up, then the variants of an item are timed alternately in one process, each
sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported with min / max.
(a) / (b) also time, in the same alternation, a pure fill of an output-sized buffer -- the yardstick of the volume builders: the
product's forward cannot be faster than writing its output -- and report the algorithmic bytes moved (forward: the volume read
once, the output written once; backward: one N-th of the gradient read, the volume gradient written) and the peak device memory
of one call of either side.  No time is fixed in advance.  `max_abs_diff_vs_baseline` is informational (parity is the business of
tests/test_mono_align.py): the baseline is fp32, and item (g) differentiates a sum over all pixels through the least-squares fit,
where the fp32 error of the stock sequence dominates the difference.
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
from tools.stereoanywhere_bench import baseline_mask  # noqa: E402


def baseline_masks(mde, N):
    """utils/utils.py:48-54"""
    B, _, H, W = mde.shape
    masks = torch.zeros(B, N, H, W, dtype=torch.float16, device=mde.device)
    for i in range(N):
        masks[:, i] = ((mde < (i + 1) / N) & (mde >= i / N)).squeeze(1)
    return masks


def baseline_masked_volume(volume, left, right, N):
    """stereoanywhere.py:170-171, 193"""
    return volume * baseline_masks(left, N).unsqueeze(4) * baseline_masks(right, N).unsqueeze(3)


def baseline_warp(disp, img, right_disp):
    """utils/utils.py:172-187"""
    B, _, H, W = disp.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=disp.dtype, device=disp.device), torch.arange(W, dtype=disp.dtype, device=disp.device),
                            indexing="ij")
    xs, ys = xs[None].repeat(B, 1, 1), ys[None].repeat(B, 1, 1)
    x = xs + disp.squeeze(1) if right_disp else xs - disp.squeeze(1)
    grid = 2 * torch.cat([x.unsqueeze(-1) / W, ys.unsqueeze(-1) / H], -1) - 1
    return F.grid_sample(img, grid, align_corners=True)


def baseline_softlrc(disp2, disp3, lrc_th=1.0):
    """utils/utils.py:189-198"""
    div = math.log(1 + math.exp(lrc_th))
    w2, w3 = baseline_warp(F.relu(disp3), disp2, True), baseline_warp(F.relu(disp2), disp3, False)
    return F.softplus(-torch.abs(disp2 - w3) + lrc_th) / div, F.softplus(-torch.abs(disp3 - w2) + lrc_th) / div


def baseline_weighted_lsq(mde, disp, conf, qmin=0.2, qmax=0.9):
    """utils/utils.py:345-384"""
    B = mde.shape[0]
    mde, disp, conf = mde.reshape(B, -1), F.relu(disp.reshape(B, -1)), conf.reshape(B, -1)
    out = torch.zeros((B, 2), device=mde.device)
    for b in range(B):
        m, s, c = mde[b].unsqueeze(0), disp[b].unsqueeze(0), conf[b].unsqueeze(0)
        keep = (torch.quantile(s.flatten(), qmin) <= s) & (s <= torch.quantile(s.flatten(), qmax))
        m, c, s = m[keep].abs().unsqueeze(0), c[keep].abs().unsqueeze(0), s[keep].abs().unsqueeze(0)
        w = torch.sqrt(c * (1 - 0.1) + 0.1)
        A = torch.cat([(m * w).unsqueeze(-1), w.unsqueeze(-1)], -1)
        out[b] = torch.linalg.lstsq(A, (s * w).unsqueeze(-1))[0].squeeze(2).squeeze(0)
    return out[:, 0:1].reshape(B, 1, 1, 1), out[:, 1:2].reshape(B, 1, 1, 1)


def baseline_mirror(sd, md, sc, mc, conf_th=0.5, gain=20):
    """utils/utils.py:255-269"""
    a = (sc * mc) * torch.sigmoid(gain * (md - sd))
    b = (1 - sc) * mc
    return torch.sigmoid(gain * (a + b - a * b - conf_th))


def baseline_align(mde2, mde3, d2, d3, c2, c3):
    """stereoanywhere.py:218-235"""
    l2, l3 = baseline_softlrc(d2, d3)
    k2, k3 = c2 * l2, c3 * l3
    scale, shift = baseline_weighted_lsq(torch.cat([mde2, mde3], 1), torch.cat([d2, d3], 1), torch.cat([k2, k3], 1))
    s2 = torch.sum(scale * mde2 + shift, dim=1, keepdim=True)
    s3 = torch.sum(scale * mde3 + shift, dim=1, keepdim=True)
    ls2, _ = baseline_softlrc(s2, s3)
    mirror = baseline_mirror(d2, s2, k2, ls2, conf_th=0.98)
    return l2, l3, k2, k3, s2, s3, ls2, mirror, baseline_mask(s2, mirror, 0.9).detach()


def product_align(*maps):
    r = SA.align_mono(*maps)
    return (r.softlrc_mono2, r.softlrc_mono3, r.conf2, r.conf3, r.scaled_mde2, r.scaled_mde3, r.softlrc_scaled_mde2, r.mirror_conf2,
            r.truncate_mask)


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
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
                                                  "stereoanywhere_align_bench.jsonl"))
    ap.add_argument("--H", type=int, default=576)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--n-masks", type=int, default=8)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stereoanywhere_align_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    h, w, N = a.H // 4, a.W // 4, a.n_masks
    lines = []

    def emit(item, what, B, t, **extra):
        rec = dict(item=item, what=what, B=B, h=h, w=w, n_masks=N, device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds)
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for B in a.batches:
        shape = (B, 1, h, w)
        vol = synthetic_tensor((B, 1, h, w, w), 7).to(dev)
        base = synthetic_tensor(shape, 8, lo=0.05, hi=0.95)
        mde2 = (base + synthetic_tensor(shape, 9, lo=-0.04, hi=0.04)).to(dev)
        mde3 = (base + synthetic_tensor(shape, 10, lo=-0.04, hi=0.04)).to(dev)
        d2 = (40.0 * base + synthetic_tensor(shape, 11, lo=-1.0, hi=1.0)).to(dev)
        d3 = (40.0 * base + synthetic_tensor(shape, 12, lo=-1.0, hi=1.0)).to(dev)
        c2, c3 = synthetic_tensor(shape, 13, lo=0.0, hi=1.0).to(dev), synthetic_tensor(shape, 14, lo=0.0, hi=1.0).to(dev)
        gw = synthetic_tensor((B, N, h, w, w), 15).to(dev)
        vol_bytes, out_bytes = vol.numel() * 4, gw.numel() * 4
        fill_buf = torch.empty_like(gw)

        def with_fill(t):
            return dict(fill_ms=round(t["fill"][0], 5), fill_over_product=round(t["fill"][0] / t["product"][0], 3))

        # (a) masked volume, forward
        with torch.no_grad():
            same = torch.equal(SA.masked_volume(vol, mde2, mde3, N), baseline_masked_volume(vol, mde2, mde3, N))
            peaks = dict(product_peak_bytes=peak_bytes(lambda: SA.masked_volume(vol, mde2, mde3, N)),
                         baseline_peak_bytes=peak_bytes(lambda: baseline_masked_volume(vol, mde2, mde3, N)))
            t = alternate({"product": lambda: SA.masked_volume(vol, mde2, mde3, N),
                           "baseline": lambda: baseline_masked_volume(vol, mde2, mde3, N), "fill": lambda: fill_buf.zero_()},
                          a.reps, a.rounds, a.warmup)
        moved = vol_bytes + out_bytes
        emit("a", "masked_volume forward", B, t, bytes_moved=moved, bytes_per_s=round(moved / (t["product"][0] * 1e-3), 1),
             equals_baseline=same, **with_fill(t), **peaks)

        # (b) masked volume, forward + backward
        leaf = vol.detach().clone().requires_grad_()

        def vol_step(fn):
            leaf.grad = None
            fn(leaf, mde2, mde3, N).backward(gw)
            return leaf.grad

        same = torch.equal(vol_step(SA.masked_volume).clone(), vol_step(baseline_masked_volume))
        leaf.grad = None
        peaks = dict(product_peak_bytes=peak_bytes(lambda: vol_step(SA.masked_volume)),
                     baseline_peak_bytes=peak_bytes(lambda: vol_step(baseline_masked_volume)))
        t = alternate({"product": lambda: vol_step(SA.masked_volume), "baseline": lambda: vol_step(baseline_masked_volume),
                       "fill": lambda: fill_buf.zero_()}, a.reps, a.rounds, a.warmup)
        moved = 2 * vol_bytes + out_bytes + out_bytes // N
        emit("b", "masked_volume forward + backward to the volume", B, t, bytes_moved=moved,
             bytes_per_s=round(moved / (t["product"][0] * 1e-3), 1), equals_baseline=same, **with_fill(t), **peaks)
        leaf.grad = None

        # (c) / (d) weighted_lsq
        trio = [torch.cat([mde2, mde3], 1), torch.cat([d2, d3], 1), torch.cat([c2, c3], 1)]
        with torch.no_grad():
            err = [(x - y).abs().max().item() for x, y in zip(SA.weighted_lsq(*trio), baseline_weighted_lsq(*trio))]
            t = alternate({"product": lambda: SA.weighted_lsq(*trio), "baseline": lambda: baseline_weighted_lsq(*trio)}, a.reps, a.rounds,
                          a.warmup)
        emit("c", "weighted_lsq forward", B, t, max_abs_diff_vs_baseline=err)
        leaves = [x.detach().clone().requires_grad_() for x in trio]

        def lsq_step(fn):
            for x in leaves:
                x.grad = None
            scale, shift = fn(*leaves)
            (scale.sum() + 0.5 * shift.sum()).backward()
            return [x.grad for x in leaves]

        err = [(x - y).abs().max().item() for x, y in zip([g.clone() for g in lsq_step(SA.weighted_lsq)], lsq_step(baseline_weighted_lsq))]
        t = alternate({"product": lambda: lsq_step(SA.weighted_lsq), "baseline": lambda: lsq_step(baseline_weighted_lsq)}, a.reps,
                      a.rounds, a.warmup)
        emit("d", "weighted_lsq forward + backward", B, t, max_abs_diff_vs_baseline=err)

        # (e) / (f) softlrc
        with torch.no_grad():
            err = [(x - y).abs().max().item() for x, y in zip(SA.softlrc(d2, d3), baseline_softlrc(d2, d3))]
            t = alternate({"product": lambda: SA.softlrc(d2, d3), "baseline": lambda: baseline_softlrc(d2, d3)}, 4 * a.reps, a.rounds,
                          a.warmup)
        emit("e", "softlrc forward", B, t, max_abs_diff_vs_baseline=err)
        pair = [d2.detach().clone().requires_grad_(), d3.detach().clone().requires_grad_()]
        gl = [synthetic_tensor(shape, 16).to(dev), synthetic_tensor(shape, 17).to(dev)]

        def lrc_step(fn):
            for x in pair:
                x.grad = None
            torch.autograd.backward(list(fn(*pair)), gl)
            return [x.grad for x in pair]

        err = [(x - y).abs().max().item() for x, y in zip([g.clone() for g in lrc_step(SA.softlrc)], lrc_step(baseline_softlrc))]
        t = alternate({"product": lambda: lrc_step(SA.softlrc), "baseline": lambda: lrc_step(baseline_softlrc)}, 4 * a.reps, a.rounds,
                      a.warmup)
        emit("f", "softlrc forward + backward", B, t, max_abs_diff_vs_baseline=err)

        # (g) align_mono end to end
        six = [x.detach().clone().requires_grad_() for x in (mde2, mde3, d2, d3, c2, c3)]

        def align_step(fn):
            for x in six:
                x.grad = None
            outs = fn(*six)
            sum(o.sum() for o in outs[:-1]).backward()
            return [x.grad for x in six]

        err = [(x - y).abs().max().item() for x, y in zip([g.clone() for g in align_step(product_align)], align_step(baseline_align))]
        t = alternate({"product": lambda: align_step(product_align), "baseline": lambda: align_step(baseline_align)}, a.reps, a.rounds,
                      a.warmup)
        emit("g", "align_mono forward + backward (stereoanywhere.py:218-235)", B, t, max_abs_diff_vs_baseline=err)
        del vol, gw, fill_buf, leaf

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
