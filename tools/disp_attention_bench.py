"""Times FoundationStereo's disparity transformer (models.FoundationStereo.CostVolumeDisparityAttention on csrc/disp_attention.hip)
against the stock PyTorch-ROCm op sequence it replaces, on one GPU, at the model's size: the 1/16 volume of a 576x960 input,
[B, 28, 26, 36, 60] -- 2160 B sequences of 26 tokens x 28 channels, four heads of 7, feed-forward 28, four layers; B = 1 and 4.

  (a) forward in eval(), no grad;
  (b) forward + backward in train() with p = 0 (gradients to the volume and every parameter);
  (c) the same with p = 0.1;
  each with the peak memory of both sides in (b) and (c);
  (d) the product's calls on their own: the forward launch with the achieved fraction of the 157.3 TFLOP/s fp32-MFMA peak for the
      FLOPs the layers need (counted from the shapes: 2.77 GFLOP per image) and the achieved bytes/s over the compulsory traffic
      (the volume read and written once).

The stock side is the reference's layer rebuilt from nn.Linear / nn.LayerNorm / F.gelu / nn.Dropout with the same weights, the
reference's permute + reshape around it, in fp32, with `flash_attn_func` replaced by (i) F.scaled_dot_product_attention and
(ii) explicit matmul + softmax; the faster of the two is the baseline.  It never calls the code under test.  Both sides get the
volume as a logical [B, C, D, H, W] view of dense channels-last storage, which is what the layers in front of it leave.

Method (tools/geo_lookup_bench.py, `alternate`): every variant is warmed up, then the variants of an item are timed alternately in
one process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported
with min / max.  One JSON line per item goes to --out.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from geo_lookup_bench import alternate  # noqa: E402
from stereo_toolbox_amd import ops  # noqa: E402
from stereo_toolbox_amd.models.FoundationStereo import CostVolumeDisparityAttention  # noqa: E402
from stereo_toolbox_amd.utils import fill_state_dict, synthetic_tensor  # noqa: E402

PEAK_TFLOPS = 157.3
C, HEADS, FF, LAYERS, D, H, W = 28, 4, 28, 4, 26, 36, 60


class _Proj(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(c, c) for _ in range(4))


class StockLayer(nn.Module):
    """The post-norm encoder layer from stock torch modules (same state-dict keys as the product)."""

    def __init__(self, c, heads, ff, p, sdpa):
        super().__init__()
        self.heads, self.sdpa = heads, sdpa
        self.self_attn = _Proj(c)
        self.linear1, self.linear2 = nn.Linear(c, ff), nn.Linear(ff, c)
        self.norm1, self.norm2 = nn.LayerNorm(c), nn.LayerNorm(c)
        self.dropout, self.dropout1, self.dropout2 = nn.Dropout(p), nn.Dropout(p), nn.Dropout(p)

    def forward(self, x):
        N, L, c = x.shape
        a = self.self_attn
        q, k, v = (m(x).view(N, L, self.heads, c // self.heads).transpose(1, 2) for m in (a.q_proj, a.k_proj, a.v_proj))
        if self.sdpa:
            o = F.scaled_dot_product_attention(q, k, v)
        else:
            o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(c // self.heads), dim=-1) @ v
        x = self.norm1(x + self.dropout1(a.out_proj(o.transpose(1, 2).reshape(N, L, c))))
        return self.norm2(x + self.dropout2(self.linear2(self.dropout(F.gelu(self.linear1(x))))))


class StockTransformer(nn.Module):
    def __init__(self, p, sdpa, pe):
        super().__init__()
        self.sa = nn.ModuleList([StockLayer(C, HEADS, FF, p, sdpa) for _ in range(LAYERS)])
        self.pe = pe

    def forward(self, cv):
        B, c, d, h, w = cv.shape
        x = cv.permute(0, 3, 4, 2, 1).reshape(B * h * w, d, c) + self.pe[None, :d]
        for layer in self.sa:
            x = layer(x)
        return x.reshape(B, h, w, d, c).permute(0, 4, 3, 1, 2)


def flops_per_sequence():
    per_layer = 3 * 2 * D * C * C + 2 * 2 * D * D * C + 2 * D * C * C + 2 * 2 * D * C * FF
    return LAYERS * per_layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disp_attention_bench.jsonl"))
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("disp_attention_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        rec.update(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def ms(rec, t):
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)

    def versus(rec, t):
        ms(rec, t)
        best = min(t["stock_sdpa"][0], t["stock_matmul"][0])
        rec["stock_over_product"] = round(best / t["product"][0], 3)
        rec["product_loses"] = bool(best < t["product"][0])
        emit(rec)

    def models(p):
        prod = CostVolumeDisparityAttention(C, HEADS, FF, dropout=p, num_transformer=LAYERS, max_len=D)
        sd = prod.state_dict()
        fill_state_dict(sd)
        prod.load_state_dict(sd)
        prod = prod.to(dev)
        pe = prod.pos_embed0.table(D, dev)
        out = {"product": prod}
        for name, sdpa in (("stock_sdpa", True), ("stock_matmul", False)):
            m = StockTransformer(p, sdpa, pe)
            m.load_state_dict(sd)
            out[name] = m.to(dev)
        return out

    def fwd_bwd(m, cv, g):
        leaf = cv.detach().requires_grad_()

        def run():
            leaf.grad = None
            for q in m.parameters():
                q.grad = None
            m(leaf).backward(g)
        return run

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)

    for B in (int(b) for b in a.batches.split(",")):
        cv = ops.to_ncdhw(synthetic_tensor((B, D, H, W, C), 1).to(dev))
        g = ops.to_ncdhw(synthetic_tensor((B, D, H, W, C), 2).to(dev))
        info = dict(B=B, sequences=B * H * W, L=D, C=C, heads=HEADS, ff=FF, layers=LAYERS)
        ms_eval = models(0.1)
        for m in ms_eval.values():
            m.eval()
        with torch.no_grad():
            diff = max((ms_eval["product"](cv) - ms_eval[k](cv)).abs().max().item() for k in ("stock_sdpa", "stock_matmul"))
            t = alternate({k: (lambda m=m: m(cv)) for k, m in ms_eval.items()}, a.reps, a.rounds, a.warmup)
        versus(dict(item="a", what="forward, eval, no grad", **info, max_abs_diff_vs_stock=diff), t)
        for item, p in (("b", 0.0), ("c", 0.1)):
            ms_train = models(p)
            fns = {k: fwd_bwd(m.train(), cv, g) for k, m in ms_train.items()}
            t = alternate(fns, a.reps, a.rounds, a.warmup)
            rec = dict(item=item, what=f"forward + backward, train, p = {p}", **info)
            for k, fn in fns.items():
                rec[k + "_peak_memory_mb"] = peak(fn)
            versus(rec, t)
        # (d) the product's forward launch on its own
        prod = ms_eval["product"]
        x = ops.to_ndhwc(cv)
        pe = prod.pos_embed0.table(D, dev)
        prm = [q.detach() for layer in prod.sa for q in layer.tensors()]
        with torch.no_grad():
            t = alternate({"forward_launch": lambda: ops.disp_attention(x, pe, prm, HEADS)}, a.reps, a.rounds, a.warmup)
        med = t["forward_launch"][0] * 1e-3
        flop = flops_per_sequence() * B * H * W
        byts = 2 * x.numel() * 4
        rec = dict(item="d", what="the forward launch (call time: device events around back-to-back calls)", **info,
                   gflop=round(flop / 1e9, 3), fraction_of_mfma_peak=round(flop / med / (PEAK_TFLOPS * 1e12), 4),
                   compulsory_mbytes=round(byts / 1e6, 2), achieved_gbytes_per_s=round(byts / med / 1e9, 1))
        ms(rec, t)
        emit(rec)
        del ms_eval, ms_train
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
