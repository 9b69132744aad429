"""Times FoundationStereo's axial-planar convolution block (models.FoundationStereo.Conv3dNormActReduced on csrc/conv3d_axial.hip)
against the stock PyTorch-ROCm op sequence it replaces, on one GPU, at B = 1 and the four hourglass shapes of a 576x960 input
with max_disp 416 and volume_dim 28 (reference foundation_stereo.py:46-124):

    1/4: 28 ch, 104x144x240    1/8: 56 ch, 52x72x120    1/16: 112 ch, 26x36x60    1/32: 168 ch, 13x18x30    (kernel_disp 17)

  (a) the block, product against stock: forward (eval mode, no grad) and forward + backward (train mode, gradients to the input
      and every parameter).  The stock side is the same block built from nn.Conv3d / nn.BatchNorm3d / nn.ReLU, filled with the same
      weights, timed in contiguous and in channels_last_3d layout; the faster one is the baseline.  It never calls the code under
      test.
  (b) the six kernel roles on their own -- planar and axial, each forward, data gradient and weight gradient (the weight gradient
      call is its MFMA kernel plus the fixed-order reduction of the partial slab) -- with the achieved fraction of the 157.3 TFLOP/s
      fp32-MFMA peak: 2 x voxels x taps x Cin x Cout operations over the call time.

Method (tools/geo_lookup_bench.py, `alternate`): every variant is warmed up, then the variants of an item are timed alternately in
one process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported
with min / max.  One JSON line per item goes to --out.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from geo_lookup_bench import alternate  # noqa: E402
from stereo_toolbox_amd import ops  # noqa: E402
from stereo_toolbox_amd.models.FoundationStereo import Conv3dNormActReduced  # noqa: E402
from stereo_toolbox_amd.utils import fill_state_dict, synthetic_tensor  # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = {"1/4": (28, 104, 144, 240), "1/8": (56, 52, 72, 120), "1/16": (112, 26, 36, 60), "1/32": (168, 13, 18, 30)}
KD = 17


def stock_block(C, kd):
    """The reference's module structure from stock torch modules (same state-dict keys)."""
    m = nn.Module()
    m.conv1 = nn.Sequential(nn.Conv3d(C, C, (1, 3, 3), padding=(0, 1, 1)), nn.BatchNorm3d(C), nn.ReLU())
    m.conv2 = nn.Sequential(nn.Conv3d(C, C, (kd, 1, 1), padding=(kd // 2, 0, 0)), nn.BatchNorm3d(C), nn.ReLU())
    m.forward = lambda x: m.conv2(m.conv1(x))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "apc_bench.jsonl"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("apc_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        rec.update(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def ms(rec, t):
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 4), round(lo, 4), round(hi, 4)

    for res in a.shapes.split(","):
        C, D, H, W = SHAPES[res]
        info = dict(resolution=res, B=1, C=C, D=D, H=H, W=W, kernel_disp=KD)
        prod = Conv3dNormActReduced(C, C, kernel_disp=KD)
        sd = prod.state_dict()
        fill_state_dict(sd)
        prod.load_state_dict(sd)
        prod = prod.to(dev)
        stock = stock_block(C, KD)
        stock.load_state_dict(sd)
        stock = stock.to(dev)
        stock_cl = stock_block(C, KD)
        stock_cl.load_state_dict(sd)
        stock_cl = stock_cl.to(dev).to(memory_format=torch.channels_last_3d)
        x_nd = synthetic_tensor((1, D, H, W, C), 1).to(dev)                  # dense NDHWC: the layout the volume builder writes
        x_cl = ops.to_ncdhw(x_nd)                                            # its logical view = channels_last_3d
        x_ct = x_cl.contiguous()
        g_cl = ops.to_ncdhw(synthetic_tensor((1, D, H, W, C), 2).to(dev))
        g_ct = g_cl.contiguous()

        # (a) forward, eval mode
        for m in (prod, stock, stock_cl):
            m.eval()
        with torch.no_grad():
            diff = (prod(x_cl) - stock(x_ct)).abs().max().item()
            t = alternate({"product": lambda: prod(x_cl), "stock_contiguous": lambda: stock(x_ct),
                           "stock_channels_last": lambda: stock_cl(x_cl)}, a.reps, a.rounds, a.warmup)
        rec = dict(item="a", what="block forward, eval mode", **info, max_abs_diff_vs_stock=diff)
        ms(rec, t)
        best = min(t["stock_contiguous"][0], t["stock_channels_last"][0])
        rec["stock_over_product"] = round(best / t["product"][0], 3)
        emit(rec)

        # (a) forward + backward, train mode
        for m in (prod, stock, stock_cl):
            m.train()

        def step(m, x, g):
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x).backward(g)

        xs = {k: v.detach().clone().requires_grad_() for k, v in (("p", x_cl), ("ct", x_ct), ("cl", x_cl))}
        t = alternate({"product": lambda: step(prod, xs["p"], g_cl), "stock_contiguous": lambda: step(stock, xs["ct"], g_ct),
                       "stock_channels_last": lambda: step(stock_cl, xs["cl"], g_cl)}, a.reps, a.rounds, a.warmup)
        rec = dict(item="a", what="block forward + backward, train mode", **info)
        ms(rec, t)
        best = min(t["stock_contiguous"][0], t["stock_channels_last"][0])
        rec["stock_over_product"] = round(best / t["product"][0], 3)
        emit(rec)
        del xs, stock, stock_cl, x_ct, g_ct
        torch.cuda.empty_cache()

        # (b) the six kernel roles
        g_nd = ops.to_ndhwc(g_cl)
        with torch.no_grad():
            for name, conv in (("planar", prod.conv1[0]), ("axial", prod.conv2[0])):
                w = conv.weight.detach()
                k = tuple(w.shape[2:])
                wp0, wp1 = ops.pack_weight_axial(w, 0), ops.pack_weight_axial(w, 1)
                flop = 2.0 * D * H * W * k[0] * k[1] * k[2] * C * C
                t = alternate({"forward": lambda: ops.conv3d_axial_forward(x_nd, wp0, C, k, want_stats=True),
                               "data_gradient": lambda: ops.conv3d_axial_forward(g_nd, wp1, C, k),
                               "weight_gradient": lambda: ops.conv3d_axial_wgrad(x_nd, g_nd, k)}, a.reps, a.rounds, a.warmup)
                rec = dict(item="b", what=f"{name} kernel roles", **info, kernel=list(k), gflop=round(flop / 1e9, 2))
                ms(rec, t)
                for role, (med, _, _) in t.items():
                    rec[role + "_fraction_of_peak"] = round(flop / (med * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
                emit(rec)
        del prod, x_nd, x_cl, g_cl, g_nd
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
