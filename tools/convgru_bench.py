"""Times the ConvGRU cell (models.IGEVStereo.ConvGRU on csrc/convgru.hip) against the stock PyTorch-ROCm op sequence it replaces,
on one GPU, at IGEV's three levels of a 576x960 input with hidden 128 (reference igev_stereo.py:97-119):

    1/4: 144x240, x = (128, 128)      1/8: 72x120, x = (128, 128)      1/16: 36x60, x = (128,)          B = 1 and B = 4

  (a) one call, product against stock: forward (no grad) and forward + backward (gradients to h, the c*, every x and every
      parameter).  The stock side is the same cell from nn.Conv2d, cat, sigmoid and tanh with the same weights, timed in
      contiguous and in channels_last layout; the faster one is the baseline.  It never calls the code under test.
  (b) the three levels as one iteration, forward and forward + backward.
  (c) `--iters` (22) iterations of the three levels, h fed back, forward + backward, with the peak memory of both sides.
  (d) the kernel roles on their own: zr and q launches, the two data gradients, the two weight gradients (MFMA kernel plus the
      fixed-order slab reduction) with the achieved fraction of the 157.3 TFLOP/s fp32-MFMA peak, and the two streaming
      passes with the fraction of the 8 TB/s HBM peak their compulsory traffic amounts to.

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
from stereo_toolbox_amd.models.IGEVStereo import ConvGRU  # noqa: E402
from stereo_toolbox_amd.utils import fill_state_dict, synthetic_tensor  # noqa: E402

PEAK_TFLOPS = 157.3
PEAK_HBM = 8.0e12
HIDDEN = 128
LEVELS = {"1/4": (144, 240, (128, 128)), "1/8": (72, 120, (128, 128)), "1/16": (36, 60, (128,))}


class StockGRU(nn.Module):
    """The cell from stock torch modules (same state-dict keys as the product)."""

    def __init__(self, hidden, cin):
        super().__init__()
        self.convz, self.convr, self.convq = (nn.Conv2d(hidden + cin, hidden, 3, padding=1) for _ in range(3))

    def forward(self, h, cz, cr, cq, *xs):
        x = torch.cat(xs, 1)
        hx = torch.cat([h, x], 1)
        z = torch.sigmoid(self.convz(hx) + cz)
        r = torch.sigmoid(self.convr(hx) + cr)
        q = torch.tanh(self.convq(torch.cat([r * h, x], 1)) + cq)
        return (1 - z) * h + z * q


def level_setup(res, B, dev):
    H, W, cx = LEVELS[res]
    prod = ConvGRU(HIDDEN, sum(cx))
    sd = prod.state_dict()
    fill_state_dict(sd)
    prod.load_state_dict(sd)
    prod = prod.to(dev)
    stock = StockGRU(HIDDEN, sum(cx))
    stock.load_state_dict(sd)
    stock = stock.to(dev)
    stock_cl = StockGRU(HIDDEN, sum(cx))
    stock_cl.load_state_dict(sd)
    stock_cl = stock_cl.to(dev).to(memory_format=torch.channels_last)
    cl = lambda c, k: synthetic_tensor((B, H, W, c), k, lo=-1.0, hi=1.0).to(dev).permute(0, 3, 1, 2)      # noqa: E731
    c3 = cl(3 * HIDDEN, 2)                                            # cz | cr | cq: channel splits of one map (igev_stereo.py:226)
    args_cl = [cl(HIDDEN, 1), *c3.split(HIDDEN, 1), *[cl(c, 10 + i) for i, c in enumerate(cx)]]
    args_ct = [t.contiguous() for t in args_cl]
    g_cl = cl(HIDDEN, 3)
    return dict(H=H, W=W, cx=cx, prod=prod, stock=stock, stock_cl=stock_cl, args_cl=args_cl, args_ct=args_ct, g_cl=g_cl,
                g_ct=g_cl.contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convgru_bench.jsonl"))
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convgru_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
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
        best = min(t["stock_contiguous"][0], t["stock_channels_last"][0])
        rec["stock_over_product"] = round(best / t["product"][0], 3)
        emit(rec)

    def fwd_bwd(m, args, g):
        leaves = [t.detach().requires_grad_() for t in args]

        def run():
            for t in leaves:
                t.grad = None
            for p in m.parameters():
                p.grad = None
            m(*leaves).backward(g)
        return run

    for B in (int(b) for b in a.batches.split(",")):
        S = {res: level_setup(res, B, dev) for res in LEVELS}
        kinds = (("product", "prod", "args_cl", "g_cl"), ("stock_contiguous", "stock", "args_ct", "g_ct"),
                 ("stock_channels_last", "stock_cl", "args_cl", "g_cl"))

        # (a) one call per level
        for res, s in S.items():
            info = dict(resolution=res, B=B, H=s["H"], W=s["W"], hidden=HIDDEN, x=list(s["cx"]))
            with torch.no_grad():
                diff = (s["prod"](*s["args_cl"]) - s["stock"](*s["args_ct"])).abs().max().item()
                t = alternate({k: (lambda m=s[m], ar=s[ar]: m(*ar)) for k, m, ar, _ in kinds}, a.reps, a.rounds, a.warmup)
            versus(dict(item="a", what="one call forward, no grad", **info, max_abs_diff_vs_stock=diff), t)
            t = alternate({k: fwd_bwd(s[m], s[ar], s[g]) for k, m, ar, g in kinds}, a.reps, a.rounds, a.warmup)
            versus(dict(item="a", what="one call forward + backward", **info), t)

        # (b) the three levels as one iteration
        def all_levels(fns):
            return lambda: [f() for f in fns]
        with torch.no_grad():
            t = alternate({k: all_levels([(lambda m=s[m], ar=s[ar]: m(*ar)) for s in S.values()]) for k, m, ar, _ in kinds},
                          a.reps, a.rounds, a.warmup)
        versus(dict(item="b", what="three levels forward, no grad", B=B), t)
        t = alternate({k: all_levels([fwd_bwd(s[m], s[ar], s[g]) for s in S.values()]) for k, m, ar, g in kinds},
                      a.reps, a.rounds, a.warmup)
        versus(dict(item="b", what="three levels forward + backward", B=B), t)

        # (c) the recurrent loop: h fed back, loss on the last state of every level
        def loop(m_key, ar_key, g_key):
            def run():
                loss = 0
                for s in S.values():
                    m, ar = s[m_key], s[ar_key]
                    for p in m.parameters():
                        p.grad = None
                    net = ar[0].detach().requires_grad_()
                    for _ in range(a.iters):
                        net = m(net, *ar[1:])
                    loss = loss + (net * s[g_key]).sum()
                loss.backward()
            return run
        rec = dict(item="c", what=f"{a.iters} iterations of the three levels, forward + backward", B=B, iters=a.iters)
        t = {}
        for k, m, ar, g in kinds:
            fn = loop(m, ar, g)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t.update(alternate({k: fn}, 1, max(3, a.rounds // 2), 1))
            rec[k + "_peak_memory_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        versus(rec, t)

        # (d) kernel roles
        for res, s in S.items():
            H, W, cx = s["H"], s["W"], s["cx"]
            P, K = B * H * W, HIDDEN + sum(cx)
            m = s["prod"]
            wz, wr, wq = m.convz.weight.detach(), m.convr.weight.detach(), m.convq.weight.detach()
            h, cz, cr, cq, *xs = [ops._cl_source(t) for t in s["args_cl"]]
            new = lambda c=HIDDEN: torch.empty(B, H, W, c, device=dev)                                      # noqa: E731
            z, r, rh, q, hn, gq, gz, gr, buf = new(), new(), new(), new(), new(), new(), new(), new(), new(K)
            g = ops._cl_source(s["g_cl"])
            nrows = ops.get_lib().raw("stx_convgru_gate_rows")(P, HIDDEN)
            rows = torch.empty(nrows, 2, HIDDEN, device=dev)
            nchw = lambda t: (t.permute(0, 3, 1, 2), t.shape[-1])                                           # noqa: E731
            pk = {k: ops._convgru_pack(*w, mode) for k, w, mode in (("zr0", (wz, wr), 0), ("q0", (wq, None), 0),
                                                                    ("zr1", (wz, wr), 1), ("q1", (wq, None), 1))}
            roles = {
                "zr": lambda: ops.convgru_gemm([h] + xs, pk["zr0"], 2 * HIDDEN, B, H, W, epi=1, split=HIDDEN, bias0=m.convz.bias,
                                               bias1=m.convr.bias, add0=cz, add1=cr, h=h, out0=z, out1=rh, out2=r),
                "q": lambda: ops.convgru_gemm([nchw(rh)] + xs, pk["q0"], HIDDEN, B, H, W, epi=2, split=HIDDEN, bias0=m.convq.bias,
                                              add0=cq, h=h, z=z, out0=hn, out1=q),
                "gate_bwd": lambda: ops._call("stx_convgru_gate_bwd", ops._p(g[0]), g[1], ops._p(z), ops._p(q), ops._p(h[0]), h[1],
                                              ops._p(gq), ops._p(gz), ops._p(rows), P, HIDDEN),
                "dgrad_q": lambda: ops.convgru_gemm([nchw(gq)], pk["q1"], K, B, H, W, out0=buf, out_pitch=K),
                "reset_bwd": lambda: ops._call("stx_convgru_reset_bwd", ops._p(buf), K, ops._p(g[0]), g[1], ops._p(z), ops._p(r),
                                               ops._p(h[0]), h[1], ops._p(gr), ops._p(rows), P, HIDDEN),
                "dgrad_zr": lambda: ops.convgru_gemm([nchw(gz), nchw(gr)], pk["zr1"], K, B, H, W, add0=(buf, K), out0=buf,
                                                     out_pitch=K),
                "wgrad_zr": lambda: ops._convgru_wgrad([h] + xs, gz, gr, B, H, W),
                "wgrad_q": lambda: ops._convgru_wgrad([nchw(rh)] + xs, gq, None, B, H, W),
            }
            unit = 2.0 * P * 9 * K * HIDDEN                                                                 # one gate convolution
            flop = {"zr": 2 * unit, "q": unit, "dgrad_q": unit, "dgrad_zr": 2 * unit, "wgrad_zr": 2 * unit, "wgrad_q": unit}
            byts = {"gate_bwd": 6 * P * HIDDEN * 4, "reset_bwd": 8 * P * HIDDEN * 4}                        # maps read + written
            with torch.no_grad():
                t = alternate(roles, a.reps, a.rounds, a.warmup)
            rec = dict(item="d", what="kernel roles", resolution=res, B=B, H=H, W=W, K=K, gflop_per_gate_conv=round(unit / 1e9, 2))
            ms(rec, t)
            for role, (med, _, _) in t.items():
                if role in flop:
                    rec[role + "_fraction_of_mfma_peak"] = round(flop[role] / (med * 1e-3) / (PEAK_TFLOPS * 1e12), 3)
                else:
                    rec[role + "_fraction_of_hbm_peak"] = round(byts[role] / (med * 1e-3) / PEAK_HBM, 3)
            emit(rec)
        del S
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
