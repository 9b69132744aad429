"""Times the SelectiveStereo stage (models.SelectiveStereo on csrc/selgru.hip, csrc/convgru.hip and csrc/csa.hip) against the stock
PyTorch-ROCm op sequence it replaces, on one GPU, at the three levels of a 576x960 input with the model's channel counts
(reference SelectiveIGEV/update.py:223-238, hidden 128):

    1/4: 144x240, x = (128, 128, 128)      1/8: 72x120, x = (128, 128, 128)      1/16: 36x60, x = (128, 128)      B = 1 and B = 4

  (a) one selective cell, product against stock: forward (no grad) and forward + backward (gradients to att, h, every x and
      every parameter).  The stock side is the same module from nn.Conv2d, cat, sigmoid and tanh with the same weights, timed in
      contiguous and in channels_last layout; the faster one is the baseline.  It never calls the code under test.
  (b) the three levels as one iteration, forward and forward + backward.
  (c) `--iters` (22) iterations of the three levels, h fed back, att fixed, forward + backward, with the peak memory of both sides.
  (d) the contextual spatial attention on the three context maps (C = 128), forward and forward + backward, against the stock
      pooling / 1x1 / 7x7 sequence.
  (e) the kernel roles on their own: the 1x1 launches with the achieved fraction of the 157.3 TFLOP/s fp32-MFMA peak, the
      streaming passes with the fraction of the 8 TB/s HBM peak their compulsory traffic amounts to.

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
from stereo_toolbox_amd.models.SelectiveStereo import (ChannelAttentionEnhancement, SelectiveConvGRU,  # noqa: E402
                                                       SpatialAttentionExtractor, contextual_spatial_attention)
from stereo_toolbox_amd.utils import fill_state_dict, synthetic_tensor  # noqa: E402

PEAK_TFLOPS = 157.3
PEAK_HBM = 8.0e12
HIDDEN = 128
LEVELS = {"1/4": (144, 240, (128, 128, 128)), "1/8": (72, 120, (128, 128, 128)), "1/16": (36, 60, (128, 128))}


class StockRaftGRU(nn.Module):
    def __init__(self, hidden, cin, k):
        super().__init__()
        self.convz, self.convr, self.convq = (nn.Conv2d(hidden + cin, hidden, k, padding=k // 2) for _ in range(3))

    def forward(self, h, x):
        hx = torch.cat([h, x], 1)
        z = torch.sigmoid(self.convz(hx))
        r = torch.sigmoid(self.convr(hx))
        q = torch.tanh(self.convq(torch.cat([r * h, x], 1)))
        return (1 - z) * h + z * q


class StockSelective(nn.Module):
    """The selective unit from stock torch modules (same state-dict keys as the product)."""

    def __init__(self, hidden, cin):
        super().__init__()
        self.small_gru, self.large_gru = StockRaftGRU(hidden, cin, 1), StockRaftGRU(hidden, cin, 3)

    def forward(self, att, h, *x):
        x = torch.cat(x, 1)
        return self.small_gru(h, x) * att + self.large_gru(h, x) * (1 - att)


class StockCSA(nn.Module):
    """cam and sam from stock torch modules, applied as the model does (same state-dict keys as the product pair)."""

    def __init__(self, C):
        super().__init__()
        self.fc = nn.Sequential(nn.Conv2d(C, C // 16, 1, bias=False), nn.ReLU(), nn.Conv2d(C // 16, C, 1, bias=False))
        self.samconv = nn.Conv2d(2, 1, 7, padding=3, bias=False)

    def forward(self, x):
        pool = torch.nn.functional
        gate = torch.sigmoid(self.fc(pool.adaptive_avg_pool2d(x, 1)) + self.fc(pool.adaptive_max_pool2d(x, 1)))
        xp = gate * x
        m = torch.cat([xp.mean(1, keepdim=True), xp.max(1, keepdim=True)[0]], 1)
        return xp, torch.sigmoid(self.samconv(m))


def filled(m):
    sd = m.state_dict()
    fill_state_dict(sd)
    m.load_state_dict(sd)
    return m


def level_setup(res, B, dev):
    H, W, cx = LEVELS[res]
    prod = filled(SelectiveConvGRU(HIDDEN, sum(cx)))
    sd = prod.state_dict()
    prod = prod.to(dev)
    stock = StockSelective(HIDDEN, sum(cx))
    stock.load_state_dict(sd)
    stock = stock.to(dev)
    stock_cl = StockSelective(HIDDEN, sum(cx))
    stock_cl.load_state_dict(sd)
    stock_cl = stock_cl.to(dev).to(memory_format=torch.channels_last)
    cl = lambda c, k, lo=-1.0, hi=1.0: synthetic_tensor((B, H, W, c), k, lo=lo, hi=hi).to(dev).permute(0, 3, 1, 2)      # noqa: E731
    args_cl = [cl(1, 4, 0.05, 0.95), torch.tanh(cl(HIDDEN, 1)), *[cl(c, 10 + i) for i, c in enumerate(cx)]]
    args_ct = [t.contiguous() for t in args_cl]
    g_cl = cl(HIDDEN, 3)
    cam, sam = filled(ChannelAttentionEnhancement(HIDDEN)), filled(SpatialAttentionExtractor(7))
    csa_sd = {**cam.state_dict(), **sam.state_dict()}                 # fc.0.weight, fc.2.weight, samconv.weight
    csa_stock, csa_stock_cl = StockCSA(HIDDEN), StockCSA(HIDDEN)
    csa_stock.load_state_dict(csa_sd)
    csa_stock_cl.load_state_dict(csa_sd)
    ctx_cl = cl(HIDDEN, 5)
    return dict(H=H, W=W, cx=cx, prod=prod, stock=stock, stock_cl=stock_cl, args_cl=args_cl, args_ct=args_ct, g_cl=g_cl,
                g_ct=g_cl.contiguous(), cam=cam.to(dev), sam=sam.to(dev), csa_stock=csa_stock.to(dev),
                csa_stock_cl=csa_stock_cl.to(dev).to(memory_format=torch.channels_last), ctx_cl=ctx_cl, ctx_ct=ctx_cl.contiguous(),
                ga_cl=cl(1, 6), gx_cl=cl(HIDDEN, 7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selective_bench.jsonl"))
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("selective_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
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
            versus(dict(item="a", what="one selective cell forward, no grad", **info, max_abs_diff_vs_stock=diff), t)
            t = alternate({k: fwd_bwd(s[m], s[ar], s[g]) for k, m, ar, g in kinds}, a.reps, a.rounds, a.warmup)
            versus(dict(item="a", what="one selective cell forward + backward", **info), t)

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

        # (c) the recurrent loop: h fed back, att fixed, loss on the last state of every level
        def loop(m_key, ar_key, g_key):
            def run():
                loss = 0
                for s in S.values():
                    m, ar = s[m_key], s[ar_key]
                    for p in m.parameters():
                        p.grad = None
                    net = ar[1].detach().requires_grad_()
                    for _ in range(a.iters):
                        net = m(ar[0], net, *ar[2:])
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

        # (d) the attention on the three context maps
        def csa_product(grad):
            def run():
                xs = [s["ctx_cl"].detach().requires_grad_(grad) for s in S.values()]
                s0 = next(iter(S.values()))
                inp, att = contextual_spatial_attention(s0["cam"], s0["sam"], xs)
                if grad:
                    for p in list(s0["cam"].parameters()) + list(s0["sam"].parameters()):
                        p.grad = None
                    torch.autograd.backward(inp + att, [s["gx_cl"] for s in S.values()] + [s["ga_cl"] for s in S.values()])
            return run

        def csa_stock(key, xkey, grad):
            def run():
                s0 = next(iter(S.values()))
                m = s0[key]
                if grad:
                    for p in m.parameters():
                        p.grad = None
                outs, gs = [], []
                for s in S.values():
                    xp, att = m(s[xkey].detach().requires_grad_(grad))
                    outs += [xp, att]
                    gs += [s["gx_cl"] if xkey == "ctx_cl" else s["gx_cl"].contiguous(), s["ga_cl"]]
                if grad:
                    torch.autograd.backward(outs, gs)
            return run
        for grad, what in ((False, "attention on the three context maps forward, no grad"),
                           (True, "attention on the three context maps forward + backward")):
            fns = {"product": csa_product(grad), "stock_contiguous": csa_stock("csa_stock", "ctx_ct", grad),
                   "stock_channels_last": csa_stock("csa_stock_cl", "ctx_cl", grad)}
            if grad:
                t = alternate(fns, a.reps, a.rounds, a.warmup)
            else:
                with torch.no_grad():
                    t = alternate(fns, a.reps, a.rounds, a.warmup)
            versus(dict(item="d", what=what, B=B, C=HIDDEN), t)

        # (e) kernel roles of the new kernels
        for res, s in S.items():
            H, W, cx = s["H"], s["W"], s["cx"]
            P, K = B * H * W, HIDDEN + sum(cx)
            m = s["prod"].small_gru
            wz, wr, wq = m.convz.weight.detach(), m.convr.weight.detach(), m.convq.weight.detach()
            att, h, *xs = [ops._cl_source(t) for t in s["args_cl"]]
            attc = att[0].contiguous()
            new = lambda c=HIDDEN: torch.empty(B, H, W, c, device=dev)                                      # noqa: E731
            z, r, rh, q, hn, gq, gz, gr, gs_, gl_, buf, prev = (new(), new(), new(), new(), new(), new(), new(), new(), new(), new(),
                                                                new(K), new(K))
            gatt = torch.empty(B, H, W, device=dev)
            g = ops._cl_source(s["g_cl"])
            nchw = lambda t: (t.permute(0, 3, 1, 2), t.shape[-1])                                           # noqa: E731
            pk = {k: ops._selgru_pack(*w, mode) for k, w, mode in (("zr0", (wz, wr), 0), ("q0", (wq, None), 0),
                                                                   ("zr1", (wz, wr), 1), ("q1", (wq, None), 1))}
            ws = ops._WS.get("selgru_col_sum", ops.get_lib().raw("stx_selgru_col_sum_workspace_floats")(P, HIDDEN), dev)
            sums = torch.empty(3, HIDDEN, device=dev)
            x_ctx, pitch = ops._cl_source(s["ctx_cl"])
            nblk, psum, pmax, pidx = ops._csa_pool(x_ctx, pitch, B, HIDDEN, H * W)
            xp, cmap, att_o = new(), new(2), torch.empty(B, 1, H, W, device=dev)
            w1, w2, wsam = s["cam"].fc[0].weight.detach(), s["cam"].fc[2].weight.detach(), s["sam"].samconv.weight.detach()
            roles = {
                "zr_1x1": lambda: ops._raft_gemm(1, [h] + xs, pk["zr0"], 2 * HIDDEN, B, H, W, epi=1, split=HIDDEN, bias0=m.convz.bias,
                                                 bias1=m.convr.bias, h=h, out0=z, out1=rh, out2=r),
                "q_1x1_blend": lambda: ops._raft_gemm(1, [nchw(rh)] + xs, pk["q0"], HIDDEN, B, H, W, epi=2, split=HIDDEN,
                                                      bias0=m.convq.bias, h=h, z=z, att=attc, other=hn, blend=1, out0=hn, out1=q),
                "blend_bwd": lambda: ops._call("stx_selgru_blend_bwd", ops._p(g[0]), g[1], ops._p(attc), ops._p(z), ops._p(q), ops._p(z),
                                               ops._p(q), ops._p(h[0]), h[1], ops._p(gs_), ops._p(gl_), ops._p(gatt), P, HIDDEN),
                "dgrad_q_1x1": lambda: ops._raft_gemm(1, [nchw(gq)], pk["q1"], K, B, H, W, out0=buf, out_pitch=K),
                "dgrad_zr_1x1": lambda: ops._raft_gemm(1, [nchw(gz), nchw(gr)], pk["zr1"], K, B, H, W, add0=(buf, K), add1=(prev, K),
                                                       out0=buf, out_pitch=K),
                "wgrad_zr_1x1": lambda: ops._raft_wgrad(1, [h] + xs, gz, gr),
                "wgrad_q_1x1": lambda: ops._raft_wgrad(1, [nchw(rh)] + xs, gq, None),
                "bias_col_sum": lambda: ops._call("stx_selgru_col_sum", ops._p(gq), ops._p(gz), ops._p(gr), ops._p(sums), ops._p(ws), P,
                                                  HIDDEN),
                "csa_pool": lambda: ops._call("stx_csa_pool", ops._p(x_ctx), pitch, ops._p(psum), ops._p(pmax), ops._p(pidx), B, H * W,
                                              HIDDEN),
                "csa_apply": lambda: ops._call("stx_csa_apply", ops._p(x_ctx), pitch, ops._p(psum), ops._p(pmax), ops._p(pidx), nblk,
                                               ops._p(w1), ops._p(w2), ops._p(xp), ops._p(cmap), None, None, None, None, B, H * W, HIDDEN),
                "csa_sam": lambda: ops._call("stx_csa_sam", ops._p(cmap), ops._p(wsam), ops._p(att_o), B, H, W, 7),
            }
            for t_ in (z, q, gq, gz, gr, buf, prev, hn):
                t_.zero_()
            unit = 2.0 * P * K * HIDDEN                                                                     # one 1x1 gate convolution
            flop = {"zr_1x1": 2 * unit, "q_1x1_blend": unit, "dgrad_q_1x1": unit, "dgrad_zr_1x1": 2 * unit, "wgrad_zr_1x1": 2 * unit,
                    "wgrad_q_1x1": unit}
            byts = {"blend_bwd": 8 * P * HIDDEN * 4, "bias_col_sum": 3 * P * HIDDEN * 4, "csa_pool": P * HIDDEN * 4,
                    "csa_apply": 2 * P * HIDDEN * 4, "csa_sam": 3 * P * 4}                                   # maps read + written
            with torch.no_grad():
                t = alternate(roles, a.reps, a.rounds, a.warmup)
            rec = dict(item="e", what="kernel roles", resolution=res, B=B, H=H, W=W, K=K, gflop_per_1x1_gate_conv=round(unit / 1e9, 2))
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
