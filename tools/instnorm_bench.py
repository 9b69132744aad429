"""Times the fused instance norm (csrc/instnorm.hip, ops.instance_norm) against the stock-PyTorch op sequence it replaces, on one
GPU, at the maps of the iterative families' encoders at 576 x 960 -- 32 x 288 x 480, 48 / 96 x 144 x 240 (IGEV's stems),
64 x 288 x 480, 128 x 144 x 240 (the RAFT encoders at 1/2 and 1/4) and one 3-D map, 8 x 48 x 144 x 240 -- with B = 1 and B = 4, the
input dense NCHW and dense channels_last:

  plain      y = leaky_relu(instance_norm(x))                    stock: F.instance_norm, F.leaky_relu
  residual   y = relu(skip + relu(instance_norm(x)))             stock: F.instance_norm, F.relu, add, F.relu (ResidualBlock's tail)
each forward and forward + backward (to x, and to skip), with the peak memory of one forward + backward above what is resident
before it, and
  modules    one ResidualBlock (128 -> 128, stride 1) and one Conv2x_IN (96 -> 48, deconv, concat) at 1/4 resolution, forward +
             backward, the product module against the same module object run through its stock children (nn.InstanceNorm2d, ...).

The baseline never calls the code under test and reads nothing outside this repository.  It is timed in both layouts and the
faster one is the baseline of a row (`baseline_layout`).  Method (tools/geo_lookup_bench.py): every variant is warmed up, then the
variants of an item are timed alternately in one process, each sample = device events around `--reps` back-to-back executions; the
median over `--rounds` samples is reported with min / max.  Tensors below 256 MiB stay in the Infinity Cache between repetitions:
WARM figures.  `fraction_of_8TBps` is the product's compulsory traffic -- forward: x (+ skip) read, y written; backward: gy, x
(+ skip) read, gx (+ gskip) written -- per second over 8 TB/s (the layout copies of a channels_last input are not compulsory and
are not counted: they show as a lower fraction).  No time is fixed in advance.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd import ops  # noqa: E402
from stereo_toolbox_amd.models.IGEVStereo import Conv2x_IN  # noqa: E402
from stereo_toolbox_amd.models.RAFTStereo import ResidualBlock  # noqa: E402
from stereo_toolbox_amd.utils import fill_state_dict, synthetic_tensor  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402

PEAK_BYTES_PER_S = 8e12
SHAPES = [(32, 288, 480), (48, 144, 240), (96, 144, 240), (64, 288, 480), (128, 144, 240), (8, 48, 144, 240)]


def stock_plain(x, skip):
    return F.leaky_relu(F.instance_norm(x))


def stock_residual(x, skip):
    return F.relu(skip + F.relu(F.instance_norm(x)))


def product_plain(x, skip):
    return ops.instance_norm(x, "lrelu")


def product_residual(x, skip):
    return ops.instance_norm(x, "relu", skip=skip)


def stock_basic_conv_in(m, x):
    x = m.conv(x)
    x = m.IN(x) if m.use_in else x
    return F.leaky_relu(x) if m.relu else x


def stock_conv2x(m, x, rem):
    x = stock_basic_conv_in(m.conv1, x)
    if x.shape != rem.shape:
        x = F.interpolate(x, size=rem.shape[-2:], mode="nearest")
    return stock_basic_conv_in(m.conv2, torch.cat((x, rem), 1) if m.concat else x + rem)


def stock_residual_block(m, x):
    y = m.relu(m.norm1(m.conv1(x)))
    y = m.relu(m.norm2(m.conv2(y)))
    return m.relu((x if m.downsample is None else m.downsample(x)) + y)


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
                                                  "instnorm_bench.jsonl"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instnorm_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(rec, t, base_key):
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t[base_key][0] / t["product"][0], 3)
        rec.update(device=name, reps=a.reps, rounds=a.rounds)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def step(fn, x, s, gy):
        """forward + backward of fn(x, skip) to x and, when there is one, to skip"""
        x.grad = None
        if s is not None:
            s.grad = None
        fn(x, s).backward(gy)

    for shape in SHAPES:
        for B in a.batches:
            full = (B,) + shape
            n = 4.0 * B * torch.Size(shape).numel()                      # bytes of one tensor
            layouts = {"nchw": torch.contiguous_format}
            if len(shape) == 3:
                layouts["channels_last"] = torch.channels_last
            data = {}
            for k, f in layouts.items():
                x, s, gy = (synthetic_tensor(full, 90 + i).to(dev).contiguous(memory_format=f) for i in range(3))
                data[k] = (x, s, gy, x.clone().requires_grad_(), s.clone().requires_grad_())
            for form, product, stock, with_skip in (("plain", product_plain, stock_plain, False),
                                                    ("residual", product_residual, stock_residual, True)):
                tensors = 2 if with_skip else 1
                fwd_base = {"baseline_" + k: (lambda d=d: stock(d[0], d[1])) for k, d in data.items()}
                both_base = {"baseline_" + k: (lambda d=d: step(stock, d[3], d[4] if with_skip else None, d[2])) for k, d in data.items()}
                for k, d in data.items():
                    x, s, gy, xl, sl = d
                    sl = sl if with_skip else None
                    with torch.no_grad():
                        err = (product(x, s) - stock(x, s)).abs().max().item()
                        t = alternate({"product": lambda: product(x, s), **fwd_base}, a.reps, a.rounds, a.warmup)
                    best = min(fwd_base, key=lambda q: t[q][0])
                    fwd_bytes = n * (tensors + 1)
                    emit(dict(item=form, what="forward", B=B, shape=list(shape), layout=k, baseline_layout=best[9:],
                              max_abs_diff_vs_baseline=err,
                              fraction_of_8TBps=round(fwd_bytes / (t["product"][0] * 1e-3) / PEAK_BYTES_PER_S, 4)), t, best)
                    pstep = lambda: step(product, xl, sl, gy)  # noqa: E731
                    t = alternate({"product": pstep, **both_base}, a.reps, a.rounds, a.warmup)
                    best = min(both_base, key=lambda q: t[q][0])
                    both_bytes = fwd_bytes + n * (1 + 2 * tensors)
                    emit(dict(item=form, what="forward + backward", B=B, shape=list(shape), layout=k, baseline_layout=best[9:],
                              fraction_of_8TBps=round(both_bytes / (t["product"][0] * 1e-3) / PEAK_BYTES_PER_S, 4),
                              product_peak_mb=peak_mb(pstep), baseline_peak_mb=peak_mb(both_base[best])), t, best)
            del data

    # modules at 1/4 of 576 x 960: the same module object, through ops.instance_norm and through its stock children
    for B in a.batches:
        for label, m, shapes, stock in (
                ("ResidualBlock(128, 128, 'instance', 1)", ResidualBlock(128, 128, "instance", 1), [(B, 128, 144, 240)], stock_residual_block),
                ("Conv2x_IN(96, 48, deconv=True)", Conv2x_IN(96, 48, deconv=True), [(B, 96, 72, 120), (B, 48, 144, 240)], stock_conv2x)):
            sd = m.state_dict()
            fill_state_dict(sd)
            m.load_state_dict(sd)
            m = m.to(dev)
            ins = [synthetic_tensor(s, 70 + i).to(dev).requires_grad_() for i, s in enumerate(shapes)]
            gy = synthetic_tensor(tuple(m(*ins).shape), 75).to(dev)

            def run(fn):
                for leaf in ins + list(m.parameters()):
                    leaf.grad = None
                fn(*ins).backward(gy)
            with torch.no_grad():
                err = (m(*ins) - stock(m, *ins)).abs().max().item()
            pr, bl = (lambda: run(m)), (lambda: run(lambda *xs: stock(m, *xs)))
            t = alternate({"product": pr, "baseline": bl}, a.reps, a.rounds, a.warmup)
            emit(dict(item="module", what=label + ", forward + backward", B=B, shape=[list(s[1:]) for s in shapes], layout="nchw",
                      max_abs_diff_vs_baseline=err, product_peak_mb=peak_mb(pr), baseline_peak_mb=peak_mb(bl)), t, "baseline")

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
