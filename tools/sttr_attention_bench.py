"""Times STTR's attention with relative positions (csrc/sttr_attention.hip behind `models.STTR.MultiheadAttentionRelative` and
`models.STTR.Transformer`) against the stock-PyTorch op sequence it replaces, on one GPU, at the transformer's shapes for a
576x960 input (downsample 3: N = 1, H = 192, W = 320) and a 384x1248 input (N = 1, H = 128, W = 416), C = 128, 8 heads:

  (a) one cross-attention call, forward (no autograd)              (b) the same, forward + backward to query, key and parameters
  (c) the 6-layer Transformer, forward (no autograd)               (d) the same, forward + backward to the features and parameters

The baseline is tests/test_sttr_attention.py's op-for-op restatement of the reference ('stock': the [W, W, C] gather of the sine
table, its C -> 2C projection, three [B, 8, W, W] einsums, softmax, bmm); in (d) every layer runs under torch.utils.checkpoint, the
way the reference runs it.  Both sides share one set of parameters and never read anything outside this repository.
Method (tools/geo_lookup_bench.py): every variant is warmed up, then the variants of an item are timed alternately in one
process, each sample = device events around `--reps` back-to-back executions; the median over `--rounds` samples is reported with
min / max.  Peak memory is torch.cuda.max_memory_allocated over one execution of each side minus what was allocated before it.
The inputs of the timed calls stay resident: these are WARM figures.  No time is fixed in advance.
One shape per invocation (`--shape 192x320`), so that each runs under its own time limit; records are appended to --out.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereo_toolbox_amd.models import STTR  # noqa: E402
from tests.golden.sttr_attention_config import fill_parameters, normal, sine_table  # noqa: E402
from tests.test_sttr_attention import attention, transformer  # noqa: E402
from tools.geo_lookup_bench import alternate  # noqa: E402
from tools.sttr_head_bench import peak_bytes  # noqa: E402

C, E, LAYERS = 128, 8, 6
NINF = float("-inf")


def max_diff(xs, ys):
    return [(x - y)[torch.isfinite(y)].abs().max().item() for x, y in zip(xs, ys)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "sttr_attention_bench.jsonl"))
    ap.add_argument("--shape", default="192x320", help="HxW of the low-resolution image (N = 1)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sttr_attention_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    H, W = (int(s) for s in a.shape.split("x"))
    shape = dict(N=1, H=H, W=W, C=C, heads=E, layers=LAYERS, device=torch.cuda.get_device_name(0))
    lines = []

    def emit(item, what, t, **extra):
        rec = dict(item=item, what=what, **shape, reps=a.reps, rounds=a.rounds)
        for k, (med, lo, hi) in t.items():
            rec[k + "_ms"], rec[k + "_ms_min"], rec[k + "_ms_max"] = round(med, 5), round(lo, 5), round(hi, 5)
        rec["speedup_vs_baseline"] = round(t["baseline"][0] / t["product"][0], 3)
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def measure(item, what, product, baseline):
        err = max_diff(product(), baseline())
        mem = dict(product_peak_bytes=peak_bytes(product), baseline_peak_bytes=peak_bytes(baseline))
        emit(item, what, alternate({"product": product, "baseline": baseline}, a.reps, a.rounds, a.warmup), max_abs_diff_vs_baseline=err, **mem)

    # ---- one cross-attention call of the last layer: causal, raw_attn wanted
    mha = fill_parameters(STTR.MultiheadAttentionRelative(C, E), 1).to(dev)
    P = dict(mha.named_parameters())
    query, key = normal((W, H, C), 2).to(dev).requires_grad_(), normal((W, H, C), 3).to(dev).requires_grad_()
    pos = sine_table(W, C).to(dev)
    mask = STTR.TransformerCrossAttnLayer(C, E)._generate_square_subsequent_mask(W, dev)
    g_vo, g_raw = normal((W, H, C), 4).to(dev), normal((H, W, W), 5).to(dev)
    leaves = [query, key] + list(P.values())

    def product_call():
        v_o, _, raw = mha(query, key, key, attn_mask=mask, pos_enc=pos, need_attn=False, need_raw=True)
        return v_o, raw

    def baseline_call():
        v_o, _, raw = attention("stock", P, "", query, key, True, pos, E)
        return v_o, raw

    def step(fn, leaves, weights):
        for t in leaves:
            t.grad = None
        outs = fn()
        sum((o.masked_fill(o == NINF, 0.0) * g).sum() for o, g in zip(outs, weights)).backward()
        return [t.grad for t in leaves if t.grad is not None]

    with torch.no_grad():
        measure("a", "cross attention (causal, raw_attn), forward", product_call, baseline_call)
    measure("b", "cross attention (causal, raw_attn), forward + backward", lambda: step(product_call, leaves, (g_vo, g_raw)),
            lambda: step(baseline_call, leaves, (g_vo, g_raw)))

    # ---- the 6-layer transformer
    model = fill_parameters(STTR.Transformer(C, E, LAYERS), 6).to(dev)
    TP = dict(model.named_parameters())
    left, right = normal((1, C, H, W), 7).to(dev).requires_grad_(), normal((1, C, H, W), 8).to(dev).requires_grad_()
    g_attn = normal((1, H, W, W), 9).to(dev)
    tleaves = [left, right] + list(TP.values())
    with torch.no_grad():
        measure("c", "Transformer (6 layers), forward", lambda: (model(left, right, pos),),
                lambda: (transformer("stock", TP, left, right, pos, LAYERS, E),))
    measure("d", "Transformer (6 layers), forward + backward (baseline under checkpoint)",
            lambda: step(lambda: (model(left, right, pos),), tleaves, (g_attn,)),
            lambda: step(lambda: (transformer("stock", TP, left, right, pos, LAYERS, E, checkpointed=True),), tleaves, (g_attn,)))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    print("appended to", a.out)


if __name__ == "__main__":
    main()
