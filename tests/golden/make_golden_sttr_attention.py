"""Golden fixture for STTR's attention and transformer (tests/test_sttr_attention.py).

  python tests/golden/make_golden_sttr_attention.py        (build container only: needs /root/reference)

The reference's OWN models/STTR/attention.py, transformer.py, pos_encoder.py and utilities/misc.py are loaded by path under a
stand-in package (the real package `__init__` pulls in the whole model zoo) and executed in fp32 and in fp64 on the seeded inputs
of tests/golden/sttr_attention_config.py.
Core records: one `MultiheadAttentionRelative` call -> v_o, raw_attn, attn and the gradients of sum(v_o g_vo) + sum(finite raw_attn
g_raw) to query, key (= value), in_proj_weight, in_proj_bias, out_proj.*.  Transformer records: `Transformer.forward` with N = 1 ->
attn_weight and the gradients of sum(finite attn_weight g_attn) to both feature maps and to every parameter (`norm.*`: asserted
absent).  Asserted: d_ref > 0 per tensor, the -inf pattern of raw_attn / attn_weight identical in both runs and equal to the causal
mask, and the reference's own sine table equal to sttr_attention_config.sine_table.
Stored per record, in the order of the config's layout: `:f64` (whole tensors up to WHOLE elements, `subsample` of the larger ones),
`:f32` (the whole tensors only), `:dref` = max|fp32 - fp64| over the finite entries and `:max` = max|fp64| over them.
-> tests/golden/sttr_attention.npz, tests/golden/state_dict_keys_sttr_transformer.json (reference Transformer(128, 8, 6))
"""
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.sttr_attention_config import (CORE, TRANSFORMER, core_inputs, core_layout, fill_parameters, is_whole,  # noqa: E402
                                                parameter_seed, sine_table, subsample, transformer_inputs, transformer_layout, transformer_parameters)

REF = "/root/reference/stereo_toolbox/models/STTR"


def reference():
    for name, path in (("sttr_ref", REF), ("sttr_ref.utilities", os.path.join(REF, "utilities"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    return tuple(importlib.import_module("sttr_ref." + m) for m in ("attention", "transformer", "pos_encoder", "utilities.misc"))


def pos_indexes(W):
    """transformer.py:100-102"""
    r, c = torch.linspace(W - 1, 0, W).view(W, 1), torch.linspace(0, W - 1, W).view(1, W)
    return (r + c).view(-1).long()


def finite_sum(x, g):
    fin = torch.isfinite(x)
    return (x[fin] * g.to(x.dtype)[fin]).sum()


def run_core(A, T, tag, dtype):
    kind, C, E, W, B, causal, table = CORE[tag]
    x = core_inputs(tag)
    mha = fill_parameters(A.MultiheadAttentionRelative(C, E), parameter_seed(tag)).to(dtype)
    query = x["query"].to(dtype).clone().requires_grad_()
    key = query if kind == "self" else x["key"].to(dtype).clone().requires_grad_()
    mask = T.TransformerCrossAttnLayer(C, E)._generate_square_subsequent_mask(W).to(dtype) if causal else None
    pos = None if x["pos"] is None else x["pos"].to(dtype)
    v_o, attn, raw = mha(query, key, key, attn_mask=mask, pos_enc=pos, pos_indexes=None if pos is None else pos_indexes(W))
    ((v_o * x["g_vo"].to(dtype)).sum() + finite_sum(raw, x["g_raw"])).backward()
    want_inf = torch.triu(torch.ones(W, W, dtype=torch.bool), 1).expand(B, W, W) if causal else torch.zeros(B, W, W, dtype=torch.bool)
    assert torch.equal(torch.isinf(raw), want_inf) and torch.isfinite(attn).all() and torch.isfinite(v_o).all(), tag
    res = {"v_o": v_o, "raw_attn": raw, "attn": attn, "g_query": query.grad}
    if kind == "cross":
        res["g_key"] = key.grad
    res.update({"g_" + n: p.grad for n, p in mha.named_parameters()})
    return {k: v.detach() for k, v in res.items()}


def run_transformer(T, tag, dtype):
    C, E, L, H, W = TRANSFORMER[tag]
    x = transformer_inputs(tag)
    model = fill_parameters(T.Transformer(C, E, L), parameter_seed(tag)).to(dtype)
    assert [(n, tuple(p.shape)) for n, p in model.named_parameters()] == transformer_parameters(tag), tag
    left, right = (x[k].to(dtype).clone().requires_grad_() for k in ("feat_left", "feat_right"))
    attn = model(left, right, x["pos"].to(dtype))
    assert attn.shape == (1, H, W, W) and torch.equal(torch.isinf(attn), torch.triu(torch.ones(W, W, dtype=torch.bool), 1).expand(1, H, W, W))
    finite_sum(attn, x["g_attn"]).backward()
    assert model.norm.weight.grad is None and model.norm.bias.grad is None
    res = {"attn_weight": attn, "g_feat_left": left.grad, "g_feat_right": right.grad}
    res.update({"g:" + n: p.grad for n, p in model.named_parameters() if not n.startswith("norm.")})
    return {k: v.detach() for k, v in res.items()}


def store_record(store, key, layout, r32, r64):
    f64, f32, dref, peak = [], [], [], []
    assert set(r32) == set(r64) == {k for k, _ in layout}, key
    for k, shape in layout:
        a, b = r32[k], r64[k]
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and tuple(a.shape) == tuple(b.shape) == shape, (key, k, a.shape, shape)
        fin = torch.isfinite(b)
        assert torch.equal(fin, torch.isfinite(a)), (key, k)
        d = (a.double() - b)[fin].abs().max().item()
        assert d > 0, (key, k)
        dref.append(d)
        peak.append(b[fin].abs().max().item())
        if is_whole(shape):
            f64.append(b.reshape(-1))
            f32.append(a.reshape(-1))
        else:
            f64.append(subsample(b))
    store[key + ":f64"] = torch.cat(f64).numpy().copy()
    if f32:
        store[key + ":f32"] = torch.cat(f32).numpy().copy()
    store[key + ":dref"], store[key + ":max"] = np.array(dref), np.array(peak)
    for (k, _), d, m in zip(layout, dref, peak):
        print(f"{key:22s} {k:52s} d_ref {d:.2e}  max {m:.3g}", flush=True)


def main():
    warnings.filterwarnings("ignore")
    A, T, P, U = reference()
    for W, C in ((17, 128), (33, 32), (320, 128)):
        ref_table = P.PositionEncodingSine1DRelative(C, normalize=False)(U.NestedTensor(torch.zeros(1, 3, 4, W), None))
        assert torch.equal(ref_table, sine_table(W, C)), (W, C)
    store = {}
    for tag in CORE:
        store_record(store, "core:" + tag, core_layout(tag), run_core(A, T, tag, torch.float32), run_core(A, T, tag, torch.float64))
    for tag in TRANSFORMER:
        store_record(store, "transformer:" + tag, transformer_layout(tag), run_transformer(T, tag, torch.float32),
                     run_transformer(T, tag, torch.float64))
    path = os.path.join(HERE, "sttr_attention.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")
    with open(os.path.join(HERE, "state_dict_keys_sttr_transformer.json"), "w") as f:
        json.dump(list(T.Transformer(128, 8, 6).state_dict()), f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
