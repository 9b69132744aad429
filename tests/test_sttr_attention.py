"""STTR's attention with relative positional encoding and its transformer (reference models/STTR/attention.py, transformer.py)
on the kernels of csrc/sttr_attention.hip: `ops.sttr_rel_attention`, `models.STTR.MultiheadAttentionRelative`, `Transformer`.

* tests/golden/sttr_attention.npz holds what the reference's OWN modules give on the seeded cases of
  tests/golden/sttr_attention_config.py, in fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| > 0 over the finite entries
  (tests/golden/make_golden_sttr_attention.py).  Tensors of more than WHOLE elements keep d_ref, max|fp64| and a strided subsample
  of the fp64 tensor.
* Two plain-torch restatements (`attention` of tests/restated.py, `transformer` here): 'stock', the reference op for op (the [W, W, C] gather of the table, its
  projection, three einsums -- also the stock side of tools/sttr_attention_bench.py), and 'table', the form the kernels compute
  (the [2W-1, C] table projected, row (W-1-w) + v read for the pair (w, v)).  Both are pinned to the fixture on the CPU -- in fp64
  to 1e-11 (whole tensors or the subsample), in fp32 to 2 x d_ref -- and the table form then serves as the fp64 oracle of the
  subsampled tensors.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with fp64: values within VALUE_FACTOR (2) x d_ref, gradients
  within GRAD_FACTOR (3) x d_ref.  Every element of every tensor is compared, -inf entries by equality, and the achieved ratios go
  to the parity report.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stereo_toolbox_amd import ops
from stereo_toolbox_amd.models import STTR
from tests.backends import be, ptr  # noqa: F401
from tests.golden.sttr_attention_config import (CORE, CORE_GPU_ONLY, TRANSFORMER, TRANSFORMER_GPU_ONLY, core_inputs, core_layout,
                                                fill_parameters, is_whole, parameter_seed, sine_table, subsample, transformer_inputs,
                                                transformer_layout, transformer_parameters)
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, Env, env, on, sync, within, within_inf  # noqa: F401
from tests.restated import attention

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sttr_attention.npz")
NINF = float("-inf")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def finite_sum(x, g):
    fin = torch.isfinite(x)
    return (x[fin] * g.to(x.dtype)[fin]).sum()


# ------------------------------------------------------------------------------------------ the restatements (plain torch)
def transformer(form, P, left, right, pos, L, E, checkpointed=False):
    """Transformer.forward -> attn_weight [N, H, W, W]; the left / right split at H * N.  checkpointed: every layer under
    torch.utils.checkpoint, the way the reference runs them."""
    from torch.utils.checkpoint import checkpoint
    N, C, H, W = left.shape
    hn = H * N
    feat = torch.cat([t.permute(1, 3, 2, 0).flatten(2).permute(1, 2, 0) for t in (left, right)], dim=1)

    def norm(x, name):
        return F.layer_norm(x, (C,), P[name + ".weight"], P[name + ".bias"])

    def self_layer(feat, p):
        f2 = norm(feat, p + "norm1")
        return feat + attention(form, P, p + "self_attn.", f2, f2, False, pos, E)[0]

    def cross_layer(fl, fr, p, last):
        l2, r2 = norm(fl, p + "norm1"), norm(fr, p + "norm1")
        fr = fr + attention(form, P, p + "cross_attn.", r2, l2, False, None if pos is None else torch.flip(pos, [0]), E)[0]
        r2 = norm(fr, p + "norm2")
        out, _, raw = attention(form, P, p + "cross_attn.", l2, r2, last, pos, E)
        return torch.cat([fl + out, fr], dim=1), raw

    run = (lambda fn, *a: checkpoint(fn, *a, use_reentrant=False)) if checkpointed else (lambda fn, *a: fn(*a))
    raw = None
    for layer in range(L):
        feat = run(self_layer, feat, f"self_attn_layers.{layer}.")
        feat, raw = run(cross_layer, feat[:, :hn], feat[:, hn:], f"cross_attn_layers.{layer}.", layer == L - 1)
    return raw.view(H, N, W, W).permute(1, 0, 2, 3)


def _parameters(module, dtype, device="cpu"):
    return {n: p.detach().to(device=device, dtype=dtype).clone().requires_grad_() for n, p in module.named_parameters()}


def _restated_core(form, tag, dtype):
    kind, C, E, W, B, causal, table = CORE[tag]
    x = core_inputs(tag)
    P = _parameters(fill_parameters(STTR.MultiheadAttentionRelative(C, E), parameter_seed(tag)), dtype)
    query = x["query"].to(dtype).clone().requires_grad_()
    key = query if kind == "self" else x["key"].to(dtype).clone().requires_grad_()
    v_o, attn, raw = attention(form, P, "", query, key, causal, None if x["pos"] is None else x["pos"].to(dtype), E)
    ((v_o * x["g_vo"].to(dtype)).sum() + finite_sum(raw, x["g_raw"])).backward()
    res = {"v_o": v_o.detach(), "raw_attn": raw.detach(), "attn": attn.detach(), "g_query": query.grad}
    if kind == "cross":
        res["g_key"] = key.grad
    res.update({"g_" + n: p.grad for n, p in P.items()})
    return res


def _restated_transformer(form, tag, dtype):
    C, E, L, H, W = TRANSFORMER[tag]
    x = transformer_inputs(tag)
    P = _parameters(fill_parameters(STTR.Transformer(C, E, L), parameter_seed(tag)), dtype)
    left, right = (x[k].to(dtype).clone().requires_grad_() for k in ("feat_left", "feat_right"))
    attn = transformer(form, P, left, right, x["pos"].to(dtype), L, E)
    finite_sum(attn, x["g_attn"]).backward()
    res = {"attn_weight": attn.detach(), "g_feat_left": left.grad, "g_feat_right": right.grad}
    res.update({"g:" + n: p.grad for n, p in P.items() if not n.startswith("norm.")})
    assert P["norm.weight"].grad is None and P["norm.bias"].grad is None
    return res


def _restated(key, form, dtype):
    group, tag = key.split(":")
    return _restated_core(form, tag, dtype) if group == "core" else _restated_transformer(form, tag, dtype)


@functools.lru_cache(maxsize=3)
def _restated64(key):
    return _restated(key, "table", torch.float64)


def _layout(key):
    group, tag = key.split(":")
    return core_layout(tag) if group == "core" else transformer_layout(tag)


def _record(gold, key):
    """tensor name -> (fp64 whole tensor or None, fp32 whole tensor or None, fp64 subsample or None, d_ref, max|fp64|)"""
    f64 = torch.from_numpy(gold[key + ":f64"])
    f32 = torch.from_numpy(gold[key + ":f32"]) if key + ":f32" in gold else None
    dref, peak = gold[key + ":dref"], gold[key + ":max"]
    rec, at64, at32 = {}, 0, 0
    for n, (k, shape) in enumerate(_layout(key)):
        numel = int(np.prod(shape))
        if is_whole(shape):
            rec[k] = (f64[at64:at64 + numel].reshape(shape), f32[at32:at32 + numel].reshape(shape), None, float(dref[n]), float(peak[n]))
            at64, at32 = at64 + numel, at32 + numel
        else:
            sub = subsample(torch.empty(numel)).numel()
            rec[k] = (None, None, f64[at64:at64 + sub], float(dref[n]), float(peak[n]))
            at64 += sub
    assert at64 == f64.numel() and (f32 is None or at32 == f32.numel()), key
    return rec


def _gap(a, b):
    """max|a - b| over the finite entries; the -inf patterns must be equal"""
    assert a.shape == b.shape and torch.equal(torch.isinf(a), torch.isinf(b))
    fin = torch.isfinite(b)
    return (a.double() - b.double())[fin].abs().max().item()


ALL_KEYS = ["core:" + t for t in CORE] + ["transformer:" + t for t in TRANSFORMER]


# (the gather form is pinned at the smaller records: it is the memory hog this project replaces)
PINNED = [(k, "table") for k in ALL_KEYS] + [(k, "stock") for k in ALL_KEYS if k not in ("core:w320_causal", "transformer:t70")]


@pytest.mark.parametrize("key,form", PINNED)
def test_restatement_matches_reference_fixture(gold, key, form):
    r64 = _restated64(key) if form == "table" else _restated(key, form, torch.float64)
    r32 = _restated(key, form, torch.float32)
    rec = _record(gold, key)
    assert set(rec) == set(r64)
    for k, (want64, want32, sub, dref, peak) in rec.items():
        assert dref > 0, k
        tol = 1e-11 * max(1.0, peak)
        fin = torch.isfinite(r64[k])
        assert abs(r64[k][fin].abs().max().item() - peak) <= tol, k
        if want64 is not None:
            assert r32[k].dtype == torch.float32
            assert _gap(r64[k], want64) <= tol, k
            assert _gap(r32[k], want64) <= 2 * dref, (k, _gap(r32[k], want64), dref)
        else:
            assert _gap(subsample(r64[k]), sub) <= tol, k
            assert _gap(r32[k], r64[k]) <= 2 * dref, (k, _gap(r32[k], r64[k]), dref)


def _want(gold, key, k):
    want64, _, _, dref, _ = _record(gold, key)[k]
    return (want64 if want64 is not None else _restated64(key)[k]), dref


# ------------------------------------------------------------------------------------------ the product vs fp64
def _core(env, tag, via):
    """The product on a core record, through the module or through ops.sttr_rel_attention between stock projections."""
    kind, C, E, W, B, causal, table = CORE[tag]
    x = core_inputs(tag)
    dev = env.device
    mha = fill_parameters(STTR.MultiheadAttentionRelative(C, E), parameter_seed(tag)).to(dev)
    query = x["query"].to(dev).requires_grad_()
    key = query if kind == "self" else x["key"].to(dev).requires_grad_()
    pos = None if x["pos"] is None else x["pos"].to(dev)
    with env.ctx():
        if via == "module":
            mask = STTR.TransformerCrossAttnLayer(C, E)._generate_square_subsequent_mask(W, dev) if causal else None
            v_o, attn, raw = mha(query, key, key, attn_mask=mask, pos_enc=pos, pos_indexes=None)
        else:
            w_in, b_in, s, hd = mha.in_proj_weight, mha.in_proj_bias, 0.25, C // E
            q = (F.linear(query, w_in[:C], b_in[:C]) * s).view(W, B, E, hd)
            k, v = (F.linear(key, w_in[n * C:(n + 1) * C], b_in[n * C:(n + 1) * C]).view(W, B, E, hd) for n in (1, 2))
            q_r = k_r = None
            if pos is not None:
                q_r = (F.linear(pos, w_in[:C], b_in[:C]) * s).view(2 * W - 1, E, hd)
                k_r = F.linear(pos, w_in[C:2 * C], b_in[C:2 * C]).view(2 * W - 1, E, hd)
            o, raw, attn = ops.sttr_rel_attention(q, k, v, q_r, k_r, causal, True, True)
            v_o = F.linear(o.view(W, B, C), mha.out_proj.weight, mha.out_proj.bias)
        assert not attn.requires_grad
        ((v_o * x["g_vo"].to(dev)).sum() + (raw.masked_fill(raw == NINF, 0.0) * x["g_raw"].to(dev)).sum()).backward()
        sync(env)
    res = {"v_o": v_o, "raw_attn": raw, "attn": attn, "g_query": query.grad}
    if kind == "cross":
        res["g_key"] = key.grad
    res.update({"g_" + n: p.grad for n, p in mha.named_parameters()})
    return res


@pytest.mark.parametrize("via", ["module", "op"])
@pytest.mark.parametrize("backend,tag", on(list(CORE), CORE_GPU_ONLY))
def test_attention_matches_reference_fp64(backend, tag, via, gold, parity_log):
    """v_o, raw_attn (-inf pattern by equality), attn (the op's `avg`) and every gradient of one attention call."""
    env = Env(backend)
    got = _core(env, tag, via)
    key = "core:" + tag
    assert set(got) == {k for k, _ in core_layout(tag)}
    for k, shape in core_layout(tag):
        assert tuple(got[k].shape) == shape and got[k].dtype == torch.float32, k
        within_inf(got[k], *_want(gold, key, k), GRAD_FACTOR if k.startswith("g_") else VALUE_FACTOR,
                    f"sttr attention {tag} {k} {via} [{backend}]", parity_log)


def _model(tag, device):
    C, E, L, H, W = TRANSFORMER[tag]
    return fill_parameters(STTR.Transformer(C, E, L), parameter_seed(tag)).to(device)


@pytest.mark.parametrize("backend,tag", on([t for t in TRANSFORMER if t != "t17b"], TRANSFORMER_GPU_ONLY))
def test_transformer_matches_reference_fp64(backend, tag, gold, parity_log):
    """attn_weight, both feature gradients and every parameter gradient; `norm.*` receive none."""
    env = Env(backend)
    x = {k: v.to(env.device) for k, v in transformer_inputs(tag).items()}
    model = _model(tag, env.device)
    left, right = x["feat_left"].requires_grad_(), x["feat_right"].requires_grad_()
    with env.ctx():
        attn = model(left, right, x["pos"])
        (attn.masked_fill(attn == NINF, 0.0) * x["g_attn"]).sum().backward()
        sync(env)
    key = "transformer:" + tag
    got = {"attn_weight": attn, "g_feat_left": left.grad, "g_feat_right": right.grad}
    got.update({"g:" + n: p.grad for n, p in model.named_parameters()})
    assert got.pop("g:norm.weight") is None and got.pop("g:norm.bias") is None
    assert set(got) == {k for k, _ in transformer_layout(tag)}
    for k, shape in transformer_layout(tag):
        assert tuple(got[k].shape) == shape, k
        within_inf(got[k], *_want(gold, key, k), GRAD_FACTOR if k.startswith("g") else VALUE_FACTOR,
                    f"sttr transformer {tag} {k} [{backend}]", parity_log)


def test_batch_of_two_gives_each_samples_record(env, gold, parity_log):  # noqa: F811
    """N = 2 (where the reference's split at H fails): t17 and t17b -- one set of parameters, two feature pairs -- stacked give,
    per sample, those records' attn_weight and feature gradients within the same bounds."""
    tags = ("t17", "t17b")
    xs = [transformer_inputs(t) for t in tags]
    cat = {k: torch.cat([x[k] for x in xs], 0).to(env.device) for k in ("feat_left", "feat_right", "g_attn")}
    model = _model("t17", env.device)
    left, right = cat["feat_left"].requires_grad_(), cat["feat_right"].requires_grad_()
    with env.ctx():
        attn = model(left, right, xs[0]["pos"].to(env.device))
        (attn.masked_fill(attn == NINF, 0.0) * cat["g_attn"]).sum().backward()
        sync(env)
    for n, tag in enumerate(tags):
        for k, t, f in (("attn_weight", attn, VALUE_FACTOR), ("g_feat_left", left.grad, GRAD_FACTOR), ("g_feat_right", right.grad, GRAD_FACTOR)):
            within_inf(t[n:n + 1], *_want(gold, "transformer:" + tag, k), f, f"sttr transformer N=2 sample {n} {k} [{env.name}]", parity_log)


# ------------------------------------------------------------------------------------------ the op alone
def _op_inputs(W, B, E, seed, tables=True):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(W, B, E, 16, generator=g) * s for s in (0.5, 1.0, 1.0))
    q_r, k_r = (0.5 * torch.randn(2 * W - 1, E, 16, generator=g) for _ in range(2))
    return [q, k, v] + ([q_r, k_r] if tables else [None, None]), torch.randn(W, B, E, 16, generator=g), torch.randn(B, W, W, generator=g)


def _op_run(env, xs, g_o, g_raw, causal, need_raw=True):
    leaves = [None if t is None else t.to(env.device).requires_grad_() for t in xs]
    with env.ctx():
        o, raw, avg = ops.sttr_rel_attention(*leaves, causal, need_raw, False)
        loss = (o * g_o.to(env.device)).sum()
        if need_raw:
            loss = loss + (raw.masked_fill(raw == NINF, 0.0) * g_raw.to(env.device)).sum()
        loss.backward()
        sync(env)
    return [o, raw] + [None if t is None else t.grad for t in leaves]


@pytest.mark.parametrize("causal", [False, True])
def test_finite_difference_gradients(causal):
    """<gradient, direction> against the central difference for q, k, v, q_r and k_r (emulator, W = 9, two heads), through o and
    raw together."""
    from tests.emu_util import emu_product_path
    xs, g_o, g_raw = _op_inputs(9, 2, 2, 11)
    eps = 2e-3

    def loss_of(ts):
        o, raw, _ = ops.sttr_rel_attention(*ts, causal, True, False)
        return (o * g_o).sum() + (raw.masked_fill(raw == NINF, 0.0) * g_raw).sum()

    with emu_product_path():
        leaves = [t.clone().requires_grad_() for t in xs]
        loss_of(leaves).backward()
        g = torch.Generator().manual_seed(3)
        for n, name in enumerate(("q", "k", "v", "q_r", "k_r")):
            d = torch.randn(xs[n].shape, generator=g)
            an = (leaves[n].grad * d).double().sum().item()
            with torch.no_grad():
                up = loss_of([t + eps * d if m == n else t for m, t in enumerate(xs)]).double().item()
                dn = loss_of([t - eps * d if m == n else t for m, t in enumerate(xs)]).double().item()
            fd = (up - dn) / (2 * eps)
            assert abs(an - fd) <= 3e-2 * max(abs(an), abs(fd), 1e-3), (name, an, fd)


@pytest.mark.parametrize("backend,tag", on(["w17_cross", "w320_causal"], ["w320_causal"]))
def test_outputs_are_bitwise_reproducible(backend, tag):
    """Forward and backward twice on fresh outputs: o, raw, dq, dk, dv and the table gradients dQr, dKr bit for bit."""
    env = Env(backend)
    kind, C, E, W, B, causal, table = CORE[tag]
    xs, g_o, g_raw = _op_inputs(W, B, E, 5)
    a, b = _op_run(env, xs, g_o, g_raw, causal), _op_run(env, xs, g_o, g_raw, causal)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(t.abs().max().item() > 0 for t in a[2:])


def test_causal_rows(env):  # noqa: F811
    """Row 0 has a single finite entry; outputs and gradients are finite; a gradient of raw at masked positions -- NaN and
    huge values planted there -- never reaches a gradient."""
    W, B, E = 21, 2, 2
    xs, g_o, g_raw = _op_inputs(W, B, E, 9)
    clean = _op_run(env, xs, g_o, g_raw, True)
    o, raw = clean[0].cpu(), clean[1].cpu()
    upper = torch.triu(torch.ones(W, W, dtype=torch.bool), 1).expand(B, W, W)
    assert torch.equal(raw == NINF, upper) and torch.isfinite(raw[~upper]).all() and (torch.isfinite(raw[:, 0]).sum(-1) == 1).all()
    assert torch.isfinite(o).all() and all(torch.isfinite(t).all() for t in clean[2:])
    # row 0 attends to key 0 alone: o[0] = v[0]
    assert torch.allclose(o[0], xs[2][0], rtol=0, atol=1e-6)
    leaves = [t.to(env.device).requires_grad_() for t in xs]
    dirty = g_raw.clone()
    dirty[upper] = float("nan")
    dirty[:, 0, 1] = 1e30
    with env.ctx():
        o2, raw2, _ = ops.sttr_rel_attention(*leaves, True, True, False)
        torch.autograd.backward([o2, raw2], [g_o.to(env.device), dirty.to(env.device)])
        sync(env)
    assert all(torch.equal(t.grad, c) for t, c in zip(leaves, clean[2:]))


def test_position_encoding_is_the_reference_table():
    x = STTR.NestedTensor(torch.zeros(1, 3, 4, 17), None)
    assert torch.equal(STTR.PositionEncodingSine1DRelative(128)(x), sine_table(17, 128))
    x.sampled_cols = torch.arange(1, 17, 3).view(1, -1)                  # 6 of 17 columns: distances stretched by 17 / 6
    assert STTR.PositionEncodingSine1DRelative(32)(x).shape == (11, 32)
    assert STTR.no_pos_encoding(x) is None

    class Args:
        position_encoding, channel_dim, nheads, num_attn_layers = "sine1d_rel", 32, 2, 1
    assert isinstance(STTR.build_position_encoding(Args), STTR.PositionEncodingSine1DRelative)
    assert isinstance(STTR.build_transformer(Args), STTR.Transformer)


def test_state_dict_keys():
    want = json.load(open(os.path.join(HERE, "golden", "state_dict_keys_sttr_transformer.json")))
    a = STTR.Transformer(128, 8, 6)
    assert list(a.state_dict()) == want
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in transformer_parameters("t70")]
    b = STTR.Transformer(128, 8, 6)
    fill_parameters(a, 3)
    b.load_state_dict(a.state_dict(), strict=True)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


# ------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_are_refused():
    xs, _, _ = _op_inputs(9, 1, 2, 1)
    with pytest.raises(ops.StxError, match="ROCm device"):
        ops.sttr_rel_attention(*xs)
    with pytest.raises(ops.StxError, match="ROCm device"):
        STTR.MultiheadAttentionRelative(32, 2)(torch.zeros(9, 1, 32), torch.zeros(9, 1, 32), torch.zeros(9, 1, 32))


def test_unsupported_arguments_are_refused(env):  # noqa: F811
    dev = env.device
    q, k, v, q_r, k_r = (t.to(dev) for t in _op_inputs(9, 2, 2, 1)[0])
    with env.ctx():
        with pytest.raises(ops.StxError, match="float32"):
            ops.sttr_rel_attention(q.double(), k, v)
        with pytest.raises(ops.StxError, match="contiguous"):
            ops.sttr_rel_attention(q.transpose(1, 2).contiguous().transpose(1, 2), k, v)
        with pytest.raises(ops.StxError, match="head dim"):
            ops.sttr_rel_attention(*(torch.zeros(9, 2, 4, 8, device=dev) for _ in range(3)))
        with pytest.raises(ops.StxError, match="outside the supported 2.."):
            ops.sttr_rel_attention(*(torch.zeros(1, 1, 2, 16, device=dev) for _ in range(3)))
        with pytest.raises(ops.StxError, match="outside the supported 2.."):
            ops.sttr_rel_attention(*(torch.zeros(ops.STTR_MAX_W + 1, 1, 1, 16, device=dev) for _ in range(3)))
        with pytest.raises(ops.StxError, match="heads"):
            ops.sttr_rel_attention(*(torch.zeros(9, 1, 9, 16, device=dev) for _ in range(3)))
        with pytest.raises(ops.StxError, match="one shape"):
            ops.sttr_rel_attention(q, k[:8].contiguous(), v)
        with pytest.raises(ops.StxError, match="go together"):
            ops.sttr_rel_attention(q, k, v, None, k_r)
        with pytest.raises(ops.StxError, match="go together"):
            ops.sttr_rel_attention(q, k, v, q_r, None)
        with pytest.raises(ops.StxError, match=r"\[2W-1, E, 16\]"):
            ops.sttr_rel_attention(q, k, v, q_r[:-1].contiguous(), k_r[:-1].contiguous())
        with pytest.raises(ops.StxError, match="backward without a gradient"):
            leaf = q.clone().requires_grad_()
            avg = ops.sttr_rel_attention(leaf, k, v, q_r, k_r, False, True, True)
            ops.SttrRelAttentionFn.backward(avg[0].grad_fn, None, None, None)
        mha = STTR.MultiheadAttentionRelative(32, 2).to(dev)
        x = torch.zeros(9, 1, 32, device=dev)
        for mask in (torch.zeros(9, 9, device=dev), torch.tril(torch.full((9, 9), NINF, device=dev), -1), torch.zeros(8, 9, device=dev)):
            with pytest.raises(ops.StxError, match="attn_mask"):
                mha(x, x, x, attn_mask=mask)
        with pytest.raises(ops.StxError, match="pos_enc"):
            mha(x, x, x, pos_enc=torch.zeros(9, 32, device=dev))
        # the reference's own mask, built by hand, is accepted
        assert mha(x, x, x, attn_mask=torch.triu(torch.full((9, 9), NINF, device=dev), 1))[2].shape == (1, 9, 9)


def test_c_entry_points_refuse_without_launching(be):  # noqa: F811
    """The C-ABI returns an error -- and writes nothing -- for W = 1 and W past the limit, head dim 8, nine heads, a lone table,
    a backward without any gradient, a lone table gradient, zero chunks and a scratch that is too small."""
    W, B, E = 8, 1, 2
    q, k, v = (be.dev(torch.zeros(W, B, E, 16)) for _ in range(3))
    tab = be.dev(torch.zeros(2 * W - 1, E, 16))
    o, raw, dq, dk, dv = be.empty(W * B * E * 16), be.empty(B * W * W), be.empty(W * B * E * 16), be.empty(W * B * E * 16), be.empty(W * B * E * 16)
    stats, dqr, dkr = be.empty(2 * B * E * W), be.empty((2 * W - 1) * E * 16), be.empty((2 * W - 1) * E * 16)
    n = ops.sttr_attn_scratch_floats(W, B, E)
    scratch = be.empty(n)

    def fwd(W_=W, E_=E, hd=16, qr=tab, kr=tab):
        return ("stx_sttr_attn_fwd", (ptr(q), ptr(k), ptr(v), qr, kr, 1, ptr(o), ptr(raw), None, ptr(stats), W_, B, E_, hd))

    def bwd(dO=o, dRaw=raw, qr=tab, dqr_=dqr, nb=1, n_=n, W_=W, hd=16):
        return ("stx_sttr_attn_bwd", (dO, dRaw, ptr(q), ptr(k), ptr(v), qr, qr, ptr(o), ptr(stats), 1, ptr(dq), ptr(dk), ptr(dv), dqr_,
                                      ptr(dkr), ptr(scratch), n_, nb, W_, B, E, hd))
    bad = [fwd(W_=1), fwd(W_=432), fwd(hd=8), fwd(E_=9), fwd(qr=None), fwd(kr=None),
           bwd(dO=None, dRaw=None), bwd(dqr_=None), bwd(nb=0), bwd(nb=2), bwd(n_=n - 1), bwd(W_=432), bwd(hd=32)]
    for name, args in bad:
        with pytest.raises(ops.StxError):
            be.call(name, *args)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (o, raw, dq, dk, dv, stats, dqr, dkr, scratch))


# ------------------------------------------------------------------------------------------ the chain
def test_transformer_feeds_the_regression_head(env):  # noqa: F811
    """Features in -> disparity and occlusion out on the project's kernels: Transformer -> RegressionHead at W = 17."""
    tag = "t17"
    C, E, L, H, W = TRANSFORMER[tag]
    x = {k: v.to(env.device) for k, v in transformer_inputs(tag).items()}
    model, head = _model(tag, env.device), STTR.RegressionHead(None, ot=True).to(env.device)
    with env.ctx():
        attn = model(x["feat_left"], x["feat_right"], x["pos"])
        out = head(attn, STTR.NestedTensor(torch.zeros(1, 3, H, W, device=env.device), torch.zeros(1, 3, H, W, device=env.device)))
        (out["disp_pred"].sum() + out["occ_pred"].sum()).backward()
        sync(env)
    assert out["disp_pred"].shape == (1, H, W) and torch.isfinite(out["disp_pred"]).all() and torch.isfinite(out["occ_pred"]).all()
    g = model.self_attn_layers[0].self_attn.in_proj_weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
