"""FoundationStereo's disparity transformer (reference FoundationStereo/submodule.py `CostVolumeDisparityAttention`) on
csrc/disp_attention.hip: all layers in one launch, forward and backward, `ops.disp_attention` and the drop-in modules of
`models.FoundationStereo`.

Every product test runs on the host emulator build (CPU, `-m "not gpu"`) and on gfx950 (`-m gpu`):
  * state-dict keys, shapes and order equal the reference's (tests/golden/state_dict_keys_disp_attn.json); the plain-torch
    restatement is pinned to the fixture (`parity.pin_fixture`: fp64 to 1e-11, fp32 to 2 x d_ref, the floor where d_ref is 0);
  * the module against the reference's own fp64 run (tests/golden/disp_attn*.npz, written by make_golden_disp_attn.py), in
    train() with p = 0 and in eval() with the default p = 0.1: `parity.within_fixture`, 2 x d_ref on y, 3 x d_ref on every
    gradient;
  * the bits do not depend on the grid (switch STX_DA_GRID) nor on the layout the sequences arrive in;
  * the backward against finite differences, skipped gradients, reproducibility;
  * dropout: the masks against the numpy restatement of the documented counter layout, their statistics, seeds, and the
    product against the pinned restatement in fp64 evaluated with the product's own masks;
  * refusals and autocast;
  * on the GPU only: the model's own sequence count (2160 sequences of 26 x 28, four layers) against the restatement in fp64.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.backends import Backend
from tests.golden.disp_attn_config import (CASES, FULL, keep_masks, load_gold, module_args, param_names, restated, run_case,
                                           to_sequences, volume_inputs)
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, Env, directional, env, filled, on, pin_fixture, sync, within, within_fixture  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SEED_A, SEED_B = 0x1234_5678_9ABC_DEF0, -(2 ** 62) + 12345              # both key words in use; a negative seed


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def _module(shape, dropout=0.0):
    from stereo_toolbox_amd.models.FoundationStereo import CostVolumeDisparityAttention
    return filled(CostVolumeDisparityAttention, **module_args(shape, dropout))[0]


def _params(m):
    named = dict(m.named_parameters())
    return [named[n] for n in param_names(len(m.sa))]


def _seed(value, dev):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _op(dev, x, params, shape, p=0.0, seed=None, training=True, table=True):
    """ops.disp_attention on the [N, L, C] form; x and params may be CPU tensors (moved to dev)."""
    from stereo_toolbox_amd import ops
    from tests.golden.disp_attn_config import sinusoid
    B, C, heads, ff, layers, D, H, W = shape
    move = lambda t: t if t.device == dev else t.to(dev)                 # noqa: E731
    pe = sinusoid(x.shape[1], C, torch.float32).to(dev) if table else None
    return ops.disp_attention(move(x), pe, [move(t) for t in params], heads, p=p, seed=None if seed is None else _seed(seed, dev),
                              training=training)


def _step(env_, m, shape, seed=None):
    """One forward + backward of the module on the case's inputs -> [y, gx, parameter gradients...] on the CPU."""
    dev = env_.device
    m.zero_grad(set_to_none=True)
    with env_.ctx():
        if seed is not None:
            torch.manual_seed(seed)
        out = run_case(lambda cv: m(cv.to(dev)), dict(m.named_parameters()), shape, torch.float32)
        sync(env_)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


# ------------------------------------------------------------------------------------------ 1. state dict, restatement
def test_state_dict_matches_reference():
    want = json.load(open(os.path.join(HERE, "golden", "state_dict_keys_disp_attn.json")))["ragged"]
    m = _module(CASES["ragged"])
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == want
    assert "pos_embed0.pe" not in dict(m.named_buffers()) and tuple(m.pos_embed0.pe.shape) == (1, 32, 12)


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_is_pinned_to_the_fixture(tag, gold):
    shape = CASES[tag]
    for dtype in (torch.float64, torch.float32):
        m = _module(shape).to(dtype)
        out = run_case(lambda cv: restated(cv, _params(m), shape[2]), dict(m.named_parameters()), shape, dtype)
        for k, v in out.items():
            is64 = dtype == torch.float64
            pin_fixture(v if is64 else None, None if is64 else v, gold, f"{tag}/{k}", zero_dref="floor")


# ------------------------------------------------------------------------------------------ 2. module vs the fixture
@pytest.mark.parametrize("mode", ["train_p0", "eval_p01"])
@pytest.mark.parametrize("backend,tag", on(list(CASES)))
def test_module_matches_reference_fp64(backend, tag, mode, gold, parity_log):
    env_ = Env(backend)
    shape = CASES[tag]
    m = _module(shape, 0.0 if mode == "train_p0" else 0.1).to(env_.device)
    m.train(mode == "train_p0")
    out = _step(env_, m, shape)
    assert out["y"].dtype == torch.float32
    for k, v in out.items():
        assert v is not None, k
        within_fixture(v, gold, f"{tag}/{k}", VALUE_FACTOR if k == "y" else GRAD_FACTOR, f"disp_attention {tag} {mode} {k} [{backend}]",
                       parity_log)


def test_one_token_projection_gradients_sit_at_the_floor(env, gold):  # noqa: F811
    """One key: the soft-max is 1 whatever q and k are.  The reference's q_proj / k_proj gradients are exactly zero in fp32 and
    fp64 (d_ref = 0); the product's must be zero up to the floor of `parity.within`, not noise."""
    shape = CASES["one_token"]
    out = _step(env, _module(shape).to(env.device), shape)
    for i in range(shape[4]):
        for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias"):
            key = f"one_token/grad/sa.{i}.self_attn.{n}"
            assert float(gold[key + ":dref"]) == 0.0 and not gold[key + ":f64"].any()
            assert out[f"grad/sa.{i}.self_attn.{n}"].abs().max().item() <= 2e-7


# ------------------------------------------------------------------------------------------ 3. grid independence
@pytest.mark.parametrize("backend", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_bits_do_not_depend_on_the_grid(backend):
    """15 sequences: one workgroup walks four rounds with a partial last one; two and three workgroups leave idle waves."""
    be = Backend(backend)
    env_ = Env(backend)
    shape = CASES["model"]
    m = _module(shape, 0.1).to(env_.device).train()
    want = _step(env_, m, shape, seed=5)
    old = be.lib.set_tuning("STX_DA_GRID", 0)
    try:
        for grid in (1, 2, 3):
            be.lib.set_tuning("STX_DA_GRID", grid)
            got = _step(env_, m, shape, seed=5)
            for k in want:
                assert torch.equal(got[k], want[k]), (grid, k)
    finally:
        be.lib.set_tuning("STX_DA_GRID", old)


# ------------------------------------------------------------------------------------------ 4. layout
def test_layouts_give_equal_bits(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    shape = CASES["ragged"]
    B, C, heads, ff, layers, D, H, W = shape
    cv, _ = volume_inputs(shape)
    m = _module(shape).to(dev).eval()
    ps = [p.detach() for p in _params(m)]
    with env.ctx(), torch.no_grad():
        dense = ops.to_ndhwc(cv.to(dev))                                  # [B, D, H, W, C] dense
        y_view = m(ops.to_ncdhw(dense))
        y_ncdhw = m(cv.to(dev).contiguous())
        y_seq = _op(dev, to_sequences(cv).contiguous(), ps, shape, training=False)
        sync(env)
    assert y_view.shape == cv.shape and y_view.permute(0, 2, 3, 4, 1).is_contiguous()
    assert torch.equal(y_view, y_ncdhw)
    assert torch.equal(to_sequences(y_view.cpu()), y_seq.cpu())


def test_single_layer_class_is_the_op_with_one_layer(env):  # noqa: F811
    from stereo_toolbox_amd.models.FoundationStereo import FlashAttentionTransformerEncoderLayer
    dev = env.device
    shape = CASES["ragged"]
    B, C, heads, ff, layers, D, H, W = shape
    layer = filled(FlashAttentionTransformerEncoderLayer, C, heads, ff, dropout=0.0)[0].to(dev)
    x = to_sequences(volume_inputs(shape)[0]).contiguous()
    with env.ctx(), torch.no_grad():
        got = layer(x.to(dev))
        want = _op(dev, x, [p.detach() for p in layer.tensors()], shape, table=False)
        sync(env)
    assert torch.equal(got, want) and tuple(got.shape) == tuple(x.shape)


# ------------------------------------------------------------------------------------------ 5. backward
def _fd_inputs():
    shape = CASES["ragged"]
    m = _module(shape)
    return [to_sequences(volume_inputs(shape)[0]).contiguous()] + [p.detach().clone() for p in _params(m)]


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_backward_matches_finite_differences(env, p):  # noqa: F811
    """With p = 0.1 and a fixed seed the function is still smooth in every input: the check holds only if forward and backward
    of one call draw the same masks.  k_proj.bias stays fixed: it adds one constant to every score of a row, the soft-max does
    not see it, its gradient is zero and a finite difference of it is rounding noise (the fixture tests cover that gradient)."""
    dev = env.device
    shape = CASES["ragged"]
    base = _fd_inputs()
    fixed = {i for i in range(1, len(base)) if (i - 1) % 16 == 3}
    free = [i for i in range(len(base)) if i not in fixed]

    def fn(*moved):
        ts = list(base)
        for i, t in zip(free, moved):
            ts[i] = t
        return _op(dev, ts[0], ts[1:], shape, p=p, seed=SEED_A if p else None).cpu()
    with env.ctx():                                          # (the backward pass runs inside `directional`)
        directional(fn, [base[i] for i in free])


def test_skipped_gradients_leave_the_others_unchanged(env):  # noqa: F811
    dev = env.device
    shape = CASES["ragged"]
    base = _fd_inputs()
    g = to_sequences(volume_inputs(shape)[1]).contiguous().to(dev)
    n = len(base)

    def run(wanted):
        ts = [t.clone().to(dev).requires_grad_(i in wanted) for i, t in enumerate(base)]
        with env.ctx():
            (_op(dev, ts[0], ts[1:], shape, p=0.1, seed=SEED_B) * g).sum().backward()
            sync(env)
        return [None if t.grad is None else t.grad.cpu() for t in ts]
    full = run(set(range(n)))
    assert all(t is not None for t in full)
    norms = {1 + 16 * layer + i for layer in range(shape[4]) for i in (12, 13, 14, 15)}
    for wanted in (set(range(1, n)), set(range(n)) - set(range(1, 17)), norms, {0}, {1 + 16 + 8}):
        part = run(wanted)                                   # no g_x; sa.0 frozen; only the LayerNorms; g_x alone; one weight of sa.1
        for i, (a, b) in enumerate(zip(part, full)):
            assert (a is not None) == (i in wanted), i
            if a is not None:
                assert torch.equal(a, b), (sorted(wanted)[:4], i)


def test_two_runs_give_equal_bits(env):  # noqa: F811
    shape = CASES["ragged"]
    m = _module(shape, 0.1).to(env.device).train()
    a, b = _step(env, m, shape, seed=9), _step(env, m, shape, seed=9)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------ 6. dropout
def _masks(env_, seed, p, shape, N):
    from stereo_toolbox_amd import ops
    B, C, heads, ff, layers, D, H, W = shape
    with env_.ctx():
        got = ops.disp_attention_masks(_seed(seed, env_.device), p, N, D, C, ff, layers)
        sync(env_)
    return got.cpu()


@pytest.mark.parametrize("tag", ["model", "ragged"])
def test_masks_equal_the_documented_counter_layout(env, tag):  # noqa: F811
    shape = CASES[tag]
    B, C, heads, ff, layers, D, H, W = shape
    N = B * H * W
    for seed, p in ((SEED_A, 0.1), (SEED_B, 0.5), (7, 0.1)):
        got = _masks(env, seed, p, shape, N)
        want = keep_masks(seed, p, N, D, C, ff, layers)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.numpy(), want), (seed, p)
    assert bool(_masks(env, SEED_A, 0.0, shape, N).all())                # p = 0: everything is kept


def test_mask_statistics(env):  # noqa: F811
    shape = CASES["model"]
    B, C, heads, ff, layers, D, H, W = shape
    masks = _masks(env, SEED_A, 0.1, shape, B * H * W).numpy()
    n = masks.size
    assert abs(masks.mean() - 0.9) <= 5 * math.sqrt(0.09 / n), (masks.mean(), n)
    flat = masks.reshape(layers * 3, -1)
    for i in range(len(flat)):
        for j in range(i):
            assert not np.array_equal(flat[i], flat[j]), (i, j)


def test_seeds(env):  # noqa: F811
    dev = env.device
    shape = CASES["ragged"]
    base = _fd_inputs()

    def run(seed):
        with env.ctx():
            y = _op(dev, base[0], base[1:], shape, p=0.1, seed=seed)
            sync(env)
        return y.cpu()
    a, b, c = run(SEED_A), run(SEED_A), run(SEED_B)
    assert torch.equal(a, b) and not torch.equal(a, c)
    m = _module(shape, 0.1).to(dev).train()
    one, two = _step(env, m, shape, seed=3), _step(env, m, shape, seed=3)
    assert all(torch.equal(one[k], two[k]) for k in one)
    cv = volume_inputs(shape)[0].to(dev)
    with env.ctx(), torch.no_grad():
        torch.manual_seed(3)
        first, second = m(cv), m(cv)                         # two consecutive calls draw two seeds
        sync(env)
    assert torch.equal(first.cpu(), one["y"]) and not torch.equal(first, second)


@pytest.mark.parametrize("backend,tag", on(["model", "ragged"]))
def test_dropout_matches_the_restatement_with_the_products_masks(backend, tag, parity_log):
    """y and all gradients against the pinned restatement evaluated in fp64 WITH THE PRODUCT'S OWN MASKS and the 1 / (1 - p)
    scale; d_ref is the restatement's own fp32 CPU run with the same masks."""
    from stereo_toolbox_amd import ops
    env_ = Env(backend)
    dev = env_.device
    shape = CASES[tag]
    B, C, heads, ff, layers, D, H, W = shape
    p = 0.1
    m = _module(shape, p).to(dev).train()
    got = _step(env_, m, shape, seed=11)
    torch.manual_seed(11)                                                 # the seed the module drew, drawn again
    with env_.ctx():
        seed = torch.randint(-2 ** 62, 2 ** 62, (1,), dtype=torch.int64, device=dev)
        masks = ops.disp_attention_masks(seed, p, B * H * W, D, C, ff, layers).cpu()
        sync(env_)
    assert np.array_equal(masks.numpy(), keep_masks(int(seed.item()), p, B * H * W, D, C, ff, layers))
    runs = []
    for dtype in (torch.float64, torch.float32):
        md = _module(shape, p).to(dtype)
        scale = float(np.float32(1.0 / (1.0 - float(np.float32(p)))))
        runs.append(run_case(lambda cv: restated(cv, _params(md), heads, masks=masks, scale=scale), dict(md.named_parameters()), shape,
                             dtype))
    r64, r32 = runs
    for k in r64:
        dref = (r32[k].double() - r64[k]).abs().max().item()
        within(got[k], r64[k], dref, VALUE_FACTOR if k == "y" else GRAD_FACTOR, f"disp_attention dropout {tag} {k} [{backend}]", parity_log)


# ------------------------------------------------------------------------------------------ 7. refusals, autocast
def test_refusals_without_a_device():
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models.FoundationStereo import (CostVolumeDisparityAttention, FlashAttentionTransformerEncoderLayer,
                                                            FlashMultiheadAttention)
    import torch.nn as nn
    shape = CASES["ragged"]
    cv, _ = volume_inputs(shape)
    with pytest.raises(ops.StxError):                       # CPU tensors on the product path
        _module(shape)(cv)
    with pytest.raises(ops.StxError):
        filled(FlashAttentionTransformerEncoderLayer, 12, 3, 20)[0](to_sequences(cv).contiguous())
    with pytest.raises(ops.StxError, match="FlashAttentionTransformerEncoderLayer"):
        FlashMultiheadAttention(12, 3)(cv, cv, cv)
    for kw in (dict(d_model=30, nhead=5, dim_feedforward=28), dict(d_model=36, nhead=4, dim_feedforward=28),     # C = 30; head dim 9
               dict(d_model=28, nhead=4, dim_feedforward=36), dict(d_model=28, nhead=2, dim_feedforward=28),     # ff = 36; head dim 14
               dict(d_model=28, nhead=4, dim_feedforward=28, act=nn.ReLU), dict(d_model=28, nhead=4, dim_feedforward=28, num_transformer=9)):
        with pytest.raises(ops.StxError):
            CostVolumeDisparityAttention(**kw)
    with pytest.raises(ops.StxError):
        FlashAttentionTransformerEncoderLayer(28, 4, 28, norm=nn.BatchNorm1d)
    assert CostVolumeDisparityAttention(28, 4, 28, norm_first=True, num_transformer=1) is not None   # accepted and ignored


def test_shape_refusals(env):  # noqa: F811
    from stereo_toolbox_amd import ops
    dev = env.device
    with env.ctx():
        m = _module((1, 28, 4, 28, 1, 1, 1, 1)).to(dev)
        assert m(torch.zeros(1, 28, 32, 1, 2, device=dev)).shape == (1, 28, 32, 1, 2)          # the edge that is served
        with pytest.raises(ops.StxError):
            m(torch.zeros(1, 28, 33, 1, 2, device=dev))                                         # L = 33
        with pytest.raises(ops.StxError):
            m(torch.zeros(1, 28, 4, 1, 2, device=dev), window_size=(3, 3))
        with pytest.raises(ops.StxError):
            m(torch.zeros(1, 28, 4, 1, 2, device=dev, dtype=torch.float16))                     # fp16 outside autocast
        with pytest.raises(ops.StxError):
            m(torch.zeros(1, 24, 4, 1, 2, device=dev))                                          # not the module's width
        ps = [p.detach() for p in _params(m)]
        with pytest.raises(ops.StxError):                                                       # training with p > 0 and no seed
            ops.disp_attention(torch.zeros(2, 4, 28, device=dev), None, ps, 4, p=0.1, seed=None, training=True)
        with pytest.raises(ops.StxError):                                                       # head dim 14
            ops.disp_attention(torch.zeros(2, 4, 28, device=dev), None, ps, 2)
        sup = ops.get_lib().raw("stx_disp_attention_supported")
        assert sup(32, 32, 4, 32, 8) == 1 and sup(1, 4, 1, 4, 1) == 1 and sup(26, 28, 4, 28, 4) == 1
        assert sup(33, 32, 4, 32, 8) == 0 and sup(0, 32, 4, 32, 8) == 0                         # L
        assert sup(32, 36, 6, 32, 8) == 0 and sup(32, 30, 5, 32, 8) == 0 and sup(32, 0, 1, 32, 8) == 0     # C
        assert sup(32, 32, 2, 32, 8) == 0 and sup(32, 32, 3, 32, 8) == 0 and sup(32, 8, 1, 32, 8) == 1 and sup(32, 12, 1, 32, 8) == 0
        assert sup(32, 32, 4, 36, 8) == 0 and sup(32, 32, 4, 30, 8) == 0 and sup(32, 32, 4, 4, 8) == 1     # feed-forward
        assert sup(32, 32, 4, 32, 9) == 0 and sup(32, 32, 4, 32, 0) == 0                        # layers
        ws = ops.get_lib().raw("stx_disp_attention_bwd_workspace_floats")
        assert ws(15, 26, 28, 28) == 4 * 4984 and ws(15, 33, 28, 28) == 0 and ws(15, 26, 30, 28) == 0


def test_autocast_is_the_fp32_path_on_the_cast_up_inputs(env):  # noqa: F811
    dev = env.device
    low = torch.float16 if dev.type == "cuda" else torch.bfloat16
    shape = CASES["ragged"]
    cv = volume_inputs(shape)[0].to(dev).to(low)
    m = _module(shape).to(dev).eval()
    with env.ctx():
        with torch.amp.autocast(dev.type, dtype=low):
            leaf = cv.clone().requires_grad_()
            under = m(leaf)
            under.sum().backward()
        with torch.no_grad():
            plain = m(cv.float())
        sync(env)
    assert under.dtype == torch.float32 and leaf.grad.dtype == low
    assert torch.equal(under.detach(), plain)


# ------------------------------------------------------------------------------------------ 8. the model's sequence count
@pytest.mark.gpu
def test_full_sequence_count_matches_the_restatement(parity_log):
    env_ = Env("hip")
    m = _module(FULL).to(env_.device).train()
    a, b = _step(env_, m, FULL), _step(env_, m, FULL)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    runs = []
    for dtype in (torch.float64, torch.float32):
        md = _module(FULL).to(dtype)
        runs.append(run_case(lambda cv: restated(cv, _params(md), FULL[2]), {}, FULL, dtype))
    for k in ("y", "gx"):
        dref = (runs[1][k].double() - runs[0][k]).abs().max().item()
        within(a[k], runs[0][k], dref, VALUE_FACTOR if k == "y" else GRAD_FACTOR, f"disp_attention full {k} [hip]", parity_log)
