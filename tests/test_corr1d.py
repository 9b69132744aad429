"""RAFT-family 1-D correlation pyramid and lookup (`CorrBlock1D` / `CorrBlockFast1D` / `PytorchAlternateCorrBlock1D`, reference
models/RAFTStereo/corr.py:31-156, and the disparity-indexed `CorrBlock1D` of models/DEFOMStereo/corr.py:113-181) on the kernels of
csrc/corr1d.hip.

* tests/golden/corr1d.npz holds what the reference's OWN classes give on the seeded cases of tests/golden/corr1d_config.py, in
  fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| (tests/golden/make_golden_corr1d.py).  The larger cases keep d_ref,
  max|fp64| and a strided subsample of the fp64 tensor.
* A plain-torch restatement of the two files in gather form (no grid_sample) lives in this file and is pinned to the fixture on
  the CPU first -- in fp64 to 1e-11 (whole tensors or the subsample), in fp32 to 2 x d_ref (two fp32 evaluations of one
  quantity) -- so the fixture and the restatement check each other.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture -- for the larger cases with the
  restatement evaluated in fp64 at test time: values within 2 x d_ref, gradients within GRAD_FACTOR (3) x d_ref; where d_ref is
  zero the floor 2e-7 * max(1, max|want|) applies.  Every element of every tensor of every case is compared.
* Tolerances against the restatement where no fixture exists (kernel-level calls on a pyramid that is given): a sample is
  (1 - f) a + f b on positions both sides hold exactly (coords * 2^-i) -- a handful of fp32 roundings on quantities of the
  tensor's scale, bounded here by 8 * 2^-24 of the tensor's max; a gradient of the feature maps is a dot product over n terms:
  n * 2^-24 of the result's scale.
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.backends import be, ptr  # noqa: F401
from tests.golden.corr1d_config import (ALL_CASES, CASES, DEFOM_SCALE_RADIUS, DEFOM_SCALES, GPU_ONLY_CASES, ITER_CALLS, ITER_CASE,
                                        SHAPE_CASES, SUBSAMPLE, columns, inputs, iter_inputs, out_channels, subsample)
from tests.parity import (EPS, GRAD_FACTOR, VALUE_FACTOR, Env, env, near, on, pin_fixture, pin_subsample, sync, within,  # noqa: F401
                          within_fixture)
from tests.restated import _pack, corr1d_pyramid as pyramid, pool, sample

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corr1d.npz")
ITER = f"iter{ITER_CALLS}"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------------------------------ the restatement (plain torch)
def raft_lookup(cp, coords, radius):
    B, _, H, W = coords.shape
    dx = torch.arange(-radius, radius + 1, dtype=coords.dtype)
    x = coords[:, 0].reshape(B, H, W, 1)
    out = [sample(c, x / 2 ** i + dx) for i, c in enumerate(cp)]
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def defom_lookup(cp, cols, disp, radius, scaling):
    B, _, H, W = disp.shape
    c, d = cols.reshape(B, H, W, 1), disp.reshape(B, H, W, 1)
    if scaling:
        sdx = torch.arange(-DEFOM_SCALE_RADIUS, DEFOM_SCALE_RADIUS + 1, dtype=disp.dtype)
        out = [sample(cp[0], sdx + c - s * d) for s in DEFOM_SCALES]
    else:
        dx = torch.arange(-radius, radius + 1, dtype=disp.dtype)
        out = [sample(r, dx + (c - d) / 2 ** i) for i, r in enumerate(cp)]
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous()


def _restated(tag, dtype):
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    f1, f2, pos, gws = inputs(tag)
    f1, f2 = (t.to(dtype).requires_grad_() for t in (f1, f2))
    cp = pyramid(f1, f2, L)
    if kind == "raft":
        outs = [raft_lookup(cp, p.to(dtype), r) for p in pos]
    else:
        cols = columns(tag).to(dtype)
        outs = [defom_lookup(cp, cols, pos[0].to(dtype), r, False), defom_lookup(cp, cols, pos[1].to(dtype), r, True)]
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws)).backward()
    return {"out_a": outs[0].detach(), "out_b": outs[1].detach(), "corr": cp[0].detach().unsqueeze(3), "g_fmap1": f1.grad,
            "g_fmap2": f2.grad}


@functools.lru_cache(maxsize=2)
def _restated64(tag):
    return _restated(tag, torch.float64)


@functools.lru_cache(maxsize=1)
def _restated_iterations():
    """ITER_CALLS lookups plus the weighted sum of every pyramid level, fp64."""
    kind, B, Cf, H, W1, W2, L, r = CASES[ITER_CASE]
    f1, f2, coords, gws, wc = iter_inputs()
    f1, f2 = (t.double().requires_grad_() for t in (f1, f2))
    cp = pyramid(f1, f2, L)
    outs = [raft_lookup(cp, c.double(), r) for c in coords]
    loss = sum((o * g.double()).sum() for o, g in zip(outs, gws)) + sum((c * w.double()).sum() for c, w in zip(cp, wc))
    loss.backward()
    return {"outs": torch.stack(outs).detach(), "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def _pinned(r64, gold, tag):
    """The fp64 restatement against the stored subsample of the reference's fp64 tensors."""
    for k, v in r64.items():
        pin_subsample(v, torch.from_numpy(gold[f"{tag}:{k}:sub"]), float(gold[f"{tag}:{k}:max"]), subsample, min(v.numel(), SUBSAMPLE),
                      f"{tag}:{k}")


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated(tag, torch.float64), _restated(tag, torch.float32)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"{tag}:{k}")


@pytest.mark.parametrize("tag", list(SHAPE_CASES))
def test_restatement_matches_reference_subsample(gold, tag):
    _pinned(_restated64(tag), gold, tag)


def test_iteration_restatement_matches_reference_subsample(gold):
    _pinned(_restated_iterations(), gold, ITER)


# ------------------------------------------------------------------------------------------ the product vs fp64
def _block(tag, f1, f2, cls=None):
    kind, B, Cf, H, W1, W2, L, r = ALL_CASES[tag]
    if kind == "raft":
        from stereo_toolbox_amd.models import RAFTStereo
        return (cls or RAFTStereo.CorrBlock1D)(f1, f2, num_levels=L, radius=r)
    from stereo_toolbox_amd.models.DEFOMStereo import CorrBlock1D
    return CorrBlock1D(f1, f2, columns(tag).to(f1.device), num_levels=L, radius=r, scale_list=list(DEFOM_SCALES),
                       scale_corr_radius=DEFOM_SCALE_RADIUS)


def _product_case(env, tag, cls=None, needs=(True, True), prepare=None, backward=True, retain=False):
    """Two calls on one object (a DEFOM case: without, then with `scaling`), the two losses summed -> (outs, grads, leaves)."""
    kind = ALL_CASES[tag][0]
    f1, f2, pos, gws = inputs(tag)
    dev = env.device
    leaves = [t.to(dev).requires_grad_(n) for t, n in zip((f1, f2), needs)]
    a1, a2 = prepare(*leaves) if prepare else leaves
    with env.ctx():
        fn = _block(tag, a1, a2, cls)
        if kind == "raft":
            outs = [fn(p.to(dev)) for p in pos]
        else:
            outs = [fn(pos[0].to(dev)), fn(pos[1].to(dev), scaling=True)]
        loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, gws))
        if backward:
            loss.backward(retain_graph=retain)
            sync(env)
    return outs, {"g_fmap1": leaves[0].grad, "g_fmap2": leaves[1].grad}, (leaves, loss, fn)


def _static_corr(env, tag):
    from stereo_toolbox_amd.models import DEFOMStereo, RAFTStereo
    f1, f2, _, _ = inputs(tag)
    cls = RAFTStereo.CorrBlock1D if ALL_CASES[tag][0] == "raft" else DEFOMStereo.CorrBlock1D
    with env.ctx():
        return cls.corr(f1.to(env.device), f2.to(env.device))


@pytest.mark.parametrize("tag", list(CASES))
def test_lookup_matches_reference_fp64(env, gold, tag):
    kind, B, Cf, H, W1, W2, L, r = CASES[tag]
    outs, grads, _ = _product_case(env, tag)
    for i, k in ((0, "out_a"), (1, "out_b")):
        n = out_channels(tag, scaling=(kind == "defom" and i == 1))
        assert outs[i].shape == (B, n, H, W1) and outs[i].dtype == torch.float32 and outs[i].is_contiguous()
        within_fixture(outs[i], gold, f"{tag}:{k}", VALUE_FACTOR, f"{tag} {k}")
    for k, g in grads.items():
        within_fixture(g, gold, f"{tag}:{k}", GRAD_FACTOR, f"{tag} {k}")
    corr = _static_corr(env, tag)
    assert corr.shape == (B, H, W1, 1, W2) and corr.dtype == torch.float32 and corr.is_contiguous()
    within_fixture(corr, gold, f"{tag}:corr", VALUE_FACTOR, f"{tag} corr")


@pytest.mark.parametrize("backend,tag", on(SHAPE_CASES, GPU_ONLY_CASES))
def test_shape_case_matches_fp64_restatement(backend, tag, gold):
    """The branching shapes (corr1d_config.py says which case reaches what) and, on the GPU, the production shape: every
    element against the restatement in fp64 (pinned to the reference's subsample above), d_ref the reference's stored number."""
    env = Env(backend)
    kind, B, Cf, H, W1, W2, L, r = SHAPE_CASES[tag]
    want = _restated64(tag)
    outs, grads, _ = _product_case(env, tag)
    for i, k in ((0, "out_a"), (1, "out_b")):
        assert outs[i].shape == (B, out_channels(tag), H, W1) and outs[i].dtype == torch.float32 and outs[i].is_contiguous()
        within(outs[i], want[k], float(gold[f"{tag}:{k}:dref"]), VALUE_FACTOR, f"{tag}:{k}")
    for k, g in grads.items():
        within(g, want[k], float(gold[f"{tag}:{k}:dref"]), GRAD_FACTOR, f"{tag}:{k}")
    within(_static_corr(env, tag), want["corr"], float(gold[f"{tag}:corr:dref"]), VALUE_FACTOR, f"{tag}:corr")


# ------------------------------------------------------------------------------------------ behaviour
def test_fast_and_alternate_blocks_are_the_same_object(env):
    from stereo_toolbox_amd.models.RAFTStereo import CorrBlock1D, CorrBlockFast1D, PytorchAlternateCorrBlock1D
    tag = "raft_l4_r4"
    want, want_g, _ = _product_case(env, tag, CorrBlock1D)
    for cls in (CorrBlockFast1D, PytorchAlternateCorrBlock1D):
        outs, grads, _ = _product_case(env, tag, cls)
        assert all(torch.equal(a, b) for a, b in zip(outs, want))
        assert all(torch.equal(grads[k], want_g[k]) for k in grads)
    f1, f2, pos, _ = inputs(tag)
    with env.ctx():
        assert torch.equal(CorrBlockFast1D.corr(f1.to(env.device), f2.to(env.device)), CorrBlock1D.corr(f1.to(env.device), f2.to(env.device)))
    # the alternate block reads the row index the model passes in channel 1: a single-channel coords is refused
    from stereo_toolbox_amd import ops
    with env.ctx():
        fn = PytorchAlternateCorrBlock1D(f1.to(env.device), f2.to(env.device))
        with pytest.raises(ops.StxError, match="row"):
            fn(pos[0][:, :1].to(env.device))
        one = CorrBlock1D(f1.to(env.device), f2.to(env.device))(pos[0][:, :1].to(env.device))
    assert torch.equal(one, want[0].detach())


@pytest.mark.parametrize("tag", ["raft_l4_r4", "defom"])
def test_two_runs_give_the_same_bits(env, tag):
    a_out, a_grad, _ = _product_case(env, tag)
    b_out, b_grad, _ = _product_case(env, tag)
    assert all(torch.equal(a, b) for a, b in zip(a_out, b_out))
    for k in a_grad:
        assert torch.equal(a_grad[k], b_grad[k]) and a_grad[k].abs().max().item() > 0, k


def _iterations(env, retain=False):
    """ITER_CALLS lookups on one object and a weighted sum of the PUBLIC pyramid tensor (another consumer of it)."""
    from stereo_toolbox_amd.models.RAFTStereo import CorrBlock1D
    kind, B, Cf, H, W1, W2, L, r = CASES[ITER_CASE]
    f1, f2, coords, gws, wc = iter_inputs()
    dev = env.device
    f1, f2 = f1.to(dev).requires_grad_(), f2.to(dev).requires_grad_()
    with env.ctx():
        fn = CorrBlock1D(f1, f2, num_levels=L, radius=r)
        outs = [fn(c.to(dev)) for c in coords]
        loss = sum((o * g.to(dev)).sum() for o, g in zip(outs, gws)) + (fn.corr_pyramid * _pack(wc).to(dev)).sum()
        loss.backward(retain_graph=retain)
        sync(env)
    return outs, (f1, f2), loss


def test_32_lookups_and_another_consumer_of_the_pyramid(env, gold):
    """A validation pass's 32 lookups with distinct positions, losses summed, plus a weighted sum of `fn.corr_pyramid`: every
    output and both gradients against the fp64 restatement of the same loss (d_ref from the reference's run of it) -- the
    shared gradient buffer must reach the build node complete and be summed with the other consumer's gradient there."""
    want = _restated_iterations()
    outs, (f1, f2), _ = _iterations(env)
    within(torch.stack(outs), want["outs"], float(gold[f"{ITER}:outs:dref"]), VALUE_FACTOR, f"{ITER}:outs")
    within(f1.grad, want["g_fmap1"], float(gold[f"{ITER}:g_fmap1:dref"]), GRAD_FACTOR, f"{ITER}:g_fmap1")
    within(f2.grad, want["g_fmap2"], float(gold[f"{ITER}:g_fmap2:dref"]), GRAD_FACTOR, f"{ITER}:g_fmap2")


def test_second_backward_on_a_retained_graph_equals_the_first(env):
    _, leaves, loss = _iterations(env, retain=True)
    first = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    with env.ctx():
        loss.backward()
        sync(env)
    assert all(torch.equal(a, t.grad) and a.abs().max().item() > 0 for a, t in zip(first, leaves))


@pytest.mark.parametrize("needs", [(True, False), (False, True)])
def test_only_one_feature_map_requires_grad(env, needs):
    _, full, _ = _product_case(env, "raft_b2_l3_r2")
    _, part, _ = _product_case(env, "raft_b2_l3_r2", needs=needs)
    for (k, g), n in zip(part.items(), needs):
        assert (g is not None) == n, k
        assert g is None or torch.equal(g, full[k]), k


def test_fp16_feature_maps_under_autocast_are_their_fp32_casts(env):
    low = torch.float16
    device_type = "cuda" if env.name == "hip" else "cpu"
    a_out, a_grad, _ = _product_case(env, "raft_b2_l3_r2", prepare=lambda f1, f2: (f1.to(low).float(), f2.to(low).float()))
    with torch.autocast(device_type, dtype=low):
        b_out, b_grad, _ = _product_case(env, "raft_b2_l3_r2", prepare=lambda f1, f2: (f1.to(low), f2.to(low)))
    for a, b in zip(a_out, b_out):
        assert b.dtype == torch.float32 and torch.equal(a, b)
    for k in a_grad:                                                     # the cast's backward rounds the fp32 gradient to fp16
        assert torch.equal(a_grad[k].to(low).float(), b_grad[k]), k


def test_channels_last_feature_maps_are_taken_as_their_dense_copies(env):
    """Cf = 8 and H * W1 = 36 are multiples of 4: the transpose kernel of ops.channel_major serves fmap1 (fmap2, H * W2 = 42,
    goes through torch's copy)."""
    cl = lambda f1, f2: (f1.contiguous(memory_format=torch.channels_last), f2.contiguous(memory_format=torch.channels_last))  # noqa: E731
    a_out, a_grad, _ = _product_case(env, "raft_b2_l3_r2")
    b_out, b_grad, _ = _product_case(env, "raft_b2_l3_r2", prepare=cl)
    assert all(torch.equal(a, b) for a, b in zip(a_out, b_out))
    assert all(torch.equal(a_grad[k], b_grad[k]) for k in a_grad)


def test_unsupported_arguments_are_refused(env):
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models import DEFOMStereo, RAFTStereo
    tag = "raft_l4_r4"
    kind, B, Cf, H, W1, W2, L, r = CASES[tag]
    f1, f2, pos, _ = inputs(tag)
    dev = env.device
    f1, f2, coords = f1.to(dev), f2.to(dev), pos[0].to(dev)
    with env.ctx():
        fn = RAFTStereo.CorrBlock1D(f1.clone().requires_grad_(), f2)
        with pytest.raises(ops.StxError, match="detach"):
            fn(coords.clone().requires_grad_())
        assert fn(coords.clone().requires_grad_().detach()).shape == (B, out_channels(tag), H, W1)
        with pytest.raises(ops.StxError):
            RAFTStereo.CorrBlock1D(f1, f2, num_levels=5)
        with pytest.raises(ops.StxError, match="radius"):
            RAFTStereo.CorrBlock1D(f1, f2, radius=9)(coords)
        with pytest.raises(ops.StxError, match="shorter than 2"):
            RAFTStereo.CorrBlock1D(f1[..., :7], f2[..., :7].contiguous(), num_levels=4)          # 7 -> 3 -> 1
        cols = columns(tag).to(dev)
        nine = DEFOMStereo.CorrBlock1D(f1, f2, cols, num_levels=2, scale_list=[0.5 + 0.1 * i for i in range(9)], scale_corr_radius=2)
        disp = torch.zeros(B, 1, H, W1, device=dev)
        assert nine(disp).shape == (B, 2 * 9, H, W1)
        with pytest.raises(ops.StxError, match="jobs"):
            nine(disp, scaling=True)
        with pytest.raises(ops.StxError, match="detach"):
            nine(disp.clone().requires_grad_())
        with pytest.raises(ops.StxError, match="detach"):
            DEFOMStereo.CorrBlock1D(f1, f2, cols.clone().requires_grad_())


# ------------------------------------------------------------------------------------------ kernel level (C-ABI)
def _jobs(rows):
    flat = [float(v) for row in rows for v in row]
    return (ctypes.c_float * len(flat))(*flat), len(rows)


def test_kernel_level_pyramid_and_lookup_at_wide(be, gold):  # noqa: F811
    """stx_corr1d_pyramid_fwd/_bwd and stx_corr1d_lookup_fwd/_bwd through the C-ABI at `wide`: all four waves, the second w2
    round, ragged tiles, four levels with an odd tail at level 2, two channel rounds and >= 5 trips of both backward sums."""
    from stereo_toolbox_amd.utils import synthetic_tensor
    tag = "wide"
    kind, B, Cf, H, W1, W2, L, r = SHAPE_CASES[tag]
    f1, f2, pos, gws = inputs(tag)
    scale = 1.0 / math.sqrt(Cf)
    cp = pyramid(f1, f2, L)
    n_c = sum(c.numel() for c in cp)
    assert be.raw("stx_corr1d_pyramid_floats")(B * H * W1, W2, L) == n_c
    assert be.raw("stx_corr1d_pyramid_floats")(B * H * W1, W2, 5) == 0
    # level 0 every element against the fp64 restatement, pooled levels = pool(level 0) exactly
    cpyr = be.empty(n_c)
    be.call("stx_corr1d_pyramid_fwd", ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(cpyr), B, Cf, H, W1, W2, L, scale)
    lv = [cpyr.cpu()[:cp[0].numel()].view(B, H, W1, W2)]
    within(lv[0].unsqueeze(3), _restated64(tag)["corr"], float(gold[f"{tag}:corr:dref"]), VALUE_FACTOR, f"{tag}:corr")
    for _ in range(L - 1):
        lv.append(pool(lv[-1]))
    assert [t.shape[-1] for t in lv] == [301, 150, 75, 37]
    assert torch.equal(cpyr.cpu(), _pack(lv))
    # backward on a seeded gradient of EVERY pyramid element, against autograd of the restatement
    gc = synthetic_tensor((n_c,), 2912)
    f164, f264 = f1.double().requires_grad_(), f2.double().requires_grad_()
    (_pack(pyramid(f164, f264, L)) * gc.double()).sum().backward()
    gf1, gf2 = be.empty(B, Cf, H, W1), be.empty(B, Cf, H, W2)
    be.call("stx_corr1d_pyramid_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(gf1), ptr(gf2), B, Cf, H, W1, W2, L, scale)
    near(gf1, f164.grad, W2 * EPS, "pyramid backward fmap1")
    near(gf2, f264.grad, W1 * EPS, "pyramid backward fmap2")
    only1, only2 = be.empty(B, Cf, H, W1), be.empty(B, Cf, H, W2)
    be.call("stx_corr1d_pyramid_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(only1), None, B, Cf, H, W1, W2, L, scale)
    be.call("stx_corr1d_pyramid_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), None, ptr(only2), B, Cf, H, W1, W2, L, scale)
    assert torch.equal(only1, gf1) and torch.equal(only2, gf2)
    # lookup forward / backward on the pyramid packed from the restatement; the backward ADDS (twice -> twice the gradient)
    jobs, nj = _jobs([(i, r, 0.0, 2.0 ** -i) for i in range(L)])
    base = pos[0][:, 0].contiguous()
    out = be.empty(B, out_channels(tag), H, W1)
    be.call("stx_corr1d_lookup_fwd", ptr(be.dev(_pack(cp))), ptr(be.dev(base)), None, jobs, nj, ptr(out), B, H, W1, W2, L)
    cp64 = [c.double().requires_grad_() for c in cp]
    o64 = raft_lookup(cp64, pos[0].double(), r)
    o64.backward(gws[0].double())
    near(out, o64, 8 * EPS, "lookup forward")
    gcp = be.empty(n_c, fill=0.0)
    for _ in range(2):
        be.call("stx_corr1d_lookup_bwd", ptr(be.dev(gws[0])), ptr(be.dev(base)), None, jobs, nj, ptr(gcp), B, H, W1, W2, L)
    near(gcp, 2 * _pack([c.grad for c in cp64]), 8 * EPS, "lookup backward")
    # refused, nothing launched: five levels, nine jobs, radius 9, a job on a level the pyramid does not have
    from stereo_toolbox_amd import ops
    untouched = be.empty(B, out_channels(tag), H, W1)
    for bad, nlev in (([(0, r, 0.0, 1.0)] * 9, L), ([(0, 9, 0.0, 1.0)], L), ([(L, r, 0.0, 1.0)], L), ([(0, r, 0.0, 1.0)], 5)):
        jb, n = _jobs(bad)
        with pytest.raises(ops.StxError):
            be.call("stx_corr1d_lookup_fwd", ptr(be.dev(_pack(cp))), ptr(be.dev(base)), None, jb, n, ptr(untouched), B, H, W1, W2, nlev)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(untouched).all()
