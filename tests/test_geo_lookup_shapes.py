"""The kernels of csrc/geo_lookup.hip at the shapes where they branch, and the autograd hand-off of the lookups.

tests/test_geo_lookup.py compares every value with whole fp64 tensors of the reference, at shapes of a few hundred pixels.  The
kernels decide on sizes those cases never reach: the four waves and the second `w2_0` round of the forward correlation
(W2 > 256), more than two trips of the backward reduction, the pixel tile of `geo_pyramid_kernel` below 16 (D * C > 963), more
than one channel quad layout (C = 12, 16), lookup grids beyond a handful of workgroups, the shape the README advertises
(144x240, W2 = 240, Cf = 96, D = 48).  This file runs them (tests/golden/geo_config.py SHAPE_CASES says which case reaches what).

What a case is compared with.  Whole tensors of these sizes are not kept in git.  tests/golden/geo_lookup_shapes.npz
(tests/golden/make_golden_geo.py, the reference's own classes in fp32 and fp64) keeps per tensor d_ref = max|fp32 - fp64| of the
REFERENCE, max|fp64| and a strided subsample of the fp64 tensor.
 (a) the fp64 restatement of tests/restated.py (`pyramids`, `lookup`, `upsample`) is pinned to that subsample to 1e-11 of
     the tensor's max -- tests/parity.pin_subsample;
 (b) EVERY element of the product's outputs and of all three gradients is compared with the restatement evaluated in fp64 at test
     time, within VALUE_FACTOR (2) x d_ref for values and GRAD_FACTOR (3) x d_ref for gradients -- d_ref being the stored number.
The kernel-level entry points get the wide and deep cases through the C-ABI with the checks that are exact today (geometry
pyramid, pooled = pool(level 0)) and the rounding-model bounds of test_kernel_level_pyramids_and_lookup.

Wall times of this file (8 cores, emulator): see the parity report entry `geo_shapes_wall_s`.
"""
import functools
import os
import time

import numpy as np
import pytest
import torch

from tests.backends import be, ptr  # noqa: F401
from tests.golden.geo_config import (EXTRA_CALLS, GPU_ONLY_SHAPE_CASES, GPU_ONLY_SHAPE_UPSAMPLE_CASES, ITER_CALLS, ITER_CASE,
                                     REFUSED_PYRAMID, SHAPE_CASES, SHAPE_UPSAMPLE_CASES, SUBSAMPLE, iter_inputs, shape_inputs,
                                     shape_out_channels, shape_upsample_inputs, subsample)
from tests.parity import EPS, GRAD_FACTOR, VALUE_FACTOR, Env, env, near, on, pin_subsample, sync, within  # noqa: F401
from tests.restated import _pack, lookup, pool, pyramids, upsample

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geo_lookup_shapes.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _check(got, want64, gold, key, factor, log):
    """Every element of `got` against the fp64 restatement, within factor x the reference's stored d_ref; the achieved ratio
    goes into `log` under the tensor's name."""
    dref = float(gold[key + ":dref"])
    assert dref > 0, key
    within(got, want64, dref, factor, key, lambda what, ratio, **_: log.update({key.split(":")[1]: round(ratio, 3)}))


def _pinned(r64, gold, tag):
    """(a): the restatement against the stored subsample of the reference's fp64 tensors."""
    for k, v in r64.items():
        pin_subsample(v, torch.from_numpy(gold[f"{tag}:{k}:sub"]), float(gold[f"{tag}:{k}:max"]), subsample, min(v.numel(), SUBSAMPLE),
                      f"{tag}:{k}")


# ------------------------------------------------------------------------------------------ the restatement, fp64, at test time
@functools.lru_cache(maxsize=2)
def _restated_shape(tag):
    B, C, D, H, W, W2, Cf, L, r = SHAPE_CASES[tag]
    geo, f1, f2, coords, disps, gws = shape_inputs(tag)
    geo, f1, f2 = (t.double().requires_grad_() for t in (geo, f1, f2))
    gp, cp = pyramids(geo, f1, f2, L)
    outs = [lookup(gp, cp, d.double(), coords.double(), r) for d in disps]
    sum((o * g.double()).sum() for o, g in zip(outs, gws)).backward()
    return {"out_a": outs[0].detach(), "out_b": outs[1].detach(), "corr": cp[0].detach().unsqueeze(3), "g_geo": geo.grad,
            "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def _extra_term(gp, cp, wg, wc):
    """The weighted sum of every level of both pyramids; gp [B,H,W,C,D_i], cp [B,H,W,W2_i] (the restatement's layout)."""
    return sum((g * w.to(g.dtype)).sum() for g, w in zip(gp, wg)) + sum((c * w.to(c.dtype)).sum() for c, w in zip(cp, wc))


@functools.lru_cache(maxsize=2)
def _restated_iterations(calls, extra):
    B, C, D, H, W, W2, Cf, L, r = ITER_CASE
    geo, f1, f2, coords, disps, gws, wg, wc = iter_inputs()
    geo, f1, f2 = (t.double().requires_grad_() for t in (geo, f1, f2))
    gp, cp = pyramids(geo, f1, f2, L)
    outs = [lookup(gp, cp, d.double(), coords.double(), r) for d in disps[:calls]]
    loss = sum((o * g.double()).sum() for o, g in zip(outs, gws))
    if extra:
        loss = loss + _extra_term(gp, cp, wg, wc)
    loss.backward()
    return {"outs": torch.stack(outs).detach(), "g_geo": geo.grad, "g_fmap1": f1.grad, "g_fmap2": f2.grad}


def _restated_upsample(tag):
    disp, wts, gw = shape_upsample_inputs(tag)
    disp, wts = disp.double().requires_grad_(), wts.double().requires_grad_()
    out = upsample(disp, wts)
    (out * gw.double()).sum().backward()
    return {"out": out.detach(), "g_disp_low": disp.grad, "g_up_weights": wts.grad}


@pytest.mark.parametrize("tag", list(SHAPE_CASES))
def test_restatement_matches_reference_subsample(gold, tag):
    _pinned(_restated_shape(tag), gold, tag)


def test_iteration_restatements_match_reference_subsample(gold):
    _pinned(_restated_iterations(ITER_CALLS, False), gold, "iter22")
    _pinned(_restated_iterations(EXTRA_CALLS, True), gold, "extra")


@pytest.mark.parametrize("tag", list(SHAPE_UPSAMPLE_CASES))
def test_upsample_restatement_matches_reference_subsample(gold, tag):
    _pinned(_restated_upsample(tag), gold, "up_" + tag)


# ------------------------------------------------------------------------------------------ (b) the product at these shapes
@pytest.mark.parametrize("backend,tag", on(SHAPE_CASES, GPU_ONLY_SHAPE_CASES))
def test_shape_case_matches_fp64_restatement(backend, tag, gold, parity_log):
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
    env = Env(backend)
    case = SHAPE_CASES[tag]
    B, C, D, H, W, W2, Cf, L, r = case
    want = _restated_shape(tag)
    geo, f1, f2, coords, disps, gws = shape_inputs(tag)
    dev = env.device
    t0 = time.time()
    geo, f1, f2 = (t.to(dev).requires_grad_() for t in (geo, f1, f2))
    with env.ctx():
        fn = Combined_Geo_Encoding_Volume(f1, f2, geo, num_levels=L, radius=r)
        outs = [fn(d.to(dev), coords.to(dev)) for d in disps]
        sum((o * g.to(dev)).sum() for o, g in zip(outs, gws)).backward()
        corr = Combined_Geo_Encoding_Volume.corr(f1.detach(), f2.detach())
        sync(env)
    wall = time.time() - t0
    log = {}
    for k, o in (("out_a", outs[0]), ("out_b", outs[1])):
        assert o.shape == (B, shape_out_channels(case), H, W) and o.dtype == torch.float32 and o.is_contiguous()
        _check(o, want[k], gold, f"{tag}:{k}", VALUE_FACTOR, log)
    assert corr.shape == (B, H, W, 1, W2) and corr.dtype == torch.float32 and corr.is_contiguous()
    _check(corr, want["corr"], gold, f"{tag}:corr", VALUE_FACTOR, log)
    for k, g in (("g_geo", geo.grad), ("g_fmap1", f1.grad), ("g_fmap2", f2.grad)):
        _check(g, want[k], gold, f"{tag}:{k}", GRAD_FACTOR, log)
    parity_log(f"geo_shapes[{backend}-{tag}]", err_over_d_ref=log, geo_shapes_wall_s=round(wall, 2))


def test_pyramid_that_does_not_fit_the_tile_is_refused(env):
    """D * C = 8256 floats per pixel: (1 + 1) pixels' rows exceed the 64 KiB tile even at WT = 1 -> StxError, nothing built."""
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
    B, C, D, H, W = REFUSED_PYRAMID
    dev = env.device
    geo = torch.zeros(B, C, D, H, W, device=dev)
    f1, f2 = torch.zeros(B, 8, H, W, device=dev), torch.zeros(B, 8, H, W, device=dev)
    with env.ctx(), pytest.raises(ops.StxError, match="does not fit"):
        Combined_Geo_Encoding_Volume(f1, f2, geo, num_levels=2, radius=4)


# ------------------------------------------------------------------------------------------ kernel level (C-ABI)
@pytest.mark.parametrize("tag", ["wide", "deep_wt8", "deep_wt4", "deep_d400"])
def test_kernel_level_pyramids_at_branching_shapes(be, gold, tag):  # noqa: F811
    """stx_geo_pyramid_fwd/_bwd and stx_geo_corr_fwd/_bwd through the C-ABI: all four waves, the second w2_0 round and >= 5 trips
    of both backward reductions (wide), the pixel tile at 8 and 4 with a partial last tile (deep_*)."""
    from stereo_toolbox_amd.utils import synthetic_tensor
    B, C, D, H, W, W2, Cf, L, r = SHAPE_CASES[tag]
    geo, f1, f2, coords, disps, gws = shape_inputs(tag)
    gp, cp = pyramids(geo, f1, f2, L)
    gp = [g.permute(0, 1, 2, 4, 3).contiguous() for g in gp]            # [B,H,W,D_i,C]
    n_g, n_c = sum(g.numel() for g in gp), sum(c.numel() for c in cp)
    assert be.raw("stx_geo_pyramid_floats")(B * H * W, D, C, L) == n_g
    assert be.raw("stx_geo_pyramid_floats")(B * H * W, W2, 1, L) == n_c
    # geometry pyramid: data movement and the reference's own averaging -- exact
    gpyr = be.empty(n_g)
    be.call("stx_geo_pyramid_fwd", ptr(be.dev(geo.permute(0, 2, 3, 4, 1))), ptr(gpyr), B, D, H, W, C, L)
    assert torch.equal(gpyr.cpu(), _pack(gp))
    # correlation pyramid: level 0 every element against the fp64 restatement, pooled levels = pool(level 0) exactly
    cpyr = be.empty(n_c)
    be.call("stx_geo_corr_fwd", ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(cpyr), B, Cf, H, W, W2, L)
    lv0 = cpyr.cpu()[:cp[0].numel()].view(B, H, W, W2)
    _check(lv0.unsqueeze(3), _restated_shape(tag)["corr"], gold, f"{tag}:corr", VALUE_FACTOR, {})
    assert torch.equal(cpyr.cpu(), _pack([lv0, pool(lv0), pool(pool(lv0))]))
    # lookup forward / backward on pyramids packed from the restatement (the geometry rows of D_i * C floats per pixel)
    out = be.empty(B, shape_out_channels(SHAPE_CASES[tag]), H, W)
    be.call("stx_geo_lookup_fwd", ptr(be.dev(_pack(gp))), ptr(be.dev(_pack(cp))), ptr(be.dev(disps[0])), ptr(be.dev(coords)), ptr(out),
            B, H, W, D, C, W2, L, r)
    gp64 = [g.double().requires_grad_() for g in gp]
    cp64 = [c.double().requires_grad_() for c in cp]
    o64 = lookup([g.permute(0, 1, 2, 4, 3) for g in gp64], cp64, disps[0].double(), coords.double(), r)
    o64.backward(gws[0].double())
    reach = max(W2, float(coords.max()) + 1)                             # the magnitude `coords - disp` is rounded at
    near(out, o64, 8 * EPS + reach * 2 * EPS, "lookup forward")
    ggp, gcp = be.empty(n_g, fill=0.0), be.empty(n_c, fill=0.0)
    be.call("stx_geo_lookup_bwd", ptr(be.dev(gws[0])), ptr(be.dev(disps[0])), ptr(be.dev(coords)), ptr(ggp), ptr(gcp),
            B, H, W, D, C, W2, L, r)
    near(ggp, _pack([g.grad for g in gp64]), 8 * EPS, "lookup backward, geometry pyramid")
    near(gcp, _pack([c.grad for c in cp64]), 8 * EPS + reach * 2 * EPS, "lookup backward, correlation pyramid")
    # pyramid backward kernels on a seeded gradient of EVERY pyramid element, against autograd of the restatement
    gg, gc = synthetic_tensor((n_g,), 911), synthetic_tensor((n_c,), 912)
    geo64, f164, f264 = (t.double().requires_grad_() for t in (geo, f1, f2))
    gp2, cp2 = pyramids(geo64, f164, f264, L)
    ((_pack([g.permute(0, 1, 2, 4, 3) for g in gp2]) * gg.double()).sum() + (_pack(cp2) * gc.double()).sum()).backward()
    gvol, gf1, gf2 = be.empty(B, D, H, W, C), be.empty(B, Cf, H, W), be.empty(B, Cf, H, W2)
    be.call("stx_geo_pyramid_bwd", ptr(be.dev(gg)), ptr(gvol), B, D, H, W, C, L)
    be.call("stx_geo_corr_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(gf1), ptr(gf2), B, Cf, H, W, W2, L)
    near(gvol.permute(0, 4, 1, 2, 3), geo64.grad, 8 * EPS, "pyramid backward")
    # a dot product over W2 (W) terms of size max|g| * max|f|: n * 2^-24 of the result's scale
    near(gf1, f164.grad, W2 * EPS, "corr backward fmap1")
    near(gf2, f264.grad, W * EPS, "corr backward fmap2")
    # one gradient only: the other launch is left out, the result is the same bits
    only1, only2 = be.empty(B, Cf, H, W), be.empty(B, Cf, H, W2)
    be.call("stx_geo_corr_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(only1), None, B, Cf, H, W, W2, L)
    be.call("stx_geo_corr_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), None, ptr(only2), B, Cf, H, W, W2, L)
    assert torch.equal(only1, gf1) and torch.equal(only2, gf2)


def test_kernel_level_refused_pyramid_launches_nothing(be):  # noqa: F811
    from stereo_toolbox_amd import ops
    B, C, D, H, W = REFUSED_PYRAMID
    vol = be.dev(torch.zeros(B, D, H, W, C))
    n = be.raw("stx_geo_pyramid_floats")(B * H * W, D, C, 2)
    gpyr, gvol = be.empty(n), be.empty(B, D, H, W, C)
    with pytest.raises(ops.StxError, match="does not fit"):
        be.call("stx_geo_pyramid_fwd", ptr(vol), ptr(gpyr), B, D, H, W, C, 2)
    with pytest.raises(ops.StxError, match="does not fit"):
        be.call("stx_geo_pyramid_bwd", ptr(gpyr), ptr(gvol), B, D, H, W, C, 2)
    if be.name == "hip":
        torch.cuda.synchronize()
    assert torch.isnan(gpyr).all() and torch.isnan(gvol).all()           # the fill of be.empty: untouched


# ------------------------------------------------------------------------------------------ the iteration pattern
class _Run:
    """One object on the ITER_CASE inputs: `calls` lookups (indices into the 22 disparities), loss = the lookups named in
    `in_loss` (default: all) weighted and summed, plus `extra` x the weighted sum of both PUBLIC pyramid tensors."""

    def __init__(self, env, calls, in_loss=None, extra=False, needs=(True, True, True), backward=True, prepare=None):
        from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
        B, C, D, H, W, W2, Cf, L, r = ITER_CASE
        geo, f1, f2, coords, disps, gws, wg, wc = iter_inputs()
        dev = env.device
        self.env = env
        self.leaves = [t.to(dev).requires_grad_(n) for t, n in zip((geo, f1, f2), needs)]
        geo_in, f1_in, f2_in = prepare(*self.leaves) if prepare else self.leaves
        with env.ctx():
            self.fn = Combined_Geo_Encoding_Volume(f1_in, f2_in, geo_in, num_levels=L, radius=r)
            self.outs = {i: self.fn(disps[i].to(dev), coords.to(dev)) for i in calls}
            used = calls if in_loss is None else in_loss
            self.loss = sum((self.outs[i] * gws[i].to(dev)).sum() for i in used) if used else 0.0
            if extra:
                self.loss = self.loss + self._extra(wg, wc)
            if backward:
                self.backward()

    def _extra(self, wg, wc):
        """The flat pixel-major buffers (level i: [pixel][D_i][C] / [pixel][W2_i]) against the layout-free weights."""
        dev = self.env.device
        w_geo = _pack([w.permute(0, 1, 2, 4, 3) for w in wg]).to(dev)
        w_corr = _pack(wc).to(dev)
        return (self.fn.geo_volume_pyramid * w_geo).sum() + (self.fn.init_corr_pyramid * w_corr).sum()

    def backward(self, **kw):
        with self.env.ctx():
            self.loss.backward(**kw)
            sync(self.env)

    @property
    def grads(self):
        return {k: t.grad for k, t in zip(("g_geo", "g_fmap1", "g_fmap2"), self.leaves)}


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or torch.equal(a[k], b[k]), k


def test_22_lookups_on_one_object(env, gold, parity_log):
    """A training step's 22 lookups with distinct disparities, losses summed: every output and all three gradients against the
    fp64 restatement, d_ref from the reference's run of the same 22 calls; a second run gives the same bits."""
    want = _restated_iterations(ITER_CALLS, False)
    t0 = time.time()
    run = _Run(env, range(ITER_CALLS))
    wall = time.time() - t0
    log = {}
    _check(torch.stack([run.outs[i] for i in range(ITER_CALLS)]), want["outs"], gold, "iter22:outs", VALUE_FACTOR, log)
    for k, g in run.grads.items():
        _check(g, want[k], gold, f"iter22:{k}", GRAD_FACTOR, log)
    parity_log(f"geo_shapes[{env.name}-iter22]", err_over_d_ref=log, geo_shapes_wall_s=round(wall, 2))
    again = _Run(env, range(ITER_CALLS))
    for i in run.outs:
        assert torch.equal(run.outs[i], again.outs[i])
    _same_bits(run.grads, again.grads)


def test_second_backward_on_a_retained_graph_equals_the_first(env):
    run = _Run(env, range(4), backward=False)
    run.backward(retain_graph=True)
    first = {k: g.clone() for k, g in run.grads.items()}
    for t in run.leaves:
        t.grad = None
    run.backward()
    _same_bits(first, run.grads)
    assert all(g.abs().max().item() > 0 for g in first.values())


def test_two_objects_alive_at_once_keep_their_own_gradients(env):
    """Two objects, calls interleaved (a0 b1 a2 b3 ...), ONE backward over the sum of both losses: each object's leaves get what
    they get when the two run apart -- the same bits (the order of one object's lookups in the backward pass is unchanged)."""
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
    B, C, D, H, W, W2, Cf, L, r = ITER_CASE
    geo, f1, f2, coords, disps, gws, wg, wc = iter_inputs()
    dev = env.device
    apart = [_Run(env, idx).grads for idx in ((0, 2, 4), (1, 3, 5))]
    leaves = [[t.clone().to(dev).requires_grad_() for t in (geo, f1, f2)] for _ in range(2)]
    with env.ctx():
        fns = [Combined_Geo_Encoding_Volume(lv[1], lv[2], lv[0], num_levels=L, radius=r) for lv in leaves]
        loss = 0.0
        for i in range(6):
            loss = loss + (fns[i % 2](disps[i].to(dev), coords.to(dev)) * gws[i].to(dev)).sum()
        loss.backward()
        sync(env)
    for lv, want in zip(leaves, apart):
        _same_bits({k: t.grad for k, t in zip(("g_geo", "g_fmap1", "g_fmap2"), lv)}, want)
    assert not torch.equal(leaves[0][0].grad, leaves[1][0].grad)


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, False, True)])
def test_a_subset_of_the_inputs_requires_grad(env, needs):
    """Only geo_volume / only the feature maps / only fmap2 require grad: those gradients are the bits of the run in which all
    three do, the others stay None."""
    full = _Run(env, range(4)).grads
    part = _Run(env, range(4), needs=needs).grads
    for (k, g), n in zip(part.items(), needs):
        assert (g is not None) == n, k
        assert g is None or torch.equal(g, full[k]), k


def test_a_lookup_outside_the_loss_changes_nothing(env):
    with_unused = _Run(env, range(4), in_loss=(0, 1, 3))
    without = _Run(env, (0, 1, 3))
    _same_bits(with_unused.grads, without.grads)
    assert torch.equal(with_unused.outs[3], without.outs[3])


def test_forward_without_grad_is_the_grad_mode_forward(env):
    run = _Run(env, range(3), backward=False)
    with torch.no_grad():
        plain = _Run(env, range(3), needs=(False, False, False), backward=False)
        under_no_grad = _Run(env, range(3), backward=False)
    for i in run.outs:
        assert run.outs[i].requires_grad and not plain.outs[i].requires_grad and not under_no_grad.outs[i].requires_grad
        assert torch.equal(run.outs[i], plain.outs[i]) and torch.equal(run.outs[i], under_no_grad.outs[i])
    assert torch.equal(run.fn.geo_volume_pyramid, plain.fn.geo_volume_pyramid)
    assert torch.equal(run.fn.init_corr_pyramid, plain.fn.init_corr_pyramid)


def test_another_consumer_of_the_pyramids_gets_the_whole_gradient(env, gold, parity_log):
    """loss = four lookups + a weighted sum of `fn.geo_volume_pyramid` and `fn.init_corr_pyramid` (public attributes, the
    reference's names).  The gradients must be those of the fp64 restatement of the same loss within GRAD_FACTOR x d_ref (d_ref
    from the reference's run of it).  Before the identity node of ops._PyramidGrads the shared buffer met the other consumer's
    gradient at the build node after the FIRST lookup and everything the later lookups added was lost: errors of 5.9 / 25.9 /
    16.9 on tensors of max 4.5 / 17.8 / 17.2, no exception."""
    want = _restated_iterations(EXTRA_CALLS, True)
    run = _Run(env, range(EXTRA_CALLS), extra=True)
    log = {}
    _check(torch.stack([run.outs[i] for i in range(EXTRA_CALLS)]), want["outs"], gold, "extra:outs", VALUE_FACTOR, log)
    for k, g in run.grads.items():
        _check(g, want[k], gold, f"extra:{k}", GRAD_FACTOR, log)
    parity_log(f"geo_shapes[{env.name}-extra_consumer]", err_over_d_ref=log)
    # the sum rule on the product itself: lookups only + extra term only, three independently rounded runs
    lookups, extra = _Run(env, range(EXTRA_CALLS)).grads, _Run(env, (), extra=True).grads
    for k, g in run.grads.items():
        err = (g.double() - (lookups[k].double() + extra[k].double())).abs().max().item()
        assert err <= GRAD_FACTOR * float(gold[f"extra:{k}:dref"]), (k, err)
    # ... and a second pass over the retained graph starts from zeros again
    again = _Run(env, range(EXTRA_CALLS), extra=True, backward=False)
    again.backward(retain_graph=True)
    for t in again.leaves:
        t.grad = None
    again.backward()
    _same_bits(again.grads, run.grads)


# ------------------------------------------------------------------------------------------ inputs that are not dense fp32
def test_channels_last_feature_maps_are_taken_as_their_dense_copies(env):
    """A channels-last fmap (strides of the 2-D CNN's output) gives the bits of its `.contiguous()` copy, values and gradients;
    Cf = 12 and H * W = 100 are multiples of 4: the transpose kernel of ops.channel_major serves it."""
    cl = lambda geo, f1, f2: (geo, f1.contiguous(memory_format=torch.channels_last), f2.contiguous(memory_format=torch.channels_last))  # noqa: E731
    a = _Run(env, range(3))
    b = _Run(env, range(3), prepare=cl)
    for i in a.outs:
        assert torch.equal(a.outs[i], b.outs[i])
    _same_bits(a.grads, b.grads)


@pytest.mark.parametrize("low", [torch.bfloat16, torch.float16])
def test_low_precision_feature_maps_under_autocast_are_their_fp32_casts(env, low):
    """Under autocast a bf16 / fp16 feature map (what the 2-D CNN hands over) is cast to fp32 on the way in: the result is
    bitwise that of `.float()` inputs, the gradient arrives at the fp32 leaf through the cast (the same bits, rounded once)."""
    device_type = "cuda" if env.name == "hip" else "cpu"
    rounded = lambda geo, f1, f2: (geo, f1.to(low).float(), f2.to(low).float())  # noqa: E731
    a = _Run(env, range(3), prepare=rounded)
    with torch.autocast(device_type, dtype=low):
        b = _Run(env, range(3), prepare=lambda geo, f1, f2: (geo, f1.to(low), f2.to(low)))
    for i in a.outs:
        assert b.outs[i].dtype == torch.float32 and torch.equal(a.outs[i], b.outs[i])
    assert torch.equal(a.grads["g_geo"], b.grads["g_geo"])
    for k in ("g_fmap1", "g_fmap2"):                                     # the cast's backward rounds the fp32 gradient to `low`
        assert torch.equal(a.grads[k].to(low).float(), b.grads[k]), k


@pytest.mark.gpu
def test_low_precision_feature_maps_outside_autocast_are_refused():
    from stereo_toolbox_amd import ops
    env = Env("hip")
    with pytest.raises(ops.StxError, match="float32"):
        _Run(env, range(1), prepare=lambda geo, f1, f2: (geo, f1.bfloat16(), f2.bfloat16()))
    with pytest.raises(ops.StxError, match="float32"):
        _Run(env, range(1), prepare=lambda geo, f1, f2: (geo.half(), f1, f2))


# ------------------------------------------------------------------------------------------ context_upsample
@pytest.mark.parametrize("backend,tag", on(SHAPE_UPSAMPLE_CASES, GPU_ONLY_SHAPE_UPSAMPLE_CASES))
def test_context_upsample_at_larger_shapes(backend, tag, gold, parity_log):
    """More than 256 low-resolution pixels per image and B = 2 (a second workgroup of context_upsample_bwd_disp_kernel, a batch
    boundary inside one), and 144x240 on the GPU."""
    from stereo_toolbox_amd.models.IGEVStereo import context_upsample
    env = Env(backend)
    B, h, w = SHAPE_UPSAMPLE_CASES[tag]
    want = _restated_upsample(tag)
    disp, wts, gw = shape_upsample_inputs(tag)
    t0 = time.time()
    disp, wts = disp.to(env.device).requires_grad_(), wts.to(env.device).requires_grad_()
    with env.ctx():
        out = context_upsample(disp, wts)
        (out * gw.to(env.device)).sum().backward()
        sync(env)
    wall = time.time() - t0
    assert out.shape == (B, 4 * h, 4 * w) and out.dtype == torch.float32 and out.is_contiguous()
    log = {}
    _check(out, want["out"], gold, f"up_{tag}:out", VALUE_FACTOR, log)
    _check(disp.grad, want["g_disp_low"], gold, f"up_{tag}:g_disp_low", GRAD_FACTOR, log)
    _check(wts.grad, want["g_up_weights"], gold, f"up_{tag}:g_up_weights", GRAD_FACTOR, log)
    parity_log(f"geo_shapes[{backend}-up_{tag}]", err_over_d_ref=log, geo_shapes_wall_s=round(wall, 2))
