"""IGEV geometry-encoding lookup (`Combined_Geo_Encoding_Volume`, reference models/IGEVStereo/geometry.py:7-70) and convex
upsampling (`context_upsample`, models/IGEVStereo/submodule.py:243-255) on the kernels of csrc/geo_lookup.hip.

* tests/golden/geo_lookup.npz holds what the reference's OWN classes give on the seeded cases of tests/golden/geo_config.py, in
  fp32 and in fp64, and per tensor d_ref = max|fp32 - fp64| (tests/golden/make_golden_geo.py).
* A plain-torch restatement of geometry.py in gather form (no grid_sample) lives in tests/restated.py and is pinned to the
  fixture on the CPU first -- in fp64 to 1e-11 (the reading of the reference), in fp32 to 2 x d_ref (two fp32 evaluations of
  one quantity; tests/parity.pin) -- so the fixture and the restatement check each other.
* The product (emulator build here, gfx950 with `-m gpu`) is compared with the fp64 fixture: values within 2 x d_ref,
  gradients within GRAD_FACTOR (3) x d_ref; where d_ref is zero the floor 2e-7 * max(1, max|want|) applies
  (tests/parity.within).  Every element of every tensor of every case is compared.
* Tolerances against the restatement where no fixture exists (kernel-level pyramid gradients, the end-to-end chain):
  a sample is (1 - f) a + f b -- a handful of fp32 roundings on quantities of the tensor's scale, bounded here by
  8 * 2^-24 of the tensor's max -- plus, for the correlation samples, the rounding of `coords - disp` (half an ulp of the
  row length W, times a slope of at most twice the tensor's max): W * 2^-23 of the max.
"""
import os

import numpy as np
import pytest
import torch

from tests.backends import be, ptr  # noqa: F401
from tests.golden.geo_config import CASES, UPSAMPLE_CASES, inputs, out_channels, upsample_inputs
from tests.parity import EPS, GRAD_FACTOR, VALUE_FACTOR, env, near, pin_fixture, within_fixture  # noqa: F401
from tests.restated import _pack, lookup, pool, pyramids, upsample

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geo_lookup.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------------------------------ the restatement vs the fixture
def _restated_case(tag, dtype):
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    geo, f1, f2, coords, disps, gws = inputs(tag)
    geo, f1, f2 = (t.to(dtype).requires_grad_() for t in (geo, f1, f2))
    gp, cp = pyramids(geo, f1, f2, L)
    outs = [lookup(gp, cp, d.to(dtype), coords.to(dtype), r) for d in disps]
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, gws)).backward()
    return {"out_a": outs[0], "out_b": outs[1], "corr": cp[0].unsqueeze(3), "g_geo": geo.grad, "g_fmap1": f1.grad, "g_fmap2": f2.grad}


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_matches_reference_fixture(gold, tag):
    r64 = _restated_case(tag, torch.float64)
    r32 = _restated_case(tag, torch.float32)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"{tag}:{k}")


def _restated_upsample(tag, dtype):
    disp, wts, gw = upsample_inputs(tag)
    disp, wts = disp.to(dtype).requires_grad_(), wts.to(dtype).requires_grad_()
    out = upsample(disp, wts)
    (out * gw.to(dtype)).sum().backward()
    return {"out": out, "g_disp_low": disp.grad, "g_up_weights": wts.grad}


@pytest.mark.parametrize("tag", list(UPSAMPLE_CASES))
def test_upsample_restatement_matches_reference_fixture(gold, tag):
    r64, r32 = _restated_upsample(tag, torch.float64), _restated_upsample(tag, torch.float32)
    for k in r64:
        pin_fixture(r64[k], r32[k], gold, f"up_{tag}:{k}")


# ------------------------------------------------------------------------------------------ the product vs the fp64 fixture
def _product_case(env, tag, calls=(0, 1), channels_last=False):
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    geo, f1, f2, coords, disps, gws = inputs(tag)
    dev = env.device
    if channels_last:                                     # the view IGEVCostAggregation returns: dense [B,D,H,W,C] underneath
        geo = geo.permute(0, 2, 3, 4, 1).contiguous().to(dev).requires_grad_()
        geo_in = geo.permute(0, 4, 1, 2, 3)
    else:
        geo = geo.to(dev).requires_grad_()
        geo_in = geo
    f1, f2 = f1.to(dev).requires_grad_(), f2.to(dev).requires_grad_()
    with env.ctx():
        fn = Combined_Geo_Encoding_Volume(f1, f2, geo_in, num_levels=L, radius=r)
        outs = {i: fn(disps[i].to(dev), coords.to(dev)) for i in calls}
        sum((outs[i] * gws[i].to(dev)).sum() for i in calls).backward()
        if env.name == "hip":
            torch.cuda.synchronize()
    g_geo = geo.grad.permute(0, 4, 1, 2, 3) if channels_last else geo.grad
    return outs, {"g_geo": g_geo, "g_fmap1": f1.grad, "g_fmap2": f2.grad}


@pytest.mark.parametrize("tag", list(CASES))
def test_lookup_matches_reference_fp64(env, gold, tag):
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    outs, grads = _product_case(env, tag, channels_last=(tag == "r2_l3_odd"))
    for i, k in ((0, "out_a"), (1, "out_b")):
        o = outs[i]
        assert o.shape == (B, out_channels(tag), H, W) and o.dtype == torch.float32 and o.is_contiguous()
        within_fixture(o, gold, f"{tag}:{k}", VALUE_FACTOR, f"{tag} {k}")
    for k, g in grads.items():
        within_fixture(g, gold, f"{tag}:{k}", GRAD_FACTOR, f"{tag} {k}")


@pytest.mark.parametrize("tag", list(CASES))
def test_corr_matches_reference_einsum(env, gold, tag):
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    _, f1, f2, *_ = inputs(tag)
    with env.ctx():
        corr = Combined_Geo_Encoding_Volume.corr(f1.to(env.device), f2.to(env.device))
    assert corr.shape == (B, H, W, 1, W2) and corr.dtype == torch.float32 and corr.is_contiguous()
    within_fixture(corr, gold, f"{tag}:corr", VALUE_FACTOR, f"{tag} corr")


@pytest.mark.parametrize("tag", list(UPSAMPLE_CASES))
def test_context_upsample_matches_reference_fp64(env, gold, tag):
    from stereo_toolbox_amd.models.IGEVStereo import context_upsample
    B, h, w = UPSAMPLE_CASES[tag]
    disp, wts, gw = upsample_inputs(tag)
    disp, wts = disp.to(env.device).requires_grad_(), wts.to(env.device).requires_grad_()
    with env.ctx():
        out = context_upsample(disp, wts)
        (out * gw.to(env.device)).sum().backward()
    assert out.shape == (B, 4 * h, 4 * w) and out.dtype == torch.float32 and out.is_contiguous()
    within_fixture(out, gold, f"up_{tag}:out", VALUE_FACTOR, "upsampled disparity")
    within_fixture(disp.grad, gold, f"up_{tag}:g_disp_low", GRAD_FACTOR, "g disp_low")
    within_fixture(wts.grad, gold, f"up_{tag}:g_up_weights", GRAD_FACTOR, "g up_weights")


# ------------------------------------------------------------------------------------------ kernel level (C-ABI)
def test_kernel_level_pyramids_and_lookup(be, gold):  # noqa: F811
    """stx_geo_pyramid_fwd/_bwd, stx_geo_corr_fwd/_bwd, stx_geo_lookup_fwd/_bwd through the C-ABI at the ragged case (odd D, odd
    W2, W = 18, B = 2, three levels)."""
    tag = "r2_l3_odd"
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    geo, f1, f2, coords, disps, gws = inputs(tag)
    gp, cp = pyramids(geo, f1, f2, L)
    gp = [g.permute(0, 1, 2, 4, 3).contiguous() for g in gp]            # [B,H,W,D_i,C]
    n_g, n_c = sum(g.numel() for g in gp), sum(c.numel() for c in cp)
    assert be.raw("stx_geo_pyramid_floats")(B * H * W, D, C, L) == n_g
    assert be.raw("stx_geo_pyramid_floats")(B * H * W, W2, 1, L) == n_c
    # pyramid of the geometry volume: data movement and the reference's own averaging -- exact
    gpyr = be.empty(n_g)
    be.call("stx_geo_pyramid_fwd", ptr(be.dev(geo.permute(0, 2, 3, 4, 1))), ptr(gpyr), B, D, H, W, C, L)
    assert torch.equal(gpyr.cpu(), _pack(gp))
    # correlation pyramid: level 0 against the reference einsum (fp64 fixture), pooled levels = pool(level 0) exactly
    cpyr = be.empty(n_c)
    be.call("stx_geo_corr_fwd", ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(cpyr), B, Cf, H, W, W2, L)
    lv0 = cpyr.cpu()[:cp[0].numel()].view(B, H, W, W2)
    within_fixture(lv0.unsqueeze(3), gold, f"{tag}:corr", VALUE_FACTOR, "corr level 0")
    assert torch.equal(cpyr.cpu(), _pack([lv0, pool(lv0), pool(pool(lv0))]))
    # lookup forward on pyramids packed from the restatement
    out = be.empty(B, out_channels(tag), H, W)
    be.call("stx_geo_lookup_fwd", ptr(be.dev(_pack(gp))), ptr(be.dev(_pack(cp))), ptr(be.dev(disps[0])), ptr(be.dev(coords)), ptr(out),
            B, H, W, D, C, W2, L, r)
    within_fixture(out, gold, f"{tag}:out_a", VALUE_FACTOR, "lookup forward")
    # lookup backward: ADDS into the buffers (twice -> twice the gradient), against autograd of the fp64 restatement
    gp64 = [g.double().requires_grad_() for g in gp]
    cp64 = [c.double().requires_grad_() for c in cp]
    o64 = lookup([g.permute(0, 1, 2, 4, 3) for g in gp64], cp64, disps[0].double(), coords.double(), r)
    o64.backward(gws[0].double())
    ggp, gcp = be.empty(n_g, fill=0.0), be.empty(n_c, fill=0.0)
    for _ in range(2):
        be.call("stx_geo_lookup_bwd", ptr(be.dev(gws[0])), ptr(be.dev(disps[0])), ptr(be.dev(coords)), ptr(ggp), ptr(gcp),
                B, H, W, D, C, W2, L, r)
    near(ggp, 2 * _pack([g.grad for g in gp64]), 8 * EPS, "lookup backward, geometry pyramid")
    near(gcp, 2 * _pack([c.grad for c in cp64]), 8 * EPS + W * 2 * EPS, "lookup backward, correlation pyramid")
    # pyramid backward kernels on a seeded pyramid gradient, against autograd of the restatement
    from stereo_toolbox_amd.utils import synthetic_tensor
    gg, gc = synthetic_tensor((n_g,), 901), synthetic_tensor((n_c,), 902)
    geo64, f164, f264 = (t.double().requires_grad_() for t in (geo, f1, f2))
    gp2, cp2 = pyramids(geo64, f164, f264, L)
    ((_pack([g.permute(0, 1, 2, 4, 3) for g in gp2]) * gg.double()).sum() + (_pack(cp2) * gc.double()).sum()).backward()
    gvol, gf1, gf2 = be.empty(B, D, H, W, C), be.empty(B, Cf, H, W), be.empty(B, Cf, H, W2)
    be.call("stx_geo_pyramid_bwd", ptr(be.dev(gg)), ptr(gvol), B, D, H, W, C, L)
    be.call("stx_geo_corr_bwd", ptr(be.dev(gc)), ptr(be.dev(f1)), ptr(be.dev(f2)), ptr(gf1), ptr(gf2), B, Cf, H, W, W2, L)
    near(gvol.permute(0, 4, 1, 2, 3), geo64.grad, 8 * EPS, "pyramid backward")
    # a dot product over W (W2) terms of size max|g| * max|f|: sqrt-free bound n * 2^-24 of the result's scale
    near(gf1, f164.grad, W2 * EPS, "corr backward fmap1")
    near(gf2, f264.grad, W * EPS, "corr backward fmap2")


def test_kernel_level_context_upsample(be, gold):  # noqa: F811
    tag = "b1_3x18"
    B, h, w = UPSAMPLE_CASES[tag]
    disp, wts, gw = upsample_inputs(tag)
    out, gd, gwt = be.empty(B, 4 * h, 4 * w), be.empty(B, 1, h, w), be.empty(B, 9, 4 * h, 4 * w)
    be.call("stx_context_upsample_fwd", ptr(be.dev(disp)), ptr(be.dev(wts)), ptr(out), B, h, w)
    be.call("stx_context_upsample_bwd", ptr(be.dev(gw)), ptr(be.dev(disp)), ptr(be.dev(wts)), ptr(gd), ptr(gwt), B, h, w)
    within_fixture(out, gold, f"up_{tag}:out", VALUE_FACTOR, "upsample forward")
    within_fixture(gd, gold, f"up_{tag}:g_disp_low", GRAD_FACTOR, "upsample g disp")
    within_fixture(gwt, gold, f"up_{tag}:g_up_weights", GRAD_FACTOR, "upsample g weights")


# ------------------------------------------------------------------------------------------ behaviour
def test_lookup_is_bitwise_reproducible(env):
    a_out, a_grad = _product_case(env, "r2_l3_odd")
    b_out, b_grad = _product_case(env, "r2_l3_odd")
    for i in a_out:
        assert torch.equal(a_out[i], b_out[i])
    for k in a_grad:
        assert torch.equal(a_grad[k], b_grad[k]), k


def test_disp_requiring_grad_is_refused(env):
    from stereo_toolbox_amd import ops
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume
    tag = "l1_r3"
    B, C, D, H, W, W2, Cf, L, r = CASES[tag]
    geo, f1, f2, coords, disps, _ = inputs(tag)
    dev = env.device
    with env.ctx():
        fn = Combined_Geo_Encoding_Volume(f1.to(dev), f2.to(dev), geo.to(dev).requires_grad_(), num_levels=L, radius=r)
        with pytest.raises(ops.StxError, match="detach"):
            fn(disps[0].to(dev).clone().requires_grad_(), coords.to(dev))
        with pytest.raises(ops.StxError):
            fn(disps[0].to(dev), coords.to(dev).clone().requires_grad_())
        out = fn(disps[0].to(dev).clone().requires_grad_().detach(), coords.to(dev))
    assert out.shape == (B, out_channels(tag), H, W)


@pytest.mark.parametrize("tag", ["igev_r4_l2", "r2_l3_odd"])
def test_two_calls_give_the_sum_of_the_single_call_gradients(env, gold, tag):
    """The iteration pattern: two lookups on one object, losses summed -> the gradients of the two single-lookup runs, added.
    (Same tolerance as the gradient check: the three runs round independently.)"""
    _, both = _product_case(env, tag, calls=(0, 1))
    _, only_a = _product_case(env, tag, calls=(0,))
    _, only_b = _product_case(env, tag, calls=(1,))
    for k in both:
        tol = GRAD_FACTOR * float(gold[f"{tag}:{k}:dref"])
        want = only_a[k].double() + only_b[k].double()
        err = (both[k].double() - want).abs().max().item()
        assert err <= tol, (k, err, tol)
        assert both[k].abs().max().item() > 0


def test_aggregation_to_lookup_to_upsample_end_to_end(env):
    """IGEVCostAggregation -> Combined_Geo_Encoding_Volume -> two lookups (init_disp, init_disp + 0.37) -> context_upsample with
    a seeded softmax mask, backward to the aggregation's parameters.  The lookup / upsampling part is compared with the
    restatement (fp64) fed with the product's own geo_encoding_volume and init_disp: values, and the gradients that part hands
    back to the aggregation (which then continue to its parameters)."""
    from stereo_toolbox_amd.models.IGEVStereo import Combined_Geo_Encoding_Volume, IGEVCostAggregation, context_upsample
    from stereo_toolbox_amd.utils import synthetic_tensor
    from tests.golden.igev_agg_config import B, FEAT_CH, H4, MAXDISP, W4, fill
    dev = env.device
    m = IGEVCostAggregation(MAXDISP)
    m.load_state_dict(fill(m.state_dict()))
    m = m.to(dev).train()
    ml, mr = synthetic_tensor((B, 96, H4, W4), 71).to(dev), synthetic_tensor((B, 96, H4, W4), 72).to(dev)
    feats = [synthetic_tensor((B, c, H4 >> i, W4 >> i), 73 + i).to(dev) for i, c in enumerate(FEAT_CH)]
    coords = torch.arange(W4, dtype=torch.float32, device=dev).view(1, 1, 1, W4).repeat(B, 1, H4, 1)
    mask = torch.softmax(synthetic_tensor((B, 9, 4 * H4, 4 * W4), 701), dim=1).to(dev)
    L, r = 2, 4
    n = L * 9 * (2 * r + 1)
    gws = [synthetic_tensor((B, n, H4, W4), 702 + i).to(dev) for i in range(2)]
    gup = synthetic_tensor((B, 4 * H4, 4 * W4), 704).to(dev)
    with env.ctx():
        geo, init_disp = m(ml, mr, feats)
        assert not geo.is_contiguous()                                   # the channels-last view: taken without a copy
        geo_in, disp_in = geo.detach().requires_grad_(), init_disp.detach().requires_grad_()
        mli, mri = ml.clone().requires_grad_(), mr.clone().requires_grad_()
        fn = Combined_Geo_Encoding_Volume(mli, mri, geo_in, num_levels=L, radius=r)
        assert fn.geo_volume_pyramid.numel() == B * H4 * W4 * 8 * (MAXDISP // 4 + MAXDISP // 8)
        outs = [fn(disp_in.detach() + s, coords) for s in (0.0, 0.37)]
        up = context_upsample(disp_in, mask)
        loss = sum((o * g).sum() for o, g in zip(outs, gws)) + (up * gup).sum()
        loss.backward()
        torch.autograd.backward([geo, init_disp], [geo_in.grad, disp_in.grad])
        if env.name == "hip":
            torch.cuda.synchronize()
    # the restatement on the product's own volume and disparity, fp64
    g64 = geo.detach().cpu().double().requires_grad_()
    d64 = init_disp.detach().cpu().double().requires_grad_()
    l64, r64 = ml.cpu().double().requires_grad_(), mr.cpu().double().requires_grad_()
    gp, cp = pyramids(g64, l64, r64, L)
    outs64 = [lookup(gp, cp, d64.detach() + s, coords.cpu().double(), r) for s in (0.0, 0.37)]
    up64 = upsample(d64, mask.cpu().double())
    (sum((o * g.cpu().double()).sum() for o, g in zip(outs64, gws)) + (up64 * gup.cpu().double()).sum()).backward()
    val = 8 * EPS + W4 * 2 * EPS
    for o, o64 in zip(outs, outs64):
        near(o, o64, val, "lookup values")
    near(up, up64, 16 * EPS, "upsampled disparity")                      # 9 products and their sum
    near(geo_in.grad, g64.grad, 2 * 8 * EPS, "g geo_encoding_volume")     # two lookups' contributions
    near(disp_in.grad, d64.grad, 144 * EPS, "g init_disp")               # 144-term sum per low-resolution pixel
    near(mli.grad, l64.grad, 2 * (8 * EPS + W4 * 2 * EPS) + W4 * EPS, "g match_left")
    near(mri.grad, r64.grad, 2 * (8 * EPS + W4 * 2 * EPS) + W4 * EPS, "g match_right")
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert sum(float(g.abs().sum()) for g in grads) > 0
