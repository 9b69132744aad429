"""Kernel-level parity: every C-ABI entry point against the CPU oracle / stock fp32 torch ops.

Runs on the host emulator build (CPU, default) and on the real gfx950 library (-m gpu).
Tolerances: builders/estimators ~1e-6 (fp32 rounding only), MFMA convolutions 1e-4 relative to the
output magnitude (K up to 27*128 fp32 products, different summation order than torch).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_oracle as O
from tests.backends import be, ndhwc, ncdhw, pack, ptr, tune  # noqa: F401


def _close(got, ref, rtol=1e-4, atol=1e-5):
    err = (got.cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= atol + rtol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


def _check_volume(vol_ndhwc, ref, G):
    """Built volume vs the oracle: the concat channels are pure data movement (copy / shift / zero) and must be
    BIT-EXACT; the group correlations are fp32 sums of 4-16 products in a different order (1e-6)."""
    got = ncdhw(vol_ndhwc).cpu()
    assert got.shape == ref.shape
    if got.shape[1] > G:
        assert torch.equal(got[:, G:], ref[:, G:]), "concat volume is not an exact copy"
    if G:
        _close(got[:, :G], ref[:, :G], rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------ cost volume
CV_CASES = [
    # B, Cg, G, Cc, H, W, D, mask_left
    (2, 16, 4, 0, 3, 11, 6, 1),       # gwc only, tiny (SURVEY 8c fixture shape)
    (1, 320, 40, 12, 2, 37, 20, 1),   # GwcNet_GC channel config, ragged W and D
    (1, 0, 0, 32, 3, 21, 18, 1),      # PSMNet concat
    (1, 0, 0, 32, 3, 21, 18, 0),      # ACVNet concat (left half unmasked)
    (1, 64, 8, 4, 2, 40, 48, 1),      # D' = 48 > W tile
    (2, 320, 40, 0, 2, 24, 12, 1),    # ACVNet gwc-only volume, batch 2
    (1, 64, 8, 4, 3, 52, 13, 0),      # 8 channels per group, left half unmasked, D not a multiple of 8
    (1, 96, 8, 0, 2, 50, 20, 1),      # IGEV-style initial volume: 12 channels per group (igev_stereo.py:206)
    (1, 64, 4, 8, 2, 35, 9, 1),       # 16 channels per group
    (1, 32, 8, 0, 2, 33, 17, 1),      # 4 channels per group
    (1, 32, 4, 4, 1, 100, 80, 1),     # D' = 80: five 16-disparity units per macro-unit (long register ring)
]


def _cv_inputs(case):
    B, Cg, G, Cc, H, W, D, ml = case
    torch.manual_seed(1)
    Lg = torch.randn(B, Cg, H, W) if G else None
    Rg = torch.randn(B, Cg, H, W) if G else None
    Lc = torch.randn(B, Cc, H, W) if Cc else None
    Rc = torch.randn(B, Cc, H, W) if Cc else None
    parts = []
    if G:
        parts.append(O.build_gwc_volume(Lg, Rg, D, G))
    if Cc:
        parts.append(O.build_concat_volume(Lc, Rc, D, mask_left=bool(ml)))
    return Lg, Rg, Lc, Rc, torch.cat(parts, 1)


@pytest.mark.parametrize("sched", ["pairs_units", "one_ahead_units", "pairs_macros", "one_ahead_macros"])
@pytest.mark.parametrize("grid", [2, 3, 5])
def test_cost_volume_fwd_launch_variants(be, grid, sched, tune):
    """The default grid gives small test volumes one unit per workgroup; STX_CV_GRID forces runs of several units per
    workgroup (register rotation of the right-feature tiles along a row, row / chunk changes inside a run, double-buffered
    LDS image).  `sched`: the feature prefetch scheme (line pairs requested every other macro-unit, the odd partner parked
    in the wave's LDS slot by LDS-DMA / one tile ahead) and runs cut at units (they begin / end INSIDE a macro-unit: with 5
    workgroups every multi-unit case has such a cut) or at whole macro-units.
    All cases on the emulator, the GwcNet_GC channel configuration on the GPU."""
    tune("STX_CV_GRID", grid)
    tune("STX_CV_PF", 1 if sched.startswith("one_ahead") else 2)          # (1 is the default: GPU call C of round 4)
    tune("STX_CV_UNITS", 0 if sched.endswith("macros") else 1)
    for case in (CV_CASES if be.name == "emu" else CV_CASES[1:2]):
        B, Cg, G, Cc, H, W, D, ml = case
        Lg, Rg, Lc, Rc, ref = _cv_inputs(case)
        vol = be.empty(B, D, H, W, G + 2 * Cc)
        be.call("stx_cost_volume_fwd", ptr(be.dev(Lg)), ptr(be.dev(Rg)), Cg, G, ptr(be.dev(Lc)), ptr(be.dev(Rc)), Cc, None,
                ptr(vol), B, H, W, D, ml)
        _check_volume(vol, ref, G)


@pytest.mark.parametrize("units", [1, 0], ids=["cut_at_units", "cut_at_macros"])
@pytest.mark.parametrize("win", [1, 2, 5])
@pytest.mark.parametrize("grid", [2, 3])
def test_cost_volume_fwd_windows(be, grid, win, units, tune):
    """STX_CV_WIN (round 6): the launch walks the volume in WINDOWS of `win` macro-units, every window split over all workgroups
    (window hand-over barrier, ring / tables / image index restarted per window, a window smaller than the grid leaving workgroups
    without work in it, runs cut inside macro-units).  Same results as the one-window launch, bit for bit."""
    for case in (CV_CASES if be.name == "emu" else CV_CASES[1:2]):
        B, Cg, G, Cc, H, W, D, ml = case
        Lg, Rg, Lc, Rc, ref = _cv_inputs(case)
        outs = []
        for w in (0, win):
            tune("STX_CV_GRID", grid)
            tune("STX_CV_UNITS", units)
            tune("STX_CV_WIN", w)
            vol = be.empty(B, D, H, W, G + 2 * Cc)
            be.call("stx_cost_volume_fwd", ptr(be.dev(Lg)), ptr(be.dev(Rg)), Cg, G, ptr(be.dev(Lc)), ptr(be.dev(Rc)), Cc, None,
                    ptr(vol), B, H, W, D, ml)
            _check_volume(vol, ref, G)
            outs.append(vol.cpu())
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("variant", ["one_workgroup", "three_workgroups", "two_chunks_in_flight", "four_chunks_in_flight",
                                     "first_generation"])
def test_cost_volume_bwd_launch_variants(be, variant, tune):
    """Backward launch variants.  Small test volumes otherwise give the matrix-core kernel one macro-unit per workgroup;
    `one_workgroup` / `three_workgroups` force runs over many macro-units: the feature ring sliding along an image row,
    ring refills at row and side changes, the register double buffer of the volume gradient crossing macro-unit
    boundaries.  `first_generation` keeps the any-shape fallback kernels covered."""
    if variant == "first_generation":
        tune("STX_CVB_OLD", 1)
    elif variant.endswith("in_flight"):      # register sets of the loader waves (default 3 for the 40-group volumes)
        tune("STX_CVB_NSET", 2 if variant.startswith("two") else 4)
        tune("STX_CVB_GRID", 2)
    else:
        tune("STX_CVB_GRID", 1 if variant == "one_workgroup" else 3)
    for case in (CV_CASES if be.name == "emu" else CV_CASES[1:2]):
        if case[2] == 0:
            continue
        _cv_fwd_bwd(be, case, fwd=False)


@pytest.mark.parametrize("case", [(1, 320, 40, 12, 10, 130, 48, 1),     # GwcNet_GC channels, 6 chunks, 9 tiles, rows 8/9 = second round
                                  (2, 64, 8, 4, 5, 140, 43, 0)])         # D' = 43 (ragged last chunk), batch 2, left half unmasked
def test_cost_volume_bwd_team_schedule(be, case, tune):
    """The matrix-core backward's row-team schedule (one team of (tile, side) members per XCD, progressive feature ring):
    taken for 9-16 tiles per row and 40 < D' <= 48, i.e. the benchmark shape -- these are its smallest eligible volumes.
    Checked against the same launch on the run schedule (STX_CVB_TEAM=0) by way of the common reference."""
    tune("STX_CVB_TEAM", 1)                          # opt-in since GPU call O of round 2 (the run schedule measured faster)
    _cv_fwd_bwd(be, case, fwd=False)
    tune("STX_CVB_TEAM", 0)
    _cv_fwd_bwd(be, case, fwd=False)


@pytest.mark.parametrize("case", CV_CASES)
def test_cost_volume_fwd_bwd(be, case):
    _cv_fwd_bwd(be, case)


@pytest.mark.parametrize("case", [c for c in CV_CASES if not (c[2] and c[1] // c[2] == 12)])
def test_cost_volume_first_generation_fallback(be, case, tune):
    """The any-shape fallback kernels of cost_volume.hip (the matrix-core builders serve every model configuration; D' > 96
    or voxels of more than 64 channels end up here), forced for the regular cases."""
    tune("STX_CV_OLD", 1)
    tune("STX_CVB_OLD", 1)
    _cv_fwd_bwd(be, case)


def _cv_fwd_bwd(be, case, fwd=True):
    B, Cg, G, Cc, H, W, D, ml = case
    torch.manual_seed(1)
    Lg = torch.randn(B, Cg, H, W) if G else None
    Rg = torch.randn(B, Cg, H, W) if G else None
    Lc = torch.randn(B, Cc, H, W) if Cc else None
    Rc = torch.randn(B, Cc, H, W) if Cc else None
    CT = G + 2 * Cc
    leaves = [t.clone().requires_grad_() if t is not None else None for t in (Lg, Rg, Lc, Rc)]
    parts = []
    if G:
        parts.append(O.build_gwc_volume(leaves[0], leaves[1], D, G))
    if Cc:
        parts.append(O.build_concat_volume(leaves[2], leaves[3], D, mask_left=bool(ml)))
    ref = torch.cat(parts, 1)
    dLg, dRg, dLc, dRc = (be.dev(t) for t in (Lg, Rg, Lc, Rc))
    if fwd:
        vol = be.empty(B, D, H, W, CT)
        be.call("stx_cost_volume_fwd", ptr(dLg), ptr(dRg), Cg, G, ptr(dLc), ptr(dRc), Cc, None, ptr(vol), B, H, W, D, ml)
        _check_volume(vol, ref.detach(), G)

    gv = torch.randn(B, D, H, W, CT)
    ref.backward(ncdhw(gv))
    dgv = be.dev(gv)
    outs = [be.empty(*t.shape) if t is not None else None for t in (Lg, Rg, Lc, Rc)]
    be.call("stx_cost_volume_bwd", ptr(dgv), ptr(dLg), ptr(dRg), Cg, G, Cc, ptr(outs[0]), ptr(outs[1]),
            ptr(outs[2]), ptr(outs[3]), B, H, W, D, ml)
    for o, leaf in zip(outs, leaves):
        if o is not None:
            _close(o, leaf.grad, rtol=2e-6, atol=1e-5)


def test_cost_volume_scale_operand(be):
    """ACVNet/acv.py:196: softmax(att, dim=2) * concat_volume fused as the `scale` operand."""
    torch.manual_seed(2)
    B, Cc, H, W, D = 1, 8, 2, 19, 7
    Lc, Rc = torch.randn(B, Cc, H, W), torch.randn(B, Cc, H, W)
    att = torch.randn(B, 1, D, H, W)
    ref = F.softmax(att, dim=2) * O.build_concat_volume(Lc, Rc, D, mask_left=False)
    datt = be.dev(att)
    prob = be.empty(B, D, H, W)
    be.call("stx_softmax_d_fwd", ptr(datt), ptr(prob), B, D, H * W)
    vol = be.empty(B, D, H, W, 2 * Cc)
    be.call("stx_cost_volume_fwd", None, None, 0, 0, ptr(be.dev(Lc)), ptr(be.dev(Rc)), Cc, ptr(prob), ptr(vol),
            B, H, W, D, 0)
    _close(ncdhw(vol), ref, rtol=1e-6, atol=1e-6)


def test_cost_volume_rejects_bad_groups(be):
    from stereo_toolbox_amd._capi import StxError
    t = be.empty(1, 10, 2, 8, fill=0.0)
    vol = be.empty(1, 4, 2, 8, 4)
    with pytest.raises(StxError):   # C % num_groups != 0, reference assert GwcNet/submodule.py:46
        be.call("stx_cost_volume_fwd", ptr(t), ptr(t), 10, 4, None, None, 0, None, ptr(vol), 1, 2, 8, 4, 1)


# ------------------------------------------------------------------------------ head / estimators
@pytest.mark.parametrize("case", [(1, 4, 5, 7, 16, 20, 28, 5.0), (2, 12, 6, 9, 48, 24, 36, 3.0), (1, 5, 4, 6, 17, 13, 22, 4.0)])
def test_head_fwd_bwd(be, case):
    B, Dc, Hc, Wc, D, H, W, gain = case
    torch.manual_seed(3)
    cost = (torch.randn(B, 1, Dc, Hc, Wc) * gain).requires_grad_()
    ref = O.regression_head(cost, D, H, W)
    dcost = be.dev(cost.detach())
    disp, stats = be.empty(B, H, W), be.empty(B, H, W, 2)
    be.call("stx_head_fwd", ptr(dcost), ptr(disp), ptr(stats), B, Dc, Hc, Wc, D, H, W)
    assert (disp.cpu() - ref.detach()).abs().max().item() < 1e-4   # disparity parity bar is 1e-3
    g = torch.randn(B, H, W)
    ref.backward(g)
    gc = be.empty(B, 1, Dc, Hc, Wc)
    ws = be.empty(be.raw("stx_head_bwd_workspace_floats")(B, Dc, H, W))
    be.call("stx_head_bwd", ptr(be.dev(g)), ptr(dcost), ptr(disp), ptr(stats), ptr(gc), ptr(ws), B, Dc, Hc, Wc, D, H, W)
    _close(gc, cost.grad, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("case", [(1, 4, 5, 7, 16, 20, 28, 5.0), (2, 12, 6, 9, 48, 24, 36, 3.0), (1, 5, 4, 6, 17, 13, 22, 4.0),
                                  (1, 1, 3, 1, 4, 9, 5, 2.0), (1, 3, 2, 75, 12, 3, 300, 40.0), (1, 9, 3, 4, 5, 4, 6, 3.0),
                                  (1, 6, 3, 5, 24, 12, 20, 3000.0), (1, 84, 2, 3, 336, 8, 12, 3.0)])
def test_head2_fwd_bwd(be, case, ac):
    """Entry points with an explicit interpolation rule: align_corners=True is the PCWNet / CFNet head.  W = 300 spans two
    workgroups with a ragged tail, D < Dc leaves coarse planes without an output disparity, gain 3000 has cost steps far
    beyond the exp range (the LDS kernel's bound-shifted sum underflows and it must redo the walk with the exact maximum),
    D' = 84 exceeds the LDS-staged forward kernel's table (the first-generation kernel serves it)."""
    B, Dc, Hc, Wc, D, H, W, gain = case
    torch.manual_seed(3)
    cost = (torch.randn(B, 1, Dc, Hc, Wc) * gain).requires_grad_()
    ref = O.regression_head(cost, D, H, W, align_corners=bool(ac))
    dcost = be.dev(cost.detach())
    disp, stats = be.empty(B, H, W), be.empty(B, H, W, 2)
    be.call("stx_head_fwd2", ptr(dcost), ptr(disp), ptr(stats), B, Dc, Hc, Wc, D, H, W, ac)
    # 1e-4 at realistic logit ranges; with logit steps of 40+ the device's fast exp (exp2(x * log2 e): the argument's
    # rounding error grows with |x|) moves near-one-hot expectations by up to 6e-4 px on gfx950 -- still inside the 1e-3 bar
    assert (disp.cpu() - ref.detach()).abs().max().item() < (1e-4 * max(1.0, D / 96.0) if gain <= 5 else 1e-3)   # (fp32 ulp grows with D)
    g = torch.randn(B, H, W)
    ref.backward(g)
    gc = be.empty(B, 1, Dc, Hc, Wc)
    ws = be.empty(be.raw("stx_head_bwd_workspace_floats")(B, Dc, H, W))
    be.call("stx_head_bwd2", ptr(be.dev(g)), ptr(dcost), ptr(disp), ptr(stats), ptr(gc), ptr(ws), B, Dc, Hc, Wc, D, H, W, ac)
    if gain <= 5:
        _close(gc, cost.grad, rtol=1e-5, atol=1e-5)
    else:                                   # (same fast-exp effect on the probabilities: 1e-4 of the gradient's scale on gfx950)
        _close(gc, cost.grad, rtol=3e-4, atol=1e-4)


def test_estimators(be):
    torch.manual_seed(4)
    x = torch.softmax(torch.randn(2, 16, 6, 10) * 3, 1)
    flat = torch.full((2, 16, 6, 10), 1.0 / 16)
    # (HW % 4 == 0: four pixels per lane, eight planes per trip; D = 21 leaves a tail; HW = 35 takes the scalar kernel)
    for t in (torch.softmax(torch.randn(1, 21, 4, 7) * 3, 1), torch.softmax(torch.randn(1, 21, 5, 7) * 3, 1)):
        o = be.empty(*t.shape[:1], *t.shape[2:])
        be.call("stx_softargmax_fwd", ptr(be.dev(t)), ptr(o), 1, 21, t.shape[2] * t.shape[3])
        _close(o, O.disparity_regression(t, 21), rtol=1e-6, atol=1e-6)
    for t in (x, flat):
        d = be.dev(t)
        o = be.empty(2, 6, 10)
        be.call("stx_softargmax_fwd", ptr(d), ptr(o), 2, 16, 60)
        _close(o, O.disparity_regression(t, 16), rtol=1e-6, atol=1e-6)
        a = be.empty(2, 6, 10, dtype=torch.int64)
        be.call("stx_argmax_fwd", ptr(d), ptr(a), 2, 16, 60)
        assert torch.equal(a.cpu(), O.argmax_disparity_estimator(t, 16).squeeze(1))
    z = torch.randn(2, 16, 6, 10)
    y = be.empty(2, 16, 6, 10)
    be.call("stx_softmax_d_fwd", ptr(be.dev(z)), ptr(y), 2, 16, 60)
    _close(y, torch.softmax(z, 1), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("case", [(2, 32, 5, 9, 21), (1, 48, 4, 7, 22), (1, 192, 6, 40, 31), (2, 16, 6, 10, 0),
                                  (1, 608, 2, 5, 3)])   # D > 600: columns walked in place instead of in LDS
def test_modal_estimators(be, case):
    """unimodal / dominant-modal estimators vs the oracle (which is pinned bitwise to the reference, tests/golden).
    The mode choice is discrete: a pixel may legitimately flip when the blurred volume (different fp32 summation order
    than conv1d) has two near-equal candidates, so a handful of mismatching pixels is tolerated, none is expected."""
    from stereo_toolbox_amd.utils import synthetic_modal_volume, synthetic_tensor
    B, D, H, W, seed = case
    x = synthetic_modal_volume(B, D, H, W, seed) if seed else torch.softmax(synthetic_tensor((B, D, H, W), 13) * 4, 1)
    d = be.dev(x)
    for entry, ref in (("stx_unimodal_fwd", O.unimodal_disparity_estimator),
                       ("stx_dominant_modal_fwd", O.dominant_modal_disparity_estimator)):
        o = be.empty(B, H * W)
        be.call(entry, ptr(d), ptr(o), B, D, H * W)
        want = ref(x, D).reshape(B, H * W)
        bad = ((o.cpu() - want).abs() > 1e-4 * (1 + want.abs())).sum().item()
        assert bad <= (0 if entry == "stx_unimodal_fwd" else B * H * W // 100), f"{entry}: {bad} pixels differ"


@pytest.mark.parametrize("case", [(2, 128, 64), (1, 136, 12), (3, 68, 320), (1, 4, 4), (2, 320, 200)])
def test_transpose(be, case):
    """stx_transpose vs Tensor.transpose: exact (a permutation); tile edges in both directions."""
    N, rows, cols = case
    torch.manual_seed(4)
    x = torch.randn(N, rows, cols)
    out = be.empty(N, cols, rows)
    out.fill_(-3.0)
    be.call("stx_transpose", ptr(be.dev(x)), ptr(out), N, rows, cols)
    assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous())


@pytest.mark.parametrize("case", [(37, (64, 128, 128)), (5, (8, 4)), (130, (12, 64, 4, 16)), (1, (32, 32))])
def test_concat_split_channels(be, case):
    """stx_concat_channels / stx_split_channels vs torch.cat / torch.split on dense channels-last tensors: exact (copies).
    Replaces the feature extractors' `torch.cat((l2, l3, l4), dim=1)` (reference gwcnet.py:59, acv.py:48) and its backward."""
    nvox, cs = case
    torch.manual_seed(3)
    parts = [torch.randn(nvox, c) for c in cs]
    want = torch.cat(parts, -1)
    dp = [be.dev(t) for t in parts]
    pad = [None] * (4 - len(cs))
    out = be.empty(nvox, sum(cs))
    out.fill_(-7.0)
    be.call("stx_concat_channels", *[ptr(t) for t in dp], *pad, *cs, *([0] * len(pad)), ptr(out), nvox)
    assert torch.equal(out.cpu(), want)
    back = [be.empty(nvox, c) for c in cs]
    be.call("stx_split_channels", ptr(out), *[ptr(t) for t in back], *pad, *cs, *([0] * len(pad)), nvox)
    for got, t in zip(back, parts):
        assert torch.equal(got.cpu(), t)


@pytest.mark.parametrize("case", [(2, 32, 5, 9, 21), (1, 48, 4, 7, 22), (1, 192, 6, 40, 31), (2, 16, 6, 10, 0),
                                  (1, 608, 2, 5, 3)])
def test_split_mode(be, case):
    """stx_split_mode vs the oracle's split_mode (pinned bitwise to loss_functions/split_mode.py:9-35 by
    tests/golden/estimators_modal.npz): the boolean mask and mode = x * mask, both exact (comparisons + one multiply)."""
    from stereo_toolbox_amd.utils import synthetic_modal_volume, synthetic_tensor
    B, D, H, W, seed = case
    x = synthetic_modal_volume(B, D, H, W, seed) if seed else torch.softmax(synthetic_tensor((B, D, H, W), 13) * 4, 1)
    mode = be.empty(B, D, H * W)
    mask = be.empty(B, D, H * W, dtype=torch.uint8)
    mask.fill_(7)
    be.call("stx_split_mode", ptr(be.dev(x)), ptr(mode), ptr(mask), B, D, H * W)
    want_mode, want_mask = O.split_mode(x, D)
    assert torch.equal(mask.cpu().view(B, D, H, W), want_mask.to(torch.uint8))
    assert torch.equal(mode.cpu().view(B, D, H, W), want_mode)


@pytest.mark.parametrize("case", [(2, 32, 5, 9, 21), (1, 48, 4, 7, 22)])
def test_modal_estimators_backward(be, case):
    """stx_modal_fwd (+aux) / stx_modal_bwd vs autograd through the oracle (whose gradients are pinned to the
    reference's, tests/golden/estimators_modal.npz)."""
    from stereo_toolbox_amd.utils import synthetic_modal_volume, synthetic_tensor
    B, D, H, W, seed = case
    x = synthetic_modal_volume(B, D, H, W, seed)
    gy = synthetic_tensor((B, 1, H, W), 40 + seed)
    d = be.dev(x)
    for kind, ref in ((0, O.unimodal_disparity_estimator), (1, O.dominant_modal_disparity_estimator)):
        o, aux, gx = be.empty(B, H * W), be.empty(B, 5, H * W), be.empty(B, D, H * W)
        be.call("stx_modal_fwd", ptr(d), ptr(o), ptr(aux), B, D, H * W, kind)
        be.call("stx_modal_bwd", ptr(be.dev(gy)), ptr(o), ptr(aux), ptr(gx), B, D, H * W)
        xr = x.clone().requires_grad_()
        want = ref(xr, D)
        want.backward(gy)
        assert ((o.cpu() - want.detach().reshape(B, H * W)).abs() > 1e-4 * (1 + want.abs().max())).sum().item() == 0
        err = (gx.cpu().view_as(xr.grad) - xr.grad).abs()
        tol = 1e-4 * (1 + xr.grad.abs())
        bad_px = (err > tol).any(1).sum().item()          # a pixel whose mode choice flipped differs everywhere
        assert bad_px <= (0 if kind == 0 else B * H * W // 100), f"kind {kind}: {bad_px} pixels differ"


# ------------------------------------------------------------------------------ convolutions
def run_conv(be, x, w, ks, stride, scale=None, bias=None, res=None, relu=0, stats=False, mode=0, cout=None):
    B, Cin, D, H, W = x.shape
    Cout = cout if cout is not None else w.shape[0]
    wp = pack(be, w, mode)
    pad = ks // 2
    Do, Ho, Wo = [(d + 2 * pad - ks) // stride + 1 for d in (D, H, W)]
    out = be.empty(B, Do, Ho, Wo, Cout)
    rows = be.raw("stx_conv3d_fwd_stat_rows")(B, D, H, W, Cin, Cout, ks, stride)
    assert 0 < rows <= B * be.raw("stx_conv3d_fwd_blocks")(Do, Ho, Wo)
    st = be.empty(rows, 2, Cout).fill_(float("nan")) if stats else None       # (every row must be written)
    xl = be.dev(ndhwc(x))
    rl = be.dev(ndhwc(res)) if res is not None else None
    be.call("stx_conv3d_fwd", ptr(xl), ptr(wp), ptr(out), ptr(be.dev(scale)), ptr(be.dev(bias)), ptr(rl), ptr(st),
            B, D, H, W, Cin, Cout, ks, stride, relu)
    return ncdhw(out).cpu(), (st.cpu() if stats else None)


CONV_CASES = [
    # B, Cin, Cout, D, H, W, ks, stride
    (1, 32, 32, 3, 5, 37, 3, 1),
    (2, 32, 64, 4, 6, 40, 3, 2),
    (1, 64, 32, 2, 3, 33, 3, 1),
    (1, 40, 32, 2, 2, 20, 3, 1),     # ACVNet dres1_att_ (Cin=40 -> 8-channel K chunks)
    (1, 32, 1, 2, 4, 35, 3, 1),      # classifier tail Conv3d(32->1)
    (1, 64, 64, 3, 4, 34, 1, 1),     # redir 1x1x1
    (2, 32, 32, 3, 5, 37, 1, 1),     # redir 1x1x1 at 32 channels (hourglass redir1)
    (1, 32, 24, 2, 4, 21, 1, 1),     # ... with 24 output channels
    (1, 64, 64, 3, 5, 37, 3, 1),     # hourglass conv2
    (1, 64, 128, 4, 4, 24, 3, 2),
    (2, 32, 64, 7, 6, 40, 3, 1),     # march kernel, 2 column blocks (NT=2), ragged H/W, several D segments
    (1, 32, 32, 9, 3, 70, 3, 1),     # march kernel, long D, W spanning 5 16-wide tiles (8 x 16 columns)
    (1, 32, 32, 3, 9, 60, 3, 1),     # march kernel, 4 x 32 columns (W = 60 wastes the same either way), ragged H
    (2, 32, 64, 4, 6, 64, 3, 1),     # march kernel, 4 x 32 columns, NT=2
    (2, 32, 24, 5, 11, 21, 3, 1),    # march kernel, 24 of a slice's 32 output channels, ragged H / W, two batch items
    (2, 32, 64, 5, 16, 32, 3, 1),    # march kernel, whole 8 x 16 tiles (the raw whole-tile epilogue), two N slices
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv3d_fwd(be, case):
    B, Cin, Cout, D, H, W, ks, s = case
    torch.manual_seed(5)
    x = torch.randn(B, Cin, D, H, W)
    w = torch.randn(Cout, Cin, ks, ks, ks) * 0.1
    ref = F.conv3d(x, w, None, s, ks // 2)
    got, st = run_conv(be, x, w, ks, s, stats=True)
    _close(got, ref)
    _close(st[:, 0].sum(0), ref.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
    _close(st[:, 1].sum(0), (ref ** 2).sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
    sc, bs, res = torch.rand(Cout) + 0.5, torch.randn(Cout), torch.randn_like(ref)
    got2, _ = run_conv(be, x, w, ks, s, sc, bs, res, 1)
    ref2 = F.relu(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1) + res)
    _close(got2, ref2)
    got4, _ = run_conv(be, x, w, ks, s, sc, bs, None, 1)             # affine + ReLU without residual (march: straight-line epilogue)
    _close(got4, F.relu(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1)))
    got3, _ = run_conv(be, x, w, ks, s, sc, bs, res, 2)              # activation code 2: Mish in the epilogue
    _close(got3, F.mish(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1) + res), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("wn", [1, 2, 3, 4])
def test_conv3d_wave_grid_variants(be, tune, wn):
    """STX_CONV_WN: the implicit-GEMM 3x3x3 kernels with their four waves arranged (4 / WN rows groups) x (WN column-block groups)
    -- 64 output channels: one row x two blocks (1) or two rows x one block (2, default; also 3, 4); 128 output channels
    (pipelined kernel): 2 x 2 (3) or 4 x 1 (4).  Every arrangement against the reference convolution, statistics rows
    included, ragged edges."""
    tune("STX_CONV_WN", wn)
    torch.manual_seed(11)
    for B, Cin, Cout, D, H, W, s in ((1, 64, 64, 3, 5, 37, 1), (2, 32, 64, 5, 6, 70, 2), (1, 128, 128, 3, 4, 33, 1),
                                    (1, 64, 128, 4, 6, 66, 2), (1, 64, 48, 2, 3, 20, 1)):
        x = torch.randn(B, Cin, D, H, W)
        w = torch.randn(Cout, Cin, 3, 3, 3) * 0.1
        ref = F.conv3d(x, w, None, s, 1)
        got, st = run_conv(be, x, w, 3, s, stats=True)
        _close(got, ref)
        _close(st[:, 0].sum(0), ref.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
        _close(st[:, 1].sum(0), (ref ** 2).sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
        sc, bs, res = torch.rand(Cout) + 0.5, torch.randn(Cout), torch.randn_like(ref)
        got2, _ = run_conv(be, x, w, 3, s, sc, bs, res, 1)
        _close(got2, F.relu(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1) + res))


def test_conv3d_64_64_on_the_march_kernel(be, tune):
    """STX_CONV_L1_MARCH: the 64 -> 64 3x3x3 stride-1 layers (hourglass conv2 and its data gradient) as 2 x 2 channel slices
    of the march kernel -- K slices accumulate through the output tensor, the epilogue (BN statistics, affine, residual,
    activation) runs in the last one."""
    tune("STX_CONV_L1_MARCH", 1)
    torch.manual_seed(5)
    for B, D, H, W in ((1, 3, 5, 37), (2, 5, 8, 16)):
        x = torch.randn(B, 64, D, H, W)
        w = torch.randn(64, 64, 3, 3, 3) * 0.1
        ref = F.conv3d(x, w, None, 1, 1)
        got, st = run_conv(be, x, w, 3, 1, stats=True)
        _close(got, ref)
        _close(st[:, 0].sum(0), ref.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
        _close(st[:, 1].sum(0), (ref ** 2).sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
        sc, bs, res = torch.rand(64) + 0.5, torch.randn(64), torch.randn_like(ref)
        got2, _ = run_conv(be, x, w, 3, 1, sc, bs, res, 1)
        _close(got2, F.relu(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1) + res))
        got3, _ = run_conv(be, x, w, 3, 1, sc, bs, None, 1)
        _close(got3, F.relu(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1)))


@pytest.mark.parametrize("dense", [1, 0])
def test_conv3d_stride2_lds_tile_layouts(be, dense, tune):
    """Stride-2 32 -> 64 convolution (the first convolution of every hourglass) with the un-padded LDS tile (default,
    STX_CONV_S2_DENSE=1) and with the padded one: same results, ragged H / W / D included."""
    tune("STX_CONV_S2_DENSE", dense)
    torch.manual_seed(15)
    for B, D, H, W in ((1, 5, 6, 45), (2, 4, 4, 70)):
        x = torch.randn(B, 32, D, H, W)
        w = torch.randn(64, 32, 3, 3, 3) * 0.1
        ref = F.conv3d(x, w, None, 2, 1)
        got, st = run_conv(be, x, w, 3, 2, stats=True)
        _close(got, ref)
        _close(st[:, 0].sum(0), ref.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("case", [(1, 64, 32, 2, 3, 33), (2, 128, 64, 2, 4, 20), (1, 32, 32, 1, 2, 40)])
def test_deconv3d_fwd(be, case):
    B, Cin, Cout, D, H, W = case
    torch.manual_seed(6)
    x = torch.randn(B, Cin, D, H, W)
    w = torch.randn(Cin, Cout, 3, 3, 3) * 0.1
    ref = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)
    wp = pack(be, w, 2)
    out = be.empty(B, 2 * D, 2 * H, 2 * W, Cout)
    nb = be.raw("stx_deconv3d_fwd_blocks")(D, H, W)
    st = be.empty(B * nb, 2, Cout)
    xl = be.dev(ndhwc(x))
    be.call("stx_deconv3d_fwd", ptr(xl), ptr(wp), ptr(out), None, None, None, ptr(st), B, D, H, W, Cin, Cout,
            2 * D, 2 * H, 2 * W, 0)
    _close(ncdhw(out), ref)
    _close(st.cpu()[:, 0].sum(0), ref.sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
    sc, bs, res = torch.rand(Cout) + 0.5, torch.randn(Cout), torch.randn_like(ref)
    rl = be.dev(ndhwc(res))
    be.call("stx_deconv3d_fwd", ptr(xl), ptr(wp), ptr(out), ptr(be.dev(sc)), ptr(be.dev(bs)), ptr(rl), None,
            B, D, H, W, Cin, Cout, 2 * D, 2 * H, 2 * W, 1)
    _close(ncdhw(out), F.relu(ref * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1) + res))


def test_dgrad_via_repacked_weights(be):
    torch.manual_seed(7)
    # stride-1 conv dgrad = stride-1 conv of dy with flipped/transposed weights (pack mode 1)
    x = torch.randn(1, 32, 3, 4, 33, requires_grad=True)
    w = torch.randn(64, 32, 3, 3, 3) * 0.1
    y = F.conv3d(x, w, None, 1, 1)
    gy = torch.randn_like(y)
    y.backward(gy)
    got, _ = run_conv(be, gy, w, 3, 1, mode=1, cout=32)
    _close(got, x.grad)
    # stride-2 conv dgrad = transposed-conv kernel on the conv weight (pack mode 2)
    x = torch.randn(1, 32, 4, 4, 40, requires_grad=True)
    y = F.conv3d(x, w, None, 2, 1)
    gy = torch.randn_like(y)
    y.backward(gy)
    wp = pack(be, w, 2)
    out = be.empty(1, 4, 4, 40, 32)
    be.call("stx_deconv3d_fwd", ptr(be.dev(ndhwc(gy))), ptr(wp), ptr(out), None, None, None, None, 1, 2, 2, 20, 64, 32,
            4, 4, 40, 0)
    _close(ncdhw(out), x.grad)
    # transposed-conv dgrad = stride-2 conv of dy with the deconv weight read as [Cout'][Cin'] (mode 0)
    x = torch.randn(1, 64, 2, 2, 20, requires_grad=True)
    wt = torch.randn(64, 32, 3, 3, 3) * 0.1
    y = F.conv_transpose3d(x, wt, None, stride=2, padding=1, output_padding=1)
    gy = torch.randn_like(y)
    y.backward(gy)
    got, _ = run_conv(be, gy, wt, 3, 2, mode=0, cout=64)
    _close(got, x.grad)


def run_wgrad(be, fine, coarse, ks, stride):
    B, CF, Df, Hf, Wf = fine.shape
    _, CC, Dc, Hc, Wc = coarse.shape
    n = be.raw("stx_conv3d_wgrad_workspace_floats")(B, Dc, Hc, Wc, CF, CC, ks, stride)
    ws = be.empty(n)
    dw = be.empty(CC, CF, ks ** 3)
    be.call("stx_conv3d_wgrad", ptr(be.dev(ndhwc(fine))), ptr(be.dev(ndhwc(coarse))), ptr(dw), ptr(ws), B, Df, Hf, Wf,
            CF, Dc, Hc, Wc, CC, ks, stride)
    return dw.cpu()


@pytest.mark.parametrize("case", [(1, 32, 32, 3, 5, 37, 3, 1), (1, 32, 32, 2, 3, 60, 3, 1), (2, 32, 64, 4, 6, 40, 3, 2), (1, 64, 64, 3, 4, 34, 1, 1),
                                  (2, 64, 64, 3, 5, 37, 3, 1), (1, 64, 64, 2, 3, 60, 3, 1),     # four channel-block pairs: un-pipelined staging, 4 x 16 / 2 x 32 tiles
                                  (1, 64, 128, 3, 7, 21, 3, 2), (2, 32, 32, 6, 8, 64, 3, 2), (1, 32, 64, 5, 10, 70, 3, 2),   # stride 2: odd / even fine extents
                                  (2, 32, 32, 5, 9, 37, 3, 1), (1, 32, 64, 4, 4, 16, 3, 1)])      # ragged H / W tiles, batch 2; exact tiles
@pytest.mark.parametrize("march", [3, 0], ids=["march", "tile_kernel"])
def test_conv3d_wgrad(be, case, tune, march):
    B, Cin, Cout, D, H, W, ks, s = case
    if march == 0 and ks != 3:
        pytest.skip("STX_WGRAD_MARCH only selects among the 3x3x3 kernels")
    tune("STX_WGRAD_MARCH", march)
    torch.manual_seed(8)
    x = torch.randn(B, Cin, D, H, W)
    w = (torch.randn(Cout, Cin, ks, ks, ks) * 0.1).requires_grad_()
    y = F.conv3d(x, w, None, s, ks // 2)
    gy = torch.randn_like(y)
    y.backward(gy)
    _close(run_wgrad(be, x, gy, ks, s).view_as(w), w.grad)


@pytest.mark.parametrize("case", [(1, 32, 32, 3, 5, 37, 1), (2, 64, 32, 2, 9, 21, 1), (1, 32, 64, 3, 4, 16, 0), (1, 64, 64, 5, 6, 40, 1)])
def test_conv3d_wgrad_bn(be, tune, case):
    """stx_conv3d_wgrad_bn (weight gradient of a 3x3x3 stride-1 conv taking the gradient BEHIND its train-mode BatchNorm + ReLU,
    dz formed inside the march kernel) vs the two-launch pipeline it replaces: stx_bn_bwd_apply2 -> stx_conv3d_wgrad.  dz to a
    few ulp (the same expression, contracted by two compilers' schedules), dw like any weight gradient.  Ragged tiles, two
    input-channel blocks (dz written once), several steps per workgroup, no activation."""
    B, Cin, Cout, D, H, W, act = case
    tune("STX_WGRAD_GRID", 3)
    torch.manual_seed(12)
    nvox = B * D * H * W
    x = torch.randn(B, D, H, W, Cin)
    z = torch.randn(B, D, H, W, Cout)
    gy = torch.randn(B, D, H, W, Cout)
    scale, shift = torch.randn(Cout), torch.randn(Cout) * 0.3
    mean, invstd, gamma = torch.randn(Cout) * 0.2, torch.rand(Cout) + 0.5, torch.rand(Cout) + 0.5
    dx, dz_in, dgy = be.dev(x), be.dev(z), be.dev(gy)
    dsc, dsh, dm, di, dgm = (be.dev(t) for t in (scale, shift, mean, invstd, gamma))
    NB = be.raw("stx_bn_reduce_blocks")()
    part, sums = be.empty(NB, 3, Cout), be.empty(3, Cout)
    be.call("stx_bn_bwd_reduce2", ptr(dgy), None, ptr(dz_in), ptr(dm), ptr(di), None, None, None, ptr(dsc), ptr(dsh), None, None,
            ptr(part), ptr(sums), nvox, Cout, act, 1)
    dz_ref = be.empty(B, D, H, W, Cout)
    be.call("stx_bn_bwd_apply2", ptr(dgy), None, ptr(dz_in), ptr(dm), ptr(di), ptr(dgm), None, None, None, None, ptr(dsc),
            ptr(dsh), None, None, ptr(sums), ptr(dz_ref), None, None, nvox, Cout, act, 1)
    n = be.raw("stx_conv3d_wgrad_workspace_floats")(B, D, H, W, Cin, Cout, 3, 1)
    ws = be.empty(n)
    dw_ref = be.empty(Cout, Cin, 27)
    be.call("stx_conv3d_wgrad", ptr(dx), ptr(dz_ref), ptr(dw_ref), ptr(ws), B, D, H, W, Cin, D, H, W, Cout, 3, 1)
    assert be.raw("stx_conv3d_wgrad_bn_supported")(B, D, H, W, Cin, Cout) == 1
    dz, dw = be.empty(B, D, H, W, Cout), be.empty(Cout, Cin, 27)
    dz.fill_(float("nan"))
    be.call("stx_conv3d_wgrad_bn", ptr(dx), ptr(dgy), ptr(dz_in), ptr(dsc), ptr(dsh), ptr(dm), ptr(di), ptr(dgm), ptr(sums),
            1.0 / nvox, act, ptr(dz), ptr(dw), ptr(ws), B, D, H, W, Cin, Cout)
    _close(dz, dz_ref.cpu(), rtol=1e-5, atol=1e-6)
    _close(dw, dw_ref.cpu(), rtol=2e-4, atol=2e-4)
    # and against autograd through conv3d on the CPU (the gradient the pair of launches stands for)
    w0 = torch.zeros(Cout, Cin, 3, 3, 3, requires_grad=True)
    F.conv3d(x.permute(0, 4, 1, 2, 3), w0, None, 1, 1).backward(dz_ref.cpu().permute(0, 4, 1, 2, 3))
    _close(dw.view_as(w0), w0.grad, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("march", [3, 0], ids=["march", "tile_kernel"])
def test_conv3d_wgrad_many_tiles_per_workgroup(be, tune, march):
    """The weight-gradient kernels' tile loop with several tiles per workgroup (STX_WGRAD_GRID caps the split-K workgroups; at
    the small test shapes every workgroup otherwise gets one tile): odd and even tile counts, stride 1 and 2.  March kernel:
    runs of several columns per workgroup, cut INSIDE a column (the window is rebuilt there), rolling plane buffers over
    more than four steps."""
    tune("STX_WGRAD_MARCH", march)
    torch.manual_seed(8)
    for grid, (B, Cin, Cout, D, H, W, s) in ((1, (1, 32, 32, 3, 5, 37, 1)), (4, (2, 32, 64, 2, 9, 21, 1)), (5, (1, 64, 32, 3, 7, 40, 1)),
                                             (3, (1, 32, 64, 4, 6, 40, 2)), (3, (1, 32, 32, 7, 8, 20, 1)), (2, (1, 32, 32, 9, 4, 16, 1)),
                                             (2, (1, 32, 32, 13, 8, 32, 2)), (1, (2, 32, 32, 6, 18, 40, 2))):
        tune("STX_WGRAD_GRID", grid)
        x = torch.randn(B, Cin, D, H, W)
        w = (torch.randn(Cout, Cin, 3, 3, 3) * 0.1).requires_grad_()
        y = F.conv3d(x, w, None, s, 1)
        gy = torch.randn_like(y)
        y.backward(gy)
        _close(run_wgrad(be, x, gy, 3, s).view_as(w), w.grad)


@pytest.mark.parametrize("march", [3, 0], ids=["march", "tile_kernel"])
@pytest.mark.parametrize("shape", [(1, 64, 32, 2, 3, 20), (2, 32, 32, 3, 5, 18)])
def test_deconv3d_wgrad(be, tune, march, shape):
    tune("STX_WGRAD_MARCH", march)
    torch.manual_seed(9)
    B, Cin, Cout, D, H, W = shape
    x = torch.randn(B, Cin, D, H, W)
    w = (torch.randn(Cin, Cout, 3, 3, 3) * 0.1).requires_grad_()
    y = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)
    gy = torch.randn_like(y)
    y.backward(gy)
    _close(run_wgrad(be, gy, x, 3, 2).view_as(w), w.grad)


@pytest.mark.parametrize("case", [(1, 32, 3, 5, 37), (2, 16, 2, 4, 32), (1, 64, 2, 9, 40), (2, 32, 7, 11, 40)])
def test_conv3d_c1_fwd_wgrad(be, case):
    """Classifier tail Conv3d(Cin, 1, 3, padding=1) on the dedicated VALU kernels."""
    B, Cin, D, H, W = case
    torch.manual_seed(11)
    x = torch.randn(B, Cin, D, H, W)
    w = (torch.randn(1, Cin, 3, 3, 3) * 0.1).requires_grad_()
    res = torch.randn(B, 1, D, H, W)
    y = F.conv3d(x, w, None, 1, 1)
    gy = torch.randn_like(y)
    y.backward(gy)
    xl = be.dev(ndhwc(x))
    out = be.empty(B, D, H, W)
    be.call("stx_conv3d_c1_fwd", ptr(xl), ptr(be.dev(w.detach())), None, ptr(out), B, D, H, W, Cin)
    _close(out, y.detach().squeeze(1))
    be.call("stx_conv3d_c1_fwd", ptr(xl), ptr(be.dev(w.detach())), ptr(be.dev(res)), ptr(out), B, D, H, W, Cin)
    _close(out, (y.detach() + res).squeeze(1))
    ws = be.empty(be.raw("stx_conv3d_c1_wgrad_workspace_floats")(Cin))
    dw = be.empty(1, Cin, 27)
    be.call("stx_conv3d_c1_wgrad", ptr(xl), ptr(be.dev(gy)), ptr(dw), ptr(ws), B, D, H, W, Cin)
    _close(dw.view_as(w), w.grad)
    xg = x.clone().requires_grad_()
    F.conv3d(xg, w.detach(), None, 1, 1).backward(gy)
    gx = be.empty(B, D, H, W, Cin)
    be.call("stx_conv3d_c1_dgrad", ptr(be.dev(gy)), ptr(be.dev(w.detach())), ptr(gx), B, D, H, W, Cin)
    _close(ncdhw(gx), xg.grad)


def test_mish(be):
    """Mish forward / backward vs torch (the reference's x * tanh(softplus(x)))."""
    torch.manual_seed(21)
    x = torch.cat((torch.randn(2, 3, 4, 5, 8) * 3, torch.tensor([-30., -5., 0., 5., 19.9, 20.1, 30., 1e-3]).repeat(2, 3, 4, 5, 1)), 0)
    xr = x.clone().requires_grad_()
    y = xr * torch.tanh(F.softplus(xr))
    g = torch.randn_like(x)
    y.backward(g)
    dx = be.dev(x)
    out = be.empty(*x.shape)
    be.call("stx_mish_fwd", ptr(dx), ptr(out), x.numel())
    _close(out, y.detach(), rtol=1e-5, atol=1e-6)
    gx = be.empty(*x.shape)
    be.call("stx_mish_bwd", ptr(be.dev(g)), ptr(dx), ptr(gx), x.numel())
    _close(gx, xr.grad, rtol=1e-5, atol=1e-6)


def test_modal_estimators_edge_cases(be):
    """Degenerate volumes: flat, one-hot at either end (a one-hot 1.0 in the last bin has no rising edge to its right, the
    support is empty and the reference returns 0/0 = NaN), a plateau around the maximum, zeros."""
    D = 12
    x = torch.zeros(6, D, 1, 4)
    x[0] = 1.0 / D                                   # flat
    x[1, 0] = 1.0                                    # one-hot at d = 0
    x[2, D - 1] = 1.0                                # one-hot at d = D-1 -> NaN
    x[3, 4:7] = 1.0 / 3                              # plateau (arg-max = first of the plateau)
    x[4, 2], x[4, 9] = 0.6, 0.4                      # two spikes
    x[5] = 0.0                                       # all zeros -> NaN
    x = x + torch.linspace(0, 1e-6, 4).view(1, 1, 1, 4) * (x > 0)      # distinct pixels
    d = be.dev(x)
    for entry, ref in (("stx_unimodal_fwd", O.unimodal_disparity_estimator),
                       ("stx_dominant_modal_fwd", O.dominant_modal_disparity_estimator)):
        o = be.empty(6, 4)
        be.call(entry, ptr(d), ptr(o), 6, D, 4)
        want = ref(x, D).reshape(6, 4)
        got = o.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (entry, got, want)
        ok = ~torch.isnan(want)
        assert (got[ok] - want[ok]).abs().max().item() < 1e-5, (entry, got, want)


# ------------------------------------------------------------------------------ ACVNet extras
def test_dwconv_hw_fwd_bwd(be):
    """Depth-wise (1,3,3) patch convolutions with per-channel dilation (acv.py:109-112,183-187)."""
    torch.manual_seed(12)
    B, C, D, H, W = 1, 40, 3, 7, 13
    x = torch.randn(B, C, D, H, W, requires_grad=True)
    w1 = torch.randn(8, 1, 1, 3, 3, requires_grad=True)
    w2 = torch.randn(16, 1, 1, 3, 3, requires_grad=True)
    w3 = torch.randn(16, 1, 1, 3, 3, requires_grad=True)
    ref = torch.cat((F.conv3d(x[:, :8], w1, None, 1, (0, 1, 1), 1, 8), F.conv3d(x[:, 8:24], w2, None, 1, (0, 2, 2), 2, 16),
                     F.conv3d(x[:, 24:40], w3, None, 1, (0, 3, 3), 3, 16)), 1)
    gy = torch.randn_like(ref)
    ref.backward(gy)
    wcat = torch.cat((w1.detach().reshape(8, 9), w2.detach().reshape(16, 9), w3.detach().reshape(16, 9)), 0)
    dil = torch.tensor([1] * 2 + [2] * 4 + [3] * 4, dtype=torch.int32)
    xl, gl, dw_, dd = be.dev(ndhwc(x.detach())), be.dev(ndhwc(gy)), be.dev(wcat), be.dev(dil)
    out = be.empty(B, D, H, W, C)
    be.call("stx_dwconv_hw_fwd", ptr(xl), ptr(dw_), ptr(dd), ptr(out), B, D, H, W, C, 0)
    _close(ncdhw(out), ref.detach(), rtol=1e-5)
    gx = be.empty(B, D, H, W, C)
    be.call("stx_dwconv_hw_fwd", ptr(gl), ptr(dw_), ptr(dd), ptr(gx), B, D, H, W, C, 1)
    _close(ncdhw(gx), x.grad, rtol=1e-5)
    ws = be.empty(be.raw("stx_dwconv_hw_wgrad_workspace_floats")(C))
    gw = be.empty(C, 9)
    be.call("stx_dwconv_hw_wgrad", ptr(xl), ptr(gl), ptr(dd), ptr(gw), ptr(ws), B, D, H, W, C)
    gref = torch.cat((w1.grad.reshape(8, 9), w2.grad.reshape(16, 9), w3.grad.reshape(16, 9)), 0)
    _close(gw, gref, rtol=1e-4)


@pytest.mark.parametrize("shape", [(1, 40, 2, 19, 61), (2, 40, 1, 9, 50), (1, 8, 2, 33, 300), (1, 40, 1, 8, 7)])
def test_dwconv_hw_rolling_window(be, tune, shape):
    """The rolling-window form of the patch convolutions (round 5: strips of columns walking down the rows with eight rows
    in LDS) against the reference and against the cache-fed kernel of rounds 3-4 (STX_DWCONV_ROLL = 0): several strips, a
    ragged last strip, row segments, both tap orders (forward / data gradient), dilations 1-3, a 2-quad volume."""
    B, C, D, H, W = shape
    torch.manual_seed(21)
    x = torch.randn(B, C, D, H, W)
    CQ = C // 4
    dils = [1 + (q * 3) // CQ for q in range(CQ)]                       # quads with dilation 1, 2, 3
    wts = torch.randn(C, 9)
    ref = torch.cat([F.conv3d(x[:, 4 * q:4 * q + 4], wts[4 * q:4 * q + 4].view(4, 1, 1, 3, 3), None, 1, (0, dils[q], dils[q]),
                              dils[q], 4) for q in range(CQ)], 1)
    reff = torch.cat([F.conv3d(x[:, 4 * q:4 * q + 4], wts[4 * q:4 * q + 4].flip(1).view(4, 1, 1, 3, 3), None, 1,
                               (0, dils[q], dils[q]), dils[q], 4) for q in range(CQ)], 1)
    xl, dw_, dd = be.dev(ndhwc(x)), be.dev(wts), be.dev(torch.tensor(dils, dtype=torch.int32))
    outs = {}
    for roll in (1, 0):
        tune("STX_DWCONV_ROLL", roll)
        for flip, want in ((0, ref), (1, reff)):
            out = be.empty(B, D, H, W, C)
            be.call("stx_dwconv_hw_fwd", ptr(xl), ptr(dw_), ptr(dd), ptr(out), B, D, H, W, C, flip)
            _close(ncdhw(out), want, rtol=1e-5)
            outs[(roll, flip)] = out
    for flip in (0, 1):                                                  # same products, same order of the nine taps
        assert torch.equal(outs[(1, flip)], outs[(0, flip)])
    # weight gradient: the rolling-window form against autograd's, and against the cache-fed kernel
    xr, wr = x.clone().requires_grad_(), wts.clone().requires_grad_()
    gy = torch.randn_like(ref)
    torch.cat([F.conv3d(xr[:, 4 * q:4 * q + 4], wr[4 * q:4 * q + 4].view(4, 1, 1, 3, 3), None, 1, (0, dils[q], dils[q]), dils[q], 4)
               for q in range(CQ)], 1).backward(gy)
    gl = be.dev(ndhwc(gy))
    gws = {}
    for roll in (1, 0):
        tune("STX_DWCONV_ROLL", roll)
        ws = be.empty(be.raw("stx_dwconv_hw_wgrad_workspace_floats")(C))
        gw = be.empty(C, 9)
        be.call("stx_dwconv_hw_wgrad", ptr(xl), ptr(gl), ptr(dd), ptr(gw), ptr(ws), B, D, H, W, C)
        _close(gw, wr.grad, rtol=1e-4, atol=1e-4)
        gws[roll] = gw
    _close(gws[1], gws[0].cpu(), rtol=1e-5, atol=1e-4)


def test_ac_volume_backward(be):
    """Gradients of softmax(att)*concat_volume (acv.py:196) w.r.t. probabilities and features."""
    torch.manual_seed(13)
    B, Cc, H, W, D = 1, 8, 3, 21, 9
    Lc = torch.randn(B, Cc, H, W, requires_grad=True)
    Rc = torch.randn(B, Cc, H, W, requires_grad=True)
    prob = torch.rand(B, D, H, W, requires_grad=True)
    ref = prob.unsqueeze(1) * O.build_concat_volume(Lc, Rc, D, mask_left=False)
    gv = torch.randn(B, D, H, W, 2 * Cc)
    ref.backward(ncdhw(gv))
    dL, dR, dp, dgv = be.dev(Lc.detach()), be.dev(Rc.detach()), be.dev(prob.detach()), be.dev(gv)
    gp = be.empty(B, D, H, W)
    be.call("stx_cost_volume_scale_bwd", ptr(dgv), ptr(dL), ptr(dR), ptr(gp), B, Cc, H, W, D, 0)
    _close(gp, prob.grad, rtol=1e-5)
    scaled = be.empty(B, D, H, W, 2 * Cc)
    be.call("stx_scale_channels", ptr(dgv), ptr(dp), ptr(scaled), B * D * H * W, 2 * Cc)
    gL, gR = be.empty(B, Cc, H, W), be.empty(B, Cc, H, W)
    be.call("stx_cost_volume_bwd", ptr(scaled), None, None, 0, 0, Cc, None, None, ptr(gL), ptr(gR), B, H, W, D, 0)
    _close(gL, Lc.grad, rtol=1e-5)
    _close(gR, Rc.grad, rtol=1e-5)
    # the same three gradients from ONE pass over the gradient volume (several shapes: batch 2, W < D, 32 channels)
    for B, Cc, H, W, D in ((1, 8, 3, 21, 9), (2, 32, 2, 37, 12), (1, 4, 2, 7, 10)):
        Lc = torch.randn(B, Cc, H, W, requires_grad=True)
        Rc = torch.randn(B, Cc, H, W, requires_grad=True)
        prob = torch.rand(B, D, H, W, requires_grad=True)
        ref = prob.unsqueeze(1) * O.build_concat_volume(Lc, Rc, D, mask_left=False)
        gv = torch.randn(B, D, H, W, 2 * Cc)
        ref.backward(ncdhw(gv))
        g1, g2, g3 = be.empty(B, Cc, H, W), be.empty(B, Cc, H, W), be.empty(B, D, H, W)
        be.call("stx_ac_volume_bwd", ptr(be.dev(gv)), ptr(be.dev(Lc.detach())), ptr(be.dev(Rc.detach())), ptr(be.dev(prob.detach())),
                ptr(g1), ptr(g2), ptr(g3), B, Cc, H, W, D, 0)
        _close(g1, Lc.grad, rtol=1e-5)
        _close(g2, Rc.grad, rtol=1e-5)
        _close(g3, prob.grad, rtol=1e-5)


# ------------------------------------------------------------------------------ CFNet sampled (cascade) volume
@pytest.mark.parametrize("variant", ["lds_window", "global_atomics"])
@pytest.mark.parametrize("case", [(1, 40, 4, 12, 5, 70, 6), (2, 20, 4, 6, 3, 33, 4), (1, 8, 8, 0, 2, 64, 3), (1, 0, 0, 8, 2, 20, 5),
                                  (1, 8, 4, 4, 2, 200, 3), (1, 40, 8, 12, 1, 66, 2)])
def test_sampled_volume_fwd_bwd(be, case, variant, tune):
    """stx_sampled_volume_fwd / _bwd against the oracle's restatement of SpatialTransformer + groupwise_correlation_4D +
    cost_volume_generator + cat (CFNet/submodule.py:306-350, 163-169, cfnet.py:470-497, 560-566): CFNet's two stage
    configurations (40 groups x 4 channels + 12 concat; 20 x 4 + 6), 8 channels per group, concat only; W = 70 / 33 leave
    a ragged 64-column tile; hypotheses reach outside the image on both sides (clamped index, zeroed contribution).
    Backward in both forms: right-feature gradients through the workgroup's LDS window (W = 200 with hypotheses up to 150
    columns puts many gather columns left of the 96-column window -> its global-atomic fallback; 320 + 12 channels split
    the groups over two workgroups) and with global atomics only (STX_SV_BWD_V1)."""
    tune("STX_SV_BWD_V1", 1 if variant == "global_atomics" else 0)
    B, G, cpg, Cc, H, W, S = case
    torch.manual_seed(11)
    Cg = G * cpg
    Lg, Rg = (torch.randn(B, Cg, H, W).requires_grad_() if G else None for _ in range(2))
    Lc, Rc = (torch.randn(B, Cc, H, W).requires_grad_() if Cc else None for _ in range(2))
    samples = torch.randint(-4, 150 if W == 200 else W // 2, (B, S, H, W)).float()
    parts = []
    if G:
        parts.append(O.cf_sampled_volume(Lg, Rg, samples, G))
    if Cc:
        parts.append(O.cf_sampled_volume(Lc, Rc, samples, None))
    parts.append(samples.unsqueeze(1))
    ref = torch.cat(parts, 1)                                   # [B, CT, S, H, W]
    CT = ref.shape[1]
    CTp = (CT + 7) // 8 * 8
    dev = [be.dev(t.detach()) if t is not None else None for t in (Lg, Rg, Lc, Rc)]
    dsm = be.dev(samples)
    vol = be.empty(B, S, H, W, CTp)
    vol.fill_(7.0)
    be.call("stx_sampled_volume_fwd", ptr(dev[0]), ptr(dev[1]), Cg, G, ptr(dev[2]), ptr(dev[3]), Cc, ptr(dsm), ptr(vol),
            B, H, W, S, CTp)
    got = vol.cpu()
    _close(got[..., :CT].permute(0, 4, 1, 2, 3), ref.detach(), rtol=1e-5, atol=1e-6)
    assert torch.equal(got[..., CT:], torch.zeros(B, S, H, W, CTp - CT))
    assert torch.equal(got[..., CT - 1], samples)
    gv = torch.randn(B, S, H, W, CTp)
    ref.backward(gv[..., :CT].permute(0, 4, 1, 2, 3))
    outs = [be.empty(*t.shape) if t is not None else None for t in (Lg, Rg, Lc, Rc)]
    for o in outs:
        if o is not None:
            o.fill_(3.0)                                          # (the entry point zeroes the atomically accumulated ones)
    be.call("stx_sampled_volume_bwd", ptr(be.dev(gv)), ptr(dev[0]), ptr(dev[1]), Cg, G, Cc, ptr(dsm), ptr(outs[0]),
            ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), B, H, W, S, CTp)
    for o, t in zip(outs, (Lg, Rg, Lc, Rc)):
        if t is not None:
            _close(o, t.grad, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------ batch norm
@pytest.mark.parametrize("two", [False, True])
def test_bn_mish_fused_fwd_bwd(be, two):
    """Activation code 2 of the BatchNorm passes (PCWNet / CFNet blocks in train mode): y = Mish(BN1(z1) [+ BN2(z2)]) from
    stx_bn_apply, gradients from stx_bn_bwd_reduce2 / _apply2, which differentiate Mish at the pre-activation value they
    recompute from z and the forward pass's scale / shift vectors -- against torch autograd of batch_norm + F.mish."""
    nvox, C = 900, 32
    torch.manual_seed(12)
    z1 = (torch.randn(nvox, C) * 2 + 1).requires_grad_()
    z2 = (torch.randn(nvox, C) + 0.5).requires_grad_() if two else None
    g1, b1 = (torch.rand(C) + 0.5).requires_grad_(), torch.randn(C).requires_grad_()
    g2, b2 = (torch.rand(C) + 0.5).requires_grad_(), torch.randn(C).requires_grad_()
    pre = F.batch_norm(z1, None, None, g1, b1, True, 0.1, 1e-5)
    if two:
        pre = pre + F.batch_norm(z2, None, None, g2, b2, True, 0.1, 1e-5)
    yr = F.mish(pre)

    def fin(z, g, b):
        chunks = z.detach().chunk(5)
        part = be.dev(torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in chunks]))
        outs = [be.empty(C) for _ in range(4)]
        be.call("stx_bn_finalize", ptr(part), len(chunks), C, float(nvox), ptr(be.dev(g.detach())), ptr(be.dev(b.detach())),
                None, None, 0.1, 1e-5, *[ptr(o) for o in outs])
        return outs

    sc1, sh1, m1, i1 = fin(z1, g1, b1)
    sc2 = sh2 = m2 = i2 = None
    if two:
        sc2, sh2, m2, i2 = fin(z2, g2, b2)
    d1, d2 = be.dev(z1.detach()), (be.dev(z2.detach()) if two else None)
    out = be.empty(nvox, C)
    be.call("stx_bn_apply", ptr(d1), ptr(sc1), ptr(sh1), ptr(d2), ptr(sc2), ptr(sh2), ptr(out), nvox, C, 2, 1)
    _close(out, yr.detach(), rtol=1e-5, atol=1e-5)
    gy = torch.randn(nvox, C)
    yr.backward(gy)
    dgy = be.dev(gy)
    NB = be.raw("stx_bn_reduce_blocks")()
    part, sums = be.empty(NB, 3, C), be.empty(3, C)
    be.call("stx_bn_bwd_reduce2", ptr(dgy), None, ptr(d1), ptr(m1), ptr(i1), ptr(d2), ptr(m2), ptr(i2), ptr(sc1), ptr(sh1),
            ptr(sc2), ptr(sh2), ptr(part), ptr(sums), nvox, C, 2, 1)
    dz1, dz2 = be.empty(nvox, C), (be.empty(nvox, C) if two else None)
    be.call("stx_bn_bwd_apply2", ptr(dgy), None, ptr(d1), ptr(m1), ptr(i1), ptr(be.dev(g1.detach())), ptr(d2), ptr(m2), ptr(i2),
            ptr(be.dev(g2.detach())) if two else None, ptr(sc1), ptr(sh1), ptr(sc2), ptr(sh2), ptr(sums), ptr(dz1), ptr(dz2), None,
            nvox, C, 2, 1)
    _close(dz1, z1.grad, rtol=1e-4, atol=1e-5)
    _close(sums[1], g1.grad, rtol=1e-4, atol=1e-4)
    _close(sums[0], b1.grad, rtol=1e-4, atol=1e-4)
    if two:
        _close(dz2, z2.grad, rtol=1e-4, atol=1e-5)
        _close(sums[2], g2.grad, rtol=1e-4, atol=1e-4)
    from stereo_toolbox_amd._capi import StxError
    with pytest.raises(StxError):          # Mish cannot be differentiated from the activated output
        be.call("stx_bn_bwd_reduce2", ptr(dgy), ptr(out), ptr(d1), ptr(m1), ptr(i1), ptr(d2), ptr(m2), ptr(i2), ptr(sc1), ptr(sh1),
                ptr(sc2), ptr(sh2), ptr(part), ptr(sums), nvox, C, 2, 1)


@pytest.mark.parametrize("case", [(1500, 32), (300, 64), (100, 32), (257, 20)])
def test_bn_finalize_many_rows(be, case):
    """stx_bn_finalize with as many partial rows as the L0 convolutions emit (the channel-quad kernel serves
    C % 4 == 0 and >= 256 rows, the first-generation kernel the rest): both against an fp64 evaluation."""
    nrows, C = case
    torch.manual_seed(5)
    part = torch.randn(nrows, 2, C)
    part[:, 1] = part[:, 1].abs() * 40 + 50          # sum z^2 comfortably above (sum z)^2 / n
    count = float(nrows * 64)
    g, b = torch.rand(C) + 0.5, torch.randn(C)
    rm, rv = torch.randn(C), torch.rand(C) + 0.5
    s1, s2 = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp(min=0)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    drm, drv = be.dev(rm.clone()), be.dev(rv.clone())      # (the emulator backend works on the host tensor itself)
    outs = [be.empty(C) for _ in range(4)]
    be.call("stx_bn_finalize", ptr(be.dev(part)), nrows, C, count, ptr(be.dev(g)), ptr(be.dev(b)), ptr(drm), ptr(drv),
            0.1, 1e-5, *[ptr(o) for o in outs])
    sc, sh, m, i = outs
    _close(m, mean.float(), rtol=1e-6, atol=1e-7)
    _close(i, invstd.float(), rtol=1e-6, atol=1e-7)
    _close(sc, (g.double() * invstd).float(), rtol=1e-6, atol=1e-7)
    _close(sh, (b.double() - mean * g.double() * invstd).float(), rtol=1e-5, atol=1e-6)
    _close(drm, (0.9 * rm.double() + 0.1 * mean).float(), rtol=1e-6, atol=1e-7)
    _close(drv, (0.9 * rv.double() + 0.1 * var * count / (count - 1)).float(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("case", [(1000, 32, False, True, False), (777, 64, True, True, False),
                                  (500, 32, False, False, True), (640, 128, False, True, True)])
def test_bn_train_fwd_bwd(be, case):
    nvox, C, two, relu, resid = case
    torch.manual_seed(10)
    z1 = (torch.randn(nvox, C) * 2 + 1).requires_grad_()
    z2 = (torch.randn(nvox, C) + 0.5).requires_grad_() if (two or resid) else None
    g1, b1 = (torch.rand(C) + 0.5).requires_grad_(), torch.randn(C).requires_grad_()
    g2, b2 = (torch.rand(C) + 0.5).requires_grad_(), torch.randn(C).requires_grad_()
    rm, rv = torch.randn(C), torch.rand(C) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    yr = F.batch_norm(z1, rm_ref, rv_ref, g1, b1, True, 0.1, 1e-5)
    if two:
        yr = yr + F.batch_norm(z2, None, None, g2, b2, True, 0.1, 1e-5)
    elif resid:
        yr = yr + z2
    if relu:
        yr = F.relu(yr)

    def fin(z, g, b, rmd, rvd):
        chunks = z.detach().chunk(7)
        part = be.dev(torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in chunks]))
        outs = [be.empty(C) for _ in range(4)]
        be.call("stx_bn_finalize", ptr(part), len(chunks), C, float(nvox), ptr(be.dev(g.detach())),
                ptr(be.dev(b.detach())), ptr(rmd), ptr(rvd), 0.1, 1e-5, *[ptr(o) for o in outs])
        return outs

    drm, drv = be.dev(rm), be.dev(rv)
    sc1, sh1, m1, i1 = fin(z1, g1, b1, drm, drv)
    if two:
        sc2, sh2, m2, i2 = fin(z2, g2, b2, None, None)
    dz1_in = be.dev(z1.detach())
    dz2_in = be.dev(z2.detach()) if z2 is not None else None
    out = be.empty(nvox, C)
    be.call("stx_bn_apply", ptr(dz1_in), ptr(sc1), ptr(sh1), ptr(dz2_in), ptr(sc2) if two else None,
            ptr(sh2) if two else None, ptr(out), nvox, C, int(relu), 1)
    _close(out, yr.detach(), rtol=1e-5, atol=1e-5)
    _close(drm, rm_ref, rtol=1e-5, atol=1e-6)
    _close(drv, rv_ref, rtol=1e-5, atol=1e-6)

    gy = torch.randn(nvox, C)
    yr.backward(gy)
    dgy = be.dev(gy)
    NB = be.raw("stx_bn_reduce_blocks")()
    part, sums = be.empty(NB, 3, C), be.empty(3, C)
    be.call("stx_bn_bwd_reduce", ptr(dgy), ptr(out), ptr(dz1_in), ptr(m1), ptr(i1), ptr(dz2_in) if two else None,
            ptr(m2) if two else None, ptr(i2) if two else None, ptr(part), ptr(sums), nvox, C, int(relu))
    dz1 = be.empty(nvox, C)
    dz2 = be.empty(nvox, C) if two else None
    gout = be.empty(nvox, C) if resid else None
    be.call("stx_bn_bwd_apply", ptr(dgy), ptr(out), ptr(dz1_in), ptr(m1), ptr(i1), ptr(be.dev(g1.detach())),
            ptr(dz2_in) if two else None, ptr(m2) if two else None, ptr(i2) if two else None,
            ptr(be.dev(g2.detach())) if two else None, ptr(sums), ptr(dz1), ptr(dz2), ptr(gout), nvox, C, int(relu))
    _close(dz1, z1.grad, rtol=1e-4, atol=1e-5)
    _close(sums[1], g1.grad, rtol=1e-4, atol=1e-4)
    _close(sums[0], b1.grad, rtol=1e-4, atol=1e-4)
    if two:
        _close(dz2, z2.grad, rtol=1e-4, atol=1e-5)
        _close(sums[2], g2.grad, rtol=1e-4, atol=1e-4)
    if resid:
        _close(gout, z2.grad, rtol=1e-6, atol=1e-6)
    if relu and not resid:
        # the y-free entry points: ReLU mask recomputed from z1 / z2 and the forward pass's scale / shift -> identical results
        part2, sums2 = be.empty(NB, 3, C), be.empty(3, C)
        be.call("stx_bn_bwd_reduce2", ptr(dgy), None, ptr(dz1_in), ptr(m1), ptr(i1), ptr(dz2_in) if two else None,
                ptr(m2) if two else None, ptr(i2) if two else None, ptr(sc1), ptr(sh1), ptr(sc2) if two else None,
                ptr(sh2) if two else None, ptr(part2), ptr(sums2), nvox, C, 1, 1)
        assert torch.equal(sums2.cpu(), sums.cpu())
        dz1b = be.empty(nvox, C)
        dz2b = be.empty(nvox, C) if two else None
        be.call("stx_bn_bwd_apply2", ptr(dgy), None, ptr(dz1_in), ptr(m1), ptr(i1), ptr(be.dev(g1.detach())),
                ptr(dz2_in) if two else None, ptr(m2) if two else None, ptr(i2) if two else None,
                ptr(be.dev(g2.detach())) if two else None, ptr(sc1), ptr(sh1), ptr(sc2) if two else None,
                ptr(sh2) if two else None, ptr(sums2), ptr(dz1b), ptr(dz2b), None, nvox, C, 1, 1)
        assert torch.equal(dz1b.cpu(), dz1.cpu())
        if two:
            assert torch.equal(dz2b.cpu(), dz2.cpu())


# ------------------------------------------------------------------------------ 2-D feature CNN glue
@pytest.mark.parametrize("case", [(1000, 32), (37, 64), (5000, 128), (3, 16), (70000, 32)])
def test_bn_stats(be, case):
    """stx_bn_stats: per-workgroup (sum, sum of squares) rows of a channels-last activation -> the column sums are the
    batch statistics torch's BatchNorm2d computes (models/GwcNet/gwcnet.py:12-65 `convbn`)."""
    nvox, C = case
    torch.manual_seed(31)
    z = torch.randn(nvox, C) * 2 + 0.5
    rows = be.raw("stx_bn_stats_rows")(nvox, C)
    assert rows >= 1
    part = be.empty(rows, 2, C)
    be.call("stx_bn_stats", ptr(be.dev(z)), ptr(part), nvox, C, 1)
    p = part.cpu().double()
    _close(p[:, 0].sum(0).float(), z.double().sum(0).float(), rtol=1e-5, atol=1e-3)
    _close(p[:, 1].sum(0).float(), (z.double() ** 2).sum(0).float(), rtol=1e-5, atol=1e-3)


def test_conv3d_march_blocked_sums(be, tune):
    """Blocked fp32 accumulation in the weights-in-LDS march kernel (STX_MARCH_BS=1, the default): one accumulator per
    (output, input plane) -- three 288-term chunks instead of one 864-term chain.  Same convolution; the result must be
    CLOSER to an fp64 evaluation than the sequential chain's (STX_MARCH_BS=0)."""
    torch.manual_seed(5)
    for B, Cin, Cout, D, H, W in ((1, 32, 32, 7, 9, 37), (1, 64, 32, 4, 8, 33), (2, 32, 64, 5, 6, 40), (1, 32, 32, 2, 3, 20)):
        x = torch.randn(B, Cin, D, H, W)
        w = torch.randn(Cout, Cin, 3, 3, 3) * 0.1
        ref64 = F.conv3d(x.double(), w.double(), None, 1, 1)
        tune("STX_MARCH_BS", 1)
        got, st = run_conv(be, x, w, 3, 1, stats=True)
        _close(got, ref64.float())
        _close(st[:, 0].sum(0), ref64.float().sum((0, 2, 3, 4)), rtol=1e-4, atol=1e-3)
        tune("STX_MARCH_BS", 0)
        seq, _ = run_conv(be, x, w, 3, 1)
        _close(seq, ref64.float())
        e_blk = (got.double() - ref64).abs().mean().item()
        e_seq = (seq.double() - ref64).abs().mean().item()
        assert e_blk < 0.85 * e_seq, (e_blk, e_seq)


def test_conv3d_march_epilogues_agree(be, tune):
    """The straight-line epilogue of the march kernel (buffer-descriptor stores, validity bits; STX_MARCH_EPI=1, the default
    for launches without partial sums / residual / Mish) and the general one produce the same bits: outputs, BN partial
    sums, affine + ReLU; ragged tiles, sliced channels, several runs per workgroup."""
    torch.manual_seed(6)
    for B, Cin, Cout, D, H, W in ((1, 32, 32, 7, 9, 37), (2, 32, 64, 5, 6, 40), (1, 64, 32, 4, 8, 33), (2, 32, 24, 3, 11, 21),
                                  (1, 32, 32, 6, 8, 48)):
        x = torch.randn(B, Cin, D, H, W)
        w = torch.randn(Cout, Cin, 3, 3, 3) * 0.1
        sc, bs = torch.rand(Cout) + 0.5, torch.randn(Cout)
        outs = []
        for epi in (1, 0):
            tune("STX_MARCH_EPI", epi)
            raw, st = run_conv(be, x, w, 3, 1, stats=True)
            act, _ = run_conv(be, x, w, 3, 1, sc, bs, None, 1)
            res, _ = run_conv(be, x, w, 3, 1, sc, bs, torch.randn(B, Cout, D, H, W, generator=torch.Generator().manual_seed(3)), 1)
            outs.append((raw, st, act, res))
        for a_, b_ in zip(*outs):
            assert torch.equal(a_, b_)


@pytest.mark.parametrize("two", [False, True])
def test_bn_groups_match_separate_calls(be, two, monkeypatch):
    """BatchNorm passes with groups = 2 (the two views of the 2-D CNN in one batch, per-view statistics): bit-identical to
    two separate calls on the two halves -- forward output, running statistics (updated half after half), input
    gradients; gamma / beta gradients are the sums over the halves."""
    from stereo_toolbox_amd import ops
    from tests.emu_util import emu_product_path
    import contextlib
    torch.manual_seed(41)
    C, shape = 32, (4, 5, 7)                       # leading axis 4 = 2 views x batch 2
    z1 = (torch.randn(*shape, C) * 1.5 + 0.3)
    z2 = torch.randn(*shape, C) if two else None
    res = None if two else torch.randn(*shape, C)
    gy = torch.randn(*shape, C)

    def run(z1_, z2_, res_, gy_, groups, rm, rv):
        dev = be.device
        a = z1_.detach().clone().contiguous().to(dev).requires_grad_()
        b = z2_.detach().clone().contiguous().to(dev).requires_grad_() if z2_ is not None else None
        r = res_.detach().clone().contiguous().to(dev).requires_grad_() if res_ is not None else None
        g1, b1 = (torch.rand(C) + 0.5).to(dev).requires_grad_(), (torch.randn(C) * 0.1).to(dev).requires_grad_()
        nvox = a.numel() // C // groups
        st = {"training": True, "partials": ops.bn_stats(a.detach(), groups), "count": nvox, "running_mean": rm[0],
              "running_var": rv[0], "momentum": 0.1, "eps": 1e-5, "sync": None}
        st2 = None
        if b is not None:
            st2 = dict(st, partials=ops.bn_stats(b.detach(), groups), running_mean=rm[1], running_var=rv[1])
        y = ops.BnActFn.apply(a, g1, b1, b, g1 if b is not None else None, b1 if b is not None else None, r, 1, st, st2, groups)
        y.backward(gy_.to(dev))
        return y.detach().cpu(), a.grad.cpu(), (b.grad.cpu() if b is not None else r.grad.cpu()), g1.grad.cpu(), b1.grad.cpu()

    ctx = emu_product_path() if be.name == "emu" else contextlib.nullcontext()
    with ctx:
        torch.manual_seed(1)
        rm = [torch.zeros(C, device=be.device), torch.zeros(C, device=be.device)]
        rv = [torch.ones(C, device=be.device), torch.ones(C, device=be.device)]
        torch.manual_seed(7)
        yg, dag, dbg, gg, bg = run(z1, z2, res, gy, 2, rm, rv)
        rm2 = [torch.zeros(C, device=be.device), torch.zeros(C, device=be.device)]
        rv2 = [torch.ones(C, device=be.device), torch.ones(C, device=be.device)]
        outs = []
        for h in range(2):
            sl = slice(2 * h, 2 * h + 2)
            torch.manual_seed(7)
            outs.append(run(z1[sl], None if z2 is None else z2[sl], None if res is None else res[sl], gy[sl], 1, rm2, rv2))
    assert torch.equal(yg, torch.cat([o[0] for o in outs]))
    assert torch.equal(dag, torch.cat([o[1] for o in outs]))
    assert torch.equal(dbg, torch.cat([o[2] for o in outs]))
    _close(gg, outs[0][3] + outs[1][3], rtol=1e-6, atol=1e-6)
    _close(bg, outs[0][4] + outs[1][4], rtol=1e-6, atol=1e-6)
    for a, b in zip(rm + rv, rm2 + rv2):
        assert torch.equal(a.cpu(), b.cpu())


# ------------------------------------------------------------------------------- dynamic-LDS grants (stx_lds_try / stx_lds_require)
@pytest.fixture
def emu_lds_limit():
    """Setter of the largest dynamic-LDS grant the emulator's hipFuncSetAttribute allows (tests/hipemu/hipemu_impl.cpp; a real
    device is never made to refuse); no limit again after the test."""
    import ctypes
    from tests.emu_util import emu_lib
    set_limit = ctypes.CDLL(emu_lib().path).hipemu_set_lds_limit
    yield set_limit
    set_limit(-1)


def test_dwconv_hw_takes_the_cache_fed_kernel_when_the_lds_grant_is_refused(emu_lds_limit):
    """The rolling-window launchers have a fallback: with grants above 64 KiB refused (tile of this shape: 8 x 56 voxels x 40
    channels x 4 B = 71 680 B) STX_DWCONV_ROLL = 1 gives what STX_DWCONV_ROLL = 0 gives, and no error.  That the cache-fed
    kernel ran is read off the emulator's records: both launchers were refused, and nothing above 64 KiB was launched (without
    the limit the same calls launch the 71 680 B tile)."""
    import ctypes
    from tests.backends import Backend
    from tests.emu_util import emu_lib
    be = Backend("emu")
    emu = ctypes.CDLL(emu_lib().path)
    refusals, max_lds = (ctypes.c_int.in_dll(emu, n) for n in ("hipemu_lds_refusals", "hipemu_max_launch_lds"))
    B, C, D, H, W = 1, 40, 2, 19, 61
    torch.manual_seed(21)
    x, gy, wts = torch.randn(B, D, H, W, C), torch.randn(B, D, H, W, C), torch.randn(C, 9)
    dd = torch.tensor([1 + (q * 3) // (C // 4) for q in range(C // 4)], dtype=torch.int32)
    old = be.lib.get_tuning("STX_DWCONV_ROLL")
    try:
        res, seen = {}, {}
        for roll, limit in ((1, -1), (1, 64 * 1024), (0, 64 * 1024)):
            emu_lds_limit(limit)
            be.lib.set_tuning("STX_DWCONV_ROLL", roll)
            out = be.empty(B, D, H, W, C)
            be.call("stx_dwconv_hw_fwd", ptr(x), ptr(wts), ptr(dd), ptr(out), B, D, H, W, C, 0)
            ws = be.empty(be.raw("stx_dwconv_hw_wgrad_workspace_floats")(C))
            gw = be.empty(C, 9)
            be.call("stx_dwconv_hw_wgrad", ptr(x), ptr(gy), ptr(dd), ptr(gw), ptr(ws), B, D, H, W, C)
            res[roll] = (out, gw)
            seen[roll, limit] = (refusals.value, max_lds.value)
    finally:
        be.lib.set_tuning("STX_DWCONV_ROLL", old)
    assert seen[1, -1] == (0, 71680), seen                                  # the measure sees the rolling-window kernel
    assert seen[1, 64 * 1024][0] >= 2 and seen[1, 64 * 1024][1] <= 64 * 1024, seen
    assert torch.equal(res[1][0], res[0][0])
    _close(res[1][1], res[0][1], rtol=1e-5, atol=1e-4)


def _conv2d_small(be):
    """stx_conv2d_fwd at the smallest 64-input-channel shape of tests/test_conv2d.py; returns (run, reference, LDS bytes)."""
    B, Ci, Co, H, W = 1, 64, 128, 16, 16
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * 0.1
    xd, wd = be.dev(x.permute(0, 2, 3, 1).contiguous()), be.dev(w.permute(0, 2, 3, 1).contiguous())

    def run():
        out = be.empty(B, H, W, Co)
        be.call("stx_conv2d_fwd", ptr(xd), ptr(wd), ptr(out), None, B, H, W, Ci, Co, 0, 1)
        return out.cpu().permute(0, 3, 1, 2)
    return run, F.conv2d(x, w, None, 1, 1), (9 * Ci * 16 + 2 * 192 * (Ci + 8) + 2 * Co) * 4


def test_conv2d_reports_a_refused_lds_grant_and_keeps_no_state(emu_lds_limit):
    """A launcher without a fallback returns the library's error, naming the call and the bytes it asked for; the same call
    succeeds in the same process once the grant is given (nothing is cached)."""
    import ctypes
    from stereo_toolbox_amd._capi import StxError
    from tests.backends import Backend
    be = Backend("emu")
    run, ref, lds = _conv2d_small(be)
    last_error = ctypes.CDLL(be.lib.path).stx_last_error
    last_error.restype = ctypes.c_char_p
    emu_lds_limit(64 * 1024)
    with pytest.raises(StxError):
        run()
    msg = last_error().decode()
    assert "conv2d_fwd" in msg and str(lds) in msg, msg
    emu_lds_limit(-1)
    err = (run() - ref).abs().max().item()
    assert err <= 2e-5 * ref.abs().max().item() + 1e-6, err


def test_conv2d_pad_clamp(be, tune):
    """STX_C2_PAD: the LDS row padding changes bank conflicts only, and a value outside {4, 8, 12} is the default 8 for the
    kernel AND for the LDS size (the emulator's AddressSanitizer build runs this test too)."""
    run, ref, _ = _conv2d_small(be)
    outs = []
    for v in (0, 4, 8, 12, 99):
        tune("STX_C2_PAD", v)
        outs.append(run())
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
    err = (outs[0] - ref).abs().max().item()
    assert err <= 2e-5 * ref.abs().max().item() + 1e-6, err
