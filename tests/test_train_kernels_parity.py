"""The other kernels of the benchmarked GwcNet_GC / ACVNet / PSMNet train step under the fp64 parity rule, in guard bands:
cost_volume.hip, cost_volume_mfma.hip, cost_volume_bwd_mfma.hip, head.hip, bn.hip, act.hip, conv2d.hip, acv.hip,
sampled_volume.hip, estimators.hip, group_normalize.hip.  (The 3-D convolution family: tests/test_conv3d_parity.py.)

The rule (tests/parity.py::within), for every call: `want64` is the operation in fp64 on the CPU from the same fp32 inputs cast up
(stock torch ops or the oracle/torch_oracle.py restatement, and autograd through them), `d_ref` = max|one-thread fp32 CPU run of
the same expression - want64| over the same tensor (recorded, see DREF_PATH), and the kernel may sit at most VALUE_FACTOR (forward
values, statistics, running buffers) or GRAD_FACTOR (gradients) times d_ref away from want64.  Every tensor goes to the parity
report.  Tensors the rule refuses are listed one by one with their ratio (PAST_THE_FACTOR, strict expected failures through
tests/parity.py::Verdict), each family of entries with a kernel-free demonstration in this module; the near misses at the end show
that the rule refuses a subtly wrong kernel of every family.

Guard bands (tests/backends.py::Guards): every buffer a kernel WRITES is cut from the middle of a larger allocation whose bands
are checked after the call and is sized by exactly the count its query function returns (stx_head_bwd_workspace_floats,
stx_dwconv_hw_wgrad_workspace_floats, stx_bn_reduce_blocks, stx_bn_stats_rows, stx_conv2d_stat_rows); every buffer a kernel READS
sits between NaN bands, so that a read past either end that reaches an output fails the parity assertion.

The shapes are those of tests/test_kernels.py / tests/test_conv2d.py, which sit at the dispatch edges; the comment of every row
names the kernel or the edge it reaches.  Both backends through the C-ABI: host emulator and gfx950.
"""
import contextlib
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_oracle as O
from tests.backends import Backend, Guards, be, ndhwc, ncdhw, tune  # noqa: F401
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, RecordedDref, listed_verdict, within

# d_ref of every tensor below, recorded (tests/parity.py::RecordedDref); STX_TRAIN_KERNELS_DREF_RECORD=<path> runs the module with
# the live values and writes them to <path> (a new or changed case).
DREF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_kernels_parity_dref.json")
_dref = RecordedDref(DREF_PATH, "STX_TRAIN_KERNELS_DREF_RECORD")

# the suffix of `what` that names a tensor of a call
TENSORS = ("vol", "prob", "dLg", "dRg", "dLc", "dRc", "gL", "gR", "gp", "fwd", "flip", "gw", "disp", "gcost", "sum", "sumsq", "mean",
           "invstd", "scale", "shift", "rm", "rv", "y", "dz1", "dz2", "gout", "dbeta", "dgamma1", "dgamma2", "gx", "out")

# Tensors the rule refuses: test name -> "tensor ratio, tensor ratio".  A name without the backend holds for both (the emulator's
# fmaf chains and the gfx950 library agree to the two decimals there); a name with it ("test_x[hip-...]") for that backend alone --
# where the device build's contraction (-ffp-contract=fast; the host build contracts nothing) is part of the value.  The gfx950 ratios are those of
# profiles/train_kernels_parity_report_gfx950.jsonl.  An entry needs a kernel-free demonstration below
# (test_one_fp32_chain_is_past_the_factor, test_a_logit_rounded_once_...); strict: a case that starts to pass must leave the table.
PAST_THE_FACTOR = {
    # csrc/conv2d.hip adds the 9 * Cin products of an output into ONE MFMA accumulator; the CPU reference blocks its sums
    # (test_one_fp32_chain_is_past_the_factor: a plain torch loop over (tap, channel) lands at 2.72 / 3.99 / 3.85 x)
    "test_conv2d_forward_and_statistics[2x64x64x19x37x2]": "out 2.78",
    "test_conv2d_forward_and_statistics[4x64x16x24x33x2]": "out 2.89",
    "test_conv2d_data_gradient[1x32x32x8x16]": "out 3.99",
    "test_conv2d_data_gradient[1x32x64x10x20]": "out 3.93",
    # gfx950 only, cost steps of thousands only: the contracted forward rounds x - max once, the backward rounds x first
    # (test_a_logit_rounded_once_in_the_forward_and_twice_in_the_backward_is_past_the_factor: 5.01 x; the emulator: 1.11 x)
    "test_head2[hip-1x6x3x5x24x12x20x3000.0-align_corners]": "gcost 5.08",
}
LISTED_SHARE = 0.15               # at most this share of the module's (case, tensor) pairs may be listed, per backend


@pytest.fixture
def verdict(request, parity_log):
    name = request.node.name
    reason = PAST_THE_FACTOR.get(name, PAST_THE_FACTOR.get(re.sub(r"\[(emu|hip)-", "[", name)))
    return listed_verdict(request, parity_log, reason, "past the factor, x d_ref: ", dref=_dref, tensors=TENSORS,
                          table="PAST_THE_FACTOR", why="(see the table's comment)")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


@contextlib.contextmanager
def _one_thread():
    """The references run on ONE thread: d_ref must not depend on the core count (tests/parity.py::RecordedDref)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _dist(ref32, want64):
    return (ref32.double() - want64).abs().max().item()


def _refs(fn, ts, gy=None, wrt=()):
    """fn(*ts) (a tensor or a tuple of tensors; None operands pass through) in fp64 from the fp32 tensors cast up, and in fp32 on
    one thread.  Returns (outs, grads): outs = [(want64, d_ref)] per output, grads = {i: (want64, d_ref)} of <outs[0], gy>
    w.r.t. ts[i], i in wrt."""
    def run(dt):
        a = [None if t is None else (t.to(dt).clone().requires_grad_(i in wrt) if t.dtype.is_floating_point else t) for i, t in enumerate(ts)]
        y = fn(*a)
        ys = y if isinstance(y, tuple) else (y,)
        if gy is not None:
            ys[0].backward(gy.to(dt))
        return [v.detach() for v in ys], {i: a[i].grad for i in wrt}
    with _one_thread():
        (y64, g64), (y32, g32) = run(torch.float64), run(torch.float32)
    return [(w, _dist(r, w)) for w, r in zip(y64, y32)], {i: (g64[i], _dist(g32[i], g64[i])) for i in wrt}


def _seq_sum(t):
    """Column sums of [n][...] added one after the other in the tensor's own precision: no kernel has the pairwise order of sum(),
    and cumsum() of fp32 accumulates in fp64 on the CPU."""
    acc = torch.zeros_like(t[0])
    for row in t:
        acc += row
    return acc


def _inp_i32(G, t):
    v = G.inp(torch.zeros(t.shape)).view(torch.int32)
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------------ cost volume
CV_CASES = [
    # B, Cg, G, Cc, H, W, D, mask_left
    (2, 16, 4, 0, 3, 11, 6, 1),       # gwc only, tiny
    (1, 320, 40, 12, 2, 37, 20, 1),   # GwcNet_GC channel config, ragged W and D
    (1, 0, 0, 32, 3, 21, 18, 1),      # PSMNet concat
    (1, 0, 0, 32, 3, 21, 18, 0),      # ACVNet concat (left half unmasked)
    (1, 64, 8, 4, 2, 40, 48, 1),      # D' = 48 > W tile
    (2, 320, 40, 0, 2, 24, 12, 1),    # ACVNet gwc-only volume, batch 2
    (1, 64, 8, 4, 3, 52, 13, 0),      # 8 channels per group, left half unmasked, D not a multiple of 8
    (1, 96, 8, 0, 2, 50, 20, 1),      # IGEV-style initial volume: 12 channels per group
    (1, 64, 4, 8, 2, 35, 9, 1),       # 16 channels per group
    (1, 32, 8, 0, 2, 33, 17, 1),      # 4 channels per group
    (1, 32, 4, 4, 1, 100, 80, 1),     # D' = 80: five 16-disparity units per macro-unit (long register ring)
]
GC = CV_CASES[1]
TEAM_CASES = [(1, 320, 40, 12, 10, 130, 48, 1),      # GwcNet_GC channels, 6 chunks, 9 tiles, rows 8/9 = second round
              (2, 64, 8, 4, 5, 140, 43, 0)]          # D' = 43 (ragged last chunk), batch 2, left half unmasked
#            variant: (tunes, forward as well)
CV_VARIANTS = {
    "mfma": ({}, True),                                                           # cost_volume_mfma.hip / cost_volume_bwd_mfma.hip
    "first_generation": ({"STX_CV_OLD": 1, "STX_CVB_OLD": 1}, True),              # the any-shape kernels of cost_volume.hip
    "grid2_bwd1": ({"STX_CV_GRID": 2, "STX_CV_UNITS": 1, "STX_CVB_GRID": 1}, True),   # runs of several units, cut at units; one workgroup
    "grid5_bwd3": ({"STX_CV_GRID": 5, "STX_CV_UNITS": 1, "STX_CVB_GRID": 3}, True),   # runs cut INSIDE macro-units; three workgroups
    "team": ({"STX_CVB_TEAM": 1}, False),                                         # the backward's row-team schedule
}
CV_PARAMS = ([("mfma", c) for c in CV_CASES] + [("first_generation", c) for c in CV_CASES if not (c[2] and c[1] // c[2] == 12)]
             + [("grid2_bwd1", GC), ("grid5_bwd3", GC)] + [("team", c) for c in TEAM_CASES])


def _cv_fn(G, D, ml):
    def fn(Lg, Rg, Lc, Rc):
        parts = []
        if Lg is not None:
            parts.append(O.build_gwc_volume(Lg, Rg, D, G))
        if Lc is not None:
            parts.append(O.build_concat_volume(Lc, Rc, D, mask_left=bool(ml)))
        return torch.cat(parts, 1)
    return fn


@functools.lru_cache(maxsize=None)
def _cv_ref(case):
    B, Cg, G, Cc, H, W, D, ml = case
    g = _gen(1)
    Lg, Rg = (_randn(g, B, Cg, H, W) if G else None for _ in range(2))
    Lc, Rc = (_randn(g, B, Cc, H, W) if Cc else None for _ in range(2))
    gv = _randn(g, B, D, H, W, G + 2 * Cc)
    ts = (Lg, Rg, Lc, Rc)
    wrt = tuple(i for i, t in enumerate(ts) if t is not None)
    fn = _cv_fn(G, D, ml)
    _, grads = _refs(fn, ts, ncdhw(gv), wrt)
    with _one_thread():
        v64, v32 = fn(*[None if t is None else t.double() for t in ts]), fn(*ts)
    return ts, gv, v64, v32, grads


@pytest.mark.parametrize("variant,case", CV_PARAMS, ids=[f"{v}-" + "x".join(map(str, c)) for v, c in CV_PARAMS])
def test_cost_volume(be, tune, verdict, variant, case):
    """stx_cost_volume_fwd / _bwd: the rule on the group-correlation channels and on all four gradients; the concat channels
    are copies and stay bit-exact."""
    tunes, fwd = CV_VARIANTS[variant]
    for k, v in tunes.items():
        tune(k, v)
    B, Cg, G, Cc, H, W, D, ml = case
    ts, gv, v64, v32, grads = _cv_ref(case)
    what = f"cost_volume[{be.name}:{variant}:" + "x".join(map(str, case)) + "]"
    Gd = Guards(be)
    dev = [Gd.inp(t) for t in ts]
    if fwd:
        vol = Gd.out(B, D, H, W, G + 2 * Cc)
        be.call("stx_cost_volume_fwd", dev[0], dev[1], Cg, G, dev[2], dev[3], Cc, None, vol, B, H, W, D, ml)
        Gd.check(what)
        got = ncdhw(vol).cpu()
        assert torch.equal(got[:, G:], v32[:, G:]), "concat volume is not an exact copy"
        if G:
            verdict.within(got[:, :G], v64[:, :G], _dist(v32[:, :G], v64[:, :G]), VALUE_FACTOR, what + ":vol")
    outs = [None if t is None else Gd.out(*t.shape) for t in ts]
    be.call("stx_cost_volume_bwd", Gd.inp(gv), dev[0], dev[1], Cg, G, Cc, *outs, B, H, W, D, ml)
    Gd.check(what + ":bwd")
    for i, name in enumerate(("dLg", "dRg", "dLc", "dRc")):
        if outs[i] is not None:
            verdict.within(outs[i].cpu(), *grads[i], GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


def test_cost_volume_scale_operand(be, verdict):
    """ACVNet/acv.py:196: softmax(att, dim=2) * concat_volume, the softmax from stx_softmax_d_fwd as the `scale` operand."""
    B, Cc, H, W, D = 1, 8, 2, 19, 7
    g = _gen(2)
    Lc, Rc, att = _randn(g, B, Cc, H, W), _randn(g, B, Cc, H, W), _randn(g, B, 1, D, H, W)
    (vol_ref, prob_ref), _ = _refs(lambda a, b, c: (F.softmax(c, dim=2) * O.build_concat_volume(a, b, D, mask_left=False), F.softmax(c, dim=2)),
                                   (Lc, Rc, att))
    what = f"cost_volume_scale[{be.name}:1x8x2x19x7]"
    Gd = Guards(be)
    prob = Gd.out(B, D, H, W)
    be.call("stx_softmax_d_fwd", Gd.inp(att), prob, B, D, H * W)
    Gd.check(what + ":prob")
    vol = Gd.out(B, D, H, W, 2 * Cc)
    be.call("stx_cost_volume_fwd", None, None, 0, 0, Gd.inp(Lc), Gd.inp(Rc), Cc, Gd.inp(prob), vol, B, H, W, D, 0)
    Gd.check(what)
    verdict.within(prob.cpu().view(B, 1, D, H, W), *prob_ref, VALUE_FACTOR, what + ":prob")
    verdict.within(ncdhw(vol).cpu(), *vol_ref, VALUE_FACTOR, what + ":vol")
    verdict.done()


# ------------------------------------------------------------------------------------------ ACVNet extras
@pytest.mark.parametrize("form", ["one_pass", "three_launches"])
@pytest.mark.parametrize("case", [(1, 8, 3, 21, 9), (2, 32, 2, 37, 12), (1, 4, 2, 7, 10)], ids=lambda c: "x".join(map(str, c)))
def test_ac_volume_bwd(be, verdict, case, form):
    """Gradients of prob * concat_volume (acv.py:196) w.r.t. features and probabilities: stx_ac_volume_bwd in one pass over the
    gradient volume, and stx_cost_volume_scale_bwd + stx_scale_channels + stx_cost_volume_bwd.  Batch 2, W < D, 32 channels."""
    B, Cc, H, W, D = case
    g = _gen(13)
    Lc, Rc, prob = _randn(g, B, Cc, H, W), _randn(g, B, Cc, H, W), torch.rand(B, D, H, W, generator=g)
    gv = _randn(g, B, D, H, W, 2 * Cc)
    _, grads = _refs(lambda a, b, p: p.unsqueeze(1) * O.build_concat_volume(a, b, D, mask_left=False), (Lc, Rc, prob), ncdhw(gv), (0, 1, 2))
    what = f"ac_volume_bwd[{be.name}:{form}:" + "x".join(map(str, case)) + "]"
    Gd = Guards(be)
    dgv, dL, dR, dp = Gd.inp(gv), Gd.inp(Lc), Gd.inp(Rc), Gd.inp(prob)
    gL, gR, gp = Gd.out(B, Cc, H, W), Gd.out(B, Cc, H, W), Gd.out(B, D, H, W)
    if form == "one_pass":
        be.call("stx_ac_volume_bwd", dgv, dL, dR, dp, gL, gR, gp, B, Cc, H, W, D, 0)
        Gd.check(what)
    else:
        be.call("stx_cost_volume_scale_bwd", dgv, dL, dR, gp, B, Cc, H, W, D, 0)
        Gd.check(what + ":scale_bwd")
        scaled = Gd.out(B, D, H, W, 2 * Cc)
        be.call("stx_scale_channels", dgv, dp, scaled, B * D * H * W, 2 * Cc)
        Gd.check(what + ":scale_channels")
        be.call("stx_cost_volume_bwd", Gd.inp(scaled), None, None, 0, 0, Cc, None, None, gL, gR, B, H, W, D, 0)
        Gd.check(what + ":volume_bwd")
    for got, i, name in ((gL, 0, "gL"), (gR, 1, "gR"), (gp, 2, "gp")):
        verdict.within(got.cpu(), *grads[i], GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


def _dw_fn(dils, flip):
    def fn(x, w):
        return torch.cat([F.conv3d(x[:, 4 * q:4 * q + 4], (w[4 * q:4 * q + 4].flip(1) if flip else w[4 * q:4 * q + 4]).view(4, 1, 1, 3, 3), None, 1,
                                   (0, d, d), d, 4) for q, d in enumerate(dils)], 1)
    return fn


@pytest.mark.parametrize("roll", [1, 0], ids=["rolling_window", "cache_fed"])
@pytest.mark.parametrize("shape", [(1, 40, 2, 19, 61), (2, 40, 1, 9, 50), (1, 8, 2, 33, 300), (1, 40, 1, 8, 7)], ids=lambda c: "x".join(map(str, c)))
def test_dwconv_hw(be, tune, verdict, shape, roll):
    """stx_dwconv_hw_fwd with both tap orders (forward / data gradient) and stx_dwconv_hw_wgrad: the rolling 8-row window in LDS
    (several strips, a ragged last strip, row segments, a 2-quad volume) and the cache-fed kernels; dilations 1-3."""
    tune("STX_DWCONV_ROLL", roll)
    B, C, D, H, W = shape
    g = _gen(21)
    x, wts = _randn(g, B, C, D, H, W), _randn(g, C, 9)
    dils = [1 + (q * 3) // (C // 4) for q in range(C // 4)]
    gy = _randn(g, B, C, D, H, W)
    (fwd_ref,), grads = _refs(_dw_fn(dils, 0), (x, wts), gy, (1,))
    (flip_ref,), _ = _refs(_dw_fn(dils, 1), (x, wts))
    what = f"dwconv_hw[{be.name}:{'roll' if roll else 'cache'}:" + "x".join(map(str, shape)) + "]"
    Gd = Guards(be)
    xl, wl, dd = Gd.inp(ndhwc(x)), Gd.inp(wts), _inp_i32(Gd, torch.tensor(dils, dtype=torch.int32))
    for flip, ref, name in ((0, fwd_ref, "fwd"), (1, flip_ref, "flip")):
        out = Gd.out(B, D, H, W, C)
        be.call("stx_dwconv_hw_fwd", xl, wl, dd, out, B, D, H, W, C, flip)
        Gd.check(f"{what}:{name}")
        verdict.within(ncdhw(out).cpu(), *ref, VALUE_FACTOR, f"{what}:{name}")
    ws, gw = Gd.out(be.raw("stx_dwconv_hw_wgrad_workspace_floats")(C)), Gd.out(C, 9)
    be.call("stx_dwconv_hw_wgrad", xl, Gd.inp(ndhwc(gy)), dd, gw, ws, B, D, H, W, C)
    Gd.check(what + ":gw")
    verdict.within(gw.cpu(), *grads[1], GRAD_FACTOR, what + ":gw")
    verdict.done()


# ------------------------------------------------------------------------------------------ CFNet sampled (cascade) volume
@pytest.mark.parametrize("variant", ["lds_window", "global_atomics"])
@pytest.mark.parametrize("case", [(1, 40, 4, 12, 5, 70, 6), (2, 20, 4, 6, 3, 33, 4), (1, 8, 8, 0, 2, 64, 3), (1, 0, 0, 8, 2, 20, 5),
                                  (1, 8, 4, 4, 2, 200, 3), (1, 40, 8, 12, 1, 66, 2)], ids=lambda c: "x".join(map(str, c)))
def test_sampled_volume(be, tune, verdict, case, variant):
    """stx_sampled_volume_fwd / _bwd: CFNet's two stage configurations, 8 channels per group, concat only; W = 70 / 33 leave a
    ragged 64-column tile; hypotheses reach outside the image on both sides.  Backward through the workgroup's LDS window
    (W = 200: its global-atomic fallback; 320 + 12 channels: two workgroups) and with global atomics only (STX_SV_BWD_V1).  The
    pad channels stay exactly zero, the hypothesis channel and the concat channels exactly equal."""
    tune("STX_SV_BWD_V1", 1 if variant == "global_atomics" else 0)
    B, G, cpg, Cc, H, W, S = case
    Cg = G * cpg
    g = _gen(11)
    Lg, Rg = (_randn(g, B, Cg, H, W) if G else None for _ in range(2))
    Lc, Rc = (_randn(g, B, Cc, H, W) if Cc else None for _ in range(2))
    samples = torch.randint(-4, 150 if W == 200 else W // 2, (B, S, H, W), generator=g).float()
    CT = G + 2 * Cc + 1
    CTp = (CT + 7) // 8 * 8
    gv = _randn(g, B, S, H, W, CTp)
    ts = (Lg, Rg, Lc, Rc)
    wrt = tuple(i for i, t in enumerate(ts) if t is not None)

    def fn(Lg, Rg, Lc, Rc):
        parts = ([O.cf_sampled_volume(Lg, Rg, samples, G)] if G else []) + ([O.cf_sampled_volume(Lc, Rc, samples, None)] if Cc else [])
        return torch.cat(parts, 1)
    (vol_ref,), grads = _refs(fn, ts, gv[..., :CT - 1].permute(0, 4, 1, 2, 3), wrt)
    with _one_thread():
        v32 = fn(*ts)
    what = f"sampled_volume[{be.name}:{variant}:" + "x".join(map(str, case)) + "]"
    Gd = Guards(be)
    dev, dsm = [Gd.inp(t) for t in ts], Gd.inp(samples)
    vol = Gd.out(B, S, H, W, CTp)
    be.call("stx_sampled_volume_fwd", dev[0], dev[1], Cg, G, dev[2], dev[3], Cc, dsm, vol, B, H, W, S, CTp)
    Gd.check(what)
    got = vol.cpu()
    assert torch.equal(got[..., CT:], torch.zeros(B, S, H, W, CTp - CT))
    assert torch.equal(got[..., CT - 1], samples)
    assert torch.equal(got[..., G:CT - 1].permute(0, 4, 1, 2, 3), v32[:, G:])
    if G:
        verdict.within(got[..., :G].permute(0, 4, 1, 2, 3), vol_ref[0][:, :G], _dist(v32[:, :G], vol_ref[0][:, :G]), VALUE_FACTOR, what + ":vol")
    outs = [None if t is None else Gd.out(*t.shape) for t in ts]
    be.call("stx_sampled_volume_bwd", Gd.inp(gv), dev[0], dev[1], Cg, G, Cc, dsm, *outs, B, H, W, S, CTp)
    Gd.check(what + ":bwd")
    for i, name in enumerate(("dLg", "dRg", "dLc", "dRc")):
        if outs[i] is not None:
            verdict.within(outs[i].cpu(), *grads[i], GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


# ------------------------------------------------------------------------------------------ regression head
HEAD_CASES = [
    # B, Dc, Hc, Wc, D, H, W, gain
    (1, 4, 5, 7, 16, 20, 28, 5.0),
    (2, 12, 6, 9, 48, 24, 36, 3.0),
    (1, 5, 4, 6, 17, 13, 22, 4.0),
    (1, 1, 3, 1, 4, 9, 5, 2.0),
    (1, 3, 2, 75, 12, 3, 300, 40.0),        # W = 300 spans two workgroups with a ragged tail
    (1, 9, 3, 4, 5, 4, 6, 3.0),             # D < Dc leaves coarse planes without an output disparity; 24 outputs
    (1, 6, 3, 5, 24, 12, 20, 3000.0),       # cost steps far beyond the exp range: the LDS kernel redoes the walk with the exact maximum
    (1, 84, 2, 3, 336, 8, 12, 3.0),         # D' = 84 exceeds the LDS-staged forward kernel's table (first-generation kernel)
    (1, 9, 6, 10, 5, 16, 36, 3.0),          # D < Dc again, 576 outputs
]


@functools.lru_cache(maxsize=None)
def _head_ref(case, ac):
    B, Dc, Hc, Wc, D, H, W, gain = case
    g = _gen(3)
    cost, gd = _randn(g, B, 1, Dc, Hc, Wc) * gain, _randn(g, B, H, W)
    (disp_ref,), grads = _refs(lambda c: O.regression_head(c, D, H, W, align_corners=bool(ac)), (cost,), gd, (0,))
    return cost, gd, disp_ref, grads[0]


def _run_head(be, verdict, case, ac, what):
    B, Dc, Hc, Wc, D, H, W, _ = case
    cost, gd, disp_ref, gcost_ref = _head_ref(case, 0 if ac is None else ac)
    rule = () if ac is None else (ac,)
    fwd, bwd = ("stx_head_fwd", "stx_head_bwd") if ac is None else ("stx_head_fwd2", "stx_head_bwd2")
    Gd = Guards(be)
    dcost = Gd.inp(cost)
    disp, stats = Gd.out(B, H, W), Gd.out(B, H, W, 2)
    be.call(fwd, dcost, disp, stats, B, Dc, Hc, Wc, D, H, W, *rule)
    Gd.check(what)
    gc, ws = Gd.out(B, 1, Dc, Hc, Wc), Gd.out(be.raw("stx_head_bwd_workspace_floats")(B, Dc, H, W))
    be.call(bwd, Gd.inp(gd), dcost, Gd.inp(disp), Gd.inp(stats), gc, ws, B, Dc, Hc, Wc, D, H, W, *rule)
    Gd.check(what + ":bwd")
    verdict.within(disp.cpu(), *disp_ref, VALUE_FACTOR, what + ":disp")
    verdict.within(gc.cpu(), *gcost_ref, GRAD_FACTOR, what + ":gcost")
    verdict.done()


@pytest.mark.parametrize("ac", [0, 1], ids=["half_pixel", "align_corners"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_head2(be, verdict, case, ac):
    """stx_head_fwd2 / stx_head_bwd2 (trilinear upsampling + softmax + expectation, fused) under both interpolation rules."""
    _run_head(be, verdict, case, ac, f"head2[{be.name}:{'ac' if ac else 'hp'}:" + "x".join(map(str, case)) + "]")


@pytest.mark.parametrize("case", HEAD_CASES[:3], ids=lambda c: "x".join(map(str, c)))
def test_head(be, verdict, case):
    """stx_head_fwd / stx_head_bwd: the entry points without an interpolation rule (align_corners=False)."""
    _run_head(be, verdict, case, None, f"head[{be.name}:" + "x".join(map(str, case)) + "]")


# ------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("case", [(1000, 32), (37, 64), (3, 16), (5000, 128)], ids=lambda c: "x".join(map(str, c)))
def test_bn_stats(be, verdict, case):
    """stx_bn_stats: the column sums of its stx_bn_stats_rows rows of (sum, sum of squares) against the fp64 sums."""
    nvox, C = case
    # 64 or 16 sums are too few for the maximum of their errors to be a measure (37 x 64 alone: 64 sums of 37 terms, each a couple
    # of ulp off in either order, and the ratio of the two maxima came out at 2.8): such a shape runs as `groups` slabs of its own
    # size with their own rows, the same launch per slab, and is judged over the 256 sums of all slabs
    groups = 1 if C >= 128 or nvox >= 1000 else 256 // C
    z = _randn(_gen(31), groups, nvox, C) * 2 + 0.5
    what = f"bn_stats[{be.name}:{nvox}x{C}]"
    rows = be.raw("stx_bn_stats_rows")(nvox, C)
    assert rows >= 1
    Gd = Guards(be)
    part = Gd.out(groups, rows, 2, C)
    be.call("stx_bn_stats", Gd.inp(z), part, nvox, C, groups)
    Gd.check(what)
    p = part.cpu().double().sum(1)
    z64 = z.double()
    seq = lambda t: torch.stack([_seq_sum(s) for s in t])  # noqa: E731
    verdict.within(p[:, 0], z64.sum(1), _dist(seq(z), z64.sum(1)), VALUE_FACTOR, what + ":sum")
    verdict.within(p[:, 1], (z64 * z64).sum(1), _dist(seq(z * z), (z64 * z64).sum(1)), VALUE_FACTOR, what + ":sumsq")
    verdict.done()


def _finalize(part, count, g, b, rm, rv, momentum=0.1, eps=1e-5):
    """stx_bn_finalize in the precision of its operands: the rows summed one after the other, then the header's formulas."""
    s1, s2 = _seq_sum(part[:, 0]), _seq_sum(part[:, 1])
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp(min=0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g * invstd
    return (scale, b - mean * scale, mean, invstd, (1 - momentum) * rm + momentum * mean,
            (1 - momentum) * rv + momentum * var * count / (count - 1))


@pytest.mark.parametrize("case", [(1500, 32), (257, 20)], ids=lambda c: "x".join(map(str, c)))
def test_bn_finalize(be, verdict, case):
    """stx_bn_finalize: the channel-quad kernel (C % 4 == 0 and >= 256 rows: 1500 x 32) and the first-generation kernel
    (257 x 20), running buffers included."""
    nrows, C = case
    g = _gen(5)
    part = _randn(g, nrows, 2, C)
    part[:, 1] = part[:, 1].abs() * 40 + 50          # sum z^2 comfortably above (sum z)^2 / n
    count = float(nrows * 64)
    gamma, beta, rm, rv = torch.rand(C, generator=g) + 0.5, _randn(g, C), _randn(g, C), torch.rand(C, generator=g) + 0.5
    with _one_thread():
        w64 = _finalize(*[t.double() for t in (part,)], count, *[t.double() for t in (gamma, beta, rm, rv)])
        w32 = _finalize(part, count, gamma, beta, rm, rv)
    what = f"bn_finalize[{be.name}:{nrows}x{C}]"
    Gd = Guards(be)
    drm, drv = Gd.out(C), Gd.out(C)
    drm.copy_(rm)
    drv.copy_(rv)
    outs = [Gd.out(C) for _ in range(4)]
    be.call("stx_bn_finalize", Gd.inp(part), nrows, C, count, Gd.inp(gamma), Gd.inp(beta), drm, drv, 0.1, 1e-5, *outs)
    Gd.check(what)
    for got, a, b, name in zip(outs + [drm, drv], w64, w32, ("scale", "shift", "mean", "invstd", "rm", "rv")):
        verdict.within(got.cpu(), a, _dist(b, a), VALUE_FACTOR, f"{what}:{name}")
    verdict.done()


FG_CASES = [(g, C, n) for g in (1, 2, 3) for C in (16, 40) for n in (1, 7)]      # groups, C, nrows: one slab, the two views, an odd count;
#                                                                                  C = 40 is no power of two; a single row, and several


@pytest.mark.parametrize("case", FG_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_finalize_groups(be, verdict, case):
    """stx_bn_finalize_groups: out [4][groups][C] against fp64 from the partial sums, the running statistics updated slab after
    slab; every bit equal to `groups` successive calls of stx_bn_finalize on the slabs (the header's promise), with the running
    buffers and with both running pointers NULL."""
    groups, C, nrows = case
    g = _gen(60 + FG_CASES.index(case))
    part = _randn(g, groups, nrows, 2, C)
    part[:, :, 1] = part[:, :, 1].abs() * 40 + 50    # sum z^2 comfortably above (sum z)^2 / n
    count = float(nrows * 64)
    gamma, beta, rm, rv = torch.rand(C, generator=g) + 0.5, _randn(g, C), _randn(g, C), torch.rand(C, generator=g) + 0.5

    def slabs(dt):
        m, v, rows = rm.to(dt), rv.to(dt), []
        for k in range(groups):
            *four, m, v = _finalize(part[k].to(dt), count, gamma.to(dt), beta.to(dt), m, v)
            rows.append(torch.stack(four))
        return torch.stack(rows, 1), m, v                                     # [4][groups][C], and the buffers behind the last slab
    with _one_thread():
        w64, w32 = slabs(torch.float64), slabs(torch.float32)
    what = f"bn_finalize_groups[{be.name}:{groups}x{C}x{nrows}]"
    Gd = Guards(be)
    dpart, dgamma, dbeta = Gd.inp(part), Gd.inp(gamma), Gd.inp(beta)

    def run(name, running):
        bufs = [Gd.out(C), Gd.out(C)] if running else [None, None]
        for b, t in zip(bufs, (rm, rv)):
            if b is not None:
                b.copy_(t)
        out = Gd.out(4, groups, C)
        if name == "stx_bn_finalize_groups":
            be.call(name, dpart, nrows, C, count, dgamma, dbeta, *bufs, 0.1, 1e-5, out, groups)
            Gd.check(f"{what}:{name}")
        else:
            one = [Gd.out(C) for _ in range(4)]
            for k in range(groups):
                be.call(name, dpart[k], nrows, C, count, dgamma, dbeta, *bufs, 0.1, 1e-5, *one)
                Gd.check(f"{what}:{name}:{k}")
                for i in range(4):
                    out[i, k].copy_(one[i])
        return [out.cpu()] + [None if b is None else b.cpu() for b in bufs]
    got = run("stx_bn_finalize_groups", True)
    for i, name in enumerate(("scale", "shift", "mean", "invstd")):
        verdict.within(got[0][i], w64[0][i], _dist(w32[0][i], w64[0][i]), VALUE_FACTOR, f"{what}:{name}")
    verdict.within(got[1], w64[1], _dist(w32[1], w64[1]), VALUE_FACTOR, f"{what}:rm")
    verdict.within(got[2], w64[2], _dist(w32[2], w64[2]), VALUE_FACTOR, f"{what}:rv")
    for a, b in zip(got, run("stx_bn_finalize", True)):
        assert torch.equal(a, b), what
    plain, plain_slabs = run("stx_bn_finalize_groups", False), run("stx_bn_finalize", False)
    assert torch.equal(plain[0], got[0]) and torch.equal(plain_slabs[0], got[0]), what
    verdict.done()


BN_CASES = {
    # nvox, C, second BatchNorm branch, activation code, plain residual
    "1000x32_relu": (1000, 32, False, 1, False),
    "777x64_two_relu": (777, 64, True, 1, False),
    "500x32_res": (500, 32, False, 0, True),
    "640x128_res_relu": (640, 128, False, 1, True),
    "900x32_mish": (900, 32, False, 2, False),
    "900x32_two_mish": (900, 32, True, 2, False),
}
# the mask / pre-activation operand of the backward passes: the activated output y (stx_bn_bwd_reduce / _apply) or the forward
# pass's scale / shift vectors (stx_bn_bwd_reduce2 / _apply2; a block with a plain residual still passes y); Mish needs the latter
BN_PARAMS = [(c, m) for c in BN_CASES for m in ("y", "scale_shift") if not (m == "y" and BN_CASES[c][3] == 2)]


def _bn_fn(two, act, resid, rm=None, rv=None):
    def fn(z1, z2, g1, b1, g2, b2):
        y = F.batch_norm(z1, rm, rv, g1, b1, True, 0.1, 1e-5)
        if two:
            y = y + F.batch_norm(z2, None, None, g2, b2, True, 0.1, 1e-5)
        elif resid:
            y = y + z2
        return (y, F.relu(y), F.mish(y))[act]
    return fn


@functools.lru_cache(maxsize=None)
def _bn_ref(name):
    nvox, C, two, act, resid = BN_CASES[name]
    g = _gen(10)
    z1 = _randn(g, nvox, C) * 2 + 1
    z2 = _randn(g, nvox, C) + 0.5 if (two or resid) else None
    g1, b1, g2, b2 = torch.rand(C, generator=g) + 0.5, _randn(g, C), torch.rand(C, generator=g) + 0.5, _randn(g, C)
    rm, rv = _randn(g, C), torch.rand(C, generator=g) + 0.5
    gy = _randn(g, nvox, C)
    ts = (z1, z2, g1, b1, g2 if two else None, b2 if two else None)
    wrt = (0, 2, 3) + ((1,) if z2 is not None else ()) + ((4,) if two else ())
    (y_ref,), grads = _refs(_bn_fn(two, act, resid), ts, gy, wrt)
    run = {}
    with _one_thread():
        for dt in (torch.float64, torch.float32):
            a, b = rm.to(dt).clone(), rv.to(dt).clone()                # (F.batch_norm updates them in place)
            y = _bn_fn(two, act, resid, a, b)(*[None if t is None else t.to(dt) for t in ts])
            run[dt] = (a, b, y)
    if act == 1:       # the ReLU mask of the fp32 and the fp64 reference agree: no gradient of the fixture hangs on a rounding
        assert torch.equal(run[torch.float64][2] > 0, run[torch.float32][2] > 0)
    rm_ref, rv_ref = ((run[torch.float64][i], _dist(run[torch.float32][i], run[torch.float64][i])) for i in (0, 1))
    return ts, rm, rv, gy, y_ref, grads, rm_ref, rv_ref


@pytest.mark.parametrize("case,mask", BN_PARAMS, ids=[f"{c}-{m}" for c, m in BN_PARAMS])
def test_bn_fwd_bwd(be, verdict, case, mask):
    """Train-mode BatchNorm (+ second branch / residual, ReLU / Mish) as the product runs it: partial rows -> stx_bn_finalize
    (running buffers) -> stx_bn_apply -> stx_bn_bwd_reduce[2] -> stx_bn_bwd_apply[2], against F.batch_norm and autograd."""
    nvox, C, two, act, resid = BN_CASES[case]
    (z1, z2, g1, b1, g2, b2), rm, rv, gy, y_ref, grads, rm_ref, rv_ref = _bn_ref(case)
    what = f"bn[{be.name}:{case}:{mask}]"
    Gd = Guards(be)

    def fin(z, gamma, beta, drm, drv):
        part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in z.chunk(7)])
        outs = [Gd.out(C) for _ in range(4)]
        be.call("stx_bn_finalize", Gd.inp(part), part.shape[0], C, float(nvox), Gd.inp(gamma), Gd.inp(beta), drm, drv, 0.1, 1e-5, *outs)
        Gd.check(what + ":finalize")
        return [Gd.inp(o) for o in outs]

    drm, drv = Gd.out(C), Gd.out(C)
    drm.copy_(rm)
    drv.copy_(rv)
    sc1, sh1, m1, i1 = fin(z1, g1, b1, drm, drv)
    sc2 = sh2 = m2 = i2 = None
    if two:
        sc2, sh2, m2, i2 = fin(z2, g2, b2, None, None)
    d1, d2, dgy = Gd.inp(z1), Gd.inp(z2), Gd.inp(gy)
    out = Gd.out(nvox, C)
    be.call("stx_bn_apply", d1, sc1, sh1, d2, sc2, sh2, out, nvox, C, act, 1)
    Gd.check(what + ":apply")
    verdict.within(out.cpu(), *y_ref, VALUE_FACTOR, what + ":y")
    verdict.within(drm.cpu(), *rm_ref, VALUE_FACTOR, what + ":rm")
    verdict.within(drv.cpu(), *rv_ref, VALUE_FACTOR, what + ":rv")

    part, sums = Gd.out(be.raw("stx_bn_reduce_blocks")(), 3, C), Gd.out(3, C)
    dz1, dz2, gout = Gd.out(nvox, C), (Gd.out(nvox, C) if two else None), (Gd.out(nvox, C) if resid else None)
    dg1, dg2 = Gd.inp(g1), Gd.inp(g2)
    z2b, m2b, i2b = (d2, m2, i2) if two else (None, None, None)
    if mask == "y":
        y = Gd.inp(out)
        be.call("stx_bn_bwd_reduce", dgy, y, d1, m1, i1, z2b, m2b, i2b, part, sums, nvox, C, act)
        Gd.check(what + ":reduce")
        be.call("stx_bn_bwd_apply", dgy, y, d1, m1, i1, dg1, z2b, m2b, i2b, dg2, Gd.inp(sums), dz1, dz2, gout, nvox, C, act)
    else:
        y = Gd.inp(out) if resid else None
        be.call("stx_bn_bwd_reduce2", dgy, y, d1, m1, i1, z2b, m2b, i2b, sc1, sh1, sc2, sh2, part, sums, nvox, C, act, 1)
        Gd.check(what + ":reduce2")
        be.call("stx_bn_bwd_apply2", dgy, y, d1, m1, i1, dg1, z2b, m2b, i2b, dg2, sc1, sh1, sc2, sh2, Gd.inp(sums), dz1, dz2, gout,
                nvox, C, act, 1)
    Gd.check(what + ":bwd_apply")
    s = sums.cpu()
    verdict.within(dz1.cpu(), *grads[0], GRAD_FACTOR, what + ":dz1")
    verdict.within(s[0], *grads[3], GRAD_FACTOR, what + ":dbeta")
    verdict.within(s[1], *grads[2], GRAD_FACTOR, what + ":dgamma1")
    if two:
        verdict.within(dz2.cpu(), *grads[1], GRAD_FACTOR, what + ":dz2")
        verdict.within(s[2], *grads[4], GRAD_FACTOR, what + ":dgamma2")
    if resid:
        verdict.within(gout.cpu(), *grads[1], GRAD_FACTOR, what + ":gout")
    verdict.done()


# ------------------------------------------------------------------------------------------ activations and estimators
def _mish_input():
    x = torch.cat((_randn(_gen(21), 2, 3, 4, 5, 8) * 3, torch.tensor([-30., -5., 0., 5., 19.9, 20.1, 30., 1e-3]).repeat(2, 3, 4, 5, 1)), 0)
    return x, _randn(_gen(22), *x.shape)


def test_mish(be, verdict):
    """stx_mish_fwd / _bwd vs the reference's x * tanh(softplus(x)), incl. both sides of softplus' threshold at 20."""
    x, gy = _mish_input()
    (y_ref,), grads = _refs(lambda x: x * torch.tanh(F.softplus(x)), (x,), gy, (0,))
    what = f"mish[{be.name}:edges]"
    Gd = Guards(be)
    dx, out, gx = Gd.inp(x), Gd.out(*x.shape), Gd.out(*x.shape)
    be.call("stx_mish_fwd", dx, out, x.numel())
    Gd.check(what)
    be.call("stx_mish_bwd", Gd.inp(gy), dx, gx, x.numel())
    Gd.check(what + ":gx")
    verdict.within(out.cpu(), *y_ref, VALUE_FACTOR, what + ":y")
    verdict.within(gx.cpu(), *grads[0], GRAD_FACTOR, what + ":gx")
    verdict.done()


def test_softmax_d(be, verdict):
    z = _randn(_gen(4), 2, 16, 6, 10)
    (ref,), _ = _refs(lambda z: torch.softmax(z, 1), (z,))
    what = f"softmax_d[{be.name}:2x16x60]"
    Gd = Guards(be)
    y = Gd.out(2, 16, 6, 10)
    be.call("stx_softmax_d_fwd", Gd.inp(z), y, 2, 16, 60)
    Gd.check(what)
    verdict.within(y.cpu(), *ref, VALUE_FACTOR, what + ":prob")
    verdict.done()


#                 name: (B, D, H, W)
SOFTARGMAX_CASES = {"hw28_d21": (1, 21, 4, 7),       # HW % 4 == 0: four pixels per lane, eight planes per trip, D = 21 leaves a tail
                    "hw35_d21": (1, 21, 5, 7),       # HW = 35 takes the scalar kernel
                    "hw60_d16": (2, 16, 6, 10)}


@pytest.mark.parametrize("case", SOFTARGMAX_CASES)
def test_softargmax(be, verdict, case):
    B, D, H, W = SOFTARGMAX_CASES[case]
    x = torch.softmax(_randn(_gen(4), B, D, H, W) * 3, 1)
    (ref,), _ = _refs(lambda x: O.disparity_regression(x, D), (x,))
    what = f"softargmax[{be.name}:{case}]"
    Gd = Guards(be)
    dx, o = Gd.inp(x), Gd.out(B, H, W)
    be.call("stx_softargmax_fwd", dx, o, B, D, H * W)
    Gd.check(what)
    verdict.within(o.cpu(), *ref, VALUE_FACTOR, what + ":disp")
    a = Gd.out(B, H, W, 2).view(torch.int64).view(B, H, W)            # discrete: the bands, and the present comparison
    be.call("stx_argmax_fwd", dx, a, B, D, H * W)
    Gd.check(what + ":argmax")
    assert torch.equal(a.cpu(), O.argmax_disparity_estimator(x, D).squeeze(1))
    verdict.done()


@pytest.mark.parametrize("case", [(2, 32, 5, 9, 21), (1, 48, 4, 7, 22), (1, 192, 6, 40, 31), (2, 16, 6, 10, 0), (1, 608, 2, 5, 3)],
                         ids=lambda c: "x".join(map(str, c)))
def test_modal_estimators_in_bands(be, case):
    """The modal estimators choose a mode: discrete outputs, no ratio.  Guard bands, and the comparison of tests/test_kernels.py."""
    from stereo_toolbox_amd.utils import synthetic_modal_volume, synthetic_tensor
    B, D, H, W, seed = case
    x = synthetic_modal_volume(B, D, H, W, seed) if seed else torch.softmax(synthetic_tensor((B, D, H, W), 13) * 4, 1)
    Gd = Guards(be)
    d = Gd.inp(x)
    for entry, ref in (("stx_unimodal_fwd", O.unimodal_disparity_estimator), ("stx_dominant_modal_fwd", O.dominant_modal_disparity_estimator)):
        o = Gd.out(B, H * W)
        be.call(entry, d, o, B, D, H * W)
        Gd.check(entry)
        want = ref(x, D).reshape(B, H * W)
        bad = ((o.cpu() - want).abs() > 1e-4 * (1 + want.abs())).sum().item()
        assert bad <= (0 if entry == "stx_unimodal_fwd" else B * H * W // 100), f"{entry}: {bad} pixels differ"


@pytest.mark.parametrize("scale", [1.0, 28.0])
def test_group_normalize(be, verdict, scale):
    """stx_group_normalize_fwd / _bwd against F.normalize and its autograd: 28 channels per group, a ragged last block of pixels,
    out_scale.  The clamped (all-zero) group's gradient is scale / eps * gy, 1e12-sized: compared on its own, as before."""
    B, C, G, H, W = 2, 56, 2, 3, 70
    g = _gen(3)
    x, gy = _randn(g, B, C, H, W), _randn(g, B, C, H, W)
    x[0, :28, 1, 5] = 0.0
    live = torch.ones(B, C, H, W, dtype=torch.bool)
    live[0, :28, 1, 5] = False
    (y_ref,), grads = _refs(lambda x: F.normalize(x.view(B, G, C // G, H, W), dim=2).view(B, C, H, W) * scale, (x,), gy, (0,))
    what = f"group_normalize[{be.name}:{scale:g}]"
    Gd = Guards(be)
    dx, y, gx = Gd.inp(x), Gd.out(B, C, H, W), Gd.out(B, C, H, W)
    be.call("stx_group_normalize_fwd", dx, y, B, C, G, H * W, scale)
    Gd.check(what)
    be.call("stx_group_normalize_bwd", dx, Gd.inp(gy), gx, B, C, G, H * W, scale)
    Gd.check(what + ":gx")
    verdict.within(y.cpu(), *y_ref, VALUE_FACTOR, what + ":y")
    want = grads[0][0]
    assert torch.allclose(gx.cpu()[~live].double(), want[~live], rtol=1e-5)
    with _one_thread():
        xr = x.clone().requires_grad_()
        (F.normalize(xr.view(B, G, C // G, H, W), dim=2).view(B, C, H, W) * scale).backward(gy)
    verdict.within(gx.cpu()[live], want[live], _dist(xr.grad[live], want[live]), GRAD_FACTOR, what + ":gx")
    verdict.done()


# ------------------------------------------------------------------------------------------ conv2d
C2_CASES = [
    # B, Cin, Cout, H, W, groups
    (1, 32, 32, 8, 16, 1),        # one tile
    (2, 64, 64, 19, 37, 2),       # ragged rows and columns, two views
    (2, 32, 48, 9, 50, 1),        # three output slices, runs crossing slices
    (4, 64, 16, 24, 33, 2),       # one slice, two images per view
    (1, 64, 128, 16, 16, 1),      # eight slices on two tiles: most workgroups idle
]
C2_DGRAD_CASES = [(1, 32, 32, 8, 16), (2, 64, 64, 19, 37), (1, 32, 64, 10, 20), (2, 64, 32, 9, 18)]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _c2_inputs(shape, seed):
    B, Ci, Co, H, W = shape
    g = _gen(seed)
    return _randn(g, B, Ci, H, W), _randn(g, Co, Ci, 3, 3) * 0.1, _randn(g, B, Co, H, W)


def _run_conv2d(be, Gd, what, x, w, dgrad, groups, want_stats):
    """x: NCHW-logical input of the launch; w: the layer's parameter [Cout][Cin][3][3] (read in its channels_last storage)."""
    Co, Ci = w.shape[:2]
    Kin, Nout = (Co, Ci) if dgrad else (Ci, Co)
    assert be.raw("stx_conv2d_supported")(Kin, Nout)
    B, _, H, W = x.shape
    out = Gd.out(B, H, W, Nout)
    rows = int(be.raw("stx_conv2d_stat_rows")(groups))
    stats = Gd.out(rows, 2, Nout) if want_stats else None
    be.call("stx_conv2d_fwd", Gd.inp(_nhwc(x)), Gd.inp(w.permute(0, 2, 3, 1).contiguous()), out, stats, B, H, W, Kin, Nout, int(dgrad), groups)
    Gd.check(what)
    return out.cpu().permute(0, 3, 1, 2), stats, rows


@functools.lru_cache(maxsize=None)
def _c2_fwd_ref(shape):
    x, w, _ = _c2_inputs(shape, 7)
    with _one_thread():
        return F.conv2d(x.double(), w.double(), None, 1, 1), F.conv2d(x, w, None, 1, 1)


@pytest.mark.parametrize("case", C2_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_forward_and_statistics(be, verdict, case):
    """stx_conv2d_fwd with its fused BatchNorm statistics, judged per view: rows [g * rows / G, (g + 1) * rows / G) belong to view g."""
    B, Ci, Co, H, W, G = case
    x, w, _ = _c2_inputs(case[:5], 7)
    r64, r32 = _c2_fwd_ref(case[:5])
    what = f"conv2d_fwd[{be.name}:" + "x".join(map(str, case)) + "]"
    got, stats, rows = _run_conv2d(be, Guards(be), what, x, w, False, G, True)
    verdict.within(got, r64, _dist(r32, r64), VALUE_FACTOR, what)
    assert rows % G == 0 and not torch.isnan(stats).any()
    st = stats.cpu().view(G, rows // G, 2, Co).double().sum(1)

    def views(r):                        # [G][C][voxels of the view] -> rows of voxels per (view, channel)
        return r.reshape(G, B // G, Co, H * W).permute(1, 3, 0, 2).reshape(-1, G, Co)
    s64, q64 = views(r64).sum(0), (views(r64) ** 2).sum(0)
    verdict.within(st[:, 0], s64, _dist(_seq_sum(views(r32)), s64), VALUE_FACTOR, what + ":sum")
    verdict.within(st[:, 1], q64, _dist(_seq_sum(views(r32) ** 2), q64), VALUE_FACTOR, what + ":sumsq")
    verdict.done()


@functools.lru_cache(maxsize=None)
def _c2_dgrad_ref(shape):
    x, w, gy = _c2_inputs(shape, 11)
    _, grads = _refs(lambda x, w: F.conv2d(x, w, None, 1, 1), (x, w), gy, (0,))
    return grads[0]


@pytest.mark.parametrize("case", C2_DGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_data_gradient(be, verdict, case):
    """The same kernel on the flipped, channel-transposed weight (dgrad = 1) against autograd through F.conv2d."""
    _, w, gy = _c2_inputs(case, 11)
    what = f"conv2d_dgrad[{be.name}:" + "x".join(map(str, case)) + "]"
    got, _, _ = _run_conv2d(be, Guards(be), what, gy, w, True, 1, False)
    verdict.within(got, *_c2_dgrad_ref(case), GRAD_FACTOR, what)
    verdict.done()


# ------------------------------------------------------------------------------------------ the entries of PAST_THE_FACTOR, without a kernel
def _one_chain2d(xp, w):
    """The 3x3 convolution of the padded xp [B][Cin][H+2][W+2] with w [Cout][Cin][3][3], every output as ONE sequential fp32 chain
    over (tap, channel) -- the MFMA accumulator of csrc/conv2d.hip: plain torch, one rounded product added per step."""
    H, W = xp.shape[2] - 2, xp.shape[3] - 2
    acc = torch.zeros(xp.shape[0], w.shape[0], H, W)
    for kh in range(3):
        for kw in range(3):
            for c in range(xp.shape[1]):
                acc += xp[:, c:c + 1, kh:kh + H, kw:kw + W] * w[:, c, kh, kw].view(1, -1, 1, 1)
    return acc


ONE_CHAIN = {"fwd_64": ("conv2d_fwd[2x64x64x19x37x2]", (2, 64, 64, 19, 37)), "dgrad_32": ("conv2d_dgrad[1x32x32x8x16]", (1, 32, 32, 8, 16)),
             "dgrad_32_64": ("conv2d_dgrad[1x32x64x10x20]", (1, 32, 64, 10, 20))}


@pytest.mark.parametrize("which", ONE_CHAIN)
def test_one_fp32_chain_is_past_the_factor(which):
    """The reason behind the conv2d rows of PAST_THE_FACTOR, on the CPU and without a kernel: the same convolution in plain fp32,
    exact but for adding the 9 * Cin products of an output one after the other, is refused by the very `within` call, with the
    very d_ref, of the listed cases -- the CPU reference blocks its sums -- yet stays below the 7 x where a bf16 split begins."""
    what, shape = ONE_CHAIN[which]
    if which.startswith("fwd"):
        x, w, _ = _c2_inputs(shape, 7)
        r64, r32 = _c2_fwd_ref(shape)
        want, live, factor, chain = r64, _dist(r32, r64), VALUE_FACTOR, _one_chain2d(F.pad(x, (1,) * 4), w)
    else:                            # gx = the convolution of gy with the weight transposed and mirrored
        _, w, gy = _c2_inputs(shape, 11)
        (want, live), factor = _c2_dgrad_ref(shape), GRAD_FACTOR
        chain = _one_chain2d(F.pad(gy, (1,) * 4), w.transpose(0, 1).flip(2, 3))
    dref = _dref(what, live)
    err = _dist(chain, want)
    print(f"one chain, {which}: {err / dref:.2f} x d_ref")
    assert err < 7 * dref, (which, err, dref)
    with pytest.raises(AssertionError, match="one chain"):
        within(chain, want, dref, factor, f"one chain, {which}")


# ------------------------------------------------------------------------------------------ the rule and the bands themselves
def _refused(near_miss, want, what, live, factor, tag):
    """The near miss is refused by the very `within` call, with the very recorded d_ref, that the kernels of `what` pass."""
    with pytest.raises(AssertionError, match=tag):
        within(near_miss, want, _dref(what, live), factor, tag)


def _bf16(t):
    return t.bfloat16().float()


def test_the_rule_refuses_a_group_correlation_from_bf16_features():
    (Lg, Rg, Lc, Rc), _, v64, v32, _ = _cv_ref(GC)
    G = GC[2]
    miss = O.build_gwc_volume(_bf16(Lg), _bf16(Rg), GC[6], G)
    _refused(miss, v64[:, :G], "cost_volume[mfma:" + "x".join(map(str, GC)) + "]:vol", _dist(v32[:, :G], v64[:, :G]), VALUE_FACTOR, "bf16 features")


def test_the_rule_refuses_the_head_with_the_other_interpolation_rule():
    case = HEAD_CASES[1]
    cost, gd, (want, live), (gwant, glive) = _head_ref(case, 0)
    B, Dc, Hc, Wc, D, H, W, _ = case
    c = cost.clone().requires_grad_()
    miss = O.regression_head(c, D, H, W, align_corners=True)
    miss.backward(gd)
    name = "head2[hp:" + "x".join(map(str, case)) + "]"
    _refused(miss.detach(), want, name + ":disp", live, VALUE_FACTOR, "other align_corners")
    _refused(c.grad, gwant, name + ":gcost", glive, GRAD_FACTOR, "other align_corners")


def test_the_rule_refuses_the_biased_variance_in_the_running_buffer():
    (z1, *_), rm, rv, _, _, _, _, (want, live) = _bn_ref("1000x32_relu")
    miss = 0.9 * rv + 0.1 * z1.var(0, unbiased=False)
    _refused(miss, want, "bn[1000x32_relu:y]:rv", live, VALUE_FACTOR, "biased variance")


def test_the_rule_refuses_a_batchnorm_backward_without_the_mean_of_the_gradient():
    (z1, z2, g1, b1, _, _), _, _, gy, _, grads, _, _ = _bn_ref("500x32_res")           # no activation: g = gy
    mean, invstd = z1.mean(0), 1.0 / torch.sqrt(z1.var(0, unbiased=False) + 1e-5)
    xhat = (z1 - mean) * invstd
    miss = g1 * invstd * (gy - xhat * (gy * xhat).mean(0))
    _refused(miss, grads[0][0], "bn[500x32_res:y]:dz1", grads[0][1], GRAD_FACTOR, "no mean-of-gradient term")


def test_the_rule_refuses_mish_by_its_large_x_shortcut():
    x, _ = _mish_input()
    (want, live), = _refs(lambda x: x * torch.tanh(F.softplus(x)), (x,))[0]
    _refused(x * torch.tanh(x), want, "mish[edges]:y", live, VALUE_FACTOR, "large-x shortcut")


def test_the_rule_refuses_a_two_term_bf16_split_of_conv2d():
    shape = C2_CASES[0][:5]
    x, w, _ = _c2_inputs(shape, 7)
    r64, r32 = _c2_fwd_ref(shape)
    (a_hi, a_lo), (b_hi, b_lo) = ((_bf16(t), _bf16(t - _bf16(t))) for t in (x, w))
    fn = lambda x, w: F.conv2d(x, w, None, 1, 1)  # noqa: E731
    with _one_thread():
        split = fn(a_hi, b_hi) + fn(a_hi, b_lo) + fn(a_lo, b_hi)
    _refused(split, r64, "conv2d_fwd[" + "x".join(map(str, C2_CASES[0])) + "]", _dist(r32, r64), VALUE_FACTOR, "bf16 split")


def test_guards_catch_a_host_write_on_either_side_of_an_output_buffer():
    """A deliberate write of the HOST (torch) one float in front of and one float behind a Guards.out buffer fails `check`; a
    write inside does not.  No kernel is made to write out of bounds."""
    Gd = Guards(Backend("emu"))
    small, ws = Gd.out(3, 2, 20), Gd.out(1000)
    Gd.check("untouched")
    for view in (small, ws):
        n, band = view.numel(), view.storage_offset()
        whole = torch.empty(0).set_(view.untyped_storage())
        view.fill_(1.0)
        Gd.check("written inside")
        for at in (band - 1, band + n):
            old = whole[at].item()
            whole[at] = 1.0
            with pytest.raises(AssertionError, match="guard band"):
                Gd.check("one float outside")
            whole[at] = old
            Gd.check("restored")


def test_listed_share():
    """At most LISTED_SHARE of the module's (case, tensor) pairs -- the entries of the recorded d_ref table -- are listed, per backend."""
    pairs = len(_dref.table()) if not _dref.record else None
    for backend in ("emu", "hip"):
        other = "hip" if backend == "emu" else "emu"
        listed = sum(len(r.split(", ")) for name, r in PAST_THE_FACTOR.items() if f"[{other}-" not in name)
        assert pairs is None or listed <= LISTED_SHARE * pairs, (backend, listed, pairs)


def _ac_lerp(n_in, n_out):
    """csrc/head.hip::hd_src under align_corners=True, in fp32: i0, i1, t of every output index."""
    s = (torch.tensor(float(n_in - 1)) / torch.tensor(float(n_out - 1))) * torch.arange(n_out, dtype=torch.float32)
    i0 = s.floor().long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.float()


def test_a_logit_rounded_once_in_the_forward_and_twice_in_the_backward_is_past_the_factor():
    """The reason behind the gfx950-only row of PAST_THE_FACTOR, on the CPU and without a kernel.  The device build contracts
    (-ffp-contract=fast); the forward kernel's `w0 * c0 + w1 * c1 - m` then reaches exp() after ONE rounding, while the backward
    kernel forms x = (1 - t) * c0 + t * c1 first and subtracts the stored maximum from the ROUNDED x.  At cost steps of thousands
    (gain 3000: ulp(x) = 2.4e-4) the backward's exp(x - m) / s, s being the forward's sum, is off by up to 1e-4 of itself and the
    probabilities of a near-tie pixel no longer add up to one.  This restatement -- plain fp32 torch in the kernels' order, the
    forward's x - m with one rounding, the exact maximum as the shift (the LDS kernel redoes its walk there) -- is refused by the
    very `within` call, with the very d_ref, of the listed gradient, at 5.01 x (gfx950: 5.08 x); the host build contracts nothing
    and sits at 1.11 x.  Nothing but this case (|logits| of thousands) is affected: at gain <= 40 both backends agree."""
    case = HEAD_CASES[6]
    name = "head2[ac:" + "x".join(map(str, case)) + "]:gcost"
    cost, gd, _, (want, live) = _head_ref(case, 1)
    B, Dc, Hc, Wc, D, H, W, _ = case
    (d0, d1, td), (h0, h1, th), (w0, w1, tw) = _ac_lerp(Dc, D), _ac_lerp(Hc, H), _ac_lerp(Wc, W)
    td, th, tw, steps = td.view(D, 1, 1), th.view(1, H, 1), tw.view(1, 1, W), torch.arange(D, dtype=torch.float32).view(D, 1, 1)
    c = cost.clone().requires_grad_()
    p = c[0, 0]
    a, b, cc, dd = p[:, h0][:, :, w0], p[:, h0][:, :, w1], p[:, h1][:, :, w0], p[:, h1][:, :, w1]
    planes = (1 - th) * ((1 - tw) * a + tw * b) + th * ((1 - tw) * cc + tw * dd)                 # hd_sample
    c0, c1 = planes[d0], planes[d1]
    x = (1 - td) * c0 + td * c1                                                                  # the backward's logit: rounded
    m = x.detach().amax(0, keepdim=True)
    once = ((1 - td).double() * c0.detach().double() + td.double() * c1.detach().double() - m.double()).float()   # the forward's x - m
    e = torch.exp(once)
    s = e.sum(0, keepdim=True)
    disp = (e * steps).sum(0, keepdim=True) / s
    gl = gd[0] * (torch.exp(x.detach() - m) / s) * (steps - disp)                                # head_bwd_pix_kernel
    (x * gl).sum().backward()
    dref = _dref(name, live)
    err = _dist(c.grad, want)
    print(f"logit rounded once / twice, gain 3000: {err / dref:.2f} x d_ref")
    assert err < 7 * dref, (err, dref)
    with pytest.raises(AssertionError, match="rounded once"):
        within(c.grad, want, dref, GRAD_FACTOR, "rounded once / twice")
