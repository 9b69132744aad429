"""The kernels a model iteration of the iterative families runs, and the 2-D refinement helpers, under the fp64 parity rule, in guard
bands: geo_lookup.hip, corr1d.hip, allpairs.hip, convex_upsample.hip, convgru.hip, refine2d.hip.  (The benchmarked train step:
tests/test_conv3d_parity.py and tests/test_train_kernels_parity.py.)

The rule (tests/parity.py::within), for every call: `want64` is the operation in fp64 on the CPU from the same fp32 inputs cast up
(stock torch ops, the oracle/torch_oracle.py or tests/restated.py restatement, and autograd through them), `d_ref` = max|one-thread
fp32 CPU run of the same expression - want64| over the same tensor (recorded, see DREF_PATH), and the kernel may sit at most
VALUE_FACTOR (forward values, pyramids, statistics, the loss) or GRAD_FACTOR (gradients) times d_ref away from want64; where d_ref
is zero (copies, lookups at integer positions) the floor of `within` applies.  Every tensor goes to the parity report.  Tensors the
rule refuses would be listed one by one with their ratio (PAST_THE_FACTOR, strict expected failures through
tests/parity.py::Verdict); none is: the table is empty on both backends.  The near misses at the end show that the rule refuses a
subtly wrong kernel of every family.

Guard bands (tests/backends.py::Guards): every buffer a kernel WRITES is cut from the middle of a larger allocation whose bands
are checked after the call; every workspace, pyramid, packed-weight and partial-sum buffer has exactly the count its query function
returns; every buffer a kernel READS sits between NaN bands, so that a read past either end that reaches an output fails the
parity assertion.  Accumulating outputs start from a non-zero addend (want64 = addend + gradient); pitched operands are 16-byte
aligned channel slices of ragged widths of ONE banded buffer whose other channels hold NaN.

Discontinuities are conditions on the INPUTS, asserted from the fp64 reference: no lookup position within 1e-3 of an integer
except those placed on one exactly, no warp pixel with an in-image weight sum within 1e-3 of 0.999, truncation confidences 1e-3
away from the threshold, gt values exact in fp32.  The comment of every case row names the edge it reaches.  Both backends through
the C-ABI: host emulator and gfx950.
"""
import contextlib
import ctypes
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_oracle as O
from tests.backends import Backend, Guards, be  # noqa: F401
from tests.golden.corr1d_config import DEFOM_SCALE_RADIUS, DEFOM_SCALES
from tests.golden.f1ops_config import CORR_CASES, VAR_CASES, WARP_CASES, corr_inputs, var_inputs, warp_inputs
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, RecordedDref, listed_verdict, within
from tests.restated import convex, corr1d_pyramid, estimates, lookup, pool, pyramids, sample, truncation_mask, upsample

# d_ref of every tensor below, recorded (tests/parity.py::RecordedDref); STX_ITERATIVE_KERNELS_DREF_RECORD=<path> runs the module
# with the live values and writes them to <path> (a new or changed case).
DREF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iterative_kernels_parity_dref.json")
_dref = RecordedDref(DREF_PATH, "STX_ITERATIVE_KERNELS_DREF_RECORD")

# the suffix of `what` that names a tensor of a call
TENSORS = ("gpyr", "cpyr", "out", "ggpyr", "gcpyr", "gvol", "gf1", "gf2", "gf1_alone", "gf2_alone", "gdisp", "gw", "gdisp_alone",
           "gw_alone", "gx", "gx_alone", "gref", "gtgt", "gref_alone", "gtgt_alone", "var", "conf", "gs", "gs_alone", "out_b",
           "disp_l", "conf_l", "disp_r", "conf_r", "g_all", "g_disp_l", "g_conf_l", "g_disp_r", "g_conf_r", "mask", "gflow", "gmask",
           "gflow_alone", "gmask_alone", "loss", "gpreds", "y0", "y0_add", "gate_z", "gate_rh", "gate_r", "gate_h", "gate_q", "gq", "gz",
           "gq_rows", "gz_rows", "gr", "gr_rows", "buf", "dw", "dw2", "rowsum", "dgrad")

# Tensors the rule refuses: test name -> "tensor ratio, tensor ratio".  A name without the backend holds for both; a name with it
# ("test_x[hip-...]") for that backend alone -- where the device build's contraction (-ffp-contract=fast; the host build contracts
# nothing) is part of the value.  The gfx950 ratios are those of profiles/iterative_kernels_parity_report_gfx950.jsonl.  An entry
# needs a kernel-free demonstration in this module (a plain torch loop in the kernel's order of additions that lands at the same
# ratio); strict: a case that starts to pass must leave the table.
# EMPTY: the candidates stay inside the factor, on both backends at the same two decimals.  Measured at most: the ConvGRU gemm
# 0.70 x on the forward values (allowed 2) and 2.34 x on the in-place data gradient of `two_src` (allowed 3), the gate epilogues
# 1.07 x, the weight gradient 1.26 x, the all-pairs estimates 0.46 x and their gradients 1.57 x.  The widest tensor of the module
# is the warp's disparity gradient at 2.57 x (allowed 3).
PAST_THE_FACTOR = {
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


def _uniform(g, lo, hi, *shape):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


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


def _refs(fn, ts, gys=(), wrt=()):
    """fn(*ts) (a tensor or a tuple of tensors; None operands pass through) in fp64 from the fp32 tensors cast up, and in fp32 on
    one thread.  Returns (outs, grads): outs = [(want64, ref32)] per output, grads = {i: (want64, ref32)} of sum_k <outs[k], gys[k]>
    (None entries of gys: no term) w.r.t. ts[i], i in wrt."""
    def run(dt):
        a = [None if t is None else (t.to(dt).clone().requires_grad_(i in wrt) if t.dtype.is_floating_point else t) for i, t in enumerate(ts)]
        y = fn(*a)
        ys = y if isinstance(y, tuple) else (y,)
        terms = [(v * g.to(dt)).sum() for v, g in zip(ys, gys) if g is not None]
        if terms and wrt:
            sum(terms).backward()
        return [v.detach() for v in ys], {i: a[i].grad for i in wrt}
    with _one_thread():
        (y64, g64), (y32, g32) = run(torch.float64), run(torch.float32)
    return list(zip(y64, y32)), {i: (g64[i], g32[i]) for i in wrt}


def _wd(ref, add=None):
    """(want64, d_ref) of a pair (want64, ref32); with `add` (fp32) both sides start from that addend: an accumulating output."""
    w, r = ref
    if add is not None:
        w, r = add.double() + w.reshape(add.shape), add + r.reshape(add.shape)
    return w, _dist(r, w)


def _call(be, Gd, what, name, *args):
    """One kernel call, and the check of every band of the test behind it."""
    be.call(name, *args)
    Gd.check(f"{what}:{name}")


def _out_from(Gd, t):
    """A Guards.out buffer that starts from `t`: an accumulating output between sentinel bands."""
    v = Gd.out(*t.shape)
    v.copy_(t)
    return v


def _ids(cases):
    return list(cases)


# ------------------------------------------------------------------------------------------ lookup positions
def _level_maps(levels):
    return [lambda t, i=i: t / 2 ** i for i in range(levels)]


def _away_from_integers(x, maps):
    """Nudges the entries of x whose position m(x), m of `maps` (the levels' x / 2^i, the scales' base - s x), comes within 2e-3
    of an integer without being one (the gradient of a linear interpolation jumps there: the fp32 and the fp64 reference would
    take different taps)."""
    x = x.clone()
    for _ in range(64):
        bad = torch.zeros_like(x, dtype=torch.bool)
        for m in maps:
            d = (m(x.double()) - m(x.double()).round()).abs()
            bad |= (d > 0) & (d < 2e-3)
        if not bad.any():
            return x
        x[bad] += 0.0137
    raise AssertionError("positions could not be moved off the integers")


def _positions(g, P, n, r, levels, call):
    """P sampling positions (level 0) on rows of n taps: seeded noise over [-r - 2, n + r + 1] off the integers, with planted
    ones -- on the FIRST and the LAST pixel of the buffer a window that straddles the left / the right end of its row (call 0)
    or lies wholly outside it (call 1: the first pixel's taps would come from in front of the buffer, the last pixel's from
    behind it), and behind the first pixel exact integers, x = n - 1, +-1e9 and the other side's edges."""
    x = _away_from_integers(_uniform(g, -r - 2.0, n + r + 1.0, P), _level_maps(levels))
    x[0], x[-1] = (-0.5, n - 1.5) if call == 0 else (-(r + 1.5), n - 1 + r + 1.25)
    plants = [0.0, n - 1.0, 1.0e9, -1.0e9, 3.0, n - 1 + r + 1.25, -(r + 1.5), n - 1.5, -0.5][:max(0, P - 2)]
    x[1:1 + len(plants)] = torch.tensor(plants)
    return x


def _assert_off_the_integers(x64, maps, what):
    """The condition on the inputs: no position within 1e-3 of an integer at any level, except those ON one exactly."""
    for i, m in enumerate(maps):
        d = (m(x64) - m(x64).round()).abs()
        assert bool(((d == 0) | (d > 1e-3)).all()), (what, i, d[(d != 0) & (d <= 1e-3)])


def _levels(flat, lead, n, C, L):
    """The flat pyramid buffer of include/stx_hip.h as views [*lead][n >> i][C], level after level."""
    out, off, rows = [], 0, math.prod(lead)
    for i in range(L):
        cnt = rows * (n >> i) * C
        out.append(flat[off:off + cnt].view(*lead, n >> i, C))
        off += cnt
    assert off == flat.numel(), (off, flat.numel())
    return out


def _pack(levels):
    return torch.cat([t.reshape(-1) for t in levels])


# ------------------------------------------------------------------------------------------ geo_lookup.hip
#                B  C   D    H  W   W2   Cf  levels radius        (tests/golden/geo_config.py)
GEO_CASES = {
    "r2_l3_odd": (2, 8, 13, 3, 18, 21, 8, 3, 2),           # three levels with odd tails dropped (13 -> 6 -> 3, 21 -> 10 -> 5), W2 != W, batch 2
    "c12": (2, 12, 13, 3, 18, 21, 8, 2, 3),                # three channel quads
    "l1_r3": (1, 4, 9, 2, 17, 17, 8, 1, 3),                # one level: the pyramids are copies (d_ref = 0)
    "deep_wt8_h1": (1, 8, 192, 1, 21, 24, 8, 3, 4),        # D * C = 1536: pixel tiles of 8 in geo_pyramid_kernel, W = 2 * 8 + 5
    "deep_wt4_h1": (1, 16, 192, 1, 11, 24, 8, 3, 4),       # D * C = 3072 > 963: pixel tiles of 4, W = 2 * 4 + 3
    "w2_301_h1": (1, 8, 12, 1, 17, 301, 8, 3, 4),          # W2 = 256 + 45: the second w2_0 round of the correlation, ragged tiles
    "px150": (2, 4, 6, 5, 15, 15, 4, 2, 1),                # 150 pixels: two lookup workgroups of 128, the batch boundary inside the first
}


@functools.lru_cache(maxsize=None)
def _geo_inputs(tag):
    B, C, D, H, W, W2, Cf, L, r = GEO_CASES[tag]
    g = _gen(100 + list(GEO_CASES).index(tag))
    P = B * H * W
    n_g, n_c = sum(P * (D >> i) * C for i in range(L)), sum(P * (W2 >> i) for i in range(L))
    vol, f1, f2 = _randn(g, B, D, H, W, C), _randn(g, B, Cf, H, W), _randn(g, B, Cf, H, W2)
    gpyr, cpyr = _randn(g, n_g), _randn(g, n_c)                        # the lookup's pyramids: any numbers, the layout is what counts
    calls = []
    for call in (0, 1):
        disp = _positions(g, P, D, r, L, call)
        xc = _positions(g, P, W2, r, L, call)
        coords = xc + disp                                             # the correlation row is sampled at coords - disp
        _assert_off_the_integers(disp.double(), _level_maps(L), f"{tag} disp")
        _assert_off_the_integers(coords.double() - disp.double(), _level_maps(L), f"{tag} coords - disp")
        calls.append((disp.view(B, 1, H, W), coords.view(B, 1, H, W), _randn(g, B, L * (C + 1) * (2 * r + 1), H, W)))
    return vol, f1, f2, gpyr, cpyr, calls, (_randn(g, n_g), _randn(g, n_c)), (_randn(g, n_g), _randn(g, n_c))


def _geo_lookup_fn(case):
    B, C, D, H, W, W2, Cf, L, r = case

    def fn(gflat, cflat, disp, coords):
        gp = [t.transpose(-1, -2) for t in _levels(gflat, (B, H, W), D, C, L)]
        cp = [t.squeeze(-1) for t in _levels(cflat, (B, H, W), W2, 1, L)]
        return lookup(gp, cp, disp, coords, r)
    return fn


def _geo_pyramid_fn(case):
    B, C, D, H, W, W2, Cf, L, r = case

    def fn(vol, f1, f2):
        gp, cp = pyramids(vol.permute(0, 4, 1, 2, 3), f1, f2, L)
        return _pack([t.transpose(-1, -2) for t in gp]), _pack(cp)
    return fn


@pytest.mark.parametrize("tag", _ids(GEO_CASES))
def test_geo_pyramids(be, verdict, tag):
    """stx_geo_pyramid_fwd / _bwd and stx_geo_corr_fwd / _bwd: every level of both pyramids in buffers of exactly
    stx_geo_pyramid_floats floats, and the gradients of every level back to the volume and the feature maps (each alone too)."""
    case = GEO_CASES[tag]
    B, C, D, H, W, W2, Cf, L, r = case
    vol, f1, f2, _, _, _, (gg, gc), _ = _geo_inputs(tag)
    (gp_ref, cp_ref), grads = _refs(_geo_pyramid_fn(case), (vol, f1, f2), (gg, gc), (0, 1, 2))
    what = f"geo_pyramids[{be.name}:{tag}]"
    n_g, n_c = (int(be.raw("stx_geo_pyramid_floats")(B * H * W, n, c, L)) for n, c in ((D, C), (W2, 1)))
    assert (n_g, n_c) == (gg.numel(), gc.numel())
    Gd = Guards(be)
    dvol, d1, d2 = Gd.inp(vol), Gd.inp(f1), Gd.inp(f2)
    gpyr, cpyr = Gd.out(n_g), Gd.out(n_c)
    _call(be, Gd, what, "stx_geo_pyramid_fwd", dvol, gpyr, B, D, H, W, C, L)
    _call(be, Gd, what, "stx_geo_corr_fwd", d1, d2, cpyr, B, Cf, H, W, W2, L)
    verdict.within(gpyr.cpu(), *_wd(gp_ref), VALUE_FACTOR, what + ":gpyr")
    verdict.within(cpyr.cpu(), *_wd(cp_ref), VALUE_FACTOR, what + ":cpyr")
    gvol, gf1, gf2 = Gd.out(B, D, H, W, C), Gd.out(B, Cf, H, W), Gd.out(B, Cf, H, W2)
    dgc = Gd.inp(gc)
    _call(be, Gd, what, "stx_geo_pyramid_bwd", Gd.inp(gg), gvol, B, D, H, W, C, L)
    _call(be, Gd, what, "stx_geo_corr_bwd", dgc, d1, d2, gf1, gf2, B, Cf, H, W, W2, L)
    verdict.within(gvol.cpu(), *_wd(grads[0]), GRAD_FACTOR, what + ":gvol")
    verdict.within(gf1.cpu(), *_wd(grads[1]), GRAD_FACTOR, what + ":gf1")
    verdict.within(gf2.cpu(), *_wd(grads[2]), GRAD_FACTOR, what + ":gf2")
    a1, a2 = Gd.out(B, Cf, H, W), Gd.out(B, Cf, H, W2)
    _call(be, Gd, what, "stx_geo_corr_bwd", dgc, d1, d2, a1, None, B, Cf, H, W, W2, L)
    _call(be, Gd, what, "stx_geo_corr_bwd", dgc, d1, d2, None, a2, B, Cf, H, W, W2, L)
    verdict.within(a1.cpu(), *_wd(grads[1]), GRAD_FACTOR, what + ":gf1_alone")
    verdict.within(a2.cpu(), *_wd(grads[2]), GRAD_FACTOR, what + ":gf2_alone")
    verdict.done()


@functools.lru_cache(maxsize=None)
def _geo_lookup_ref(tag):
    case = GEO_CASES[tag]
    _, _, _, gpyr, cpyr, calls, _, _ = _geo_inputs(tag)
    fn = _geo_lookup_fn(case)
    (da, ca, ga), (db, cb, gb) = calls
    return _refs(lambda g, c: (fn(g, c, da.to(g.dtype), ca.to(g.dtype)), fn(g, c, db.to(g.dtype), cb.to(g.dtype))), (gpyr, cpyr), (ga, gb), (0, 1))


@pytest.mark.parametrize("tag", _ids(GEO_CASES))
def test_geo_lookup(be, verdict, tag):
    """stx_geo_lookup_fwd / _bwd with two position sets: a window that leaves its row reads zeros, not the neighbouring pixel's
    row or the NaN band (first / last pixel of the buffer); the backward ADDS, twice into one buffer that starts from a non-zero
    addend, as the product's iterations do -- want64 = addend + both gradients; either pyramid's gradient alone."""
    B, C, D, H, W, W2, Cf, L, r = GEO_CASES[tag]
    _, _, _, gpyr, cpyr, calls, _, (add_g, add_c) = _geo_inputs(tag)
    outs, grads = _geo_lookup_ref(tag)
    what = f"geo_lookup[{be.name}:{tag}]"
    Gd = Guards(be)
    dg, dc = Gd.inp(gpyr), Gd.inp(cpyr)
    ggpyr, gcpyr, only_g, only_c = (_out_from(Gd, t) for t in (add_g, add_c, add_g, add_c))
    for k, (disp, coords, gout) in enumerate(calls):
        dd, dco, dgo = Gd.inp(disp), Gd.inp(coords), Gd.inp(gout)
        out = Gd.out(B, L * (C + 1) * (2 * r + 1), H, W)
        _call(be, Gd, what, "stx_geo_lookup_fwd", dg, dc, dd, dco, out, B, H, W, D, C, W2, L, r)
        verdict.within(out.cpu(), *_wd(outs[k]), VALUE_FACTOR, what + (":out", ":out_b")[k])
        _call(be, Gd, what, "stx_geo_lookup_bwd", dgo, dd, dco, ggpyr, gcpyr, B, H, W, D, C, W2, L, r)
        _call(be, Gd, what, "stx_geo_lookup_bwd", dgo, dd, dco, only_g, None, B, H, W, D, C, W2, L, r)
        _call(be, Gd, what, "stx_geo_lookup_bwd", dgo, dd, dco, None, only_c, B, H, W, D, C, W2, L, r)
    verdict.within(ggpyr.cpu(), *_wd(grads[0], add_g), GRAD_FACTOR, what + ":ggpyr")
    verdict.within(gcpyr.cpu(), *_wd(grads[1], add_c), GRAD_FACTOR, what + ":gcpyr")
    assert torch.equal(only_g.cpu(), ggpyr.cpu()) and torch.equal(only_c.cpu(), gcpyr.cpu())
    verdict.done()


UP_CASES = {"b2_5x7": (2, 5, 7), "b1_3x18": (1, 3, 18)}          # B, h, w (tests/golden/geo_config.py): batch stride; W across a tile


@functools.lru_cache(maxsize=None)
def _up_inputs(tag):
    B, h, w = UP_CASES[tag]
    g = _gen(150 + list(UP_CASES).index(tag))
    return _uniform(g, 0.0, 40.0, B, 1, h, w), torch.softmax(2 * _randn(g, B, 9, 4 * h, 4 * w), 1), _randn(g, B, 4 * h, 4 * w)


@pytest.mark.parametrize("tag", _ids(UP_CASES))
def test_context_upsample(be, verdict, tag):
    """stx_context_upsample_fwd / _bwd: the 3 x 3 taps at the image border read zeros; each gradient alone."""
    B, h, w = UP_CASES[tag]
    disp, wts, gy = _up_inputs(tag)
    (out_ref,), grads = _refs(upsample, (disp, wts), (gy,), (0, 1))
    what = f"context_upsample[{be.name}:{tag}]"
    Gd = Guards(be)
    dd, dw, dg = Gd.inp(disp), Gd.inp(wts), Gd.inp(gy)
    out, gd, gw, gd1, gw1 = Gd.out(B, 4 * h, 4 * w), Gd.out(B, 1, h, w), Gd.out(B, 9, 4 * h, 4 * w), Gd.out(B, 1, h, w), Gd.out(B, 9, 4 * h, 4 * w)
    _call(be, Gd, what, "stx_context_upsample_fwd", dd, dw, out, B, h, w)
    _call(be, Gd, what, "stx_context_upsample_bwd", dg, dd, dw, gd, gw, B, h, w)
    _call(be, Gd, what, "stx_context_upsample_bwd", dg, dd, dw, gd1, None, B, h, w)
    _call(be, Gd, what, "stx_context_upsample_bwd", dg, dd, dw, None, gw1, B, h, w)
    verdict.within(out.cpu(), *_wd(out_ref), VALUE_FACTOR, what + ":out")
    for got, i, name in ((gd, 0, "gdisp"), (gw, 1, "gw"), (gd1, 0, "gdisp_alone"), (gw1, 1, "gw_alone")):
        verdict.within(got.cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


# ------------------------------------------------------------------------------------------ corr1d.hip
#                    kind    B  Cf  H  W1  W2   L  r        (tests/golden/corr1d_config.py)
C1_CASES = {
    "raft_l4_r4": ("raft", 1, 12, 3, 20, 27, 4, 4),        # 27 -> 13 -> 6 -> 3: an odd tail dropped at levels 0 and 1; W1 = 16 + 4
    "raft_b2_l3_r2": ("raft", 2, 8, 2, 18, 21, 3, 2),      # batch 2, 21 -> 10 -> 5
    "defom": ("defom", 1, 8, 3, 20, 20, 2, 4),             # disparity-indexed jobs (alpha = 1), then the scaling list's eight jobs
    "w2_301_h1": ("raft", 1, 8, 1, 17, 301, 4, 4),         # W2 = 256 + 45: a second w2 round, 301 -> 150 -> 75 -> 37
    "px150": ("raft", 2, 4, 5, 15, 15, 2, 2),              # 150 pixels: two lookup workgroups, disp == NULL like every raft row
}


def _c1_jobs(case, call):
    kind, B, Cf, H, W1, W2, L, r = case
    if kind == "defom" and call == 1:
        return [(0, DEFOM_SCALE_RADIUS, s, 1.0) for s in DEFOM_SCALES]
    return [(i, r, 1.0 if kind == "defom" else 0.0, 2.0 ** -i) for i in range(L)]


def _c1_lookup(cp, base, disp, jobs):
    """The header's job list in plain torch: job (level, radius, alpha, mult) samples at (base - alpha disp) mult + k."""
    out = []
    for lvl, r, alpha, mult in jobs:
        x = base if disp is None else base - alpha * disp
        out.append(sample(cp[lvl], (x * mult).unsqueeze(-1) + torch.arange(-r, r + 1, dtype=base.dtype)))
    return torch.cat(out, -1).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _c1_inputs(tag):
    case = C1_CASES[tag]
    kind, B, Cf, H, W1, W2, L, r = case
    g = _gen(200 + list(C1_CASES).index(tag))
    P = B * H * W1
    n_c = sum(P * (W2 >> i) for i in range(L))
    f1, f2, cpyr = _randn(g, B, Cf, H, W1), _randn(g, B, Cf, H, W2), _randn(g, n_c)
    calls = []
    for call in (0, 1):
        jobs = _c1_jobs(case, call)
        x = _positions(g, P, W2, max(j[1] for j in jobs), 1 if kind == "defom" and call == 1 else L, call)
        if kind == "defom":                          # base = the pixel's column, disp such that base - disp is the position
            base = torch.arange(W1, dtype=torch.float32).repeat(B * H)
            maps = [lambda d, a=alpha, m=mult: (base.double() - a * d) * m for _, _, alpha, mult in jobs]
            disp = _away_from_integers(base - x, maps)
            _assert_off_the_integers(disp.double(), maps, f"{tag} jobs")
            disp = disp.view(B, H, W1)
        else:
            base, disp = x, None
            _assert_off_the_integers(x.double(), _level_maps(L), f"{tag} base")
        calls.append((base.view(B, H, W1), disp, jobs, _randn(g, B, sum(2 * j[1] + 1 for j in jobs), H, W1)))
    return f1, f2, cpyr, calls, _randn(g, n_c), _randn(g, n_c)


def _jobs_array(jobs):
    flat = [float(v) for job in jobs for v in job]
    return (ctypes.c_float * len(flat))(*flat), len(jobs)


@pytest.mark.parametrize("tag", _ids(C1_CASES))
def test_corr1d_pyramid(be, verdict, tag):
    """stx_corr1d_pyramid_fwd / _bwd: level 0 on the matrix cores and the pooled levels in stx_corr1d_pyramid_floats floats; the
    gradient of every level back to the feature maps, each alone too."""
    kind, B, Cf, H, W1, W2, L, r = C1_CASES[tag]
    f1, f2, _, _, gc, _ = _c1_inputs(tag)
    (cp_ref,), grads = _refs(lambda a, b: _pack(corr1d_pyramid(a, b, L)), (f1, f2), (gc,), (0, 1))
    what = f"corr1d_pyramid[{be.name}:{tag}]"
    n_c = int(be.raw("stx_corr1d_pyramid_floats")(B * H * W1, W2, L))
    assert n_c == gc.numel()
    scale = 1.0 / math.sqrt(Cf)
    Gd = Guards(be)
    d1, d2, dgc = Gd.inp(f1), Gd.inp(f2), Gd.inp(gc)
    cpyr = Gd.out(n_c)
    _call(be, Gd, what, "stx_corr1d_pyramid_fwd", d1, d2, cpyr, B, Cf, H, W1, W2, L, scale)
    verdict.within(cpyr.cpu(), *_wd(cp_ref), VALUE_FACTOR, what + ":cpyr")
    gf1, gf2, a1, a2 = Gd.out(B, Cf, H, W1), Gd.out(B, Cf, H, W2), Gd.out(B, Cf, H, W1), Gd.out(B, Cf, H, W2)
    _call(be, Gd, what, "stx_corr1d_pyramid_bwd", dgc, d1, d2, gf1, gf2, B, Cf, H, W1, W2, L, scale)
    _call(be, Gd, what, "stx_corr1d_pyramid_bwd", dgc, d1, d2, a1, None, B, Cf, H, W1, W2, L, scale)
    _call(be, Gd, what, "stx_corr1d_pyramid_bwd", dgc, d1, d2, None, a2, B, Cf, H, W1, W2, L, scale)
    for got, i, name in ((gf1, 0, "gf1"), (gf2, 1, "gf2"), (a1, 0, "gf1_alone"), (a2, 1, "gf2_alone")):
        verdict.within(got.cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


@functools.lru_cache(maxsize=None)
def _c1_lookup_ref(tag):
    kind, B, Cf, H, W1, W2, L, r = C1_CASES[tag]
    _, _, cpyr, calls, _, _ = _c1_inputs(tag)

    def fn(flat):
        cp = [t.squeeze(-1) for t in _levels(flat, (B, H, W1), W2, 1, L)]
        return tuple(_c1_lookup(cp, base.to(flat.dtype), None if disp is None else disp.to(flat.dtype), jobs) for base, disp, jobs, _ in calls)
    return _refs(fn, (cpyr,), [c[3] for c in calls], (0,))


@pytest.mark.parametrize("tag", _ids(C1_CASES))
def test_corr1d_lookup(be, verdict, tag):
    """stx_corr1d_lookup_fwd / _bwd with two position sets (a DEFOM row: the level jobs, then the scaling list's eight jobs; a RAFT
    row: disp == NULL); the backward twice into one buffer that starts from a non-zero addend."""
    kind, B, Cf, H, W1, W2, L, r = C1_CASES[tag]
    _, _, cpyr, calls, _, add = _c1_inputs(tag)
    outs, grads = _c1_lookup_ref(tag)
    what = f"corr1d_lookup[{be.name}:{tag}]"
    Gd = Guards(be)
    dc = Gd.inp(cpyr)
    gcpyr = _out_from(Gd, add)
    for k, (base, disp, jobs, gout) in enumerate(calls):
        arr, nj = _jobs_array(jobs)
        db, dd = Gd.inp(base), Gd.inp(disp)
        out = Gd.out(*gout.shape)
        _call(be, Gd, what, "stx_corr1d_lookup_fwd", dc, db, dd, arr, nj, out, B, H, W1, W2, L)
        verdict.within(out.cpu(), *_wd(outs[k]), VALUE_FACTOR, what + (":out", ":out_b")[k])
        _call(be, Gd, what, "stx_corr1d_lookup_bwd", Gd.inp(gout), db, dd, arr, nj, gcpyr, B, H, W1, W2, L)
    verdict.within(gcpyr.cpu(), *_wd(grads[0], add), GRAD_FACTOR, what + ":gcpyr")
    verdict.done()


# ------------------------------------------------------------------------------------------ refine2d.hip
#             B  C  H  W   lo    hi      (tests/golden/f1ops_config.py, and a one-column image)
WARP = {**{n: c for n, *c in WARP_CASES}, "w1": (1, 2, 3, 1, -0.4, 0.4)}


@functools.lru_cache(maxsize=None)
def _warp_inputs(tag):
    B, C, H, W, lo, hi = WARP[tag]
    x, d, g = warp_inputs(B, C, H, W, lo, hi, 100 + 10 * list(WARP).index(tag))
    if W == 1:                                     # a one-column image is sampled at -disp - 1/2: inside only at disp = -1/2 exactly
        d = d.clone()
        d[0, 0, 0, 0] = d[0, 0, 2, 0] = -0.5
    # the condition on the inputs: the validity mask is a step at an in-image weight sum of 0.999
    xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W).expand(B, 1, H, W)
    yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1).expand(B, 1, H, W)
    grid = torch.cat((2.0 * (xx - d.double()) / max(W - 1, 1) - 1.0, 2.0 * yy / max(H - 1, 1) - 1.0), 1).permute(0, 2, 3, 1)
    wsum = F.grid_sample(torch.ones(B, 1, H, W, dtype=torch.float64), grid, align_corners=False)
    assert bool(((wsum - 0.999).abs() > 1e-3).all()), (tag, (wsum - 0.999).abs().min())
    return x, d, g


@pytest.mark.parametrize("tag", _ids(WARP))
def test_warp(be, verdict, tag):
    """stx_warp_fwd / _bwd against the oracle's grid_sample form; each gradient alone."""
    B, C, H, W, _, _ = WARP[tag]
    x, d, g = _warp_inputs(tag)
    (out_ref,), grads = _refs(O.pcw_warp, (x, d), (g,), (0, 1))
    what = f"warp[{be.name}:{tag}]"
    Gd = Guards(be)
    dx, dd, dg = Gd.inp(x), Gd.inp(d), Gd.inp(g)
    out, gx, gd, gx1, gd1 = Gd.out(B, C, H, W), Gd.out(B, C, H, W), Gd.out(B, 1, H, W), Gd.out(B, C, H, W), Gd.out(B, 1, H, W)
    _call(be, Gd, what, "stx_warp_fwd", dx, dd, out, B, C, H, W)
    _call(be, Gd, what, "stx_warp_bwd", dg, dx, dd, gx, gd, B, C, H, W)
    _call(be, Gd, what, "stx_warp_bwd", dg, dx, dd, gx1, None, B, C, H, W)
    _call(be, Gd, what, "stx_warp_bwd", dg, dx, dd, None, gd1, B, C, H, W)
    verdict.within(out.cpu(), *_wd(out_ref), VALUE_FACTOR, what + ":out")
    for got, i, name in ((gx, 0, "gx"), (gd, 1, "gdisp"), (gx1, 0, "gx_alone"), (gd1, 1, "gdisp_alone")):
        verdict.within(got.cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


#              B  C   H  W    maxdisp groups
CORR = {**{n: c for n, *c in CORR_CASES},                  # W = 37 (odd), 52, 140 (two column tiles)
        "md0": (2, 3, 3, 5, 0, 3),                         # maxdisp = 0: one slice
        "md_eq_w": (1, 40, 2, 24, 24, 1),                  # maxdisp = W
        "md48_w130": (1, 4, 1, 130, 48, 2),                # the 48-disparity instantiation, W = 128 + 2: the halo across the tile edge
        "cpg33": (1, 66, 2, 21, 3, 2)}                     # C / groups = 33: a second staged channel pass


@pytest.mark.parametrize("tag", _ids(CORR))
def test_corr_volume(be, verdict, tag):
    """stx_corr_volume_fwd / _bwd against the oracle's literal slices; each gradient alone."""
    B, C, H, W, md, G = CORR[tag]
    a, b, g = corr_inputs(B, C, H, W, md, G, 200 + 10 * list(CORR).index(tag))
    (vol_ref,), grads = _refs(lambda a, b: O.pcw_correlation_volume(a, b, md, G), (a, b), (g,), (0, 1))
    what = f"corr_volume[{be.name}:{tag}]"
    Gd = Guards(be)
    da, db, dg = Gd.inp(a), Gd.inp(b), Gd.inp(g)
    vol, ga, gb, ga1, gb1 = Gd.out(B, G, 2 * md + 1, H, W), Gd.out(B, C, H, W), Gd.out(B, C, H, W), Gd.out(B, C, H, W), Gd.out(B, C, H, W)
    _call(be, Gd, what, "stx_corr_volume_fwd", da, db, vol, B, C, H, W, md, G)
    _call(be, Gd, what, "stx_corr_volume_bwd", dg, da, db, ga, gb, B, C, H, W, md, G)
    _call(be, Gd, what, "stx_corr_volume_bwd", dg, da, db, ga1, None, B, C, H, W, md, G)
    _call(be, Gd, what, "stx_corr_volume_bwd", dg, da, db, None, gb1, B, C, H, W, md, G)
    verdict.within(vol.cpu(), *_wd(vol_ref), VALUE_FACTOR, what + ":out")
    for got, i, name in ((ga, 0, "gref"), (gb, 1, "gtgt"), (ga1, 0, "gref_alone"), (gb1, 1, "gtgt_alone")):
        verdict.within(got.cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


VAR = {n: c for n, *c in VAR_CASES}                        # B, D, H, W


@pytest.mark.parametrize("samples", [0, 1], ids=["variance", "confidence"])
@pytest.mark.parametrize("tag", _ids(VAR))
def test_disparity_variance(be, verdict, tag, samples):
    """stx_disparity_variance_fwd / _bwd without and with `samples`; each of the gradients alone."""
    B, D, H, W = VAR[tag]
    x, d, s, g = var_inputs(B, D, H, W, 300 + 10 * list(VAR).index(tag))
    s = s if samples else None
    fn = (lambda x, d, s: O.cf_disparity_variance_confidence(x, s, d)) if samples else (lambda x, d, s: O.cf_disparity_variance(x, D, d))
    wrt = (0, 1, 2) if samples else (0, 1)
    (out_ref,), grads = _refs(fn, (x, d, s), (g,), wrt)
    what = f"disparity_variance[{be.name}:{tag}:{'conf' if samples else 'var'}]"
    Gd = Guards(be)
    dx, dd, ds, dg = Gd.inp(x), Gd.inp(d), Gd.inp(s), Gd.inp(g)
    out = Gd.out(B, 1, H, W)
    _call(be, Gd, what, "stx_disparity_variance_fwd", dx, dd, ds, out, B, D, H * W)
    verdict.within(out.cpu(), *_wd(out_ref), VALUE_FACTOR, what + (":conf" if samples else ":var"))
    shapes = ((B, D, H, W), (B, 1, H, W), (B, D, H, W))
    full = [Gd.out(*shapes[i]) if i in wrt else None for i in range(3)]
    _call(be, Gd, what, "stx_disparity_variance_bwd", dg, dx, dd, ds, *full, B, D, H * W)
    for i, name in enumerate(("gx", "gdisp", "gs")):
        if i not in wrt:
            continue
        verdict.within(full[i].cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
        alone = [Gd.out(*shapes[j]) if j == i else None for j in range(3)]
        _call(be, Gd, what, "stx_disparity_variance_bwd", dg, dx, dd, ds, *alone, B, D, H * W)
        verdict.within(alone[i].cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}_alone")
    verdict.done()


# ------------------------------------------------------------------------------------------ convex_upsample.hip
from tests.golden import convex_upsample_config as CU  # noqa: E402
from tests.golden import stereoanywhere_config as SA  # noqa: E402


@pytest.mark.parametrize("tag", _ids(CU.CASES))
def test_convex_upsample(be, verdict, tag):
    """stx_convex_upsample_fwd / _bwd on every row of tests/golden/convex_upsample_config.py (f = 2, 4, 8; D = 1, 2, 3: the second
    register chunk; H = 1, W = 1; H W = 70 and 335 across workgroups; logits around +-90; use_scale_factor on and off), the
    flow-gradient workspace of exactly stx_convex_upsample_bwd_workspace_floats floats; each gradient alone, the other NULL."""
    N, D, H, W, n, use_scale, _ = CU.CASES[tag]
    f = 2 ** n
    scale = float(f) if use_scale else 1.0
    flow, mask, gy = CU.inputs(tag)
    (out_ref,), grads = _refs(lambda a, b: convex(a, b, f, scale), (flow, mask), (gy,), (0, 1))
    what = f"convex_upsample[{be.name}:{tag}]"
    Gd = Guards(be)
    df, dm, dg = Gd.inp(flow), Gd.inp(mask), Gd.inp(gy)
    out, gf, gm, gf1, gm1 = Gd.out(N, D, f * H, f * W), Gd.out(N, D, H, W), Gd.out(N, 9 * f * f, H, W), Gd.out(N, D, H, W), Gd.out(N, 9 * f * f, H, W)
    ws = Gd.out(int(be.raw("stx_convex_upsample_bwd_workspace_floats")(N, D, H, W)))
    _call(be, Gd, what, "stx_convex_upsample_fwd", df, dm, out, N, D, H, W, 9 * f * f, f, scale)
    _call(be, Gd, what, "stx_convex_upsample_bwd", dg, df, dm, gf, gm, ws, N, D, H, W, 9 * f * f, f, scale)
    _call(be, Gd, what, "stx_convex_upsample_bwd", dg, df, dm, gf1, None, ws, N, D, H, W, 9 * f * f, f, scale)
    _call(be, Gd, what, "stx_convex_upsample_bwd", dg, df, dm, None, gm1, None, N, D, H, W, 9 * f * f, f, scale)
    verdict.within(out.cpu(), *_wd(out_ref), VALUE_FACTOR, what + ":out")
    for got, i, name in ((gf, 0, "gflow"), (gm, 1, "gmask"), (gf1, 0, "gflow_alone"), (gm1, 1, "gmask_alone")):
        verdict.within(got.cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


@pytest.mark.parametrize("tag", _ids(CU.PIXEL_CASES))
def test_softmax_context_upsample(be, verdict, tag):
    """stx_softmax_context_upsample_fwd / _bwd (the pixel layout) at 1x1, b2_3x17 and 5x67; each gradient alone."""
    B, h, w = CU.PIXEL_CASES[tag]
    disp, logits, gy = CU.pixel_inputs(tag)
    (out_ref,), grads = _refs(lambda d, l: upsample(d * CU.PIXEL_SCALE, torch.softmax(l, 1)), (disp, logits), (gy,), (0, 1))
    what = f"softmax_context_upsample[{be.name}:{tag}]"
    Gd = Guards(be)
    dd, dl, dg = Gd.inp(disp), Gd.inp(logits), Gd.inp(gy)
    out, gd, gl, gd1, gl1 = Gd.out(B, 4 * h, 4 * w), Gd.out(B, 1, h, w), Gd.out(B, 9, 4 * h, 4 * w), Gd.out(B, 1, h, w), Gd.out(B, 9, 4 * h, 4 * w)
    ws = Gd.out(int(be.raw("stx_convex_upsample_bwd_workspace_floats")(B, 1, h, w)))
    _call(be, Gd, what, "stx_softmax_context_upsample_fwd", dd, dl, out, B, h, w, CU.PIXEL_SCALE)
    _call(be, Gd, what, "stx_softmax_context_upsample_bwd", dg, dd, dl, gd, gl, ws, B, h, w, CU.PIXEL_SCALE)
    _call(be, Gd, what, "stx_softmax_context_upsample_bwd", dg, dd, dl, gd1, None, ws, B, h, w, CU.PIXEL_SCALE)
    _call(be, Gd, what, "stx_softmax_context_upsample_bwd", dg, dd, dl, None, gl1, None, B, h, w, CU.PIXEL_SCALE)
    verdict.within(out.cpu(), *_wd(out_ref), VALUE_FACTOR, what + ":out")
    for got, i, name in ((gd, 0, "gflow"), (gl, 1, "gmask"), (gd1, 0, "gflow_alone"), (gl1, 1, "gmask_alone")):
        verdict.within(got.cpu(), *_wd(grads[i]), GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


def _sequence_loss(preds, gt, maxdisp, weights):
    """The header's loss in plain torch: sum_k w_k (sum_valid smooth_l1(preds[k] - gt)) / max(1, #valid); an excluded gt (zero,
    >= maxdisp - 1, NaN, inf) is replaced before it is subtracted, never multiplied."""
    valid = (gt > 0) & (gt < maxdisp - 1)
    inv = 1.0 / valid.sum().clamp_min(1).to(gt.dtype)
    loss = 0.0
    for p, w in zip(preds, weights):
        d = p - torch.where(valid, gt, p.detach())
        loss = loss + w * F.smooth_l1_loss(d, torch.zeros_like(d), reduction="none").sum() * inv
    return loss


LOSS_CASES = {"k1": (1, False, ()), "k2": (2, False, ()), "k23": (23, False, (0, 5, 22)), "k33": (33, False, ()),
              "k2_all_invalid": (2, True, (1,))}          # K, an all-invalid gt (count = 0: max(1, count)), NULL entries of gpreds


@pytest.mark.parametrize("tag", _ids(LOSS_CASES))
def test_sequence_loss(be, verdict, tag):
    """stx_sequence_loss_fwd / _bwd on n = 2 * 7 * 67 pixels: host arrays of device pointers, every prediction and every gpreds
    entry banded, the workspace of exactly stx_sequence_loss_workspace_floats floats; gt holds zeros, maxdisp - 1 exactly, NaN and
    inf; gpreds with NULL entries."""
    K, all_invalid, nulls = LOSS_CASES[tag]
    gt, preds = CU.loss_inputs(K)
    if all_invalid:
        gt = torch.where(gt > 0, gt + CU.LOSS_MAXDISP, gt)
    finite = gt[torch.isfinite(gt)]
    assert torch.equal(finite * 4, (finite * 4).round())                      # the condition on the inputs: gt exact, on quarters
    preds = [p.reshape(-1) for p in preds]
    n = gt.numel()
    weights = CU.trainer_weights(K - 1) if K >= 3 else [1.0, 0.7][:K]
    gloss = torch.tensor([0.7])
    maxdisp = float(CU.LOSS_MAXDISP)
    valid = (gt > 0) & (gt < maxdisp - 1)
    assert int(valid.sum()) == 0 if all_invalid else 0 < int(valid.sum()) < n
    (loss_ref,), grads = _refs(lambda *p: _sequence_loss(p, gt.reshape(-1).to(p[0].dtype), maxdisp, weights).reshape(1), preds, (gloss,),
                               tuple(range(K)))
    what = f"sequence_loss[{be.name}:{tag}]"
    Gd = Guards(be)
    dp = [Gd.inp(p) for p in preds]
    gp = [None if k in nulls else Gd.out(n) for k in range(K)]
    tab = (ctypes.c_void_p * K)(*[t.data_ptr() for t in dp])
    gtab = (ctypes.c_void_p * K)(*[None if t is None else t.data_ptr() for t in gp])
    w = (ctypes.c_double * K)(*weights)
    dgt, loss = Gd.inp(gt), Gd.out(1)
    count = Gd.out(1).view(torch.int32)
    ws = Gd.out(int(be.raw("stx_sequence_loss_workspace_floats")(n)))
    _call(be, Gd, what, "stx_sequence_loss_fwd", tab, w, K, dgt, maxdisp, loss, count, ws, n)
    assert int(count.item()) == int(valid.sum())
    _call(be, Gd, what, "stx_sequence_loss_bwd", Gd.inp(gloss), tab, w, K, dgt, maxdisp, Gd.inp(count.view(torch.float32)), gtab, n)
    verdict.within(loss.cpu(), *_wd(loss_ref), VALUE_FACTOR, what + ":loss")
    kept = [k for k in range(K) if k not in nulls]
    got = torch.stack([gp[k].cpu() for k in kept])
    assert bool((got[:, ~valid.reshape(-1)] == 0).all())                      # exactly 0 at excluded pixels
    want = torch.stack([grads[k][0] for k in kept]), torch.stack([grads[k][1] for k in kept])
    verdict.within(got, *_wd(want), GRAD_FACTOR, what + ":gpreds")
    verdict.done()


# ------------------------------------------------------------------------------------------ allpairs.hip
#           B  H  W1   W2   s        (tests/golden/stereoanywhere_config.py)
EST = {"b2_13": SA.EST_CASES["b2_13"],                     # below one wave, 78 rows: the last workgroup of four rows is half empty
       "w70_66": SA.EST_CASES["w70_66"],                   # W1 != W2, a second 64-column strip
       "w260": SA.EST_CASES["w260"]}                       # W = 260 at H = 1: the fifth register of the row
# every mask the product uses (all four, each output alone) and one single-direction mask (both left outputs)
WHICH = (15, 1, 2, 4, 8, 3)


@functools.lru_cache(maxsize=None)
def _est_ref(tag, which):
    vol, gws = SA.est_inputs(tag)
    gys = [g if which & (1 << i) else None for i, g in enumerate(gws)]
    return _refs(estimates, (vol,), gys, (0,))


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("tag", _ids(EST))
def test_allpairs_estimates(be, verdict, tag, which):
    """stx_allpairs_estimates_fwd / _bwd: exactly the outputs `which` names, `stats` of the 4 * (B H W1 + B H W2) floats the header
    states; the backward with all the gradients of the mask and, after the full forward, with each single gradient."""
    B, H, W1, W2, _ = EST[tag]
    vol, gws = SA.est_inputs(tag)
    what = f"allpairs_estimates[{be.name}:{tag}:{which}]"
    Gd = Guards(be)
    dvol = Gd.inp(vol)
    stats = Gd.out(4 * (B * H * W1 + B * H * W2))
    outs = [Gd.out(B, 1, H, W2 if i >= 2 else W1) if which & (1 << i) else None for i in range(4)]
    _call(be, Gd, what, "stx_allpairs_estimates_fwd", dvol, which, *outs, stats, B, H, W1, W2)
    refs, grads = _est_ref(tag, which)
    for i, name in enumerate(SA.OUTPUTS):
        if outs[i] is not None:
            verdict.within(outs[i].cpu(), *_wd(refs[i]), VALUE_FACTOR, f"{what}:{name}")
    dst = Gd.inp(stats)
    dg = [Gd.inp(g) if which & (1 << i) else None for i, g in enumerate(gws)]
    gvol = Gd.out(B, 1, H, W1, W2)
    _call(be, Gd, what, "stx_allpairs_estimates_bwd", *dg, dvol, dst, gvol, B, H, W1, W2)
    verdict.within(gvol.cpu(), *_wd(grads[0]), GRAD_FACTOR, what + ":g_all")
    if which == 15:
        for i, name in enumerate(SA.OUTPUTS):
            one = Gd.out(B, 1, H, W1, W2)
            _call(be, Gd, what, "stx_allpairs_estimates_bwd", *[d if j == i else None for j, d in enumerate(dg)], dvol, dst, one, B, H, W1, W2)
            verdict.within(one.cpu(), *_wd(_est_ref(tag, 1 << i)[1][0]), GRAD_FACTOR, f"{what}:g_{name}")
    verdict.done()


@pytest.mark.parametrize("trunc", [0, 1], ids=["plain", "truncated"])
def test_corr1d_volume_pyramid(be, verdict, trunc):
    """stx_corr1d_volume_pyramid_fwd / _bwd at 4 levels with an odd W2 (37 -> 18 -> 9 -> 4), without and with tdisp / tconf, in
    stx_corr1d_pyramid_floats floats."""
    B, H, W1, W2, L = 1, 3, 37, 37, 4
    g = _gen(400)
    vol = _randn(g, B, H, W1, W2) * 2
    tdisp, tconf = (_uniform(g, 0.0, 12.0, B, 1, H, W1), _uniform(g, 0.0, 1.0, B, 1, H, W1)) if trunc else (None, None)
    n_c = int(be.raw("stx_corr1d_pyramid_floats")(B * H * W1, W2, L))
    gc = _randn(g, n_c)

    def fn(v):
        cp = [v if not trunc else truncation_mask(tdisp.to(v.dtype), tconf.to(v.dtype), None, SA.ATTENUATION)[:, 0] * v]
        for _ in range(L - 1):
            cp.append(pool(cp[-1]))
        return _pack(cp)
    (cp_ref,), grads = _refs(fn, (vol,), (gc,), (0,))
    what = f"corr1d_volume_pyramid[{be.name}:{'trunc' if trunc else 'plain'}]"
    Gd = Guards(be)
    dt, dcf = Gd.inp(tdisp), Gd.inp(tconf)
    cpyr, gvol = Gd.out(n_c), Gd.out(B, H, W1, W2)
    _call(be, Gd, what, "stx_corr1d_volume_pyramid_fwd", Gd.inp(vol), dt, dcf, SA.ATTENUATION, cpyr, B, H, W1, W2, L)
    _call(be, Gd, what, "stx_corr1d_volume_pyramid_bwd", Gd.inp(gc), dt, dcf, SA.ATTENUATION, gvol, B, H, W1, W2, L)
    verdict.within(cpyr.cpu(), *_wd(cp_ref), VALUE_FACTOR, what + ":cpyr")
    verdict.within(gvol.cpu(), *_wd(grads[0]), GRAD_FACTOR, what + ":gvol")
    verdict.done()


@pytest.mark.parametrize("name", _ids(SA.MASK_THRESHOLDS))
def test_truncate_mask(be, verdict, name):
    """stx_truncate_mask_fwd without and with the confidence threshold (a step: no confidence within 1e-3 of it)."""
    th = SA.MASK_THRESHOLDS[name]
    B, H, W = SA.MASK_SHAPE
    disp, conf = SA.mask_inputs()
    assert th is None or bool(((conf.double() - th).abs() > 1e-3).all())
    (ref,), _ = _refs(lambda d, c: truncation_mask(d, c, th, SA.ATTENUATION), (disp, conf))
    what = f"truncate_mask[{be.name}:{name}]"
    Gd = Guards(be)
    mask = Gd.out(B, 1, H, W, W)
    _call(be, Gd, what, "stx_truncate_mask_fwd", Gd.inp(disp), Gd.inp(conf), int(th is not None), float(th or 0.0), SA.ATTENUATION, mask, B, H, W)
    verdict.within(mask.cpu(), *_wd(ref), VALUE_FACTOR, what + ":mask")
    verdict.done()


# ------------------------------------------------------------------------------------------ convgru.hip
from tests.parity import on  # noqa: E402

#             B  hidden  x channels  H   W        (tests/golden/convgru_config.py)
GRU_CASES = {
    "one_src": (2, 16, (16,), 5, 19),          # batch stride; W across a 16-pixel line, H below a tile; 190 pixels
    "two_src": (1, 16, (16, 16), 9, 7),        # source seams in K; H across a tile edge
    "ragged": (1, 16, (20, 4, 8), 3, 33),      # K chunks that end inside a source; three x sources; 99 pixels: a partly idle workgroup
    "wide_n": (1, 32, (32,), 4, 6),            # N = 64 in the zr launch
    "real_1src": (1, 128, (128,), 2, 5),       # the real width
    "real_2src": (1, 128, (128, 128), 3, 17),  # 51 pixels: two workgroups of 32 in the gate kernels, the last one partly idle
    "px300": (1, 16, (8,), 12, 25),            # 300 pixels: two gate workgroups of 256, 44 pixels in the last; its row of partial sums
    "tile8": (4, 16, (8,), 57, 129),           # 4 x 8 x 9 = 288 pixel tiles: the launcher's 8-row tiles (GPU only)
}
GRU_PARAMS = on(list(GRU_CASES), gpu_only=("tile8",))
GAP = 4                                        # NaN channels behind every slice of a pitched buffer (16 bytes: the slices stay aligned)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _pitched(Gd, parts):
    """Channels-last maps [B][H][W][c_i] as channel slices of ONE banded buffer, GAP channels of NaN behind each: a read past a
    slice's channels inside a pixel poisons an output.  Returns the flat source arguments (slice, channels, pitch) per part."""
    cols = []
    for p in parts:
        cols += [p, torch.full(p.shape[:-1] + (GAP,), float("nan"))]
    buf = Gd.inp(torch.cat(cols, -1))
    out, off = [], 0
    for p in parts:
        out.append((buf[..., off:off + p.shape[-1]], p.shape[-1], buf.shape[-1]))
        off += p.shape[-1] + GAP
    return out


def _src_args(srcs):
    flat = [v for s in srcs for v in s]
    return flat + [None, 0, 0] * (4 - len(srcs))


@functools.lru_cache(maxsize=None)
def _gru_inputs(tag):
    """Everything logical NCHW: h, the x sources, cz / cr / cq, the three weights and biases, and stand-ins of the saved tensors
    (z, r in (0, 1), q in (-1, 1)) and of the gradients for the backward kernels, which are tested on their own."""
    B, hidden, cx, H, W = GRU_CASES[tag]
    g = _gen(500 + list(GRU_CASES).index(tag))
    K = hidden + sum(cx)
    t = lambda c: _randn(g, B, c, H, W)  # noqa: E731
    d = dict(h=torch.tanh(t(hidden)), xs=[t(c) for c in cx], cz=t(hidden), cr=t(hidden), cq=t(hidden))
    for n in "zrq":
        d["w" + n], d["b" + n] = _randn(g, hidden, K, 3, 3) * (2.0 / (9 * K)) ** 0.5, _randn(g, hidden) * 0.1
    d.update(z=torch.sigmoid(t(hidden)), r=torch.sigmoid(t(hidden)), q=torch.tanh(t(hidden)), rh=torch.tanh(t(hidden)),
             g=t(hidden), g_rh=t(hidden), gz=t(hidden), gr=t(hidden), gq=t(hidden), addend=t(K), rows=_randn(g, 37, 2 * hidden))
    return d


def _packed(be, Gd, what, w0, w1, mode):
    """Weights [A][Bd][3][3] packed into a banded buffer of exactly stx_convgru_packed_floats floats."""
    A, Bd = w0.shape[:2]
    nw = 1 if w1 is None else 2
    K, N = (Bd, nw * A) if mode == 0 else (nw * A, Bd)
    n = int(be.raw("stx_convgru_packed_floats")(K, N))
    assert n > 0
    wp = Gd.out(n)
    _call(be, Gd, what, "stx_convgru_pack_weight", Gd.inp(w0), Gd.inp(w1), wp, A, Bd, mode)
    return wp


def _gemm(be, Gd, what, srcs, wp, N, B, H, W, epi=0, split=0, bias0=None, bias1=None, add0=(None, 0), add1=(None, 0), h=(None, 0),
          z=None, out0=None, out1=None, out2=None, out_pitch=0):
    _call(be, Gd, what, "stx_convgru_gemm", *_src_args(srcs), wp, N, epi, split, bias0, bias1, *add0, *add1, *h, z, out0, out1, out2,
          out_pitch, B, H, W)


@functools.lru_cache(maxsize=None)
def _gru_gemm_refs(tag):
    d = _gru_inputs(tag)
    x, w, gy = torch.cat([d["h"]] + d["xs"], 1), torch.cat([d["wz"], d["wr"]]), torch.cat([d["gz"], d["gr"]], 1)
    (y_ref,), grads = _refs(lambda x, w: F.conv2d(x, w, None, 1, 1), (x, w), (gy,), (0,))
    return {"y0": _wd(y_ref), "dgrad": _wd((_nhwc(grads[0][0]), _nhwc(grads[0][1])), _nhwc(d["addend"]))}


@pytest.mark.parametrize("backend,tag", GRU_PARAMS)
def test_convgru_gemm_raw(backend, tag, verdict):
    """stx_convgru_pack_weight in both modes and stx_convgru_gemm with the raw epilogue: the forward convolution of the pitched
    source list [h | x..] with the stacked z | r weights, and the data gradient on mode-1 weights from the pitched maps [gz | gr]
    added IN PLACE (out0 == add0) to a non-zero addend."""
    be = Backend(backend)
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    K, N = hidden + sum(cx), 2 * hidden
    refs = _gru_gemm_refs(tag)
    what = f"convgru_gemm[{be.name}:{tag}]"
    Gd = Guards(be)
    y = Gd.out(B, H, W, N)
    _gemm(be, Gd, what, _pitched(Gd, [_nhwc(d["h"])] + [_nhwc(t) for t in d["xs"]]), _packed(be, Gd, what, d["wz"], d["wr"], 0), N, B, H, W,
          out0=y, out_pitch=N)
    verdict.within(_nchw(y.cpu()), *refs["y0"], VALUE_FACTOR, what + ":y0")
    add = _nhwc(d["addend"])
    buf = _out_from(Gd, add)
    _gemm(be, Gd, what, _pitched(Gd, [_nhwc(d["gz"]), _nhwc(d["gr"])]), _packed(be, Gd, what, d["wz"], d["wr"], 1), K, B, H, W,
          add0=(buf, K), out0=buf, out_pitch=K)
    verdict.within(buf.cpu(), *refs["dgrad"], GRAD_FACTOR, what + ":dgrad")
    verdict.done()


@functools.lru_cache(maxsize=None)
def _gru_gates_refs(tag):
    d = _gru_inputs(tag)

    def zr(h, cz, cr, wz, bz, wr, br, *xs):
        hx = torch.cat([h, *xs], 1)
        z, r = torch.sigmoid(F.conv2d(hx, wz, bz, padding=1) + cz), torch.sigmoid(F.conv2d(hx, wr, br, padding=1) + cr)
        return z, r * h, r

    def hq(rh, h, z, cq, wq, bq, *xs):
        q = torch.tanh(F.conv2d(torch.cat([rh, *xs], 1), wq, bq, padding=1) + cq)
        return (1 - z) * h + z * q, q
    zr_ref, _ = _refs(zr, (d["h"], d["cz"], d["cr"], d["wz"], d["bz"], d["wr"], d["br"], *d["xs"]))
    hq_ref, _ = _refs(hq, (d["rh"], d["h"], d["z"], d["cq"], d["wq"], d["bq"], *d["xs"]))
    return {n: _wd(r) for n, r in zip(("gate_z", "gate_rh", "gate_r", "gate_h", "gate_q"), zr_ref + hq_ref)}


@pytest.mark.parametrize("backend,tag", GRU_PARAMS)
def test_convgru_gates(backend, tag, verdict):
    """stx_convgru_gemm with the gate epilogues: 1 (z, r h, r; without out2 the others keep their bits) and 2 (h', q; without
    out1), biases and the pitched context addends, h read at the centre pixel of its slice."""
    be = Backend(backend)
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    refs = _gru_gates_refs(tag)
    what = f"convgru_gates[{be.name}:{tag}]"
    Gd = Guards(be)
    hs, rhs, *xsrc = _pitched(Gd, [_nhwc(d["h"]), _nhwc(d["rh"])] + [_nhwc(t) for t in d["xs"]])
    cz, cr, cq = _pitched(Gd, [_nhwc(d["cz"]), _nhwc(d["cr"]), _nhwc(d["cq"])])
    new = lambda: Gd.out(B, H, W, hidden)  # noqa: E731
    z, rh, r, z2, rh2 = new(), new(), new(), new(), new()
    wzr, wq = _packed(be, Gd, what, d["wz"], d["wr"], 0), _packed(be, Gd, what, d["wq"], None, 0)
    kw = dict(epi=1, split=hidden, bias0=Gd.inp(d["bz"]), bias1=Gd.inp(d["br"]), add0=(cz[0], cz[2]), add1=(cr[0], cr[2]), h=(hs[0], hs[2]))
    _gemm(be, Gd, what, [hs] + xsrc, wzr, 2 * hidden, B, H, W, out0=z, out1=rh, out2=r, **kw)
    _gemm(be, Gd, what, [hs] + xsrc, wzr, 2 * hidden, B, H, W, out0=z2, out1=rh2, out2=None, **kw)
    for got, name in ((z, "gate_z"), (rh, "gate_rh"), (r, "gate_r")):
        verdict.within(_nchw(got.cpu()), *refs[name], VALUE_FACTOR, f"{what}:{name}")
    assert torch.equal(z2.cpu(), z.cpu()) and torch.equal(rh2.cpu(), rh.cpu())
    hn, q, hn2 = new(), new(), new()
    kw = dict(epi=2, split=hidden, bias0=Gd.inp(d["bq"]), add0=(cq[0], cq[2]), h=(hs[0], hs[2]), z=Gd.inp(_nhwc(d["z"])))
    _gemm(be, Gd, what, [rhs] + xsrc, wq, hidden, B, H, W, out0=hn, out1=q, **kw)
    _gemm(be, Gd, what, [rhs] + xsrc, wq, hidden, B, H, W, out0=hn2, out1=None, **kw)
    verdict.within(_nchw(hn.cpu()), *refs["gate_h"], VALUE_FACTOR, what + ":gate_h")
    verdict.within(_nchw(q.cpu()), *refs["gate_q"], VALUE_FACTOR, what + ":gate_q")
    assert torch.equal(hn2.cpu(), hn.cpu())
    verdict.done()


def _seq_sum(t):
    """Column sums of [n][...] added one after the other in the tensor's own precision (no kernel has the pairwise order of sum())."""
    acc = torch.zeros_like(t[0])
    for row in t:
        acc += row
    return acc


@functools.lru_cache(maxsize=None)
def _gru_bwd_refs(tag):
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    g, z, q, h, r, g_rh = (_nhwc(d[k]).reshape(-1, hidden) for k in ("g", "z", "q", "h", "r", "g_rh"))
    (gq, gz), _ = _refs(lambda g, z, q, h: (g * z * (1 - q * q), g * (q - h) * z * (1 - z)), (g, z, q, h))
    (gr, buf), _ = _refs(lambda g_rh, g, z, r, h: (g_rh * h * r * (1 - r), g * (1 - z) + g_rh * r), (g_rh, g, z, r, h))
    out = {"gq": _wd(gq), "gz": _wd(gz), "gr": _wd(gr), "buf": _wd(buf)}
    for name, ref in (("gq_rows", gq), ("gz_rows", gz), ("gr_rows", gr)):           # the bias gradients: column sums, added in order
        out[name] = (ref[0].sum(0), _dist(_seq_sum(ref[1]), ref[0].sum(0)))
    out["rowsum"] = (d["rows"].double().sum(0), _dist(_seq_sum(d["rows"]), d["rows"].double().sum(0)))
    return out


@pytest.mark.parametrize("backend,tag", GRU_PARAMS)
def test_convgru_gate_backward(backend, tag, verdict):
    """stx_convgru_gate_bwd, stx_convgru_reset_bwd (buf updated in place in the first `hidden` channels of its pitch, the others
    untouched) and stx_convgru_row_sum: g and h pitched, partial-sum rows of exactly stx_convgru_gate_rows rows, with and
    without `rows`."""
    be = Backend(backend)
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    P, K = B * H * W, hidden + sum(cx)
    flat = lambda t: _nhwc(t).reshape(P, hidden)  # noqa: E731
    g, z, q, h, r, g_rh = (flat(d[k]) for k in ("g", "z", "q", "h", "r", "g_rh"))
    refs = _gru_bwd_refs(tag)
    what = f"convgru_gate_bwd[{be.name}:{tag}]"
    nrows = int(be.raw("stx_convgru_gate_rows")(P, hidden))
    assert nrows >= 1
    Gd = Guards(be)
    (gs, _, gp), (hs, _, hp) = _pitched(Gd, [_nhwc(d["g"]), _nhwc(d["h"])])
    dz, dq, dr = Gd.inp(z), Gd.inp(q), Gd.inp(r)
    gq, gz, gq2, gz2, rows = Gd.out(P, hidden), Gd.out(P, hidden), Gd.out(P, hidden), Gd.out(P, hidden), Gd.out(nrows, 2, hidden)
    _call(be, Gd, what, "stx_convgru_gate_bwd", gs, gp, dz, dq, hs, hp, gq, gz, rows, P, hidden)
    _call(be, Gd, what, "stx_convgru_gate_bwd", gs, gp, dz, dq, hs, hp, gq2, gz2, None, P, hidden)
    verdict.within(gq.cpu(), *refs["gq"], GRAD_FACTOR, what + ":gq")
    verdict.within(gz.cpu(), *refs["gz"], GRAD_FACTOR, what + ":gz")
    assert torch.equal(gq2.cpu(), gq.cpu()) and torch.equal(gz2.cpu(), gz.cpu())
    sums = rows.cpu().double().sum(0)
    for i, name in enumerate(("gq_rows", "gz_rows")):
        verdict.within(sums[i], *refs[name], GRAD_FACTOR, f"{what}:{name}")
    # reset backward: buf [P][K], g_rh in its first `hidden` channels, a gradient of the x sources (to be left alone) behind them
    start = torch.cat([g_rh, _nhwc(d["addend"]).reshape(P, K)[:, hidden:]], 1)
    buf, buf2, gr, gr2, rows_r = _out_from(Gd, start), _out_from(Gd, start), Gd.out(P, hidden), Gd.out(P, hidden), Gd.out(nrows, hidden)
    _call(be, Gd, what, "stx_convgru_reset_bwd", buf, K, gs, gp, dz, dr, hs, hp, gr, rows_r, P, hidden)
    _call(be, Gd, what, "stx_convgru_reset_bwd", buf2, K, gs, gp, dz, dr, hs, hp, gr2, None, P, hidden)
    verdict.within(gr.cpu(), *refs["gr"], GRAD_FACTOR, what + ":gr")
    verdict.within(buf.cpu()[:, :hidden], *refs["buf"], GRAD_FACTOR, what + ":buf")
    assert torch.equal(buf.cpu()[:, hidden:], start[:, hidden:]) and torch.equal(buf2.cpu(), buf.cpu()) and torch.equal(gr2.cpu(), gr.cpu())
    verdict.within(rows_r.cpu().double().sum(0), *refs["gr_rows"], GRAD_FACTOR, what + ":gr_rows")
    # the row sum, in row order, of 37 seeded rows
    out = Gd.out(2 * hidden)
    _call(be, Gd, what, "stx_convgru_row_sum", Gd.inp(d["rows"]), out, d["rows"].shape[0], 2 * hidden)
    verdict.within(out.cpu(), *refs["rowsum"], VALUE_FACTOR, what + ":rowsum")
    verdict.done()


@functools.lru_cache(maxsize=None)
def _gru_wgrad_refs(tag):
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    K, out = hidden + sum(cx), {}
    for first, gmaps, name in ((d["h"], (d["gz"], d["gr"]), "dw2"), (d["rh"], (d["gq"],), "dw")):
        x, w, gy = torch.cat([first] + d["xs"], 1), torch.zeros(hidden * len(gmaps), K, 3, 3), torch.cat(gmaps, 1)
        out[name] = _wd(_refs(lambda x, w: F.conv2d(x, w, None, 1, 1), (x, w), (gy,), (1,))[1][1])
    return out


GRU_REFS = {"convgru_gemm": _gru_gemm_refs, "convgru_gates": _gru_gates_refs, "convgru_gate_bwd": _gru_bwd_refs, "convgru_wgrad": _gru_wgrad_refs}


def test_the_gpu_only_case_has_its_recorded_dref():
    """`tile8` runs on the GPU alone, d_ref is a CPU quantity: recorded (and held within DREF_DRIFT) here."""
    for family, fn in GRU_REFS.items():
        for name, (_, live) in fn("tile8").items():
            assert _dref(f"{family}[tile8]:{name}", live) > 0


@pytest.mark.parametrize("backend,tag", GRU_PARAMS)
def test_convgru_wgrad(backend, tag, verdict):
    """stx_convgru_wgrad with two gradient maps (z | r over [h | x..]) and with one (q over [r h | x..]), the workspace of exactly
    stx_convgru_wgrad_workspace_floats floats."""
    be = Backend(backend)
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    K = hidden + sum(cx)
    refs = _gru_wgrad_refs(tag)
    what = f"convgru_wgrad[{be.name}:{tag}]"
    Gd = Guards(be)
    hs, rhs, *xsrc = _pitched(Gd, [_nhwc(d["h"]), _nhwc(d["rh"])] + [_nhwc(t) for t in d["xs"]])
    for first, src0, gmaps, name in ((d["h"], hs, (d["gz"], d["gr"]), "dw2"), (d["rh"], rhs, (d["gq"],), "dw")):
        CC = hidden * len(gmaps)
        ws = Gd.out(int(be.raw("stx_convgru_wgrad_workspace_floats")(B, H, W, K, CC)))
        dw = Gd.out(CC, K, 9)
        g0, g1 = Gd.inp(_nhwc(gmaps[0])), Gd.inp(_nhwc(gmaps[1])) if len(gmaps) > 1 else None
        _call(be, Gd, what, "stx_convgru_wgrad", *_src_args([src0] + xsrc), g0, g1, hidden, dw, ws, B, H, W)
        verdict.within(dw.cpu().view(CC, K, 3, 3), *refs[name], GRAD_FACTOR, f"{what}:{name}")
    verdict.done()


# ------------------------------------------------------------------------------------------ the rule itself
def test_listed_share():
    """At most LISTED_SHARE of the module's (case, tensor) pairs -- the entries of the recorded d_ref table -- are listed, per backend."""
    pairs = len(_dref.table()) if not _dref.record else None
    for backend in ("emu", "hip"):
        other = "hip" if backend == "emu" else "emu"
        listed = sum(len(r.split(", ")) for name, r in PAST_THE_FACTOR.items() if f"[{other}-" not in name)
        assert pairs is None or listed <= LISTED_SHARE * pairs, (backend, listed, pairs)


def _refused(near_miss, ref, what, factor, tag, add=None):
    """The near miss is refused by the very `within` call, with the very recorded d_ref, that the kernels of `what` pass."""
    want, live = _wd(ref, add)
    with pytest.raises(AssertionError, match=tag):
        within(near_miss.reshape(want.shape), want, _dref(what, live), factor, tag)


def test_the_rule_refuses_a_lookup_with_the_level_0_fraction_at_level_1():
    tag = "r2_l3_odd"
    B, C, D, H, W, W2, Cf, L, r = GEO_CASES[tag]
    _, _, _, gpyr, cpyr, calls, _, _ = _geo_inputs(tag)
    disp, coords, _ = calls[0]
    gp = [t.transpose(-1, -2) for t in _levels(gpyr, (B, H, W), D, C, L)]
    cp = [t.squeeze(-1) for t in _levels(cpyr, (B, H, W), W2, 1, L)]
    dx = torch.arange(-r, r + 1, dtype=torch.float32)
    d, c = disp.reshape(B, H, W, 1), coords.reshape(B, H, W, 1)

    def miss_sample(rows, x, x_level0):
        i0, f = torch.floor(x).long(), x_level0 - torch.floor(x_level0)
        tap = lambda i: torch.gather(rows, -1, i.clamp(0, rows.shape[-1] - 1)) * ((i >= 0) & (i < rows.shape[-1]))  # noqa: E731
        return (1 - f) * tap(i0) + f * tap(i0 + 1)
    out = []
    for i in range(L):
        xg = (d / 2 ** i + dx).unsqueeze(3).expand(B, H, W, C, 2 * r + 1)
        out.append(miss_sample(gp[i], xg, (d + dx).unsqueeze(3).expand_as(xg)).reshape(B, H, W, -1))
        out.append(miss_sample(cp[i], (c - d) / 2 ** i + dx, c - d + dx))
    miss = torch.cat(out, -1).permute(0, 3, 1, 2)
    _refused(miss, _geo_lookup_ref(tag)[0][0], f"geo_lookup[{tag}]:out", VALUE_FACTOR, "level-0 fraction")


def test_the_rule_refuses_a_pool_that_keeps_the_odd_tail():
    tag = "raft_l4_r4"
    kind, B, Cf, H, W1, W2, L, r = C1_CASES[tag]
    f1, f2, *_ = _c1_inputs(tag)
    (ref,), _ = _refs(lambda a, b: _pack(corr1d_pyramid(a, b, L)), (f1, f2))
    cp = [corr1d_pyramid(f1, f2, 1)[0]]
    for _ in range(L - 1):                                     # pairs counted from the END of an odd row: the tail kept, the head dropped
        x = cp[-1]
        cp.append(pool(x[..., x.shape[-1] % 2:]))
    _refused(_pack(cp), ref, f"corr1d_pyramid[{tag}]:cpyr", VALUE_FACTOR, "odd tail kept")


def test_the_rule_refuses_a_lookup_backward_that_assigns():
    tag = "raft_l4_r4"
    _, _, _, calls, _, add = _c1_inputs(tag)
    _, grads = _c1_lookup_ref(tag)
    kind, B, Cf, H, W1, W2, L, r = C1_CASES[tag]
    cpyr = _c1_inputs(tag)[2].clone().requires_grad_()
    base, disp, jobs, gout = calls[1]
    cp = [t.squeeze(-1) for t in _levels(cpyr, (B, H, W1), W2, 1, L)]
    (_c1_lookup(cp, base, disp, jobs) * gout).sum().backward()
    _refused(cpyr.grad, grads[0], f"corr1d_lookup[{tag}]:gcpyr", GRAD_FACTOR, "assigned", add=add)


def test_the_rule_refuses_a_convex_upsample_normalised_over_8_of_9_taps():
    tag = "b2_d2_5x7_n2"
    N, D, H, W, n, _, _ = CU.CASES[tag]
    f = 2 ** n
    flow, mask, _ = CU.inputs(tag)
    (ref,), _ = _refs(lambda a, b: convex(a, b, f, float(f)), (flow, mask))
    e = torch.exp(mask.view(N, 9, f, f, H, W) - mask.view(N, 9, f, f, H, W).amax(1, keepdim=True))
    s = e / e[:, :8].sum(1, keepdim=True)
    p = F.pad(float(f) * flow, (1, 1, 1, 1))
    out = sum(s[:, t].unsqueeze(1) * p[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W].reshape(N, D, 1, 1, H, W) for t in range(9))
    _refused(out.permute(0, 1, 4, 2, 5, 3).reshape(N, D, f * H, f * W), ref, f"convex_upsample[{tag}]:out", VALUE_FACTOR, "8 of 9 taps")


def test_the_rule_refuses_a_context_upsample_with_transposed_taps():
    tag = "b2_5x7"
    disp, wts, _ = _up_inputs(tag)
    (ref,), _ = _refs(upsample, (disp, wts))
    swapped = wts[:, [3 * (t % 3) + t // 3 for t in range(9)]]
    _refused(upsample(disp, swapped), ref, f"context_upsample[{tag}]:out", VALUE_FACTOR, "transposed taps")


def test_the_rule_refuses_a_sequence_loss_divided_by_n():
    gt, preds = CU.loss_inputs(2)
    preds = [p.reshape(-1) for p in preds]
    maxdisp = float(CU.LOSS_MAXDISP)
    (ref,), _ = _refs(lambda *p: _sequence_loss(p, gt.reshape(-1).to(p[0].dtype), maxdisp, [1.0, 0.7]).reshape(1), preds)
    valid = (gt > 0) & (gt < maxdisp - 1)
    miss = _sequence_loss(preds, gt.reshape(-1), maxdisp, [1.0, 0.7]) * valid.sum() / gt.numel()
    _refused(miss.reshape(1), ref, "sequence_loss[k2]:loss", VALUE_FACTOR, "divided by n")


def test_the_rule_refuses_the_convgru_update_with_z_and_1_minus_z_swapped():
    tag = "one_src"
    d = _gru_inputs(tag)

    def hq(rh, h, z, cq, wq, bq, *xs, swap=False):
        q = torch.tanh(F.conv2d(torch.cat([rh, *xs], 1), wq, bq, padding=1) + cq)
        return (1 - z) * q + z * h if swap else (1 - z) * h + z * q
    ts = (d["rh"], d["h"], d["z"], d["cq"], d["wq"], d["bq"], *d["xs"])
    (ref,), _ = _refs(hq, ts)
    _refused(hq(*ts, swap=True), ref, f"convgru_gates[{tag}]:gate_h", VALUE_FACTOR, "z and 1 - z swapped")


def test_the_rule_refuses_a_reset_backward_without_the_update_gate_term():
    tag = "one_src"
    B, hidden, cx, H, W = GRU_CASES[tag]
    d = _gru_inputs(tag)
    g_rh, g, z, r = (_nhwc(d[k]).reshape(-1, hidden) for k in ("g_rh", "g", "z", "r"))
    (ref,), _ = _refs(lambda g_rh, g, z, r: g * (1 - z) + g_rh * r, (g_rh, g, z, r))
    _refused(g_rh * r, ref, f"convgru_gate_bwd[{tag}]:buf", GRAD_FACTOR, "no update-gate term")


def test_the_rule_refuses_a_gemm_with_a_bf16_rounded_operand():
    tag = "one_src"
    d = _gru_inputs(tag)
    x, w = torch.cat([d["h"]] + d["xs"], 1), torch.cat([d["wz"], d["wr"]])
    (ref,), _ = _refs(lambda x, w: F.conv2d(x, w, None, 1, 1), (x, w))
    _refused(F.conv2d(x.bfloat16().float(), w, None, 1, 1), ref, f"convgru_gemm[{tag}]:y0", VALUE_FACTOR, "bf16 operand")


def test_the_rule_refuses_a_warp_with_align_corners():
    x, d, _ = _warp_inputs("a")
    B, C, H, W = x.shape
    (ref,), _ = _refs(O.pcw_warp, (x, d))
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(B, 1, H, W)
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(B, 1, H, W)
    grid = torch.cat((2.0 * (xx - d) / (W - 1) - 1.0, 2.0 * yy / (H - 1) - 1.0), 1).permute(0, 2, 3, 1)
    _refused(F.grid_sample(x, grid, align_corners=True), ref, "warp[a]:out", VALUE_FACTOR, "align_corners")


def test_the_rule_refuses_a_correlation_volume_divided_by_all_channels():
    B, C, H, W, md, G = CORR["a"]
    a, b, _ = corr_inputs(B, C, H, W, md, G, 200)
    (ref,), _ = _refs(lambda a, b: O.pcw_correlation_volume(a, b, md, G), (a, b))
    _refused(O.pcw_correlation_volume(a, b, md, G) / G, ref, "corr_volume[a]:out", VALUE_FACTOR, "divided by C")


def test_the_rule_refuses_a_variance_gradient_of_the_wrong_sign():
    B, D, H, W = VAR["a"]
    x, d, _, g = var_inputs(B, D, H, W, 300)
    _, grads = _refs(lambda x, d: O.cf_disparity_variance(x, D, d), (x, d), (g,), (0, 1))
    _refused(-grads[1][1], grads[1], "disparity_variance[a:var]:gdisp", GRAD_FACTOR, "wrong sign")


def test_the_rule_refuses_an_entropy_in_nats():
    refs, _ = _est_ref("b2_13", 15)
    vol, _ = SA.est_inputs("b2_13")
    pl = torch.softmax(vol.squeeze(1), 3)
    miss = 1 + torch.sum(pl * torch.log(pl + 1e-6), 3) / math.log2(vol.shape[-1])
    _refused(miss.unsqueeze(1), refs[1], "allpairs_estimates[b2_13:15]:conf_l", VALUE_FACTOR, "ln for log2")
