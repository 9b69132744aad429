"""The last two kernel files of the FoundationStereo path under the fp64 parity rule, in guard bands: conv3d_axial.hip (section A)
and disp_attention.hip (section B), all 13 C-ABI entry points of theirs.  (The benchmarked train step: tests/test_conv3d_parity.py
and tests/test_train_kernels_parity.py; the iterative families: tests/test_iterative_kernels_parity.py; STTR's transformer and head:
tests/test_attention_kernels_parity.py.)  tests/test_apc.py and tests/test_disp_attention.py keep the blocks, the modules and the
product path; this module calls the kernels themselves.

The rule (tests/parity.py::within), for every call: `want64` is the operation in fp64 on the CPU from the same fp32 inputs cast up
(F.conv3d; tests/restated.py::disp_encoder; autograd through them), `d_ref` = max|one-thread fp32 CPU run of the same expression -
want64| over the same tensor (recorded, see DREF_PATH), and the kernel may sit at most VALUE_FACTOR (forward values, statistics)
or GRAD_FACTOR (gradients) times d_ref away from want64; where d_ref is zero the floor of `within` applies.  Every tensor goes to
the parity report.  Tensors the rule refuses are listed one by one with their ratio (PAST_THE_FACTOR, strict expected failures
through tests/parity.py::Verdict), each with a kernel-free demonstration.  The near misses at the end of either section show that
the rule refuses a subtly wrong kernel.

Guard bands (tests/backends.py::Guards): every buffer a kernel WRITES is cut from the middle of a larger allocation whose bands
are checked after every call and starts as NaN; workspaces, packed weights, statistics rows and `saved` have exactly the count
their query or the header gives, and a workspace is filled with NaN again before every call; every buffer a kernel READS sits
between NaN bands.  The sequences of the transformer are channel slices of wider NaN-filled volumes: the floats between the
slices must still be NaN afterwards.

Discontinuities are conditions on the INPUTS, asserted from fp64 before a kernel runs: no pre-activation within 1e-3 of the kink
of ReLU / LeakyReLU, every LayerNorm input with a per-token variance of at least MIN_VARIANCE.  The comment of every case row
names the edge it reaches.  Both backends through the C-ABI: host emulator and gfx950.
"""
import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stereo_toolbox_amd._capi import StxError
from tests.backends import Guards, be  # noqa: F401
from tests.golden.disp_attn_config import MIN_VARIANCE, keep_masks
from tests.parity import GRAD_FACTOR, RATIO_STEP, VALUE_FACTOR, RecordedDref, listed_verdict, within
from tests.restated import disp_encoder

# d_ref of every tensor below, recorded (tests/parity.py::RecordedDref); STX_FOUNDATION_KERNELS_DREF_RECORD=<path> runs the module
# with the live values and writes them to <path> (a new or changed case).
DREF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foundation_kernels_parity_dref.json")
_dref = RecordedDref(DREF_PATH, "STX_FOUNDATION_KERNELS_DREF_RECORD")

# Tensors the rule refuses: test name -> "tensor ratio, tensor ratio".  A name without the backend holds for both; a name with it
# ("test_x[hip-...]") for that backend alone.  An entry needs a kernel-free demonstration in this module (plain torch in the
# kernel's order of additions that lands at the same ratio); strict: a case that starts to pass must leave the table.
PAST_THE_FACTOR = {
    # 17 x 192 = 3264 products per output in two fp32 chains of 1632 (NS = 2 at four N tiles), where the CPU blocks finer
    # (test_the_kernels_order_of_additions_is_past_the_factor_axial: _ax_kernel_order)
    "test_axial[ax_192_k17]": "z 2.23",
    # two tiles of 16 x 16 voxels, each ONE fp32 chain of 256 products per weight (the same test: _ax_wgrad_kernel_order)
    "test_axial[pl_h16_w16_c4]": "gw 3.44",
}
LISTED_SHARE = 0.15               # at most this share of the module's (case, tensor) pairs may be listed, per backend


class _AnyTensor:
    """Every suffix behind the last colon of `what` names a tensor of this module (tests/parity.py::Verdict)."""

    def __contains__(self, name):
        return True


@pytest.fixture
def verdict(request, parity_log):
    name = request.node.name
    reason = PAST_THE_FACTOR.get(name, PAST_THE_FACTOR.get(re.sub(r"\[(emu|hip)-", "[", name)))
    return listed_verdict(request, parity_log, reason, "past the factor, x d_ref: ", dref=_dref, tensors=_AnyTensor(),
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


def _both(run):
    """run(dtype) in fp64 and, on one thread, in fp32 -> {name: (want64, ref32)}"""
    with _one_thread():
        r64, r32 = run(torch.float64), run(torch.float32)
    assert set(r64) == set(r32)
    return {k: (r64[k], r32[k]) for k in r64}


def _wd(ref):
    """(want64, d_ref) of a pair (want64, ref32)"""
    w, r = ref
    return w, _dist(r, w)


def _call(be, Gd, what, name, *args):
    """One kernel call, and the check of every band of the test behind it."""
    be.call(name, *args)
    Gd.check(f"{what}:{name}")


def _refuses(be, Gd, what, name, *args):
    """The call returns an error, and no band is touched."""
    with pytest.raises(StxError):
        be.call(name, *args)
    Gd.check(f"{what}:{name} refused")


def _typed(Gd, dtype, count):
    """`count` elements of `dtype` cut from a Guards.out float view of exactly ceil(bytes / 4) floats, so that the sentinel bands
    start at the buffer's last float; where the byte length is no multiple of 4 the 1-3 bytes behind the buffer are sentinel
    bytes INSIDE that view, and `check` asserts them untouched."""
    size = torch.empty(0, dtype=dtype).element_size()
    nbytes = count * size
    f = Gd.out((nbytes + 3) // 4)
    raw = f.view(torch.uint8)
    tail = raw[nbytes:].clone()
    view = raw[:nbytes].view(dtype)

    def check(what=""):
        assert torch.equal(raw[nbytes:], tail), f"{what}: the {tail.numel()} bytes behind a {dtype} buffer of {count} were overwritten"
    Gd.checks.append(check)
    return view


def _typed_inp(Gd, t):
    """A non-fp32 tensor a kernel reads, between NaN bands."""
    nbytes = t.numel() * t.element_size()
    f = Gd.inp(torch.zeros((nbytes + 3) // 4))
    v = f.view(torch.uint8)[:nbytes].view(t.dtype).view(t.shape)
    v.copy_(t)
    return v


def _nan(*ts):
    for t in ts:
        if t is not None:
            t.fill_(float("nan"))


def _all_nan(*ts):
    return all(t is None or bool(torch.isnan(t).all()) for t in ts)


def _finite(t):
    return bool(torch.isfinite(t).all())


# ================================================================================================ A. conv3d_axial.hip
# The forward kernel: a workgroup owns AX_ROWS = 16 M tiles of 16 voxels -- axial: 16 planes d x 16 columns (h, w) of one batch
# element; planar: 16 rows h x 16 columns w of one plane -- and up to 4 N tiles of 16 output channels; wider outputs are further
# workgroups (whole slices of 64 channels) and a narrower remainder launch.  K is walked per channel chunk CK (the largest
# multiple of 4 up to 32 that divides Cin) in 16-float groups through the taps x CK run of a line.  The weight gradient: 32 x 32
# channel block pairs, tiles of 8 planes x 16 columns (axial) / 16 x 16 (planar), min(1024 / pairs, tiles) chunks of tiles, a
# reduce kernel whose four waves take every fourth chunk; three taps per wave up to 12 taps, five above.
#                    B   D   H   W  Cin Cout kd (0: the planar (1,3,3))
AX_CASES = {
    "ax_d15_p17_c4_o1_k3": (1, 15, 1, 17, 4, 1, 3),       # D 15 x 17 columns; Cin 4: CK 4, a run of 12 floats in one group; Cout 1; kd 3
    "ax_d16_p16_c12_o5": (1, 16, 4, 4, 12, 5, 5),         # exactly one full tile; Cin 12; Cout 5 (forward only)
    "ax_d17_p15_c32_o30_k17": (1, 17, 3, 5, 32, 30, 17),  # D 17 x 15 columns; CK 32: the 16-float pad branch of the line stride, 17 x 32 =
                                                          # 544 without a zero tail; Cout 30: a ragged second N tile, NS = 4
    "ax_b2_p9_c16_o48_k11": (2, 5, 3, 3, 16, 48, 11),     # B = 2 with a ragged plane of 9 columns; Cout 48: NT 3, NS = 2; 11 taps: three per wave
    "ax_k17_d1": (1, 1, 2, 3, 8, 8, 17),                  # kd > D at D = 1; the weight gradient's single tile (one chunk)
    "ax_k17_d3": (1, 3, 2, 3, 8, 16, 17),                 # kd > D at D = 3
    "ax_c44_o64_k13_d7": (1, 7, 2, 4, 44, 64, 13),        # Cin 44: CK 4, eleven chunks; Cout 64: one whole slice, no remainder launch; 13 taps:
                                                          # five per wave; D 7 against the weight gradient's 8 planes
    "ax_c64_o72_d8": (1, 8, 2, 2, 64, 72, 3),             # Cin 64: two chunks of 32; Cout 72: a whole slice plus NT = 1; D 8
    "ax_c28_o100_d9": (1, 9, 3, 2, 28, 100, 5),           # Cout 100: a whole slice plus NT = 3; D 9: two D tiles of the weight gradient
    "ax_c32_o32_t3": (1, 17, 1, 3, 32, 32, 5),            # CF / CC 32: exactly one block pair; three tiles of the weight gradient
    "ax_192_k17": (1, 2, 1, 2, 192, 192, 17),             # Cin 192: six chunks of 32; Cout 192: three whole slices; 17 taps
    "pl_h15_w17_c16": (1, 1, 15, 17, 16, 16, 0),          # planar 15 x 17; Cin 16: 3 x 16 = 48, no zero tail
    "pl_h16_w16_c4": (1, 2, 16, 16, 4, 8, 0),             # planar, exactly one tile per plane; Cin 4: a run of 12
    "pl_b2_h17_w15_o30": (2, 1, 17, 15, 12, 30, 0),       # planar 17 x 15, B = 2; Cout 30 (forward only)
    "pl_t4_c12_o32": (2, 1, 17, 3, 12, 32, 0),            # four tiles of the weight gradient
    "pl_t3_c28_o36": (1, 3, 2, 2, 28, 36, 0),             # CF 28 / CC 36 against the 32 x 32 block pairs; three tiles
    "pl_t5_c36_o28": (1, 5, 1, 2, 36, 28, 0),             # CF 36 / CC 28; five tiles: the reduce kernel's first wave adds two chunks
    "pl_192": (1, 2, 1, 2, 192, 192, 0),                  # planar 192 -> 192: six chunks of 32, three whole slices
    "ax_192_t28": (28, 1, 1, 1, 192, 192, 3, "w"),        # 192 x 192 in the weight gradient alone: 36 block pairs, 28 chunks of one tile
}
AX_STAT_TENSORS = ("sum", "sumsq")


def _ax_k(kd):
    return (kd, 1, 1) if kd else (1, 3, 3)


def _nd(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _cd(t):
    return t.permute(0, 4, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def _ax_inputs(tag):
    B, D, H, W, Cin, Cout, kd = AX_CASES[tag][:7]
    g = _gen(700 + list(AX_CASES).index(tag))
    return _randn(g, B, Cin, D, H, W), 0.3 * _randn(g, Cout, Cin, *_ax_k(kd)), _randn(g, B, Cout, D, H, W)


def _ax_conv(x, w):
    return F.conv3d(x, w, padding=tuple(v // 2 for v in w.shape[2:]))


@functools.lru_cache(maxsize=None)
def _ax_ref(tag):
    x, w, gz = _ax_inputs(tag)

    def run(dt):
        xs, ws = x.to(dt).requires_grad_(), w.to(dt).requires_grad_()
        z = _ax_conv(xs, ws)
        gx, gw = torch.autograd.grad((z * gz.to(dt)).sum(), (xs, ws))
        z = z.detach()
        return {"z": z, "sum": z.sum((0, 2, 3, 4)), "sumsq": (z * z).sum((0, 2, 3, 4)), "gx": gx, "gw": gw}
    return _both(run)


def _ax_pack(be, Gd, what, w, mode):
    """stx_conv3d_axial_pack_weight into exactly stx_conv3d_axial_packed_floats floats -> the packed weights between NaN bands"""
    A, Bd, k = w.shape[0], w.shape[1], tuple(w.shape[2:])
    K, N = (Bd, A) if mode == 0 else (A, Bd)
    assert be.raw("stx_conv3d_axial_supported")(K, N, *k) == 1, what
    n = be.raw("stx_conv3d_axial_packed_floats")(K, N, *k)
    assert n > 0, what
    wp = Gd.out(n)
    _call(be, Gd, what, "stx_conv3d_axial_pack_weight", Gd.inp(w.reshape(A, Bd, -1)), wp, A, Bd, *k, mode)
    assert _finite(wp), f"{what}: packed weights left unwritten"
    return Gd.inp(wp)


def _ax_fwd(be, Gd, what, x_nd, wp, Cout, k, scale=None, bias=None, residual=None, act=0, stats=True):
    """stx_conv3d_axial_fwd -> (out [B][D][H][W][Cout], stats [rows][2][Cout] with exactly the query's rows, or None)"""
    B, D, H, W, Cin = x_nd.shape
    out, st = Gd.out(B, D, H, W, Cout), None
    if stats:
        rows = be.raw("stx_conv3d_axial_fwd_stat_rows")(B, D, H, W, Cin, Cout, *k)
        assert rows > 0, what
        st = Gd.out(rows, 2, Cout)
    _call(be, Gd, what, "stx_conv3d_axial_fwd", x_nd, wp, out, scale, bias, residual, st, B, D, H, W, Cin, Cout, *k, act)
    return out, st


def _ax_wgrad(be, Gd, what, x_nd, g_nd, ws, k):
    B, D, H, W, CF = x_nd.shape
    CC = g_nd.shape[-1]
    dw = Gd.out(CC, CF, k[0] * k[1] * k[2])
    _nan(ws)
    _call(be, Gd, what, "stx_conv3d_axial_wgrad", x_nd, g_nd, dw, ws, B, D, H, W, CF, CC, *k)
    return dw


def _ax_weight_gradient(be, Gd, verdict, what, ref, xd, gd, k):
    """stx_conv3d_axial_wgrad twice into the same NaN-refilled workspace of exactly the query's count: the same bits"""
    B, D, H, W, Cin = xd.shape
    Cout = gd.shape[-1]
    n = be.raw("stx_conv3d_axial_wgrad_workspace_floats")(B, D, H, W, Cin, Cout, *k)
    assert n > 0, what
    ws = Gd.out(n)
    dw = _ax_wgrad(be, Gd, what, xd, gd, ws, k)
    verdict.within(dw.cpu().view(Cout, Cin, *k), *_wd(ref["gw"]), GRAD_FACTOR, what + ":gw")
    again = _ax_wgrad(be, Gd, what, xd, gd, ws, k)
    assert torch.equal(again.cpu(), dw.cpu()), what


@pytest.mark.parametrize("tag", list(AX_CASES))
def test_axial(be, verdict, tag):
    """The raw forward with its statistics rows (and without: the same bits) against fp64 F.conv3d; where Cout % 4 == 0 the data
    gradient (the forward on mode-1 weights, Cin / Cout exchanged) and the weight gradient, twice into the same NaN-refilled
    workspace of exactly the query's count (the same bits)."""
    B, D, H, W, Cin, Cout, kd = AX_CASES[tag][:7]
    parts = (AX_CASES[tag] + ("fdw",))[7]                               # forward, data gradient, weight gradient
    k = _ax_k(kd)
    x, w, gz = _ax_inputs(tag)
    ref = _ax_ref(tag)
    what = f"axial[{be.name}:{tag}]"
    Gd = Guards(be)
    xd = Gd.inp(_nd(x))
    if "f" not in parts:
        _ax_weight_gradient(be, Gd, verdict, what, ref, xd, Gd.inp(_nd(gz)), k)
        verdict.done()
        return
    wp = _ax_pack(be, Gd, what, w, 0)
    z, st = _ax_fwd(be, Gd, what, xd, wp, Cout, k)
    verdict.within(_cd(z.cpu()), *_wd(ref["z"]), VALUE_FACTOR, what + ":z")
    st = st.cpu()
    assert _finite(st), f"{what}: a row of the statistics was not written"
    rows = st.double().sum(0)                                            # the rows added in double
    verdict.within(rows[0], *_wd(ref["sum"]), VALUE_FACTOR, what + ":sum")
    verdict.within(rows[1], *_wd(ref["sumsq"]), VALUE_FACTOR, what + ":sumsq")
    z_plain, _ = _ax_fwd(be, Gd, what, xd, wp, Cout, k, stats=False)
    assert torch.equal(z_plain.cpu(), z.cpu()), what
    if Cout % 4:
        assert be.raw("stx_conv3d_axial_wgrad_workspace_floats")(B, D, H, W, Cin, Cout, *k) == 0, what
        verdict.done()
        return
    gd = Gd.inp(_nd(gz))
    gx, _ = _ax_fwd(be, Gd, what, gd, _ax_pack(be, Gd, what, w, 1), Cin, k, stats=False)
    verdict.within(_cd(gx.cpu()), *_wd(ref["gx"]), GRAD_FACTOR, what + ":gx")
    _ax_weight_gradient(be, Gd, verdict, what, ref, xd, gd, k)
    verdict.done()


# ------------------------------------------------------------------------------------------ the epilogue
#                   B  D  H  W  Cin Cout kd
EPI_CASES = {
    "ax_o12": (1, 5, 2, 3, 8, 12, 3),            # axial; Cout 12: four idle lanes of the N tile read no scale / bias
    "pl_o72": (1, 1, 3, 3, 4, 72, 0),            # planar; Cout 72: scale / bias / residual indexed past a whole slice (nt0 = 4)
}
EPI_ACTS = (0, 1, 2, 3)                          # none, ReLU, Mish, LeakyReLU(0.01)
EPI_OPERANDS = {"scale": (1, 0, 0), "bias": (0, 1, 0), "res": (0, 0, 1), "all": (1, 1, 1)}
KINK = 1e-3
LEAKY_SLOPE = 0.01


def _epi_pre(z, sc, bs, res, use):
    v = z
    if use[0]:
        v = v * sc.to(z.dtype).view(1, -1, 1, 1, 1)
    if use[1]:
        v = v + bs.to(z.dtype).view(1, -1, 1, 1, 1)
    if use[2]:
        v = v + res.to(z.dtype)
    return v


def _epi_act(v, act, slope=LEAKY_SLOPE):
    return v if act == 0 else (F.relu(v) if act == 1 else (F.mish(v) if act == 2 else F.leaky_relu(v, slope)))


def _epi_draw(tag, seed):
    B, D, H, W, Cin, Cout, kd = EPI_CASES[tag]
    g = _gen(seed)
    x, w = _randn(g, B, Cin, D, H, W), 0.3 * _randn(g, Cout, Cin, *_ax_k(kd))
    sc = 0.5 + torch.rand(Cout, generator=g)
    return x, w, sc, 0.5 * _randn(g, Cout), _randn(g, B, Cout, D, H, W)


@functools.lru_cache(maxsize=None)
def _epi_inputs(tag):
    """The first seed from the case's base with no pre-activation of any operand set within KINK of zero, in fp64 and in fp32."""
    base = 800 + 40 * list(EPI_CASES).index(tag)
    for seed in range(base, base + 40):
        x, w, sc, bs, res = _epi_draw(tag, seed)
        if all(bool((_epi_pre(_ax_conv(x.to(dt), w.to(dt)), sc, bs, res, use).abs() >= KINK).all())
               for dt in (torch.float64, torch.float32) for use in EPI_OPERANDS.values()):
            return x, w, sc, bs, res
    raise AssertionError(f"{tag}: no seed in {base}..{base + 39} keeps every pre-activation {KINK} away from the kink")


@functools.lru_cache(maxsize=None)
def _epi_ref(tag):
    x, w, sc, bs, res = _epi_inputs(tag)

    def run(dt):
        z = _ax_conv(x.to(dt), w.to(dt))
        return {f"a{act}_{ops}": _epi_act(_epi_pre(z, sc, bs, res, use), act) for act in EPI_ACTS for ops, use in EPI_OPERANDS.items()}
    return _both(run)


@pytest.mark.parametrize("tag", list(EPI_CASES))
def test_axial_epilogue(be, verdict, tag):
    """act(conv(x) * scale + bias + residual) with each of scale / bias / residual alone and all together, activation codes
    0 / 1 / 2 / 3, against the same expression in fp64."""
    B, D, H, W, Cin, Cout, kd = EPI_CASES[tag]
    k = _ax_k(kd)
    x, w, sc, bs, res = _epi_inputs(tag)
    z64 = _ax_conv(x.double(), w.double())
    for use in EPI_OPERANDS.values():                                    # the condition on the inputs, before any kernel runs
        assert bool((_epi_pre(z64, sc, bs, res, use).abs() >= KINK).all()), tag
    ref = _epi_ref(tag)
    what = f"axial_epilogue[{be.name}:{tag}]"
    Gd = Guards(be)
    xd, wp = Gd.inp(_nd(x)), _ax_pack(be, Gd, what, w, 0)
    dsc, dbs, dres = Gd.inp(sc), Gd.inp(bs), Gd.inp(_nd(res))
    for act in EPI_ACTS:
        for ops, use in EPI_OPERANDS.items():
            y, _ = _ax_fwd(be, Gd, what, xd, wp, Cout, k, dsc if use[0] else None, dbs if use[1] else None, dres if use[2] else None, act,
                           stats=False)
            verdict.within(_cd(y.cpu()), *_wd(ref[f"a{act}_{ops}"]), VALUE_FACTOR, f"{what}:a{act}_{ops}")
    verdict.done()


def test_axial_refusals(be):
    """Shapes and codes that are not served: the queries return 0, the calls return an error and launch nothing -- outputs,
    statistics and workspaces stay NaN, bands intact."""
    what = f"axial_refusals[{be.name}]"
    Gd = Guards(be)
    B, D, H, W = 1, 3, 2, 3
    q = {n: be.raw("stx_conv3d_axial_" + n) for n in ("supported", "packed_floats", "fwd_stat_rows", "wgrad_workspace_floats")}
    wbuf, wp_out = Gd.inp(torch.zeros(4096)), Gd.out(4096)
    #            Cin Cout  k
    for bad in ((8, 8, (2, 1, 1)), (8, 8, (19, 1, 1)), (8, 8, (3, 3, 3)), (30, 8, (1, 3, 3)), (196, 8, (5, 1, 1)), (30, 8, (5, 1, 1)),
                (8, 196, (1, 3, 3)), (8, 8, (1, 1, 1)), (8, 8, (1, 5, 5)), (8, 8, (4, 1, 1))):
        Cin, Cout, k = bad
        assert q["supported"](Cin, Cout, *k) == 0 and q["packed_floats"](Cin, Cout, *k) == 0, bad
        assert q["fwd_stat_rows"](B, D, H, W, Cin, Cout, *k) == 0 and q["wgrad_workspace_floats"](B, D, H, W, Cin, Cout, *k) == 0, bad
        _refuses(be, Gd, what, "stx_conv3d_axial_pack_weight", wbuf, wp_out, Cout, Cin, *k, 0)
        x, out, st = Gd.inp(torch.zeros(B, D, H, W, Cin)), Gd.out(B, D, H, W, Cout), Gd.out(4, 2, Cout)
        _refuses(be, Gd, what, "stx_conv3d_axial_fwd", x, wbuf, out, None, None, None, st, B, D, H, W, Cin, Cout, *k, 0)
        gz, dw, ws = Gd.inp(torch.zeros(B, D, H, W, Cout)), Gd.out(Cout, Cin, k[0] * k[1] * k[2]), Gd.out(4096)
        _refuses(be, Gd, what, "stx_conv3d_axial_wgrad", x, gz, dw, ws, B, D, H, W, Cin, Cout, *k)
        assert _all_nan(wp_out, out, st, dw, ws), bad
    # the weight gradient with CC = 30 (the forward serves it), pack mode 2, activation code 4 and -1
    k = (5, 1, 1)
    assert q["supported"](8, 30, *k) == 1 and q["wgrad_workspace_floats"](B, D, H, W, 8, 30, *k) == 0
    x, gz, dw, ws = Gd.inp(torch.zeros(B, D, H, W, 8)), Gd.inp(torch.zeros(B, D, H, W, 30)), Gd.out(30, 8, 5), Gd.out(4096)
    _refuses(be, Gd, what, "stx_conv3d_axial_wgrad", x, gz, dw, ws, B, D, H, W, 8, 30, *k)
    _refuses(be, Gd, what, "stx_conv3d_axial_pack_weight", wbuf, wp_out, 8, 8, *k, 2)
    out, st = Gd.out(B, D, H, W, 8), Gd.out(be.raw("stx_conv3d_axial_fwd_stat_rows")(B, D, H, W, 8, 8, *k), 2, 8)
    for act in (4, -1):
        _refuses(be, Gd, what, "stx_conv3d_axial_fwd", x, wbuf, out, None, None, None, st, B, D, H, W, 8, 8, *k, act)
    assert _all_nan(dw, ws, wp_out, out, st)


# ================================================================================================ B. disp_attention.hip
DA_SHORT = ("qw", "qb", "kw", "kb", "vw", "vb", "ow", "ob", "w1", "b1", "w2", "b2", "g1", "e1", "g2", "e2")
SEED_A, SEED_B = 0x1234_5678_9ABC_DEF0, -(2 ** 62) + 12345              # both key words in use; a negative seed


def _vol(B, D, H, W, Cw, c0, gap=0):
    """The channel slice [c0 : c0 + C] of a [B][D][H][W][Cw] volume (`gap` floats between the batch elements) -> N and the view"""
    return B * H * W, dict(hw=H * W, sb=D * H * W * Cw + gap, sp=Cw, st=H * W * Cw, c0=c0, total=B * (D * H * W * Cw + gap))


def _seq(N, L, Cw, c0):
    """The channel slice of a pitched [N][L][Cw] tensor, hw = 1"""
    return N, dict(hw=1, sb=L * Cw, sp=0, st=Cw, c0=c0, total=N * L * Cw)


def _dense(N, L, C):
    return dict(hw=1, sb=L * C, sp=0, st=C, c0=0, total=N * L * C)


def _da_case(L, C, nhead, F_, layers, pe, where):
    N, view = where
    return N, L, C, nhead, F_, layers, pe, view


# The kernels: a wave owns a sequence; every product is up to 2 x 2 tiles of 16 x 16 (L, C, F against 16); the parameter
# gradients are added per UNIT of four consecutive sequences and the units in four chunks of ceil(units / 4).
#                          L   C  heads F layers pe   the view
DA_CASES = {
    "l1_c4_hd1": _da_case(1, 4, 4, 4, 1, True, _vol(1, 1, 1, 1, 8, 4)),             # the minimum: one token, C 4, F 4, head dim 1, one sequence
    "l15_c16_f20": _da_case(15, 16, 2, 20, 2, True, _vol(1, 15, 1, 3, 24, 4)),      # L 15 / C 16 / F 20 > C; head dim 8; N 3: a partial unit
    "l16_c20_f4": _da_case(16, 20, 5, 4, 1, False, _vol(2, 16, 1, 2, 28, 8, gap=64)),   # L 16 / C 20 / F 4 < C; head dim 4; N 4: one whole unit; a batch gap; no pe
    "l17_c32_f32": _da_case(17, 32, 4, 32, 2, True, _seq(5, 17, 40, 4)),            # L 17 / C 32 / F 32; pitched [N][L][Cw], hw = 1; N 5: a unit of one
    "l31_c28_hd7": _da_case(31, 28, 4, 20, 1, True, _vol(1, 31, 3, 3, 32, 4)),      # L 31; head dim 7; N 9: three units in chunks of one, the last chunk empty
    "l32_c4_one_head": _da_case(32, 4, 1, 32, 1, True, _vol(1, 32, 3, 1, 12, 8)),   # L 32; nhead 1; F 32 > C 4
    "l5_c16_layers8": _da_case(5, 16, 4, 16, 8, True, _seq(5, 5, 20, 4)),           # eight layers
    "l16_c16_n18": _da_case(16, 16, 2, 16, 1, False, _vol(1, 16, 3, 6, 20, 4)),     # N 18: five units (the last of two sequences) in chunks of 2 / 2 / 1 / 0
}


def _da_index(case, view=None):
    """[N][L][C] flat offsets of the floats of every token, by the header's address function"""
    N, L, C = case[:3]
    v = view or case[7]
    n, t, c = torch.arange(N).view(N, 1, 1), torch.arange(L).view(1, L, 1), torch.arange(C).view(1, 1, C)
    return (n // v["hw"]) * v["sb"] + (n % v["hw"]) * v["sp"] + t * v["st"] + c + v["c0"]


def _da_embed(case, seq, view=None):
    """The sequences inside a NaN-filled flat buffer of the view's size"""
    v = view or case[7]
    flat = torch.full((v["total"],), float("nan"))
    flat[_da_index(case, view).view(-1)] = seq.reshape(-1)
    return flat


def _da_extract(case, flat, what, view=None):
    """The sequences out of the flat buffer; every float between them must still be NaN"""
    flat = flat.cpu()
    idx = _da_index(case, view).view(-1)
    gap = torch.ones(flat.numel(), dtype=torch.bool)
    gap[idx] = False
    assert bool(torch.isnan(flat[gap]).all()), f"{what}: a float outside the channel slice was written"
    return flat[idx].view(case[0], case[1], case[2])


def _da_shapes(C, F_):
    return [(C, C), (C,), (C, C), (C,), (C, C), (C,), (C, C), (C,), (F_, C), (F_,), (C, F_), (C,), (C,), (C,), (C,), (C,)]


def _da_draw(tag, seed):
    N, L, C, nhead, F_, layers, pe, _ = DA_CASES[tag]
    g = _gen(seed)
    params = []
    for _ in range(layers):
        for i, s in enumerate(_da_shapes(C, F_)):
            t = _randn(g, *s)
            params.append(0.3 * t if len(s) == 2 else (1.0 + 0.1 * t if i in (12, 14) else 0.1 * t))
    return _randn(g, N, L, C), (0.5 * _randn(g, L, C) if pe else None), params, _randn(g, N, L, C)


def _da_scale(p):
    return float(np.float32(1.0 / (1.0 - float(np.float32(p)))))


def _da_masks(tag, drop):
    if drop is None:
        return None, 1.0
    N, L, C, nhead, F_, layers, _, _ = DA_CASES[tag]
    p, seed = drop
    return torch.from_numpy(keep_masks(seed, p, N, L, C, F_, layers)), _da_scale(p)


def _da_variances_ok(tag, x, pe, params, eps, drop):
    nhead = DA_CASES[tag][3]
    masks, scale = _da_masks(tag, drop)
    zs = []
    disp_encoder(x.double(), None if pe is None else pe.double(), [t.double() for t in params], nhead, eps=eps, masks=masks, scale=scale,
                 norm_inputs=zs)
    return all(bool((z.var(-1, unbiased=False) >= MIN_VARIANCE).all()) for z in zs)


@functools.lru_cache(maxsize=None)
def _da_inputs(tag, eps=1e-5, drop=None):
    """The first seed from the case's base whose LayerNorm inputs all have a per-token variance of at least MIN_VARIANCE in fp64."""
    base = 900 + 10 * list(DA_CASES).index(tag)
    for seed in range(base, base + 10):
        x, pe, params, gy = _da_draw(tag, seed)
        if _da_variances_ok(tag, x, pe, params, eps, drop):
            return x, pe, params, gy
    raise AssertionError(f"{tag}: no seed in {base}..{base + 9} keeps every LayerNorm input's variance at {MIN_VARIANCE}")


def _da_names(layers):
    return [f"l{i}.{n}" for i in range(layers) for n in DA_SHORT]


@functools.lru_cache(maxsize=None)
def _da_ref(tag, eps=1e-5, drop=None, miss=None):
    """y, gx and the 16 x layers parameter gradients of the restatement (with the keep masks of `drop` = (p, seed))"""
    N, L, C, nhead, F_, layers, _, _ = DA_CASES[tag]
    x, pe, params, gy = _da_inputs(tag, eps, drop)
    masks, scale = _da_masks(tag, drop)

    def run(dt):
        xs = x.to(dt).requires_grad_()
        ps = [t.to(dt).requires_grad_() for t in params]
        y = disp_encoder(xs, None if pe is None else pe.to(dt), ps, nhead, eps=eps, masks=masks, scale=scale, miss=miss)
        gs = torch.autograd.grad((y * gy.to(dt)).sum(), [xs] + ps, allow_unused=True)
        gs = [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(gs, [xs] + ps)]
        return {"y": y.detach(), "gx": gs[0], **dict(zip(_da_names(layers), gs[1:]))}
    return _both(run)


class _DaDev:
    """The operands of one case on the backend: parameters and pe between NaN bands, the pointer tables of the C-ABI."""

    def __init__(self, be, Gd, tag, eps=1e-5, drop=None):
        self.be, self.Gd, self.case = be, Gd, DA_CASES[tag]
        self.N, self.L, self.C, self.nhead, self.F, self.layers, _, self.view = self.case
        self.x, self.pe, self.params, self.gy = _da_inputs(tag, eps, drop)
        self.dparams = [Gd.inp(t) for t in self.params]
        self.dpe = Gd.inp(self.pe)
        self.ptab = self.table(self.dparams)
        self.eps, self.p, self.seed, self.grads = eps, 0.0, None, None
        if drop is not None:
            self.p, self.seed = drop[0], _typed_inp(Gd, torch.tensor([drop[1]], dtype=torch.int64))

    @staticmethod
    def table(tensors):
        return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])

    def dims(self, view, **over):
        d = dict(N=self.N, L=self.L, C=self.C, nhead=self.nhead, F=self.F, layers=self.layers, hw=view["hw"], sb=view["sb"], sp=view["sp"],
                 st=view["st"])
        d.update(over)
        return tuple(d[k] for k in ("N", "L", "C", "nhead", "F", "layers", "hw", "sb", "sp", "st"))

    def inp(self, seq, view):
        """The sequences in a NaN-filled buffer of the view's size, between NaN bands -> (buffer, the slice's base pointer)"""
        buf = self.Gd.inp(_da_embed(self.case, seq, view))
        return buf, buf[view["c0"]:]

    def out(self, view):
        buf = self.Gd.out(view["total"])
        return buf, buf[view["c0"]:]

    def fwd(self, what, view=None, saved=True, pe=True, refused=False, **over):
        """stx_disp_attention_fwd -> (y [N][L][C] on the CPU, saved [layers][N][L][C] or None)"""
        view = view or self.view
        _, xp = self.inp(self.x, view)
        ybuf, yp = self.out(view)
        sv = self.Gd.out(self.layers, self.N, self.L, self.C) if saved else None
        args = (xp, self.dpe if pe else None, self.ptab, yp, sv, self.seed, over.pop("p", self.p), self.eps, *self.dims(view, **over))
        if refused:
            _refuses(self.be, self.Gd, what, "stx_disp_attention_fwd", *args)
            assert _all_nan(ybuf, sv), f"{what}: a refused call wrote"
            return None, None
        _call(self.be, self.Gd, what, "stx_disp_attention_fwd", *args)
        return _da_extract(self.case, ybuf, what, view), sv

    def bwd(self, what, saved, view=None, wanted=None, gx=True, gbuf=True, extra=0, short=0, refused=False, **over):
        """stx_disp_attention_bwd with a workspace of exactly the query's count (+ `extra`, declared - `short`), NaN before the
        call -> (gx [N][L][C] or None, the gradients of the wanted tensors by name; unwanted: None), all on the CPU"""
        view = view or self.view
        names = _da_names(self.layers)
        wanted = set(names) if wanted is None else set(wanted)
        _, gyp = self.inp(self.gy, view)
        gxbuf, gxp = self.out(view) if gx else (None, None)
        if self.grads is None:                                            # one set of banded buffers per case, NaN before every call
            self.grads = [self.Gd.out(*s) for s in _da_shapes(self.C, self.F) * self.layers]
        grads = self.grads
        _nan(*grads)
        gtab = self.table([g_ if n in wanted else None for g_, n in zip(grads, names)])
        n = self.be.raw("stx_disp_attention_bwd_workspace_floats")(self.N, self.L, self.C, self.F)
        assert n > 0, what
        ws = self.Gd.out(n + extra)
        gb = self.Gd.out(self.N, self.L, self.C) if gbuf else None
        args = (gyp, self.Gd.inp(saved), self.ptab, gtab, gxp, gb, ws, n + extra - short, self.seed, over.pop("p", self.p), self.eps,
                *self.dims(view, **over))
        if refused:
            _refuses(self.be, self.Gd, what, "stx_disp_attention_bwd", *args)
            assert _all_nan(gxbuf, gb, ws, *grads), f"{what}: a refused call wrote"
            return None, None
        _call(self.be, self.Gd, what, "stx_disp_attention_bwd", *args)
        out = {}
        for g_, name in zip(grads, names):
            if name in wanted:
                out[name] = g_.cpu()
            else:
                assert _all_nan(g_), f"{what}: the gradient of the frozen {name} was written"
                out[name] = None
        return (_da_extract(self.case, gxbuf, what, view) if gx else None), out


def _da_check_all(verdict, what, ref, y, gx, grads):
    verdict.within(y, *_wd(ref["y"]), VALUE_FACTOR, what + ":y")
    verdict.within(gx, *_wd(ref["gx"]), GRAD_FACTOR, what + ":gx")
    for name, g_ in grads.items():
        verdict.within(g_, *_wd(ref[name]), GRAD_FACTOR, f"{what}:{name}")


@pytest.mark.parametrize("tag", list(DA_CASES))
def test_disp_attention(be, verdict, tag):
    """stx_disp_attention_fwd and _bwd on a channel slice of a wider NaN-filled volume against the restatement in fp64 (y, gx, all
    16 x layers parameter gradients); `saved == NULL` gives the same y; the dense [N][L][C] form of the same data gives the same
    bits of everything; one layer runs without gbuf."""
    dev = _DaDev(be, Guards(be), tag)
    ref = _da_ref(tag)
    what = f"disp_attention[{be.name}:{tag}]"
    pe = dev.pe is not None
    assert be.raw("stx_disp_attention_supported")(dev.L, dev.C, dev.nhead, dev.F, dev.layers) == 1
    y, saved = dev.fwd(what, pe=pe)
    assert _finite(saved), what
    y_plain, _ = dev.fwd(what, pe=pe, saved=False)
    assert torch.equal(y_plain, y), what
    gx, grads = dev.bwd(what, saved, gbuf=dev.layers > 1)
    _da_check_all(verdict, what, ref, y, gx, grads)
    dense = _dense(dev.N, dev.L, dev.C)
    y_d, saved_d = dev.fwd(what, view=dense, pe=pe)
    gx_d, grads_d = dev.bwd(what, saved_d, view=dense, gbuf=dev.layers > 1)
    assert torch.equal(y_d, y) and torch.equal(saved_d.cpu(), saved.cpu()) and torch.equal(gx_d, gx), what
    assert all(torch.equal(grads_d[n], grads[n]) for n in grads), what
    verdict.done()


def test_disp_attention_optional_operands(be, verdict):
    """Two layers: gx == NULL; layer 0 frozen with gx == NULL and gbuf == NULL (the walk stops at layer 1, layer 0's buffers stay
    NaN); a single wanted tensor; a workspace larger than the query's count -- the same bits as the full call every time; pe ==
    NULL and eps = 1e-3 against the restatement."""
    tag = "l15_c16_f20"
    Gd = Guards(be)
    dev = _DaDev(be, Gd, tag)
    what = f"disp_attention_optional[{be.name}:{tag}]"
    names = _da_names(dev.layers)
    y, saved = dev.fwd(what)
    gx, full = dev.bwd(what, saved)
    verdict.within(y, *_wd(_da_ref(tag)["y"]), VALUE_FACTOR, what + ":y")

    def same(got, wanted):
        assert all((got[n] is not None) == (n in wanted) for n in names), what
        assert all(torch.equal(got[n], full[n]) for n in wanted), what
    gx_, got = dev.bwd(what, saved, gx=False)
    assert gx_ is None
    same(got, names)
    upper = [n for n in names if n.startswith("l1.")]
    for gbuf in (True, False):
        _, got = dev.bwd(what, saved, gx=False, wanted=upper, gbuf=gbuf)
        same(got, upper)
    _, got = dev.bwd(what, saved, gx=False, wanted=["l1.w1"], gbuf=False)
    same(got, ["l1.w1"])
    gx_, got = dev.bwd(what, saved, wanted=["l0.g1"])
    same(got, ["l0.g1"])
    assert torch.equal(gx_, gx), what
    gx_, got = dev.bwd(what, saved, extra=68)
    same(got, names)
    assert torch.equal(gx_, gx), what
    # eps = 1e-3 and no pe: their own references
    dev3 = _DaDev(be, Gd, tag, eps=1e-3)
    y3, saved3 = dev3.fwd(what, pe=False)
    gx3, grads3 = dev3.bwd(what, saved3)
    x, pe, params, gy = _da_inputs(tag, 1e-3)

    def run(dt):
        xs, ps = x.to(dt).requires_grad_(), [t.to(dt).requires_grad_() for t in params]
        yr = disp_encoder(xs, None, ps, dev.nhead, eps=1e-3)
        gs = torch.autograd.grad((yr * gy.to(dt)).sum(), [xs] + ps)
        return {"y": yr.detach(), "gx": gs[0], **dict(zip(names, gs[1:]))}
    _da_check_all(verdict, what + ":eps3_nope", _both(run), y3, gx3, grads3)
    verdict.done()


DROP_CASES = {"p01": ("l17_c32_f32", 0.1, SEED_A), "p05": ("l15_c16_f20", 0.5, SEED_B)}


@pytest.mark.parametrize("which", list(DROP_CASES))
def test_disp_attention_dropout(be, verdict, which):
    """Dropout on a pitched view: stx_disp_attention_masks writes exactly [layers][3][N][L][max(C, F)] bytes, equal to the
    documented counter layout; y and every gradient against the restatement evaluated with those masks -- forward and backward
    draw the same mask."""
    tag, p, seed = DROP_CASES[which]
    drop = (p, seed)
    Gd = Guards(be)
    dev = _DaDev(be, Gd, tag, drop=drop)
    what = f"disp_attention_dropout[{be.name}:{which}]"
    Cm = max(dev.C, dev.F)
    masks = _typed(Gd, torch.uint8, dev.layers * 3 * dev.N * dev.L * Cm)
    _call(be, Gd, what, "stx_disp_attention_masks", dev.seed, p, masks, dev.N, dev.L, dev.C, dev.F, dev.layers)
    want = keep_masks(seed, p, dev.N, dev.L, dev.C, dev.F, dev.layers)
    assert np.array_equal(masks.cpu().numpy().reshape(want.shape), want), what
    assert 0 < want.mean() < 1
    ref = _da_ref(tag, drop=drop)
    y, saved = dev.fwd(what)
    gx, grads = dev.bwd(what, saved)
    _da_check_all(verdict, what, ref, y, gx, grads)
    y0, _ = dev.fwd(what, p=0.0)                                          # p = 0 with a seed: nothing is drawn
    verdict.within(y0, *_wd(_da_ref(tag)["y"]), VALUE_FACTOR, what + ":y_p0")
    verdict.done()


def test_disp_attention_refusals(be):
    """Views, sizes and operands that are not served: an error, nothing launched -- y, saved, gx, gbuf, the workspace and every
    gradient stay NaN, bands intact; the queries return 0."""
    tag = "l15_c16_f20"
    Gd = Guards(be)
    dev = _DaDev(be, Gd, tag)
    what = f"disp_attention_refusals[{be.name}]"
    _, saved = dev.fwd(what)
    v = dev.view
    sup, wsq = be.raw("stx_disp_attention_supported"), be.raw("stx_disp_attention_bwd_workspace_floats")
    # a stride that is no multiple of 4 or negative; N % hw != 0 (N = 3)
    for over in (dict(st=v["st"] + 2), dict(sp=v["sp"] + 1), dict(sb=v["sb"] + 3), dict(hw=2), dict(hw=0), dict(sp=-4)):
        dev.fwd(what, refused=True, **over)
        dev.bwd(what, saved, refused=True, **over)
    for over in (dict(L=33), dict(C=36, nhead=6), dict(C=36, nhead=4), dict(nhead=1), dict(F=36), dict(F=30), dict(layers=9), dict(layers=0),
                 dict(p=1.0), dict(p=-0.1), dict(N=0)):
        dev.fwd(what, refused=True, **over)
        dev.bwd(what, saved, refused=True, **over)
    assert sup(33, 16, 2, 20, 2) == 0 and sup(15, 36, 6, 20, 2) == 0 and sup(15, 36, 4, 20, 2) == 0 and sup(15, 16, 1, 20, 2) == 0
    assert sup(15, 16, 2, 36, 2) == 0 and sup(15, 16, 2, 20, 9) == 0 and sup(15, 16, 2, 20, 2) == 1
    assert wsq(3, 33, 16, 20) == 0 and wsq(3, 15, 36, 20) == 0 and wsq(3, 15, 16, 30) == 0 and wsq(0, 15, 16, 20) == 0
    assert wsq(3, 15, 16, 20) == 4 * 16 * 16 + 2 * 16 * 20 + 9 * 16 + 20 and wsq(5, 15, 16, 20) == 2 * wsq(3, 15, 16, 20)
    dev.bwd(what, saved, short=1, refused=True)                           # a workspace one float short
    dev.bwd(what, saved, gbuf=False, refused=True)                        # two layers, a gradient wanted from layer 0, no gbuf
    dev.bwd(what, saved, gbuf=False, gx=False, wanted=["l0.e2"], refused=True)
    dev.bwd(what, saved, gx=False, wanted=[], refused=True)               # no gradient wanted
    masks = _typed(Gd, torch.uint8, 64)
    seed = _typed_inp(Gd, torch.tensor([SEED_A], dtype=torch.int64))
    for n_, l_, c_, f_, layers, p in ((1, 33, 4, 4, 1, 0.1), (1, 4, 36, 4, 1, 0.1), (1, 4, 4, 4, 9, 0.1), (1, 4, 4, 4, 1, 1.0), (0, 4, 4, 4, 1, 0.1)):
        _refuses(be, Gd, what, "stx_disp_attention_masks", seed, p, masks, n_, l_, c_, f_, layers)
    assert _all_nan(masks.view(torch.float32))


# ================================================================================================ the entries of PAST_THE_FACTOR, without a kernel
def _fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then to fp32 (a
    double rounding differs from fmaf in about one sum of 2^29)."""
    return (a.double() * b.double() + c.double()).float()


def _listed(prefix):
    """(test name, {tensor: ratio}) of the rows of PAST_THE_FACTOR whose test name starts with `prefix`"""
    return [(name, {t: float(r) for t, r in (tr.split() for tr in row.split(", "))}) for name, row in PAST_THE_FACTOR.items()
            if name.startswith(prefix)]


def _demonstrated(chain, ref, what, tensors, factor_of):
    """Every listed tensor, evaluated kernel-free in the kernel's order of additions, is refused by the very `within` call with the
    very d_ref of its row, and lands at the row's ratio to the two decimals written down (tests/parity.py::RATIO_STEP)."""
    for t, ratio in tensors.items():
        want, live = _wd(ref[t])
        dref = _dref(f"{what}:{t}", live)
        got = _dist(chain[t], want) / dref
        print(f"{what}:{t} in the kernel's order: {got:.2f} x d_ref, listed {ratio:.2f}")
        assert abs(got - ratio) <= RATIO_STEP, (what, t, got, ratio)
        with pytest.raises(AssertionError, match="kernel order"):
            within(chain[t], want, dref, factor_of(t), "kernel order")


def _ax_kernel_order(x, w):
    """conv3d_axial_kernel in plain torch: x [B][Cin][D][H][W], w [Cout][Cin][*k] -> z [B][Cout][D][H][W].  Per channel chunk CK
    (the largest multiple of 4 up to 32 that divides Cin) and run (the taps along a line: all kd of the axial kernel, the three
    kw of one kh of the planar one) the taps x CK floats of a voxel are walked in groups of 16; inside a group the MFMA with
    index j = 0..3 contracts the elements 16 g + 4 q + j over q = 0..3, each one fmaf; group s of a chunk adds into accumulator
    set s % NS (NS = 4 up to two N tiles of the launch, 2 at three and four), and the sets are summed at the end as (0 + 1) +
    (2 + 3) or 0 + 1.  Elements behind the run's end are zeros and leave the sum unchanged."""
    Cout, Cin = w.shape[:2]
    kd, kh, kw = w.shape[2:]
    planar = kd == 1
    tpr, nrun = (3, 3) if planar else (kd, 1)
    CK = next(c for c in range(32, 3, -4) if Cin % c == 0)
    ng = (tpr * CK + 15) // 16
    xp = F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2, kd // 2, kd // 2))
    B, _, D, H, W = x.shape

    def tap_view(tap):
        a, b, c = (0, tap // 3, tap % 3) if planar else (tap, 0, 0)
        return xp[:, :, a:a + D, b:b + H, c:c + W]
    out = torch.empty(B, Cout, D, H, W)
    NTall = -(-Cout // 16)
    for nt_lo in range(0, NTall, 4):
        NT = min(4, NTall - nt_lo)
        NS = 4 if NT <= 2 else 2
        n0, n1 = 16 * nt_lo, min(Cout, 16 * (nt_lo + NT))
        acc = [torch.zeros(B, n1 - n0, D, H, W) for _ in range(NS)]
        for ch in range(Cin // CK):
            for s in range(nrun * ng):
                r, grp = divmod(s, ng)
                for j in range(4):
                    for q in range(4):
                        kk = 16 * grp + 4 * q + j
                        if kk >= tpr * CK:
                            continue
                        tap, c = r * tpr + kk // CK, ch * CK + kk % CK
                        wv = w[n0:n1, c].reshape(n1 - n0, -1)[:, tap].view(1, -1, 1, 1, 1)
                        acc[s % NS] = _fma(tap_view(tap)[:, c:c + 1], wv, acc[s % NS])
        out[:, n0:n1] = (acc[0] + acc[1]) + (acc[2] + acc[3]) if NS == 4 else acc[0] + acc[1]
    return out


def _ax_wgrad_kernel_order(x, gz, k):
    """conv3d_axial_wgrad_kernel and its reduce kernel in plain torch -> dw [CC][CF][*k].  A workgroup adds the voxels of its
    tiles (planar: 16 rows h x 16 columns w of a plane; axial: 8 planes d x 16 columns (h, w)) into ONE fp32 chain per output,
    one fmaf per voxel, in the order position-along-the-line outside (w; d), line inside (h; column); the tiles are dealt to
    min(1024 / block pairs, tiles) chunks; the reduce kernel's wave q adds the chunks q, q + 4, ... and the four sums are added
    as ((0 + 1) + 2) + 3."""
    B, CF, D, H, W = x.shape
    CC = gz.shape[1]
    kd, kh, kw = k
    planar = kd == 1
    xp = F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2, kd // 2, kd // 2))
    cdiv = lambda a, b: -(-a // b)                                        # noqa: E731
    if planar:
        nA, nB = cdiv(H, 16), cdiv(W, 16)
        ntiles = B * D * nA * nB
    else:
        nA, nB = cdiv(D, 8), cdiv(H * W, 16)
        ntiles = B * nA * nB
    nchunks = min(max(1024 // (cdiv(CF, 32) * cdiv(CC, 32)), 1), ntiles)
    parts = []
    for chunk in range(nchunks):
        acc = torch.zeros(CC, CF, kd * kh * kw)
        for t in range(ntiles * chunk // nchunks, ntiles * (chunk + 1) // nchunks):
            tb, ta, bd = t % nB, (t // nB) % nA, t // (nB * nA)
            for v in range(16 if planar else 8):
                for line in range(16):
                    if planar:
                        b, d, h, w_ = bd // D, bd % D, 16 * ta + line, 16 * tb + v
                        ok = h < H and w_ < W
                    else:
                        b, d, p = bd, 8 * ta + v, 16 * tb + line
                        ok = d < D and p < H * W
                        h, w_ = divmod(p, W)
                    if ok:
                        win = xp[b, :, d:d + kd, h:h + kh, w_:w_ + kw].reshape(1, CF, -1)
                        acc = _fma(win, gz[b, :, d, h, w_].view(CC, 1, 1), acc)
        parts.append(acc)
    waves = []
    for q in range(4):
        s_ = torch.zeros_like(parts[0])
        for c in range(q, nchunks, 4):
            s_ = s_ + parts[c]
        waves.append(s_)
    return (((waves[0] + waves[1]) + waves[2]) + waves[3]).view(CC, CF, kd, kh, kw)


def _ax_chain(tag, tensors):
    x, w, gz = _ax_inputs(tag)
    chain = {}
    if "z" in tensors:
        chain["z"] = _ax_kernel_order(x, w)
    if "gx" in tensors:
        chain["gx"] = _ax_kernel_order(gz, w.transpose(0, 1).flip(2, 3, 4))
    if "gw" in tensors:
        chain["gw"] = _ax_wgrad_kernel_order(x, gz, tuple(w.shape[2:]))
    return chain


@pytest.mark.parametrize("name", [n for n, _ in _listed("test_axial[")])
def test_the_kernels_order_of_additions_is_past_the_factor_axial(name):
    """The reason behind the axial rows of PAST_THE_FACTOR, kernel-free: plain fp32 torch in the forward kernel's order of
    additions (_ax_kernel_order; the data gradient is the same kernel on flipped, transposed weights; _ax_wgrad_kernel_order)
    lands where the kernel lands."""
    tag = re.search(r"\[(?:hip-|emu-)?(\w+)\]", name).group(1)
    tensors = dict(_listed(name)[0][1])
    _demonstrated(_ax_chain(tag, tensors), _ax_ref(tag), f"axial[{tag}]", tensors, lambda t: VALUE_FACTOR if t == "z" else GRAD_FACTOR)


# ================================================================================================ the rule itself: near misses
def _refused(near_miss, ref, what, factor, tag):
    """The near miss is refused by the very `within` call, with the very recorded d_ref, that the kernels of `what` pass."""
    want, live = _wd(ref)
    with pytest.raises(AssertionError, match=tag):
        within(near_miss.detach().reshape(want.shape), want, _dref(what, live), factor, tag)


AX_MISS = "ax_b2_p9_c16_o48_k11"


def test_the_rule_refuses_forward_taps_in_the_data_gradient():
    x, w, gz = _ax_inputs(AX_MISS)
    _refused(_ax_conv(gz, w.transpose(0, 1)), _ax_ref(AX_MISS)["gx"], f"axial[{AX_MISS}]:gx", GRAD_FACTOR, "taps not flipped")


def test_the_rule_refuses_a_padding_one_short():
    x, w, gz = _ax_inputs(AX_MISS)
    pad = w.shape[2] // 2
    z = F.conv3d(F.pad(x, (0, 0, 0, 0, pad - 1, pad + 1)), w)
    _refused(z, _ax_ref(AX_MISS)["z"], f"axial[{AX_MISS}]:z", VALUE_FACTOR, "padding kd // 2 - 1")


def test_the_rule_refuses_a_bf16_rounded_weight():
    x, w, gz = _ax_inputs(AX_MISS)
    _refused(_ax_conv(x, w.bfloat16().float()), _ax_ref(AX_MISS)["z"], f"axial[{AX_MISS}]:z", VALUE_FACTOR, "bf16 weight")


def test_the_rule_refuses_statistics_of_the_activated_output():
    x, w, gz = _ax_inputs(AX_MISS)
    z = F.relu(_ax_conv(x, w))
    _refused(z.sum((0, 2, 3, 4)), _ax_ref(AX_MISS)["sum"], f"axial[{AX_MISS}]:sum", VALUE_FACTOR, "sum of the activated")
    _refused((z * z).sum((0, 2, 3, 4)), _ax_ref(AX_MISS)["sumsq"], f"axial[{AX_MISS}]:sumsq", VALUE_FACTOR, "sumsq of the activated")


def test_the_rule_refuses_relu_before_the_residual():
    tag = "ax_o12"
    x, w, sc, bs, res = _epi_inputs(tag)
    y = F.relu(_ax_conv(x, w) * sc.view(1, -1, 1, 1, 1) + bs.view(1, -1, 1, 1, 1)) + res
    _refused(y, _epi_ref(tag)["a1_all"], f"axial_epilogue[{tag}]:a1_all", VALUE_FACTOR, "ReLU before the residual")


def test_the_rule_refuses_a_leaky_slope_of_a_tenth():
    tag = "ax_o12"
    x, w, sc, bs, res = _epi_inputs(tag)
    y = _epi_act(_epi_pre(_ax_conv(x, w), sc, bs, res, (1, 1, 1)), 3, slope=0.1)
    _refused(y, _epi_ref(tag)["a3_all"], f"axial_epilogue[{tag}]:a3_all", VALUE_FACTOR, "slope 0.1")


DA_MISSES = {"unbiased": "l17_c32_f32", "tanh_gelu": "l17_c32_f32", "over_hd": "l17_c32_f32", "pe_every_layer": "l17_c32_f32",
             "pre_norm": "l17_c32_f32", "query_softmax": "l17_c32_f32"}


@pytest.mark.parametrize("miss", list(DA_MISSES))
def test_the_rule_refuses_a_subtly_different_layer(miss):
    """tests/restated.py::DISP_ENCODER_MISSES, each in fp32: y and gx are refused by the rows the kernels pass."""
    tag = DA_MISSES[miss]
    near, ref = _da_ref(tag, miss=miss), _da_ref(tag)
    _refused(near["y"][1], ref["y"], f"disp_attention[{tag}]:y", VALUE_FACTOR, miss)
    _refused(near["gx"][1], ref["gx"], f"disp_attention[{tag}]:gx", GRAD_FACTOR, miss)


def test_the_rule_refuses_the_masks_of_site_1_at_site_2():
    tag, p, seed = DROP_CASES["p01"]
    near, ref = _da_ref(tag, drop=(p, seed), miss="site1_at_site2"), _da_ref(tag, drop=(p, seed))
    _refused(near["y"][1], ref["y"], "disp_attention_dropout[p01]:y", VALUE_FACTOR, "site 1 at site 2")
    _refused(near["gx"][1], ref["gx"], "disp_attention_dropout[p01]:gx", GRAD_FACTOR, "site 1 at site 2")


def test_listed_share():
    """At most LISTED_SHARE of the module's (case, tensor) pairs -- the entries of the recorded d_ref table -- are listed, per
    backend."""
    if _dref.record:
        return
    pairs = len(_dref.table())
    for backend in ("emu", "hip"):
        other = "hip" if backend == "emu" else "emu"
        listed = sum(len(r.split(", ")) for name, r in PAST_THE_FACTOR.items() if f"[{other}-" not in name)
        assert listed <= LISTED_SHARE * pairs, (backend, listed, pairs)
