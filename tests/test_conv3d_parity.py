"""The 3-D convolution family (csrc/conv3d.hip, csrc/wgrad_march.hip, csrc/conv_c1.hip) under the fp64 parity rule, in guard bands.

The rule (tests/parity.py::within), for every call: `want64` is the operation in fp64 on the CPU from the same fp32 inputs cast
up (F.conv3d / F.conv_transpose3d and autograd through them), `d_ref` = max|fp32 CPU torch run - want64| over the same tensor
(recorded, see DREF_PATH), and the kernel may sit at most VALUE_FACTOR (forward outputs, epilogues and BN statistics included) or
GRAD_FACTOR (data and weight gradients) times d_ref away from want64.  A two-term bf16 split of the same convolution sits at
7-25 x d_ref and is refused (test_the_rule_refuses_a_two_term_bf16_split).  Every weight gradient, the classifier tail, the
march kernel with its default split accumulators and the outputs of the 1x1x1 kernels pass; the kernels that add all 27 * Cin
products of an output into one fp32 accumulator sit at 2-5 x d_ref (data gradients up to 6.6 x) by the order of their additions
alone (test_one_fp32_chain_is_past_the_factor: so does a plain torch loop) and are kept as strict expected failures
(SUMMATION_ORDER), tensor by tensor: only a listed tensor may be past the factor and only at its recorded ratio; a NaN, a touched
guard band, another tensor past the factor or a listed one at another ratio fails the test (Verdict).

Guard bands (tests/backends.py::Backend.banded): every buffer a kernel WRITES (out, stats, dw, dz, gx, workspace, packed weights)
is cut from the middle of a larger allocation whose bands are checked after the call, and is sized by exactly the count its query
function returns; every buffer a kernel READS sits between NaN bands, so that a read past either end that reaches an output fails
the parity assertion (reads the buffer descriptors range-check to zero stay legitimate).

The shapes are the smallest ragged ones at which stx_conv3d_fwd's conv_plan / the weight-gradient dispatch pick each kernel; the
comment of every row names the kernel and the epilogue it reaches.  Both backends through the C-ABI: host emulator and gfx950.
"""
import contextlib
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests.backends import Backend, Guards, be, ndhwc, ncdhw, tune  # noqa: F401
from tests.parity import GRAD_FACTOR, VALUE_FACTOR, PastTheFactor, RecordedDref, Verdict, listed_verdict, within

NAN = float("nan")

# d_ref of every tensor below, RECORDED from the fp32 CPU torch run on one thread (tests/golden/conv3d_parity_dref.json, keyed by the
# parity-report name without the backend; why it is recorded and how the live value guards the record: tests/parity.py::RecordedDref).
# STX_CONV3D_DREF_RECORD=<path> runs the module with the live values and writes them to <path> (a new or changed case).
DREF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3d_parity_dref.json")
_dref = RecordedDref(DREF_PATH, "STX_CONV3D_DREF_RECORD")


@pytest.fixture
def verdict(request, parity_log):
    """The tensors of a call are named by the suffix of `what`: sum, sumsq, dz, dw; none: "out" (tests/parity.py::Verdict)."""
    reason = SUMMATION_ORDER.get(re.sub(r"\[(emu|hip)-", "[", request.node.name))
    return listed_verdict(request, parity_log, reason, "summation order only, x d_ref: ", dref=_dref)


# Cases the rule refuses although nothing but the order of the fp32 additions separates the kernel from the reference: test name
# (without the backend: the gfx950 library and the emulator's fmaf chains agree to the bit at every one of these shapes) -> the
# tensors past the factor with their measured ratios.  Each of these kernels adds the 27 * Cin products of an output into ONE fp32
# accumulator in one chain (the MFMA accumulator of the implicit-GEMM, pipelined and transposed kernels; the march kernel with
# STX_MARCH_BS=0), or sums statistics of such outputs; the CPU reference blocks its sums, so its d_ref is that of shorter chains.
# test_one_fp32_chain_is_past_the_factor shows the same without a kernel, per family: a plain fp32 loop in torch over
# (tap, channel) lands at 3.0 / 2.4 / 5.5 x d_ref for the 32 / 64 / 128-channel forward shapes, at 4.7 x (factor 3) for the 64 -> 64
# data gradient and at 2.3 x for the transposed 32 -> 32 shape; the march kernel with one accumulator per input plane
# (STX_MARCH_BS=1, three chains of 9 * 32) passes at the same shapes with the same epilogues.  No approximate intrinsic, ragged
# edge or slice order is involved: the epilogues that fail here pass behind the split accumulators.
#   * stride-1 and stride-2 forward, data gradients: within a family the ratios grow with the chain (864 -> 3456 products, 2.3 ->
#     4.8 x), not with the raggedness; the reference's d_ref barely moves (6e-6 -> 9e-6).
#   * transposed kernel: the chains are the shortest (8 taps * Cin at most: 256 .. 1024 products) and yet 32 -> 32 sits highest
#     (3.3-3.7 x, 128 -> 64: 1.9-2.1 x).  Here it is d_ref that is small, not the error that is large: the CPU reference multiplies
#     one tap at a time (a GEMM over Cin per tap) and adds the <= 8 tap planes afterwards, so at Cin = 32 its d_ref is about 1 ulp
#     of the output (6.0e-7) and any single chain of 256 roundings is a few times that (the torch loop: 2.3 x).  d_ref grows with
#     the reference's own dot products, 6.0e-7 / 1.7e-6 / 7.2e-6 at Cin 32 / 64 / 128, faster than the kernel's chain error, and the
#     ratio falls to the factor.
# The statistics of the 32 -> 1 and the 1x1x1 32 -> 24 case are 1 and 24 numbers: their d_ref is the draw of so few sums, the
# kernel's error (2 ulp of the sum of 280 outputs that are themselves at 0.8 x d_ref) is what the outputs' own rounding adds up to.
# strict: a case that starts to pass must leave this table.
SUMMATION_ORDER = {f"{fn}[{case}]": ratios for fn, rows in {
    "test_conv3d_fwd": {
        "march_32_32_ragged-bs0-epi1-none": "out 2.43, sumsq 3.64",
        "march_32_32_ragged-bs0-epi1-affine": "out 2.25",
        "march_32_32_ragged-bs0-epi1-affine_res": "out 2.21",
        "march_32_32_ragged-bs0-epi1-mish": "sumsq 3.64",
        "march_32_32_ragged-bs0-epi1-res": "out 2.47",
        "march_32_32_ragged-bs0-epi0-none": "out 2.43, sumsq 3.64",
        "march_32_32_ragged-bs0-epi0-affine": "out 2.25",
        "march_32_32_ragged-bs0-epi0-affine_res": "out 2.21",
        "march_32_32_ragged-bs0-epi0-mish": "sumsq 3.64",
        "march_32_32_ragged-bs0-epi0-res": "out 2.47",
        "march_32_1_partial-none": "sum 3.57, sumsq 2.93",
        "pgemm_128_128-none": "out 4.81, sum 2.70, sumsq 3.65",
        "pgemm_128_128-affine_res_relu": "out 4.31",
        "pgemm_128_128-leaky": "out 4.32",
        "pgemm_64_128_s2-none": "out 3.19, sumsq 4.02",
        "pgemm_64_128_s2-affine_res_relu": "out 3.48",
        "pgemm_64_128_s2-leaky": "out 3.45",
        "pgemm_64_104-none": "out 3.55, sum 2.19, sumsq 2.46",
        "pgemm_64_104-affine_res_relu": "out 2.70",
        "pgemm_64_104-leaky": "out 2.97",
        "igemm_64_64-none": "out 2.33, sum 2.41, sumsq 2.51",
        "igemm_64_64-affine_res_relu": "out 2.78",
        "igemm_64_64-leaky": "out 2.70",
        "igemm_40_32-none": "out 2.26, sumsq 2.70",
        "igemm_40_32-affine_res_relu": "out 2.22",
        "igemm_40_32-leaky": "out 2.22",
        "igemm_64_48-none": "out 3.42, sum 2.64, sumsq 2.01",
        "igemm_64_48-affine_res_relu": "out 2.32",
        "igemm_64_48-leaky": "out 2.24",
        "igemm_32_64_s2_dense-none": "out 2.39, sum 2.61, sumsq 2.69",
        "igemm_32_64_s2_padded-none": "out 2.39, sum 2.61, sumsq 2.69",
        "igemm_32_32_s2-none": "out 2.39, sumsq 2.51",
        "igemm_1x1x1_32_24-none": "sumsq 2.40",
        "igemm_64_64_wn1-none": "out 2.33, sum 2.42, sumsq 2.51",
        "igemm_64_64_wn1-affine_res_relu": "out 2.78",
        "igemm_64_64_wn2-none": "out 2.33, sum 2.41, sumsq 2.51",
        "igemm_64_64_wn2-affine_res_relu": "out 2.78",
        "igemm_64_64_wn3-none": "out 2.33, sum 2.41, sumsq 2.51",
        "igemm_64_64_wn3-affine_res_relu": "out 2.78",
        "igemm_64_64_wn4-none": "out 2.33, sum 2.41, sumsq 2.51",
        "igemm_64_64_wn4-affine_res_relu": "out 2.78",
        "pgemm_128_128_wn1-none": "out 4.81, sum 2.70, sumsq 3.65",
        "pgemm_128_128_wn1-affine_res_relu": "out 4.31",
        "pgemm_128_128_wn2-none": "out 4.81, sum 2.70, sumsq 3.65",
        "pgemm_128_128_wn2-affine_res_relu": "out 4.31",
        "pgemm_128_128_wn3-none": "out 4.81, sum 2.71, sumsq 3.59",
        "pgemm_128_128_wn3-affine_res_relu": "out 4.31",
        "pgemm_128_128_wn4-none": "out 4.81, sum 2.67, sumsq 3.84",
        "pgemm_128_128_wn4-affine_res_relu": "out 4.31",
    },
    "test_deconv3d_fwd": {
        "64_32-full-none": "out 2.65",
        "64_32-full-affine_res_relu": "out 2.26",
        "64_32-d-none": "out 2.65",
        "64_32-d-affine_res_relu": "out 2.15",
        "64_32-h-none": "out 2.65",
        "64_32-h-affine_res_relu": "out 2.34",
        "64_32-w-none": "out 2.65",
        "64_32-w-affine_res_relu": "out 2.42",
        "64_32-dhw-none": "out 2.65, sumsq 2.18",
        "64_32-dhw-affine_res_relu": "out 2.12",
        "128_64-full-affine_res_relu": "out 2.10",
        "128_64-d-affine_res_relu": "out 2.08",
        "128_64-h-affine_res_relu": "out 2.06",
        "32_32-full-none": "out 3.27, sumsq 2.46",
        "32_32-full-affine_res_relu": "out 3.73",
        "32_32-d-none": "out 3.68",
        "32_32-d-affine_res_relu": "out 3.41",
        "32_32-h-none": "out 3.68",
        "32_32-h-affine_res_relu": "out 3.13",
        "32_32-w-none": "out 3.27, sumsq 3.12",
        "32_32-w-affine_res_relu": "out 3.37",
        "32_32-dhw-none": "out 3.68",
        "32_32-dhw-affine_res_relu": "out 3.34",
    },
    "test_dgrad_via_repacked_weights": {
        "s1_64_64": "out 6.60",
        "s2_32_64_odd": "out 3.52",
        "s2_64_128_odd_w": "out 3.52",
    },
}.items() for case, ratios in rows.items()}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _cv(t):
    return t.view(1, -1, 1, 1, 1)


@contextlib.contextmanager
def _one_thread():
    """The references run on ONE thread: with more, the CPU convolution splits its sums differently from box to box (measured on
    a 64 -> 64 3x3x3 layer: d_ref 9.3e-6 on 1, 2 or 4 threads, 5.1e-6 on 16), and d_ref must not depend on the core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _pair(fn, *ts):
    """fn on the fp32 tensors cast up, and d_ref = the distance of its fp32 run from that."""
    with _one_thread():
        want = fn(*[t.double() for t in ts])
        ref = fn(*ts)
    return want, (ref.double() - want).abs().max().item()


def _grad_pair(fn, wrt, *ts):
    """Autograd gradient of fn(*ts[:-1]) against the output gradient ts[-1], w.r.t. ts[wrt]: fp64 and d_ref."""
    def grad(*a):
        a = [t.clone() for t in a]
        a[wrt].requires_grad_()
        fn(*a[:-1]).backward(a[-1])
        return a[wrt].grad
    return _pair(grad, *ts)


def _seq_sums(t):
    """Per-channel sum and sum of squares of [B][C][D][H][W], added one after the other in the tensor's own precision (no kernel
    has the pairwise order of sum())."""
    v = t.transpose(0, 1).reshape(t.shape[1], -1)
    return torch.cumsum(v, 1, dtype=t.dtype)[:, -1], torch.cumsum(v * v, 1, dtype=t.dtype)[:, -1]


def _stat_pair(raw64, raw32):
    """BN statistics: want64 = sums of the fp64 raw output; d_ref = the fp32 reference output summed sequentially in fp32."""
    (s64, q64), (s32, q32) = _seq_sums(raw64), _seq_sums(raw32)
    return (s64, (s32.double() - s64).abs().max().item()), (q64, (q32.double() - q64).abs().max().item())


def _check_stats(st, raw64, raw32, what, v):
    assert not torch.isnan(st).any(), f"{what}: {int(torch.isnan(st).any(-1).any(-1).sum())} of {st.shape[0]} statistics rows unwritten"
    (s64, ds), (q64, dq) = _stat_pair(raw64, raw32)
    rows = st.cpu().double().sum(0)
    v.within(rows[0], s64, ds, VALUE_FACTOR, what + ":sum")
    v.within(rows[1], q64, dq, VALUE_FACTOR, what + ":sumsq")


def _packed(be, G, w, mode, what):
    """stx_conv3d_pack_weight into a buffer of exactly stx_conv3d_packed_floats floats; handed on between NaN bands."""
    A, Bd, T = w.shape[0], w.shape[1], w[0, 0].numel()
    K, N = (Bd, A) if mode == 0 else (A, Bd)
    wp = G.out(be.raw("stx_conv3d_packed_floats")(K, N, T))
    be.call("stx_conv3d_pack_weight", G.inp(w.reshape(A, Bd, T)), wp, A, Bd, T, mode)
    G.check(what + ":pack")
    return G.inp(wp)


# ------------------------------------------------------------------------------------------ forward
#            name: (affine, residual, activation code, BN statistics of the raw output asked for as well)
EPILOGUES = {"none": (False, False, 0, True),
             "affine": (True, False, 0, False),
             "affine_res": (True, True, 0, False),           # (64 -> 32: the residual together with the second K slice)
             "affine_relu": (True, False, 1, False),
             "mish": (True, True, 2, True),
             "leaky": (True, False, 3, False),
             "res": (False, True, 0, False),
             "affine_res_relu": (True, True, 1, False)}
ALL7 = ("none", "affine", "affine_res", "affine_relu", "mish", "leaky", "res")
SOME = ("none", "affine_res_relu", "leaky")


def _act(v, code):
    return (v, F.relu(v), F.mish(v), F.leaky_relu(v, 0.01))[code]


@functools.lru_cache(maxsize=None)
def _fwd_inputs(shape, ks, stride, transposed, out_dims):
    B, Cin, Cout, D, H, W = shape
    g = _gen(5)
    x = _randn(g, B, Cin, D, H, W)
    if transposed:
        w = _randn(g, Cin, Cout, 3, 3, 3) * 0.1
        op = tuple(o - (2 * i - 1) for o, i in zip(out_dims, (D, H, W)))
        conv = lambda x, w: F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=op)  # noqa: E731
    else:
        w = _randn(g, Cout, Cin, ks, ks, ks) * 0.1
        conv = lambda x, w: F.conv3d(x, w, None, stride, ks // 2)  # noqa: E731
    with _one_thread():
        raw64, raw32 = conv(x.double(), w.double()), conv(x, w)
    sc, bs, res = torch.rand(Cout, generator=g) + 0.5, _randn(g, Cout), _randn(g, *raw32.shape)
    return x, w, conv, raw64, raw32, sc, bs, res


@functools.lru_cache(maxsize=None)
def _fwd_ref(shape, ks, stride, epi, transposed=False, out_dims=None):
    x, w, conv, raw64, raw32, sc, bs, res = _fwd_inputs(shape, ks, stride, transposed, out_dims)
    affine, residual, act, _ = EPILOGUES[epi]

    def f(x, w, sc, bs, res):
        v = conv(x, w)
        if affine:
            v = v * _cv(sc) + _cv(bs)
        if residual:
            v = v + res
        return _act(v, act)
    return _pair(f, x, w, sc, bs, res)


def _march_rows():
    rows = []
    for bs in (1, 0):
        for ef in (1, 0):
            t = {"STX_MARCH_BS": bs, "STX_MARCH_EPI": ef}
            # march kernel, one 32 x 32 slice, ragged H / W tiles.  STX_MARCH_EPI=1: none -> raw (4), affine / affine_relu -> plain (0),
            # affine_res / res -> residual (3), mish / leaky -> general (1);  STX_MARCH_EPI=0: the general epilogue (1) for all
            rows.append((f"march_32_32_ragged-bs{bs}-epi{ef}", (1, 32, 32, 3, 5, 37), 3, 1, t, ALL7))
            # march kernel, two K slices: the first leaves raw partial sums in `out` (4), the second adds them (2), with a residual
            # or activation code >= 2 in the general epilogue (1); two batch items, ragged
            rows.append((f"march_64_32_kslices-bs{bs}-epi{ef}", (2, 64, 32, 3, 5, 21), 3, 1, t, ALL7))
    return rows


FWD_CASES = _march_rows() + [
    # march kernel, whole 8 x 16 tiles and 32 channels: the raw whole-tile epilogue (5)
    ("march_32_32_whole", (1, 32, 32, 2, 8, 16), 3, 1, {}, SOME),
    # march kernel, two N slices of 32 channels each (the data gradient of a 64 -> 32 layer), ragged: raw (4) / residual (3) / general (1)
    ("march_32_64_nslices", (1, 32, 64, 2, 9, 33), 3, 1, {}, SOME),
    # march kernel, 24 of a slice's 32 output channels (ncout < 32: raw (4) even on whole tiles)
    ("march_32_24_partial", (1, 32, 24, 2, 9, 21), 3, 1, {}, SOME),
    # march kernel, one output channel of the slice (the classifier tail when it runs as a convolution)
    ("march_32_1_partial", (1, 32, 1, 2, 4, 35), 3, 1, {}, SOME),
    # march kernel under STX_CONV_L1_MARCH: 64 -> 64 as 2 x 2 slices, partial sums through `out` in both N slices
    ("march_64_64_l1", (1, 64, 64, 3, 5, 37), 3, 1, {"STX_CONV_L1_MARCH": 1}, SOME),
    # pipelined persistent kernel (conv_plan kind 1: four column blocks), stride 1
    ("pgemm_128_128", (1, 128, 128, 3, 4, 33), 3, 1, {}, SOME),
    # pipelined persistent kernel, stride 2, odd fine extents H / W
    ("pgemm_64_128_s2", (1, 64, 128, 4, 6, 37), 3, 2, {}, SOME),
    # pipelined persistent kernel, 104 of its 128 output channels
    ("pgemm_64_104", (1, 64, 104, 3, 4, 33), 3, 1, {}, SOME),
    # implicit GEMM <3,1>, two column blocks, two rows x one block per wave (STX_CONV_WN = 2, the default)
    ("igemm_64_64", (1, 64, 64, 3, 5, 37), 3, 1, {}, SOME),
    # implicit GEMM <3,1>, one column block, Cin = 40: five 8-channel K chunks
    ("igemm_40_32", (1, 40, 32, 2, 2, 20), 3, 1, {}, SOME),
    # implicit GEMM <3,1>, 48 of two column blocks' 64 channels
    ("igemm_64_48", (1, 64, 48, 2, 3, 20), 3, 1, {}, SOME),
    # implicit GEMM <3,2>, 32 -> 64 on the dense LDS tile (STX_CONV_S2_DENSE = 1), odd fine extents in D, H and W
    ("igemm_32_64_s2_dense", (1, 32, 64, 5, 7, 45), 3, 2, {"STX_CONV_S2_DENSE": 1}, SOME),
    # ... and on the padded LDS tile (conv_dispatch<3, 2>, two column blocks)
    ("igemm_32_64_s2_padded", (1, 32, 64, 5, 7, 45), 3, 2, {"STX_CONV_S2_DENSE": 0}, SOME),
    # implicit GEMM <3,2>, one column block (never the dense tile)
    ("igemm_32_32_s2", (1, 32, 32, 5, 7, 45), 3, 2, {}, SOME),
    # implicit GEMM <1,1>: 1x1x1 with 32-channel K chunks, two / one column block(s), 24 of a block's channels
    ("igemm_1x1x1_64_64", (1, 64, 64, 3, 4, 34), 1, 1, {}, SOME),
    ("igemm_1x1x1_32_32", (2, 32, 32, 3, 5, 37), 1, 1, {}, SOME),
    ("igemm_1x1x1_32_24", (1, 32, 24, 2, 4, 21), 1, 1, {}, SOME),
] + [
    # STX_CONV_WN: 64 channels as one row x two blocks per wave (1) or two rows x one block (2, 3, 4)
    (f"igemm_64_64_wn{wn}", (1, 64, 64, 3, 5, 37), 3, 1, {"STX_CONV_WN": wn}, ("none", "affine_res_relu")) for wn in (1, 2, 3, 4)
] + [
    # STX_CONV_WN: the pipelined kernel as one row x four blocks per wave (1, 2), 2 x 2 (3), 4 x 1 (4)
    (f"pgemm_128_128_wn{wn}", (1, 128, 128, 3, 4, 33), 3, 1, {"STX_CONV_WN": wn}, ("none", "affine_res_relu")) for wn in (1, 2, 3, 4)
]


def _run_fwd(be, G, what, x, wp, B, Cin, Cout, D, H, W, ks, stride, sc, bs, res, act, stats):
    pad = ks // 2
    Do, Ho, Wo = [(d + 2 * pad - ks) // stride + 1 for d in (D, H, W)]
    out = G.out(B, Do, Ho, Wo, Cout)
    st = None
    if stats:
        rows = be.raw("stx_conv3d_fwd_stat_rows")(B, D, H, W, Cin, Cout, ks, stride)
        assert 0 < rows <= B * be.raw("stx_conv3d_fwd_blocks")(Do, Ho, Wo), rows
        st = G.out(rows, 2, Cout)
    be.call("stx_conv3d_fwd", x, wp, out, G.inp(sc), G.inp(bs), G.inp(None if res is None else ndhwc(res)), st,
            B, D, H, W, Cin, Cout, ks, stride, act)
    G.check(what)
    return ncdhw(out).cpu(), st


FWD_PARAMS = [(c, epi) for c in FWD_CASES for epi in c[5]]


@pytest.mark.parametrize("case,epi", FWD_PARAMS, ids=[f"{c[0]}-{epi}" for c, epi in FWD_PARAMS])
def test_conv3d_fwd(be, tune, verdict, case, epi):
    name, shape, ks, stride, tunes, _ = case
    for k, v in tunes.items():
        tune(k, v)
    B, Cin, Cout, D, H, W = shape
    x, w, _, raw64, raw32, sc, bs, res = _fwd_inputs(shape, ks, stride, False, None)
    G = Guards(be)
    xl, wp = G.inp(ndhwc(x)), _packed(be, G, w, 0, name)
    affine, residual, act, stats = EPILOGUES[epi]
    what = f"conv3d_fwd[{be.name}:{name}:{epi}]"
    want, dref = _fwd_ref(shape, ks, stride, epi)
    got, st = _run_fwd(be, G, what, xl, wp, B, Cin, Cout, D, H, W, ks, stride, sc if affine else None, bs if affine else None,
                       res if residual else None, act, stats)
    verdict.within(got, want, dref, VALUE_FACTOR, what)
    if stats:
        _check_stats(st, raw64, raw32, what, verdict)
    verdict.done()


# ------------------------------------------------------------------------------------------ transposed kernel
DECONV_SHAPES = {"64_32": (1, 64, 32, 2, 3, 33),       # deconv3d_igemm_kernel<1, 8>: one column block, two W tiles (33 = 32 + 1)
                 "128_64": (2, 128, 64, 2, 4, 20),     # deconv3d_igemm_kernel<2, 8>: two column blocks, 16 K chunks, two batch items
                 "32_32": (1, 32, 32, 1, 2, 40)}       # <1, 8>, a single input plane (output depth 2, or 1 = 2 * 1 - 1)
DECONV_CUTS = {"full": (0, 0, 0), "d": (1, 0, 0), "h": (0, 1, 0), "w": (0, 0, 1), "dhw": (1, 1, 1)}    # outputs 2 * in - cut


@pytest.mark.parametrize("epi", ["none", "affine_res_relu"])
@pytest.mark.parametrize("cut", DECONV_CUTS)
@pytest.mark.parametrize("shape", DECONV_SHAPES)
def test_deconv3d_fwd(be, verdict, shape, cut, epi):
    """Outputs 2 * in and 2 * in - 1 (output_padding 1 / 0) in each of D, H, W: raw with statistics, and the fused epilogue."""
    B, Cin, Cout, D, H, W = DECONV_SHAPES[shape]
    od = tuple(2 * i - c for i, c in zip((D, H, W), DECONV_CUTS[cut]))
    x, w, _, raw64, raw32, sc, bs, res = _fwd_inputs(DECONV_SHAPES[shape], 3, 2, True, od)
    G = Guards(be)
    xl, wp = G.inp(ndhwc(x)), _packed(be, G, w, 2, shape)
    affine, residual, act, stats = EPILOGUES[epi]
    what = f"deconv3d_fwd[{be.name}:{shape}:{cut}:{epi}]"
    want, dref = _fwd_ref(DECONV_SHAPES[shape], 3, 2, epi, True, od)
    out = G.out(B, *od, Cout)
    st = G.out(B * be.raw("stx_deconv3d_fwd_blocks")(D, H, W), 2, Cout) if stats else None
    be.call("stx_deconv3d_fwd", xl, wp, out, G.inp(sc if affine else None), G.inp(bs if affine else None),
            G.inp(ndhwc(res) if residual else None), st, B, D, H, W, Cin, Cout, *od, act)
    G.check(what)
    verdict.within(ncdhw(out).cpu(), want, dref, VALUE_FACTOR, what)
    if stats:
        _check_stats(st, raw64, raw32, what, verdict)
    verdict.done()


# ------------------------------------------------------------------------------------------ data gradients
DGRAD_CASES = [
    # stride-1 conv 32 -> 64: a stride-1 convolution of gy with pack mode 1 -> the march kernel 64 -> 32 (two K slices)
    ("s1_32_64", 1, (1, 32, 64, 3, 4, 33)),
    # stride-1 conv 64 -> 64: pack mode 1 -> implicit GEMM <3, 1>, two column blocks
    ("s1_64_64", 1, (1, 64, 64, 2, 5, 21)),
    # stride-2 conv 32 -> 64 over even fine extents: transposed kernel <1, 8> on the conv weight (pack mode 2), outputs 2 * in
    ("s2_32_64_even", 2, (1, 32, 64, 4, 4, 40)),
    # ... over odd fine extents (1/32-scale KITTI: W = 39): outputs 2 * in - 1 in D, H and W
    ("s2_32_64_odd", 2, (1, 32, 64, 3, 5, 39)),
    # ... odd in W only, 64 -> 128: transposed kernel <2, 8>
    ("s2_64_128_odd_w", 2, (1, 64, 128, 2, 4, 39)),
    # transposed conv 64 -> 32: a stride-2 convolution of gy with the deconv weight in pack mode 0 -> implicit GEMM <3, 2>, dense tile
    ("deconv_64_32", 0, (1, 64, 32, 2, 2, 20)),
    # transposed conv 128 -> 64: -> pipelined kernel, stride 2
    ("deconv_128_64", 0, (1, 128, 64, 2, 3, 17)),
]


@functools.lru_cache(maxsize=None)
def _dgrad_ref(mode, shape):
    B, Cin, Cout, D, H, W = shape
    g = _gen(7)
    x = _randn(g, B, Cin, D, H, W)
    if mode == 0:
        w = _randn(g, Cin, Cout, 3, 3, 3) * 0.1
        fn = lambda x, w: F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)  # noqa: E731
    else:
        w = _randn(g, Cout, Cin, 3, 3, 3) * 0.1
        fn = lambda x, w: F.conv3d(x, w, None, mode, 1)  # noqa: E731
    gy = _randn(g, *fn(x, w).shape)
    return (w, gy) + _grad_pair(fn, 0, x, w, gy)


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_dgrad_via_repacked_weights(be, verdict, case):
    name, mode, (B, Cin, Cout, D, H, W) = case
    w, gy, want, dref = _dgrad_ref(mode, case[2])
    what = f"conv3d_dgrad[{be.name}:{name}]"
    G = Guards(be)
    gl, wp = G.inp(ndhwc(gy)), _packed(be, G, w, mode, name)
    Dg, Hg, Wg = gy.shape[2:]
    if mode == 2:
        gx = G.out(B, D, H, W, Cin)
        be.call("stx_deconv3d_fwd", gl, wp, gx, None, None, None, None, B, Dg, Hg, Wg, Cout, Cin, D, H, W, 0)
        G.check(what)
        got = ncdhw(gx).cpu()
    else:
        got, _ = _run_fwd(be, G, what, gl, wp, B, gy.shape[1], Cin, Dg, Hg, Wg, 3, 2 if mode == 0 else 1, None, None, None, 0, False)
    verdict.within(got, want, dref, GRAD_FACTOR, what)
    verdict.done()


# ------------------------------------------------------------------------------------------ weight gradients
def _run_wgrad(be, G, what, fine, coarse, ks, stride):
    B, CF, Df, Hf, Wf = fine.shape
    _, CC, Dc, Hc, Wc = coarse.shape
    ws = G.out(be.raw("stx_conv3d_wgrad_workspace_floats")(B, Dc, Hc, Wc, CF, CC, ks, stride))
    dw = G.out(CC, CF, ks ** 3)
    be.call("stx_conv3d_wgrad", G.inp(ndhwc(fine)), G.inp(ndhwc(coarse)), dw, ws, B, Df, Hf, Wf, CF, Dc, Hc, Wc, CC, ks, stride)
    G.check(what)
    return dw.cpu()


# tile kernel (STX_WGRAD_MARCH = 0): the instantiation behind WG_LAUNCH from wgrad_pipe (stride 2 or <= 2 channel-block pairs) and
# wgrad_tile (16-wide tiles where they waste fewer columns than 32-wide ones); march form (3): conv3d_wgrad_march_kernel<false> at
# stride 1, conv3d_wgrad_march_s2_kernel at stride 2, in 4 x 16 steps.          B, Cin, Cout, D, H, W, ks, stride, STX_WGRAD_GRID
WGRAD_CASES = [
    ("s1_4x16_pipe", (1, 32, 32, 3, 5, 37, 3, 1, 0)),          # one pair, W = 37: 48 < 64 columns -> <3,1,4,16,pipelined>
    ("s1_4x16_plain", (1, 64, 64, 3, 5, 37, 3, 1, 0)),         # four pairs -> <3,1,4,16,plain>
    ("s1_4x32_pipe", (1, 32, 64, 2, 3, 60, 3, 1, 0)),          # two pairs, W = 60: 64 columns either way -> <3,1,4,32,pipelined>
    ("s1_2x32_plain", (1, 64, 64, 2, 3, 60, 3, 1, 0)),         # four pairs -> <3,1,2,32,plain>
    ("s1_exact_tiles", (2, 32, 32, 4, 4, 16, 3, 1, 0)),        # whole 4 x 16 tiles, two batch items
    ("s2_even", (2, 32, 64, 4, 6, 40, 3, 2, 0)),               # <3,2,4,16,pipelined>, even fine extents, two batch items
    ("s2_odd", (1, 64, 128, 3, 7, 21, 3, 2, 0)),               # ... odd fine extents in D, H and W, eight pairs
    ("s2_odd_w", (1, 32, 32, 4, 6, 39, 3, 2, 0)),              # ... odd in W only
    ("s1_grid2", (1, 32, 32, 7, 8, 20, 3, 1, 2)),              # STX_WGRAD_GRID = 2: 14 tiles / 28 march steps on two workgroups
    ("s2_grid3", (1, 32, 64, 4, 6, 40, 3, 2, 3)),              # STX_WGRAD_GRID = 3: several tiles per workgroup, cut inside a column
]


@pytest.mark.parametrize("march", [3, 0], ids=["march", "tile_kernel"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv3d_wgrad(be, tune, verdict, case, march):
    name, (B, Cin, Cout, D, H, W, ks, s, grid) = case
    tune("STX_WGRAD_MARCH", march)
    if grid:
        tune("STX_WGRAD_GRID", grid)
    g = _gen(8)
    x, w = _randn(g, B, Cin, D, H, W), _randn(g, Cout, Cin, ks, ks, ks) * 0.1
    fn = lambda x, w: F.conv3d(x, w, None, s, ks // 2)  # noqa: E731
    gy = _randn(g, *fn(x, w).shape)
    want, dref = _grad_pair(fn, 1, x, w, gy)
    what = f"conv3d_wgrad[{be.name}:{name}:{'march' if march else 'tile'}]"
    got = _run_wgrad(be, Guards(be), what, x, gy, ks, s)
    verdict.within(got.view_as(want), want, dref, GRAD_FACTOR, what)
    verdict.done()


@pytest.mark.parametrize("shape", [(1, 64, 64, 3, 4, 34), (2, 32, 64, 2, 5, 21)])
def test_conv3d_wgrad_1x1x1(be, verdict, shape):
    """conv3d_wgrad_kernel<1,1,2,32,4 waves,plain>: four pairs, ragged 2 x 32 tiles; two pairs, two batch items."""
    B, Cin, Cout, D, H, W = shape
    g = _gen(8)
    x, w = _randn(g, B, Cin, D, H, W), _randn(g, Cout, Cin, 1, 1, 1) * 0.1
    fn = lambda x, w: F.conv3d(x, w)  # noqa: E731
    gy = _randn(g, *fn(x, w).shape)
    want, dref = _grad_pair(fn, 1, x, w, gy)
    what = f"conv3d_wgrad[{be.name}:1x1x1_{Cin}_{Cout}]"
    got = _run_wgrad(be, Guards(be), what, x, gy, 1, 1)
    verdict.within(got.view_as(want), want, dref, GRAD_FACTOR, what)
    verdict.done()


@pytest.mark.parametrize("march", [3, 0], ids=["march", "tile_kernel"])
@pytest.mark.parametrize("shape", [(1, 64, 32, 2, 3, 20), (2, 32, 32, 3, 5, 18)])
def test_deconv3d_wgrad(be, tune, verdict, march, shape):
    """Transposed conv: fine = the output gradient, coarse = the layer input (stride-2 kernels; two pairs / one, two batch items)."""
    tune("STX_WGRAD_MARCH", march)
    B, Cin, Cout, D, H, W = shape
    g = _gen(9)
    x, w = _randn(g, B, Cin, D, H, W), _randn(g, Cin, Cout, 3, 3, 3) * 0.1
    fn = lambda x, w: F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)  # noqa: E731
    gy = _randn(g, *fn(x, w).shape)
    want, dref = _grad_pair(fn, 1, x, w, gy)
    what = f"deconv3d_wgrad[{be.name}:{Cin}_{Cout}:{'march' if march else 'tile'}]"
    got = _run_wgrad(be, Guards(be), what, gy, x, 3, 2)
    verdict.within(got.view_as(want), want, dref, GRAD_FACTOR, what)
    verdict.done()


def _bn_dz(x, gy, z, scale, shift, mean, invstd, gamma, sums, inv_n, act):
    """The header's formula of stx_conv3d_wgrad_bn in the precision of its operands (channels last), and dw from it."""
    g = gy * (z * scale + shift > 0).to(gy.dtype) if act else gy
    xhat = (z - mean) * invstd
    dz = gamma * invstd * (g - sums[0] * inv_n - xhat * sums[1] * inv_n)
    w0 = torch.zeros(z.shape[-1], x.shape[-1], 3, 3, 3, dtype=x.dtype, requires_grad=True)
    F.conv3d(x.permute(0, 4, 1, 2, 3), w0, None, 1, 1).backward(dz.permute(0, 4, 1, 2, 3))
    return dz, w0.grad


# conv3d_wgrad_march_kernel<true>:      B, Cin, Cout, D, H, W, act, gamma, STX_WGRAD_GRID
WGRAD_BN_CASES = [("relu", (1, 32, 32, 3, 5, 37, 1, True, 0)),               # one pair, ragged 4 x 16 steps
                  ("relu_two_cf_blocks", (2, 64, 32, 2, 9, 21, 1, True, 3)),  # two input-channel blocks (dz written once), three workgroups
                  ("no_act", (1, 32, 64, 3, 4, 16, 0, True, 0)),              # whole tiles, two output-channel blocks
                  ("relu_no_gamma", (1, 32, 32, 2, 6, 19, 1, False, 0)),      # gamma = NULL
                  ("no_act_no_gamma", (1, 64, 64, 2, 5, 18, 0, False, 2))]    # four pairs, two workgroups


@pytest.mark.parametrize("case", WGRAD_BN_CASES, ids=[c[0] for c in WGRAD_BN_CASES])
def test_conv3d_wgrad_bn(be, tune, verdict, case):
    """dz and dw of stx_conv3d_wgrad_bn against the header's formula in fp64; `sums` come from fp64, rounded to fp32, so that only
    this kernel is under test; no z * scale + shift within 1e-4 of zero (the ReLU mask then is the same in fp32 and fp64)."""
    name, (B, Cin, Cout, D, H, W, act, has_gamma, grid) = case
    if grid:
        tune("STX_WGRAD_GRID", grid)
    g = _gen(12)
    nvox = B * D * H * W
    x, z, gy = _randn(g, B, D, H, W, Cin), _randn(g, B, D, H, W, Cout), _randn(g, B, D, H, W, Cout)
    scale = (torch.rand(Cout, generator=g) + 0.5) * (1 - 2.0 * (torch.rand(Cout, generator=g) < 0.5))
    shift = _randn(g, Cout) * 0.3
    pre = z * scale + shift
    z = torch.where(pre.abs() < 1e-2, z + 0.05 * torch.sign(pre) / scale, z)       # |scale| <= 1.5: moves `pre` away from zero by 0.05
    assert ((z.double() * scale.double() + shift.double()).abs() >= 1e-4).all() and ((z * scale + shift).abs() >= 1e-4).all()
    mean, invstd = _randn(g, Cout) * 0.2, torch.rand(Cout, generator=g) + 0.5
    gamma = torch.rand(Cout, generator=g) + 0.5 if has_gamma else torch.ones(Cout)
    inv_n = torch.tensor(1.0 / nvox, dtype=torch.float32)
    mask = ((z * scale + shift > 0) if act else torch.ones_like(z)).double()
    xhat64 = (z.double() - mean.double()) * invstd.double()
    sums = torch.stack([(gy.double() * mask).sum((0, 1, 2, 3)), (gy.double() * mask * xhat64).sum((0, 1, 2, 3))]).float()
    ops = (x, gy, z, scale, shift, mean, invstd, gamma, sums, inv_n)
    with _one_thread():
        dz64, dw64 = _bn_dz(*[t.double() for t in ops], act)
        dz32, dw32 = _bn_dz(*ops, act)
    what = f"conv3d_wgrad_bn[{be.name}:{name}]"
    assert be.raw("stx_conv3d_wgrad_bn_supported")(B, D, H, W, Cin, Cout) == 1
    G = Guards(be)
    ws = G.out(be.raw("stx_conv3d_wgrad_workspace_floats")(B, D, H, W, Cin, Cout, 3, 1))
    dz, dw = G.out(B, D, H, W, Cout), G.out(Cout, Cin, 27)
    be.call("stx_conv3d_wgrad_bn", G.inp(x), G.inp(gy), G.inp(z), G.inp(scale), G.inp(shift), G.inp(mean), G.inp(invstd),
            G.inp(gamma) if has_gamma else None, G.inp(sums), float(inv_n), act, dz, dw, ws, B, D, H, W, Cin, Cout)
    G.check(what)
    verdict.within(dz.cpu(), dz64, (dz32.double() - dz64).abs().max().item(), GRAD_FACTOR, what + ":dz")
    verdict.within(dw.cpu().view_as(dw64), dw64, (dw32.double() - dw64).abs().max().item(), GRAD_FACTOR, what + ":dw")
    verdict.done()


# ------------------------------------------------------------------------------------------ classifier tail
@pytest.mark.parametrize("op", ["fwd", "fwd_res", "wgrad", "dgrad"])
@pytest.mark.parametrize("shape", [(2, 16, 2, 5, 33), (1, 32, 3, 5, 37), (1, 64, 2, 9, 41)], ids=["16", "32", "64"])
def test_conv3d_c1(be, verdict, shape, op):
    """Conv3d(Cin, 1, 3, padding=1) on the VALU kernels of conv_c1.hip: forward without / with residual, weight and data gradient;
    ragged extents, two batch items at 16 channels."""
    B, Cin, D, H, W = shape
    g = _gen(11)
    x, w, res = _randn(g, B, Cin, D, H, W), _randn(g, 1, Cin, 3, 3, 3) * 0.1, _randn(g, B, 1, D, H, W)
    gy = _randn(g, B, 1, D, H, W)
    fn = lambda x, w: F.conv3d(x, w, None, 1, 1)  # noqa: E731
    what = f"conv3d_c1_{op}[{be.name}:{Cin}]"
    G = Guards(be)
    xl, wl, gl = G.inp(ndhwc(x)), G.inp(w.reshape(1, Cin, 27)), G.inp(gy.reshape(B, D, H, W))
    if op in ("fwd", "fwd_res"):
        want, dref = _pair(fn, x, w) if op == "fwd" else _pair(lambda x, w, r: fn(x, w) + r, x, w, res)
        got, factor = G.out(B, D, H, W), VALUE_FACTOR
        be.call("stx_conv3d_c1_fwd", xl, wl, G.inp(res.reshape(B, D, H, W)) if op == "fwd_res" else None, got, B, D, H, W, Cin)
        got = got.view(B, 1, D, H, W)
    elif op == "wgrad":
        (want, dref), factor = _grad_pair(fn, 1, x, w, gy), GRAD_FACTOR
        ws, dw = G.out(be.raw("stx_conv3d_c1_wgrad_workspace_floats")(Cin)), G.out(1, Cin, 27)
        be.call("stx_conv3d_c1_wgrad", xl, gl, dw, ws, B, D, H, W, Cin)
        got = dw.view_as(want)
    else:
        (want, dref), factor = _grad_pair(fn, 0, x, w, gy), GRAD_FACTOR
        gx = G.out(B, D, H, W, Cin)
        be.call("stx_conv3d_c1_dgrad", gl, wl, gx, B, D, H, W, Cin)
        got = ncdhw(gx)
    G.check(what)
    verdict.within(got.cpu(), want, dref, factor, what)
    verdict.done()


# ------------------------------------------------------------------------------------------ the rule and the bands themselves
def _bf16_split(t):
    hi = t.bfloat16().float()
    return hi, (t - hi).bfloat16().float()


@pytest.mark.parametrize("which", ["forward", "weight_gradient"])
def test_the_rule_refuses_a_two_term_bf16_split(which):
    """The rule has teeth: the convolution of one forward and one weight-gradient case above as x_hi w_hi + x_hi w_lo + x_lo w_hi over
    bf16 halves (torch on the CPU, no kernel) sits 7-25 x d_ref away from fp64 and is refused by the very `within` call, with the
    very d_ref, the kernels of that case pass."""
    fn = lambda x, w: F.conv3d(x, w, None, 1, 1)  # noqa: E731
    if which == "forward":
        x, w = _fwd_inputs((1, 32, 32, 3, 5, 37), 3, 1, False, None)[:2]
        (a_hi, a_lo), (b_hi, b_lo) = _bf16_split(x), _bf16_split(w)
        want, live = _pair(fn, x, w)
        what, factor = "conv3d_fwd[march_32_32_ragged-bs1-epi1:none]", VALUE_FACTOR
        with _one_thread():
            split = fn(a_hi, b_hi) + fn(a_hi, b_lo) + fn(a_lo, b_hi)
    else:
        g = _gen(8)                                                              # (the inputs of WGRAD_CASES' s1_4x16_pipe)
        x, w = _randn(g, 1, 32, 3, 5, 37), _randn(g, 32, 32, 3, 3, 3) * 0.1
        gy = _randn(g, *fn(x, w).shape)
        (a_hi, a_lo), (b_hi, b_lo) = _bf16_split(x), _bf16_split(gy)
        want, live = _grad_pair(fn, 1, x, w, gy)
        what, factor = "conv3d_wgrad[s1_4x16_pipe:march]", GRAD_FACTOR
        wg = lambda x, gy: _grad_pair(fn, 1, x, w, gy)[0].float()  # noqa: E731      (fp64 products of the halves: the split alone)
        split = wg(a_hi, b_hi) + wg(a_hi, b_lo) + wg(a_lo, b_hi)
    with pytest.raises(AssertionError, match="bf16 split"):
        within(split, want, _dref(what, live), factor, f"bf16 split, {which}")


def _one_chain(xp, w, stride, out_dims):
    """The convolution of the padded xp [B][Cin][...] with w [Cout][Cin][3][3][3], every output as ONE sequential fp32 chain over
    (tap, channel): plain torch, one rounded product added per step to an accumulator holding all outputs."""
    acc = torch.zeros(xp.shape[0], w.shape[0], *out_dims)
    span = [stride * (o - 1) + 1 for o in out_dims]
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                xs = xp[:, :, kd:kd + span[0]:stride, kh:kh + span[1]:stride, kw:kw + span[2]:stride]
                for c in range(xp.shape[1]):
                    acc += xs[:, c:c + 1] * w[:, c, kd, kh, kw].view(1, -1, 1, 1, 1)
    return acc


ONE_CHAIN = {"fwd_32_32": "conv3d_fwd[march_32_32_ragged-bs0-epi1:none]", "fwd_64_64": "conv3d_fwd[igemm_64_64:none]",
             "fwd_128_128": "conv3d_fwd[pgemm_128_128:none]", "dgrad_64_64": "conv3d_dgrad[s1_64_64]",
             "deconv_32_32": "deconv3d_fwd[32_32:full:none]"}


@pytest.mark.parametrize("which", ONE_CHAIN)
def test_one_fp32_chain_is_past_the_factor(which):
    """The reason behind every row of SUMMATION_ORDER, on the CPU and without a kernel: the same convolution in plain fp32, exact
    but for adding the 27 * Cin products of an output one after the other, is refused by the very `within` call, with the very
    d_ref, of one case per family of the table -- yet stays below the 7 x where the two-term bf16 split begins."""
    what = ONE_CHAIN[which]
    if which.startswith("fwd"):
        shape = {"fwd_32_32": (1, 32, 32, 3, 5, 37), "fwd_64_64": (1, 64, 64, 3, 5, 37), "fwd_128_128": (1, 128, 128, 3, 4, 33)}[which]
        x, w = _fwd_inputs(shape, 3, 1, False, None)[:2]
        (want, live), factor = _fwd_ref(shape, 3, 1, "none"), VALUE_FACTOR
        chain = _one_chain(F.pad(x, (1,) * 6), w, 1, x.shape[2:])
    elif which == "dgrad_64_64":                  # gx = the stride-1 convolution of gy with the weight transposed and mirrored
        w, gy, want, live = _dgrad_ref(1, (1, 64, 64, 2, 5, 21))
        chain, factor = _one_chain(F.pad(gy, (1,) * 6), w.transpose(0, 1).flip(2, 3, 4), 1, gy.shape[2:]), GRAD_FACTOR
    else:                                         # transposed: the same over the input with zeros between its voxels (0 adds exactly)
        shape, od = DECONV_SHAPES["32_32"], (2, 4, 80)
        x, w = _fwd_inputs(shape, 3, 2, True, od)[:2]
        (want, live), factor = _fwd_ref(shape, 3, 2, "none", True, od), VALUE_FACTOR
        xz = torch.zeros(*x.shape[:2], *(2 * i - 1 for i in x.shape[2:]))
        xz[:, :, ::2, ::2, ::2] = x
        chain = _one_chain(F.pad(xz, (1, 2) * 3), w.transpose(0, 1).flip(2, 3, 4), 1, od)
    dref = _dref(what, live)
    err = (chain.double() - want).abs().max().item()
    print(f"one chain, {which}: {err / dref:.2f} x d_ref")
    assert err < 7 * dref, (which, err, dref)
    with pytest.raises(AssertionError, match="one chain"):
        within(chain, want, dref, factor, f"one chain, {which}")


def test_verdict_excuses_only_a_listed_tensor_at_its_recorded_ratio():
    """The expected failure is no blanket: with `out` listed at 2.43 x d_ref, only that ends in PastTheFactor; a NaN, another
    ratio (a 25 x kernel), a listed tensor that passes, an unlisted tensor past the factor each fail as a plain AssertionError."""
    what, want, dref = "made up", torch.zeros(4, dtype=torch.float64), 1e-5

    def run(out_ratio, sumsq_ratio=1.0, nan=False):
        v = Verdict(None, {"out": 2.43}, dref=lambda what, live: live)
        got = torch.tensor([0.0, out_ratio * dref, NAN if nan else 0.0, 0.0], dtype=torch.float64)
        v.within(got, want, dref, VALUE_FACTOR, what)
        v.within(torch.full((4,), sumsq_ratio * 1e-3, dtype=torch.float64), want, 1e-3, VALUE_FACTOR, what + ":sumsq")
        v.done()

    with pytest.raises(PastTheFactor):
        run(2.43)
    for kw in (dict(out_ratio=2.43, nan=True), dict(out_ratio=25.0), dict(out_ratio=2.45), dict(out_ratio=1.5),
               dict(out_ratio=2.43, sumsq_ratio=2.5)):
        with pytest.raises(AssertionError) as e:
            run(**kw)
        assert e.type is AssertionError, (kw, e.type)
    with pytest.raises(AssertionError) as e:             # listed but never compared
        Verdict(None, {"out": 2.43}).done()
    assert e.type is AssertionError
    Verdict(None, {}).done()


def test_banded_catches_a_write_on_either_side_and_none_inside():
    be = Backend("emu")
    view, check = be.banded(3, 5, 7, fill=0.0)
    n, band = view.numel(), view.storage_offset()
    assert band % 128 == 0 and band >= 4096 and view.is_contiguous() and (view == 0).all()
    whole = torch.empty(0).set_(view.untyped_storage())
    assert whole.numel() == 2 * band + n and (whole.numel() - band - n) % 128 == 0
    check("untouched")
    view.fill_(3.0)
    view[2, 4, 6] = NAN
    check("written inside")
    for at in (band - 1, band + n):                      # one float before the view, one float after it
        old = whole[at].item()
        whole[at] = 1.0
        with pytest.raises(AssertionError, match="guard band"):
            check("one float outside")
        whole[at] = old
        check("restored")
    wide, _ = be.banded(2, 70, 64, fill=0.0)             # a row (W * C floats) longer than the least band
    assert wide.storage_offset() == 4480
    flat, _ = be.banded(10000, fill=0.0)                 # a 1-D workspace has no rows: the least band, not its own length
    assert flat.storage_offset() == 4096
    rd, check = be.banded(4, fill=1.0, nan_bands=True)
    whole = torch.empty(0).set_(rd.untyped_storage())
    assert torch.isnan(whole[:rd.storage_offset()]).all() and torch.isnan(whole[rd.storage_offset() + 4:]).all()
    check("NaN bands compare by bit pattern")
