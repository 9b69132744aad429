"""Test backends: the same kernel-level parity tests run
  * on the host SIMT emulator build of the kernel sources (CPU tensors, `-m "not gpu"`), and
  * on the gfx950 library through the C-ABI with ROCm tensors (`-m gpu`).
Both are compared against the CPU oracle (oracle/torch_oracle.py or plain torch fp32 ops).
"""
import ctypes

import pytest
import torch

BAND_MIN = 4096                 # floats: the least length of a guard band of Backend.banded
SENTINEL_BITS = 0x5EA1BA9D      # a finite float (5.8e18): the guard bands of a buffer a kernel writes
NAN_BITS = 0x7FC00000           # the guard bands of a buffer a kernel reads


class Backend:
    def __init__(self, name):
        self.name = name
        if name == "emu":
            from tests.emu_util import emu_lib
            self.lib = emu_lib()
            self.device = torch.device("cpu")
        else:
            from stereo_toolbox_amd._capi import get_lib
            if not torch.cuda.is_available():
                pytest.skip("no ROCm device")
            self.lib = get_lib()
            self.device = torch.device("cuda:0")

    @property
    def stream(self):
        if self.name == "emu":
            return None
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dev(self, t):
        return None if t is None else t.to(self.device).contiguous()

    def empty(self, *shape, dtype=torch.float32, fill=float("nan")):
        t = torch.empty(*shape, dtype=dtype, device=self.device)
        if dtype.is_floating_point:
            t.fill_(fill)
        else:
            t.zero_()
        return t

    def banded(self, *shape, fill=float("nan"), nan_bands=False):
        """(view, check): a dense fp32 view of `shape`, filled with `fill`, cut from the middle of ONE larger allocation, and a
        `check(what)` asserting that the guard band in front of it and the one behind it still hold their bit pattern -- an
        out-of-bounds WRITE of the kernel under test lands there, not in allocator padding or a neighbouring tensor.  Both bands
        are multiples of 128 floats (the view keeps the allocation's 512-byte alignment, which every product tensor has), at least
        one row of the view (its last two extents; none for a 1-D workspace) and at least 4096 floats long.  The bands hold a finite sentinel
        (buffers a kernel writes) or, with `nan_bands`, NaN (buffers it reads: a READ past either end that reaches an output
        poisons it).  Only memory of this allocation is ever inspected."""
        n = 1
        for s in shape:
            n *= int(s)
        row = int(shape[-1]) * int(shape[-2]) if len(shape) > 1 else 0         # a 1-D buffer has no rows: the least band
        band = (max(row, BAND_MIN) + 127) // 128 * 128
        pattern = NAN_BITS if nan_bands else SENTINEL_BITS
        raw = torch.empty(2 * band + n, dtype=torch.float32, device=self.device)
        bits = raw.view(torch.int32)
        bits[:band].fill_(pattern)
        bits[band + n:].fill_(pattern)
        view = raw[band:band + n].view(*shape)
        view.fill_(fill)
        assert view.is_contiguous() and view.data_ptr() == raw.data_ptr() + 4 * band

        def check(what=""):
            for side, got in (("in front of", bits[:band]), ("behind", bits[band + n:])):
                bad = (got != pattern).nonzero().flatten().cpu()
                assert bad.numel() == 0, (f"{what}: {bad.numel()} floats of the guard band {side} the buffer {tuple(shape)} were "
                                          f"overwritten, the first at band offset {int(bad[0])} of {band}")
        return view, check

    def call(self, name, *args):
        """Tensors may be passed directly; they stay referenced for the duration of the call."""
        conv = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        self.lib.call(name, *conv, self.stream)

    def raw(self, name):
        return self.lib.raw(name)


class Guards:
    """The banded buffers of one test: `out` for what a kernel writes, `inp` for what it reads; `check` after every call."""

    def __init__(self, be):
        self.be, self.checks = be, []

    def out(self, *shape):
        v, chk = self.be.banded(*shape, fill=float("nan"))
        self.checks.append(chk)
        return v

    def inp(self, t):
        if t is None:
            return None
        t = t.detach()
        v, chk = self.be.banded(*t.shape, fill=0.0, nan_bands=True)
        v.copy_(t)
        self.checks.append(chk)
        return v

    def check(self, what):
        for chk in self.checks:
            chk(what)


def ptr(t):
    """Identity marker for pointer arguments: Backend.call converts tensors to device pointers."""
    return t


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def pack(be, w, mode):
    """w [A][B][T] in the MFMA operand order of stx_conv3d_pack_weight (the modes: include/stx_hip.h)."""
    A, Bd = w.shape[0], w.shape[1]
    T = w[0, 0].numel()
    K, N = (Bd, A) if mode == 0 else (A, Bd)
    n = be.raw("stx_conv3d_packed_floats")(K, N, T)
    wp = be.empty(n)
    be.call("stx_conv3d_pack_weight", ptr(be.dev(w)), ptr(wp), A, Bd, T, mode)
    return wp


BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    return Backend(request.param)


@pytest.fixture
def tune(be):
    """Set a tuning / A-B switch of the library under test for the duration of a test (stx_set_tuning; the library reads
    its STX_* environment variables only once, when it is loaded)."""
    saved = {}

    def set_(name, value):
        old = be.lib.set_tuning(name, value)
        saved.setdefault(name, old)
    yield set_
    for name, old in saved.items():
        be.lib.set_tuning(name, old)
