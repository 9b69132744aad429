"""the evaluation-path input step on the device (pad_to_2x + ToTensor + Normalize in one kernel)
and the IGEV-family initial volume (8 groups of 12 channels at D' = max_disp / 4, softmax + regression at 1/4 resolution).

* oracle vs the reference's own outputs (tests/golden/igev_preprocess.npz, made by tests/golden/make_golden_igev.py);
* kernels / product functions vs the oracle, on the host emulator (CPU) and on the GPU (`-m gpu`), bit-exact for the
  byte / copy work and within fp32 rounding for the correlation."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from stereo_toolbox_amd.utils import synthetic_tensor
from tests.backends import be, ptr  # noqa: F401
from tests.golden.make_golden_igev import IMG_SHAPES, synthetic_image
from tests.parity import Env

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igev_preprocess.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def test_oracle_matches_reference_fixture():
    g = np.load(GOLD)
    for tag, (H, W) in IMG_SHAPES.items():
        left, right = synthetic_image(H, W, 51), synthetic_image(H, W, 52)
        disp = synthetic_tensor((H, W), 53, lo=0.0, hi=100.0)
        mask = synthetic_tensor((H, W), 54, lo=0.0, hi=1.0) > 0.4
        l, r, d, m = O.pad_to_2x(left, right, disp, mask)
        assert np.array_equal(l.numpy(), g[f"{tag}_left"]) and np.array_equal(r.numpy(), g[f"{tag}_right"])
        assert np.array_equal(d.numpy(), g[f"{tag}_disp"]) and np.array_equal(m.numpy(), g[f"{tag}_mask"])
        assert l.shape[0] % 96 == 0 and l.shape[1] % 96 == 0
    dist = synthetic_tensor((5, 37, 125), 55, lo=0.0, hi=1.0)
    _, _, d3, _ = O.pad_to_2x(synthetic_image(37, 125, 51), synthetic_image(37, 125, 52), dist, None)
    assert np.array_equal(d3.numpy(), g["kitti_like_dist"])
    # IGEV initial volume and 1/4-resolution regression, forward and backward
    B, C, H4, W4, maxdisp = 1, 96, 4, 40, 64
    ml, mr = synthetic_tensor((B, C, H4, W4), 61).requires_grad_(), synthetic_tensor((B, C, H4, W4), 62).requires_grad_()
    vol = O.igev_init_volume(ml, mr, maxdisp)
    assert (vol.detach() - torch.from_numpy(g["igev_volume"])).abs().max() < 1e-6   # (12-element means: summation order)
    vol.backward(synthetic_tensor(tuple(vol.shape), 63))
    assert (ml.grad - torch.from_numpy(g["igev_grad_left"])).abs().max() < 1e-6
    assert (mr.grad - torch.from_numpy(g["igev_grad_right"])).abs().max() < 1e-6
    cost = (synthetic_tensor((B, 1, maxdisp // 4, H4, W4), 64) * 3).requires_grad_()
    disp = O.igev_init_disparity(cost, maxdisp)
    disp.backward(synthetic_tensor(tuple(disp.shape), 65))
    assert torch.equal(disp.detach(), torch.from_numpy(g["igev_init_disp"]))
    assert (cost.grad - torch.from_numpy(g["igev_init_grad"])).abs().max() < 1e-6


@pytest.mark.parametrize("shape", [(37, 125), (96, 192), (100, 7), (540, 960)])
def test_pad_normalize_kernel(be, shape):
    """stx_pad_normalize_u8 == pad_to_2x + ToTensor + Normalize, bit for bit (batch of 2 different images)."""
    H, W = shape
    if be.name == "emu" and H * W > 100000:
        pytest.skip("full-size image: GPU only")
    imgs = torch.stack([synthetic_image(H, W, 70), synthetic_image(H, W, 71)])
    Hp, Wp = -(-H // 96) * 96, -(-W // 96) * 96
    out = be.empty(2, 3, Hp, Wp)
    import ctypes
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    be.call("stx_pad_normalize_u8", ptr(be.dev(imgs)), ptr(out), 2, H, W, Hp, Wp, Hp - H, m, s)
    for b in range(2):
        want = O.prepare_view(imgs[b])
        assert want.shape == (3, Hp, Wp)
        assert torch.equal(out[b].cpu(), want), (out[b].cpu() - want).abs().max()


@pytest.mark.gpu
def test_prepare_pair_and_unpad_gpu():
    """The product API on the device: normalised padded views, padded ground truth, crop back."""
    from stereo_toolbox_amd.preprocess import pad_to_2x, prepare_pair, unpad
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda:0")
    H, W = 375, 1242
    left, right = synthetic_image(H, W, 80), synthetic_image(H, W, 81)
    disp = synthetic_tensor((H, W), 82, lo=0.0, hi=190.0)
    mask = (synthetic_tensor((H, W), 83, lo=0.0, hi=1.0) > 0.3).float()
    out = prepare_pair(left.to(dev), right.to(dev), disp.to(dev), mask.to(dev))
    assert out["left"].shape == (1, 3, 384, 1248) and out["pad"] == (9, 6)
    assert torch.equal(out["left"][0].cpu(), O.prepare_view(left)) and torch.equal(out["right"][0].cpu(), O.prepare_view(right))
    _, _, d, m = O.pad_to_2x(left, right, disp, mask)
    assert torch.equal(out["gt_disp"].cpu(), d) and torch.equal(out["noc_mask"].cpu(), m)
    assert torch.equal(unpad(out["gt_disp"], H, W).cpu(), disp)
    l2, r2, d2, m2 = pad_to_2x(left.to(dev), right.to(dev), disp.to(dev), mask.to(dev))
    lo, ro, _, _ = O.pad_to_2x(left, right, disp, mask)
    assert torch.equal(l2.cpu(), lo) and torch.equal(r2.cpu(), ro) and torch.equal(d2.cpu(), d) and torch.equal(m2.cpu(), m)


@pytest.mark.parametrize("envname", ["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def test_igev_initial_volume_api(envname):
    """models.IGEVStereo: build_gwc_volume at 8 groups x 12 channels (igev_stereo.py:206) and the 1/4-resolution
    softmax + disparity_regression (igev_stereo.py:211-212), forward and backward, vs the oracle."""
    from stereo_toolbox_amd.models.IGEVStereo import init_disparity, init_gwc_volume
    env = Env(envname)
    B, C, H4, W4, maxdisp = (1, 96, 3, 40, 64) if envname == "emu" else (2, 96, 80, 184, 192)
    ml, mr = synthetic_tensor((B, C, H4, W4), 61), synthetic_tensor((B, C, H4, W4), 62)
    gv = synthetic_tensor((B, 8, maxdisp // 4, H4, W4), 63)
    a, b_ = ml.clone().to(env.device).requires_grad_(), mr.clone().to(env.device).requires_grad_()
    with env.ctx():
        vol = init_gwc_volume(a, b_, maxdisp)
        vol.backward(gv.to(env.device))
    ra, rb = ml.clone().requires_grad_(), mr.clone().requires_grad_()
    ref = O.igev_init_volume(ra, rb, maxdisp)
    ref.backward(gv)
    assert vol.shape == ref.shape == (B, 8, maxdisp // 4, H4, W4)
    assert (vol.detach().cpu() - ref.detach()).abs().max().item() < 1e-6
    assert (a.grad.cpu() - ra.grad).abs().max().item() < 2e-5 and (b_.grad.cpu() - rb.grad).abs().max().item() < 2e-5
    cost = synthetic_tensor((B, 1, maxdisp // 4, H4, W4), 64) * 3
    gd = synthetic_tensor((B, 1, H4, W4), 65)
    c = cost.clone().to(env.device).requires_grad_()
    with env.ctx():
        disp = init_disparity(c, maxdisp)
        disp.backward(gd.to(env.device))
    rc = cost.clone().requires_grad_()
    rd = O.igev_init_disparity(rc, maxdisp)
    rd.backward(gd)
    assert disp.shape == rd.shape == (B, 1, H4, W4)
    assert (disp.detach().cpu() - rd.detach()).abs().max().item() < 1e-4
    assert (c.grad.cpu() - rc.grad).abs().max().item() < 1e-5
