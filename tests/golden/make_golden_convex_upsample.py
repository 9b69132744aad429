"""Golden fixtures for convex upsampling from logits and the sequence loss (tests/test_convex_upsample.py).

  python tests/golden/make_golden_convex_upsample.py <the reference's stereo_toolbox directory>

The reference's OWN code is executed, in fp32 and in fp64, on the seeded inputs of tests/golden/convex_upsample_config.py:
  * RAFT layout: `convex_upflow` of models/StereoAnywhere/utils/utils.py:97-110 (a free function; the file is loaded under a
    stand-in package with a stub `kornia.filters`, as make_golden_stereoanywhere.py does).  For the cases with the scale factor
    `RAFT.upsample_disp` of models/SelectiveStereo/SelectiveRAFT/raft.py:72-84 is called unbound on a namespace that carries
    `args.n_downsample` and must give the same bits.  `RAFTStereo.upsample_flow` and `DEFOMStereo.upsample_flow` are the same
    lines, but their modules do not import where this generator was run (their packages need `opt_einsum`), so they are not called.
  * pixel layout: `context_upsample(disp * 4., F.softmax(logits, 1))`, the two lines of models/IGEVStereo/igev_stereo.py:158-166,
    with `context_upsample` from models/IGEVStereo/submodule.py:243-255.
  * sequence loss: `Trainer._train_iteration` of trainer/trainer_torchrun.py:264-303 itself, called unbound on a namespace, with a
    stub model that returns leaf tensors (the initial disparity and 22 predictions) and a stub optimizer; the gradients are what its
    `loss.backward()` leaves on the leaves.
Stored per tensor: `:f32`, `:f64` and d_ref = max|fp32 - fp64| (`:dref`).  Data only.
  -> tests/golden/convex_upsample.npz (RAFT layout), convex_upsample_pixel.npz, sequence_loss.npz
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.convex_upsample_config import (CASES, LOSS_MAXDISP, LOSS_PREDICTIONS, PIXEL_CASES, PIXEL_SCALE, inputs,  # noqa: E402
                                                 loss_inputs, pixel_inputs)


def reference(ref):
    kornia, filters = types.ModuleType("kornia"), types.ModuleType("kornia.filters")
    filters.spatial_gradient = None
    kornia.filters = filters
    sys.modules.setdefault("kornia", kornia)
    sys.modules.setdefault("kornia.filters", filters)
    for name, path in (("sa_ref", "models/StereoAnywhere"), ("sa_ref.utils", "models/StereoAnywhere/utils"),
                       ("sel_ref", "models/SelectiveStereo/SelectiveRAFT"), ("igev_ref", "models/IGEVStereo")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(ref, path)]
        sys.modules[name] = pkg
    spec = importlib.util.spec_from_file_location("trainer_ref", os.path.join(ref, "trainer", "trainer_torchrun.py"))
    trainer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trainer)
    return (importlib.import_module("sa_ref.utils.utils").convex_upflow, importlib.import_module("sel_ref.raft").RAFT.upsample_disp,
            importlib.import_module("igev_ref.submodule").context_upsample, trainer.Trainer)


def run_raft(convex_upflow, upsample_disp, tag, dtype):
    N, D, H, W, n, use_scale, _ = CASES[tag]
    flow, mask, gw = inputs(tag)
    flow, mask = flow.to(dtype).requires_grad_(), mask.to(dtype).requires_grad_()
    out = convex_upflow(flow, mask, n_downsample=n, use_scale_factor=use_scale)
    if use_scale:
        holder = types.SimpleNamespace(args=types.SimpleNamespace(n_downsample=n))
        assert torch.equal(upsample_disp(holder, flow, mask), out)
    (out * gw.to(dtype)).sum().backward()
    return {"out": out, "g_flow": flow.grad, "g_mask": mask.grad}


def run_pixel(context_upsample, tag, dtype):
    disp, logits, gw = pixel_inputs(tag)
    disp, logits = disp.to(dtype).requires_grad_(), logits.to(dtype).requires_grad_()
    out = context_upsample(disp * PIXEL_SCALE, F.softmax(logits, 1))
    (out * gw.to(dtype)).sum().backward()
    return {"out": out, "g_disp": disp.grad, "g_logits": logits.grad}


def run_trainer(Trainer, dtype):
    gt, preds = loss_inputs(LOSS_PREDICTIONS + 1)
    leaves = [p.to(dtype).requires_grad_() for p in preds]
    trainer = types.SimpleNamespace(device=torch.device("cpu"), max_disp=LOSS_MAXDISP,
                                    config=types.SimpleNamespace(amp=False, clip_grad=None))
    optimizer = types.SimpleNamespace(zero_grad=lambda: None, step=lambda: None)
    data = {"left": torch.zeros(1), "right": torch.zeros(1), "gt_disp": gt.to(dtype).unsqueeze(1)}
    loss = Trainer._train_iteration(trainer, lambda left, right: (leaves[0], leaves[1:]), data, optimizer, None, None)
    return {"loss": torch.tensor(loss, dtype=dtype), "grads": torch.stack([p.grad for p in leaves])}


def main():
    convex_upflow, upsample_disp, context_upsample, Trainer = reference(sys.argv[1])
    files = {
        "convex_upsample.npz": [(t, lambda dt, t=t: run_raft(convex_upflow, upsample_disp, t, dt)) for t in CASES],
        "convex_upsample_pixel.npz": [(t, lambda dt, t=t: run_pixel(context_upsample, t, dt)) for t in PIXEL_CASES],
        "sequence_loss.npz": [("trainer", lambda dt: run_trainer(Trainer, dt))],
    }
    for name, jobs in files.items():
        store = {}
        for tag, fn in jobs:
            r32, r64 = fn(torch.float32), fn(torch.float64)
            for k in r32:
                a, b = r32[k].detach(), r64[k].detach()
                assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, (tag, k, a.dtype, b.dtype)
                assert torch.isfinite(b).all(), (tag, k)
                dref = (a.double() - b).abs().max().item()
                store[f"{tag}:{k}:dref"] = np.float64(dref)
                store[f"{tag}:{k}:f32"] = a.numpy()
                store[f"{tag}:{k}:f64"] = b.numpy()
                print(f"{tag:20s} {k:9s} {tuple(a.shape)}  max|ref| {b.abs().max().item():.4g}  d_ref {dref:.3e}", flush=True)
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
