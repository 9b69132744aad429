"""Golden vectors of FoundationStereo's axial-planar convolution block, generated from the reference's own class:
/root/reference/stereo_toolbox/models/FoundationStereo/submodule.py:89-114 `Conv3dNormActReduced`.

  python tests/golden/make_golden_apc.py         (build container only: needs /root/reference; seconds)

The reference module imports packages this image lacks (flash_attn etc.) for OTHER classes of the file; empty placeholder
modules are registered under those names, as in make_golden_foundation.py -- nothing of them is called.

Per case of apc_config.CASES the block runs on CPU in fp32 and in fp64, in train(): y, loss = (y * g).sum(), backward.  Stored
as `tag/key:f64` (the fp64 run) and `tag/key:dref` (max|fp32 - fp64|): y, the input gradient `gx`, every parameter gradient
`grad/<name>`, both BatchNorms' running statistics after the step `state/<name>`, and `y_eval`, an eval() forward of a freshly
filled block (the filled running statistics).  `tag/seeds` records the seeds used.

Condition on the fixture (asserted here, next seed pair on failure; not a tolerance): every fp64 pre-activation of both ReLUs of
the train run is farther from zero than 8 x that tensor's own dref -- a product within the tests' 2 x bound then cannot flip a
ReLU, i.e. change a gradient discontinuously (the eval run stores values only, which are continuous across a flip).  The state-dict keys / shapes / order of the reference class go to state_dict_keys_apc.json.
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/stereo_toolbox/models")


class _Placeholder(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Placeholder(self.__name__ + "." + name)


for _name in ("flash_attn", "torchvision", "imageio", "cv2", "transformations"):
    try:
        __import__(_name)
    except ModuleNotFoundError:
        _m = _Placeholder(_name)
        _m.__path__ = []
        sys.modules[_name] = _m

from FoundationStereo.submodule import Conv3dNormActReduced  # noqa: E402

from stereo_toolbox_amd.utils import fill_state_dict  # noqa: E402
from tests.golden.apc_config import CASES, PART_BYTES, PARTS, SEED_G, SEED_X, block_args, inputs  # noqa: E402

MARGIN = 8.0


def _block(tag, dtype):
    m = Conv3dNormActReduced(**block_args(tag))
    sd = m.state_dict()
    fill_state_dict(sd)
    m.load_state_dict(sd)
    return m.to(dtype)


def _run(tag, dtype, sx, sg):
    x, g = inputs(tag, sx, sg)
    x, g = x.to(dtype).requires_grad_(), g.to(dtype)
    out, pre = {}, {}
    m = _block(tag, dtype).train()
    hooks = [m.conv1[1].register_forward_hook(lambda mod, i, o: pre.__setitem__("pre1", o.detach())),
             m.conv2[1].register_forward_hook(lambda mod, i, o: pre.__setitem__("pre2", o.detach()))]
    y = m(x)
    (y * g).sum().backward()
    out["y"], out["gx"] = y.detach(), x.grad
    for n, p in m.named_parameters():
        out["grad/" + n] = p.grad
    for n, b in m.named_buffers():
        if n.endswith(("running_mean", "running_var")):
            out["state/" + n] = b.detach().clone()
    e = _block(tag, dtype).eval()
    for h in hooks:
        h.remove()
    with torch.no_grad():
        out["y_eval"] = e(x.detach())
    return out, pre


def _case(tag):
    for k in range(32):
        sx, sg = SEED_X + 2 * k, SEED_G + 2 * k
        o32, p32 = _run(tag, torch.float32, sx, sg)
        o64, p64 = _run(tag, torch.float64, sx, sg)
        margins = {}
        for n in p64:
            dref = (p32[n].double() - p64[n]).abs().max().item()
            margins[n] = p64[n].abs().min().item() / dref
        if min(margins.values()) > MARGIN:
            return o32, o64, (sx, sg), margins
        print(f"  {tag}: seeds {(sx, sg)} miss the ReLU margin ({min(margins.values()):.1f} x), next")
    raise RuntimeError(f"{tag}: no seed pair meets the ReLU margin")


def main():
    out = {}
    for tag in CASES:
        o32, o64, seeds, margins = _case(tag)
        out[f"{tag}/seeds"] = np.asarray(seeds, dtype=np.int64)
        for k in o64:
            out[f"{tag}/{k}:f64"] = o64[k].numpy()
            out[f"{tag}/{k}:dref"] = np.float64((o32[k].double() - o64[k]).abs().max().item())
        worst = {k: float(out[f"{tag}/{k}:dref"]) for k in ("y", "gx", "y_eval")}
        print(tag, "seeds", seeds, "margins", {k: round(v, 1) for k, v in margins.items()}, "dref", worst)
    # deal the keys to parts below the size limit of a committed file, in order
    parts, cur, size = [], {}, 0
    for k, v in out.items():
        nb = np.asarray(v).nbytes + 256
        if cur and size + nb > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += nb
    parts.append(cur)
    assert len(parts) <= len(PARTS), f"{len(parts)} parts needed, apc_config.PARTS lists {len(PARTS)}"
    for name in PARTS:
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            os.remove(path)
    for name, part in zip(PARTS, parts):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB, {len(part)} keys)")
    m = Conv3dNormActReduced(**block_args("short"))
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "state_dict_keys_apc.json"), "w") as f:
        json.dump({"short": keys}, f, indent=1)
    print("wrote state_dict_keys_apc.json")


if __name__ == "__main__":
    main()
