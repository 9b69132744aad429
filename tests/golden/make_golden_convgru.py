"""Golden vectors of the ConvGRU cell, generated from the reference's own class:
/root/reference/stereo_toolbox/models/IGEVStereo/update.py:25-40 `ConvGRU` (that file imports nothing but torch).

  python tests/golden/make_golden_convgru.py         (build container only: needs /root/reference; seconds)

Per case of convgru_config.CASES the module runs on CPU in fp32 and in fp64 with loss = sum over the iterations of
(h_i * g_i).sum().  Stored as `tag/key:f64`, `tag/key:f32` and `tag/key:dref` (max|fp32 - fp64|): the last state `h` and the
gradients of h, cz, cr, cq, every x source and the six parameters.  The keys are dealt to convgru.npz (+ parts) below the size
limit of a committed file; the state-dict keys / shapes / order of the reference class go to state_dict_keys_convgru.json.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

warnings.filterwarnings("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/stereo_toolbox/models/IGEVStereo")

from update import ConvGRU  # noqa: E402

from stereo_toolbox_amd.utils import fill_state_dict  # noqa: E402
from tests.golden.convgru_config import CASES, PART_BYTES, PARTS, module_args, run_case  # noqa: E402


def _module(tag, dtype):
    m = ConvGRU(**module_args(tag))
    sd = m.state_dict()
    fill_state_dict(sd)
    m.load_state_dict(sd)
    return m.to(dtype)


def _run(tag, dtype):
    m = _module(tag, dtype)
    return run_case(lambda h, cz, cr, cq, xs: m(h, cz, cr, cq, *xs), dict(m.named_parameters()), tag, dtype)


def main():
    out = {}
    for tag in CASES:
        o32, o64 = _run(tag, torch.float32), _run(tag, torch.float64)
        for k in o64:
            out[f"{tag}/{k}:f64"] = o64[k].numpy()
            out[f"{tag}/{k}:f32"] = o32[k].numpy()
            out[f"{tag}/{k}:dref"] = np.float64((o32[k].double() - o64[k]).abs().max().item())
        print(tag, {k: f"{float(out[f'{tag}/{k}:dref']):.2e}" for k in o64})
    parts, cur, size = [], {}, 0
    for k, v in out.items():
        nb = np.asarray(v).nbytes + 256
        if cur and size + nb > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += nb
    parts.append(cur)
    assert len(parts) <= len(PARTS), f"{len(parts)} parts needed, convgru_config.PARTS lists {len(PARTS)}"
    for name in PARTS:
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            os.remove(path)
    for name, part in zip(PARTS, parts):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB, {len(part)} keys)")
    m = ConvGRU(**module_args("two_src"))
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "state_dict_keys_convgru.json"), "w") as f:
        json.dump({"two_src": keys}, f, indent=1)
    print("wrote state_dict_keys_convgru.json")


if __name__ == "__main__":
    main()
