"""Golden vectors of the SelectiveStereo stage, generated from the reference's own classes:
/root/reference/stereo_toolbox/models/SelectiveStereo/SelectiveRAFT/update.py `SelectiveConvGRU` (:61-71, on `RaftConvGRU`
:15-30), `ChannelAttentionEnhancement` (:106-121) and `SpatialAttentionExtractor` (:123-135); that file imports nothing but torch
(the SelectiveIGEV copy of the same class text needs opt_einsum).

  python tests/golden/make_golden_selective.py         (build container only: needs /root/reference; seconds)

Per case of selective_config.CELL_CASES the cell runs on CPU in fp32 and in fp64 with loss = sum over the iterations of
(h_i * g_i).sum(); per case of CSA_CASES `inp = cam(x) * x; att = sam(inp)` (SelectiveIGEV/igev_stereo.py:225-226) with loss =
(inp g1).sum() + (att g2).sum().  Stored as `tag/key:f64`, `tag/key:f32` and `tag/key:dref` (max|fp32 - fp64|): outputs and the
gradients of every input and parameter.  For every attention case, the GPU-only one included, the fp64 run must keep the margins
of selective_config.CSA_MARGINS (distance of the MLP pre-activations from 0, gaps between the two best values of every max): the
fp32 and fp64 runs, and the kernels, then take the same branches.  The keys are dealt to selective.npz (+ parts) below the size
limit of a committed file; the state-dict keys / shapes / order of the reference classes go to state_dict_keys_selective.json.
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
sys.path.insert(0, "/root/reference/stereo_toolbox/models/SelectiveStereo/SelectiveRAFT")

from update import ChannelAttentionEnhancement, SelectiveConvGRU, SpatialAttentionExtractor  # noqa: E402

from stereo_toolbox_amd.utils import fill_state_dict  # noqa: E402
from tests.golden.selective_config import (CELL_CASES, CSA_CASES, CSA_GPU_CASE, CSA_KERNEL, CSA_MARGINS, PART_BYTES, PARTS,  # noqa: E402
                                           csa_inputs, csa_margins, csa_shape, module_args, run_cell_case, run_csa_case)


def _filled(m, dtype):
    sd = m.state_dict()
    fill_state_dict(sd)
    m.load_state_dict(sd)
    return m.to(dtype)


def _run_cell(tag, dtype):
    m = _filled(SelectiveConvGRU(**module_args(tag)), dtype)
    return run_cell_case(lambda att, h, xs: m(att, h, *xs), dict(m.named_parameters()), tag, dtype)


def _csa_modules(tag, dtype):
    return _filled(ChannelAttentionEnhancement(csa_shape(tag)[1]), dtype), _filled(SpatialAttentionExtractor(CSA_KERNEL), dtype)


def _run_csa(tag, dtype):
    cam, sam = _csa_modules(tag, dtype)

    def step(x):
        inp = cam(x) * x
        return inp, sam(inp)
    params = {"cam/" + k: v for k, v in cam.named_parameters()}
    params.update({"sam/" + k: v for k, v in sam.named_parameters()})
    return run_csa_case(step, params, tag, dtype)


def _check_margins(tag):
    cam, _ = _csa_modules(tag, torch.float64)
    got = csa_margins(csa_inputs(tag)[0].double(), cam.fc[0].weight.detach(), cam.fc[2].weight.detach())
    print(tag, "margins: pre-activation %.1e, pool gap %.1e, channel gap %.1e" % got)
    for name, g, least in zip(("MLP pre-activation", "global max pool gap", "per-pixel channel max gap"), got, CSA_MARGINS):
        assert g >= least, f"{tag}: {name} {g:.2e} below {least:.0e}: choose another seed in selective_config.CSA_SEED"


def main():
    out = {}
    runs = [(tag, _run_cell) for tag in CELL_CASES] + [(tag, _run_csa) for tag in CSA_CASES]
    for tag in list(CSA_CASES) + [CSA_GPU_CASE[0]]:
        _check_margins(tag)
    for tag, run in runs:
        o32, o64 = run(tag, torch.float32), run(tag, torch.float64)
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
    assert len(parts) <= len(PARTS), f"{len(parts)} parts needed, selective_config.PARTS lists {len(PARTS)}"
    for name in PARTS:
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            os.remove(path)
    for name, part in zip(PARTS, parts):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB, {len(part)} keys)")
    keys = {}
    for name, m in (("SelectiveConvGRU", SelectiveConvGRU(**module_args("two_src"))),
                    ("ChannelAttentionEnhancement", ChannelAttentionEnhancement(32)),
                    ("SpatialAttentionExtractor", SpatialAttentionExtractor(CSA_KERNEL))):
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "state_dict_keys_selective.json"), "w") as f:
        json.dump(keys, f, indent=1)
    print("wrote state_dict_keys_selective.json")


if __name__ == "__main__":
    main()
