"""Golden vectors of the instance-norm blocks, generated from the reference's own classes: `BasicConv_IN` and `Conv2x_IN` of
stereo_toolbox/models/IGEVStereo/submodule.py (:82-150) and `ResidualBlock` of stereo_toolbox/models/RAFTStereo/extractor.py (:6-60);
both files import nothing but torch and numpy.

  python tests/golden/make_golden_instnorm.py <directory that holds the reference's stereo_toolbox/>     (seconds)

Per case of instnorm_config.MODULE_CASES the module runs on the CPU, on one thread, in fp32 and in fp64 with loss =
(out * gy).sum().  Stored in instnorm.npz (+ parts, each below the size limit of a committed file) as `tag/key:f64`, `tag/key:f32` and `tag/key:dref` (max|fp32 - fp64|): the output, the
gradient of every input and of every parameter.  The state-dict keys / shapes / order of the reference classes (instance, group,
batch and no norm for the residual block) go to state_dict_keys_instnorm.json.
"""
import importlib.util
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

from tests.golden.instnorm_config import KEY_CASES, KEYS, MODULE_CASES, PART_BYTES, PARTS, build, run_module_case, state_keys  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    models = os.path.join(sys.argv[1], "stereo_toolbox", "models")
    sub = _load(os.path.join(models, "IGEVStereo", "submodule.py"), "ref_igev_submodule")
    ext = _load(os.path.join(models, "RAFTStereo", "extractor.py"), "ref_raft_extractor")
    classes = {"BasicConv_IN": sub.BasicConv_IN, "Conv2x_IN": sub.Conv2x_IN, "ResidualBlock": ext.ResidualBlock}
    torch.set_num_threads(1)
    out = {}
    for tag in MODULE_CASES:
        o32 = run_module_case(build(classes, tag), tag, torch.float32)
        o64 = run_module_case(build(classes, tag), tag, torch.float64)
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
    assert len(parts) <= len(PARTS), f"{len(parts)} parts needed, instnorm_config.PARTS lists {len(PARTS)}"
    for name in PARTS:
        if os.path.exists(os.path.join(HERE, name)):
            os.remove(os.path.join(HERE, name))
    for name, part in zip(PARTS, parts):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB, {len(part)} keys)")
    with open(KEYS, "w") as f:
        json.dump({name: state_keys(build(classes, name, KEY_CASES)) for name in KEY_CASES}, f, indent=1)
    print(f"wrote {KEYS}")


if __name__ == "__main__":
    main()
