"""What make_golden_instnorm.py and tests/test_instnorm.py share: the module cases (class, constructor arguments, input shapes),
their inputs and the loss whose gradients are compared.  The classes come from the caller (`classes[name]`): the reference's own in
the generator, the product's in the test."""
import os

import numpy as np
import torch

from stereo_toolbox_amd.utils import fill_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
PARTS = ("instnorm.npz", "instnorm_2.npz", "instnorm_3.npz")      # dealt below the size limit of a committed file
PART_BYTES = 900_000
KEYS = os.path.join(HERE, "state_dict_keys_instnorm.json")

# tag: (class, positional arguments, keyword arguments, input shapes).  B = 2, channels 8 -> 16, 12 x 20.
MODULE_CASES = {
    "basic2d": ("BasicConv_IN", (8, 16), dict(kernel_size=3, stride=1, padding=1), [(2, 8, 12, 20)]),
    "basic2d_deconv_noact": ("BasicConv_IN", (8, 16), dict(deconv=True, relu=False, kernel_size=4, stride=2, padding=1), [(2, 8, 6, 10)]),
    "basic3d": ("BasicConv_IN", (8, 16), dict(is_3d=True, kernel_size=3, stride=1, padding=1), [(2, 8, 2, 12, 20)]),
    "basic3d_deconv": ("BasicConv_IN", (8, 16), dict(deconv=True, is_3d=True, kernel_size=(1, 4, 4), stride=(1, 2, 2), padding=(0, 1, 1)),
                       [(2, 8, 2, 6, 10)]),
    "conv2x_deconv_concat": ("Conv2x_IN", (8, 16), dict(deconv=True), [(2, 8, 6, 10), (2, 16, 12, 20)]),
    "conv2x_resize_add": ("Conv2x_IN", (8, 16), dict(concat=False), [(2, 8, 12, 20), (2, 16, 7, 11)]),      # 6 x 10 -> the odd 7 x 11
    "res_s1": ("ResidualBlock", (16, 16), dict(norm_fn="instance", stride=1), [(2, 16, 12, 20)]),
    "res_s2": ("ResidualBlock", (8, 16), dict(norm_fn="instance", stride=2), [(2, 8, 12, 20)]),
}
# the constructions whose state-dict keys, shapes and order are recorded
KEY_CASES = {
    "BasicConv_IN": ("BasicConv_IN", (8, 16), dict(kernel_size=3, stride=1, padding=1)),
    "BasicConv_IN/3d_deconv": ("BasicConv_IN", (8, 16), dict(deconv=True, is_3d=True, kernel_size=4, stride=2, padding=1)),
    "Conv2x_IN": ("Conv2x_IN", (8, 16), dict(deconv=True)),
    "Conv2x_IN/3d_keep_dispc": ("Conv2x_IN", (8, 16), dict(deconv=True, is_3d=True, keep_dispc=True, keep_concat=False)),
    "ResidualBlock/instance_s1": ("ResidualBlock", (16, 16), dict(norm_fn="instance", stride=1)),
    "ResidualBlock/instance_s2": ("ResidualBlock", (8, 16), dict(norm_fn="instance", stride=2)),
    "ResidualBlock/group_s2": ("ResidualBlock", (8, 16), dict(norm_fn="group", stride=2)),
    "ResidualBlock/batch_s2": ("ResidualBlock", (8, 16), dict(norm_fn="batch", stride=2)),
    "ResidualBlock/none_s2": ("ResidualBlock", (8, 16), dict(norm_fn="none", stride=2)),
}


def build(classes, tag, cases=MODULE_CASES):
    name, args, kwargs = cases[tag][:3]
    m = classes[name](*args, **kwargs)
    sd = m.state_dict()
    fill_state_dict(sd)
    m.load_state_dict(sd)
    return m


def state_keys(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items()]


def module_inputs(tag):
    g = torch.Generator().manual_seed(1000 + list(MODULE_CASES).index(tag))
    return [torch.randn(s, generator=g) for s in MODULE_CASES[tag][3]], g


def run_module_case(m, tag, dtype, device="cpu"):
    """{out, g/in<i>, g/<parameter>} of loss = (m(*inputs) * gy).sum(), as CPU tensors of `dtype`; `m` already has the case's weights."""
    ins, g = module_inputs(tag)
    m = m.to(device=device, dtype=dtype).train()
    xs = [t.to(device=device, dtype=dtype).requires_grad_() for t in ins]
    out = m(*xs)
    gy = torch.randn(out.shape, generator=g).to(device=device, dtype=dtype)
    params = dict(m.named_parameters())
    grads = torch.autograd.grad((out * gy).sum(), xs + list(params.values()))
    res = {"out": out.detach()}
    res.update({f"g/in{i}": t for i, t in enumerate(grads[:len(xs)])})
    res.update({f"g/{k}": t for k, t in zip(params, grads[len(xs):])})
    return {k: v.detach().cpu() for k, v in res.items()}


def load_gold():
    gold = {}
    for name in PARTS:
        path = os.path.join(HERE, name)
        if os.path.exists(path):
            gold.update(np.load(path))
    return gold
