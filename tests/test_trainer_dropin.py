"""The drop-in modules under the callers SURVEY.md 8(b) names: the reference's own `Trainer.prepare_model`
(trainer/trainer_torchrun.py:105-123: `SyncBatchNorm.convert_sync_batchnorm` + `DistributedDataParallel`) and torch DDP on a ROCm
device.

* without a GPU (`-m "not gpu"`): `_TorchrunTrainer` below plays the caller -- the steps of the reference's torchrun trainer
  (rank from the environment, process group, optional `SyncBatchNorm` conversion, `DDP` wrap, one train iteration), written
  here with torch's public API so that the test needs nothing outside this repository.  Two gloo ranks run the product
  modules on the host-emulator build of the kernels; the iteration is GwcNet's (a list of four predictions).
* GPU box (`-m gpu`): `init_process_group("nccl", world_size=1)` + `DDP(model.cuda(), device_ids=[0])`, gradients bitwise equal to
  the un-wrapped module; `find_unused_parameters` for `ACVNet(attn_weights_only=True)`; `FlatGradSync(overlap=True)` with the
  collectives forced on in the 1-rank RCCL group, so that hook -> async all-reduce (AVG) -> finish() runs on a real stream.
"""
import os
import socket
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
from torch.nn.parallel import DistributedDataParallel as DDP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_W = (0.5, 0.5, 0.7, 1.0)
H, W, D = 16, 64, 32


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _TorchrunTrainer:
    """The caller the product drops in under (the reference's trainer/trainer_torchrun.py: Trainer.__init__,
    setup_distributed, prepare_model, _train_iteration): a torchrun-style trainer that takes its rank from the environment,
    seeds per rank, joins the process group, converts BatchNorm to SyncBatchNorm on request, wraps the model in
    DistributedDataParallel and runs one iteration.  CPU ranks: DDP is given no device_ids."""

    def __init__(self, config):
        self.config = config
        self.local_rank = int(os.environ.get("LOCAL_RANK", -1))
        self.world_size = int(os.environ.get("WORLD_SIZE", -1))
        self.global_rank = int(os.environ.get("RANK", -1))
        self.device = torch.device("cpu")
        torch.manual_seed(config.seed + max(self.global_rank, 0))
        self.max_disp = config.max_disp

    def is_distributed(self):
        return self.local_rank != -1

    def setup_distributed(self):
        if not dist.is_initialized():
            dist.init_process_group(backend=self.config.dist_backend)
        self.world_size = dist.get_world_size()
        self.global_rank = dist.get_rank()

    def prepare_model(self, model):
        model = model.to(self.device)
        if self.is_distributed():
            if self.config.sync_bn:
                model = nn.SyncBatchNorm.convert_sync_batchnorm(model)
            model = DDP(model, find_unused_parameters=self.config.find_unused_parameters)
        return model

    def train_iteration(self, model, data, optimizer):
        """GwcNet's iteration: a list of four predictions, the product's masked multi-output loss."""
        from stereo_toolbox_amd.losses import masked_smooth_l1_multi
        optimizer.zero_grad()
        left = data["left"].to(self.device, non_blocking=True)
        right = data["right"].to(self.device, non_blocking=True)
        gt = data["gt_disp"].to(self.device, non_blocking=True).squeeze(1)
        preds = model(left, right)
        loss = masked_smooth_l1_multi(preds, gt, self.max_disp, LOSS_W)
        loss.backward()
        optimizer.step()
        return loss.item()


def _filled_model(ctor_name, *a, bn_beta_shift=0.0, **k):
    from stereo_toolbox_amd import models
    from stereo_toolbox_amd.utils import fill_state_dict
    m = getattr(models, ctor_name)(*a, **k)
    sd = m.state_dict()
    fill_state_dict(sd, bn_beta_shift=bn_beta_shift)
    m.load_state_dict(sd)
    return m


def _batch(world):
    from stereo_toolbox_amd.utils import synthetic_tensor
    return {"left": synthetic_tensor((world, 3, H, W), 1), "right": synthetic_tensor((world, 3, H, W), 2),
            "gt_disp": synthetic_tensor((world, 1, H, W), 3, lo=0.0, hi=float(D - 2))}


def _trainer_worker(rank, world, port, q, sync_bn):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    from tests.emu_util import emu_product_path
    from stereo_toolbox_amd.distributed import FlatGradSync, broadcast_parameters
    from stereo_toolbox_amd.losses import masked_smooth_l1_multi

    config = types.SimpleNamespace(seed=7, max_disp=D, sync_bn=sync_bn, dist_backend="gloo", find_unused_parameters=False)
    trainer = _TorchrunTrainer(config)
    trainer.setup_distributed()
    assert trainer.is_distributed() and trainer.world_size == world and dist.get_backend() == "gloo"
    real_ddp = DDP
    # torch's DDP constructor refuses SyncBatchNorm layers inside CPU modules (their stock forward needs a GPU).  The
    # product never calls that forward (the modules are parameter containers; aggregation._bn_state all-reduces the
    # statistics itself), so the check -- which only stamps `_specify_ddp_gpu_num(1)` on the layers -- is skipped here.
    real_ddp._passing_sync_batchnorm_handle = lambda self, module: None

    data = {k: v[rank:rank + 1] for k, v in _batch(world).items()}
    with emu_product_path():
        model = _filled_model("GwcNet_GC", D)
        if rank != 0:                                  # DDP's constructor must restore rank 0's parameters
            with torch.no_grad():
                for p in model.parameters():
                    p.add_(0.25)
        model = trainer.prepare_model(model).train()
        assert isinstance(model, real_ddp)
        n_sync = sum(isinstance(m, nn.SyncBatchNorm) for m in model.modules())
        assert (n_sync > 0) == bool(sync_bn)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)          # (lr 0: the gradients are what is compared)
        loss = trainer.train_iteration(model, data, opt)
        ddp_grads = [p.grad.clone() for p in model.module.parameters()]
        ddp_stats = {k: v.clone() for k, v in model.module.state_dict().items() if "running" in k or "num_batches" in k}

        # the lean path of bench.py on the same shard: flat buffer + one averaged all-reduce
        twin = _filled_model("GwcNet_GC", D)
        if sync_bn:
            twin = nn.SyncBatchNorm.convert_sync_batchnorm(twin)
        twin.train()
        broadcast_parameters(twin)
        gs = FlatGradSync(twin)
        gs.detach_grads()
        preds = twin(data["left"], data["right"])
        loss2 = masked_smooth_l1_multi(preds, data["gt_disp"].squeeze(1), D, LOSS_W)
        loss2.backward()
        gs.finish()
    worst = 0.0
    for (name, p), g in zip(twin.named_parameters(), ddp_grads):
        assert p.grad is not None and g is not None, name
        err = (p.grad - g).abs().max().item()
        worst = max(worst, err / (g.abs().max().item() + 1e-12))
        # same kernels, same shard; DDP averages as (g0/2 + g1/2), the flat path as (g0 + g1)/2: equal up to one rounding
        assert err <= 1e-6 * g.abs().max().item() + 1e-12, (name, err)
    tsd = twin.state_dict()
    for k, v in ddp_stats.items():
        assert torch.equal(tsd[k], v), k
    assert int(tsd["dres0.0.1.num_batches_tracked"]) == 1
    assert abs(loss - loss2.item()) <= 1e-6 * max(1.0, abs(loss))
    q.put((rank, float(loss), worst, [g.numpy().copy() for g in ddp_grads[:4] + ddp_grads[-4:]]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("sync_bn", [False, True], ids=["per_replica_bn", "sync_bn"])
def test_reference_trainer_prepare_model_two_ranks(sync_bn):
    """north_star: "drops in under the existing trainer".  GwcNet_GC through the trainer's prepare_model (`_TorchrunTrainer`:
    optionally SyncBatchNorm-converted, then DDP-wrapped) on two gloo ranks, one train iteration: every rank ends with
    the same gradients, they equal the FlatGradSync path's, BatchNorm running statistics and counters agree."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from emu_util import emu_lib
    emu_lib()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_trainer_worker, args=(r, 2, port, q, sync_bn)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    import queue as _queue
    for _ in range(1500):                               # a rank that dies must fail the test at once, not after a timeout
        try:
            res.append(q.get(timeout=1.0))
        except _queue.Empty:
            assert all(p.is_alive() or p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        if len(res) == len(procs):
            break
    assert len(res) == len(procs)
    res.sort(key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for a, b in zip(res[0][3], res[1][3]):            # DDP left identical averaged gradients on both ranks
        assert (torch.from_numpy(a) - torch.from_numpy(b)).abs().max().item() == 0.0
    assert res[0][1] != res[1][1]                      # ... computed from different shards


# ----------------------------------------------------------------------------------------------- GPU box: 1-rank RCCL group
def _init_single_rank_nccl():
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))


@pytest.fixture
def nccl_world1():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    _init_single_rank_nccl()
    yield
    dist.destroy_process_group()


def _grad_distance(named_params, want):
    """Worst relative distance (to the tensor's max) between the gradients of a module and a reference list, separately for
    the 2-D feature CNN and for everything behind it; parameters without a gradient on either side must agree on that."""
    worst = {"2d": 0.0, "3d": 0.0}
    n_exact, n = 0, 0
    for (name, p), g in zip(named_params, want):
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        n += 1
        if torch.equal(p.grad, g):
            n_exact += 1
            continue
        rel = (p.grad - g).abs().max().item() / (g.abs().max().item() + 1e-30)
        k = "2d" if name.startswith("feature_extraction.") else "3d"
        worst[k] = max(worst[k], rel)
    return worst, n_exact, n


def _same_grads(named_params, want, noise, what, parity_log=None):
    """Gradients of a wrapped / synchronised module against the plain module's.  Two runs of the SAME plain step on this box
    are not bit-identical: the stock 2-D CNN's MIOpen kernels differ from run to run (atomics in backward-weights, algorithm
    choice per module instance), and at these tiny shapes (a few hundred voxels per channel at the 1/16 level) train-mode
    BatchNorm amplifies one-ulp feature differences to 1e-3 .. 1e-2 of a gradient's max (GPU call D of round 4: 0 of 269
    tensors bitwise equal between two plain runs, worst 0.6 % / 4 %).  `noise` is that run-to-run distance measured in the
    same test (plain vs two more plain instances); the wrapped module may be at most 5 x as far from plain as plain is from
    itself (floor: see below -- a few runs are a noisy estimate of that distance: 0.2 % .. 3 % for the 3-D path over the calls of
    round 4, 9.5 % once in round 5).  A wrapper that dropped, doubled or
    mis-scaled a gradient would be off by O(1); the exact-equality form of this check runs on the deterministic CPU /
    gloo / emulator path (test_reference_trainer_prepare_model_two_ranks: 1e-6)."""
    worst, n_exact, n = _grad_distance(named_params, want)
    if parity_log is not None:
        parity_log(what, tensors=n, bitwise_equal=n_exact, worst_rel_2d_cnn=worst["2d"], worst_rel_3d_path=worst["3d"],
                   plain_run_to_run_2d=noise["2d"], plain_run_to_run_3d=noise["3d"])
    # floor 5 % (round 6; rounds 4-5: 10 % -> 25 % at the chaotic 64x128 toy configuration).  The smoke steps now run at the
    # fixture tests' shape and weight profile (B=2 128x256 D=128, shifted BatchNorm betas): two plain runs differ by 0.3-2.2 %
    # (2-D CNN tensors) / 0.03-0.7 % (3-D path) over the calls of round 6.  The EXACT check is
    # test_ddp_and_flat_sync_are_exact_behind_fixed_features_rccl_world1 below (bitwise, no stock 2-D CNN in the graph).
    for k in ("2d", "3d"):
        assert worst[k] <= max(5.0 * noise[k], 0.05), (what, k, worst[k], noise[k])
    return n_exact, n


def _plain_reference(ctor, *a, **k):
    """The un-wrapped module's gradients / BatchNorm statistics for one step, and the run-to-run noise of that step."""
    plain = _filled_model(ctor, *a, **k).cuda().train()
    _gpu_step(plain)
    want = [p.grad.clone() if p.grad is not None else None for p in plain.parameters()]
    stats = {kk: v.clone() for kk, v in plain.state_dict().items() if "running" in kk or "num_batches" in kk}
    noise = {"2d": 0.0, "3d": 0.0}
    for _ in range(2):                                  # two more plain instances: the larger of their distances to the first
        again = _filled_model(ctor, *a, **k).cuda().train()
        _gpu_step(again)
        d, _, _ = _grad_distance(again.named_parameters(), want)
        noise = {kk: max(noise[kk], d[kk]) for kk in noise}
    return want, stats, noise


TOY_D = 128     # the GPU smoke steps run at the fixture tests' well-conditioned shape (tests/golden/toy_train_config.py)


def _gpu_step(model, Hh=128, Ww=256, Dd=TOY_D, B=2):
    from stereo_toolbox_amd.losses import masked_smooth_l1_multi
    from stereo_toolbox_amd.utils import synthetic_tensor
    left, right = synthetic_tensor((B, 3, Hh, Ww), 1).cuda(), synthetic_tensor((B, 3, Hh, Ww), 2).cuda()
    gt = synthetic_tensor((B, Hh, Ww), 3, lo=0.0, hi=float(Dd - 2)).cuda()
    preds = model(left, right)
    loss = masked_smooth_l1_multi(preds, gt, Dd, LOSS_W[-len(preds):])
    loss.backward()
    return loss


@pytest.mark.gpu
def test_ddp_wrapped_module_matches_unwrapped_rccl_world1(nccl_world1, parity_log):
    """`DDP(model.cuda(), device_ids=[0])` over a 1-rank RCCL group (what Trainer.prepare_model builds, :116-121): the
    reducer's hooks see the ctypes-backed autograd Functions, the deferred BatchNorm counters and the channels_last 2-D
    weights; gradients must equal the un-wrapped module's bit for bit (deterministic kernels; a 1-rank AVG is the
    identity), the wrapped module must keep working for a second step, and SyncBatchNorm conversion must not change a
    1-rank result."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    torch.backends.cudnn.benchmark = False
    want, want_stats, noise = _plain_reference("GwcNet_GC", TOY_D, bn_beta_shift=1.0)

    for convert in (False, True):
        m = _filled_model("GwcNet_GC", TOY_D, bn_beta_shift=1.0).cuda()
        if convert:
            m = nn.SyncBatchNorm.convert_sync_batchnorm(m)
        ddp = DDP(m.train(), device_ids=[0], output_device=0, find_unused_parameters=False)
        _gpu_step(ddp)
        torch.cuda.synchronize()
        _same_grads(ddp.module.named_parameters(), want, noise, f"ddp_world1[sync_bn_converted={convert}]", parity_log)
        sd = ddp.module.state_dict()
        for k, v in want_stats.items():
            assert torch.equal(sd[k], v) or (sd[k] - v).abs().max().item() <= 1e-4 * (1 + v.abs().max().item()), (convert, k)
        ddp.zero_grad(set_to_none=True)
        _gpu_step(ddp)                                 # the reducer re-arms: a second iteration works
        assert all(p.grad is not None for p in ddp.module.parameters())


@pytest.mark.gpu
def test_ddp_find_unused_parameters_acvnet_attention_only(nccl_world1, parity_log):
    """ACVNet(attn_weights_only=True) leaves the whole main branch without gradients (reference acv.py:164-176,232-245): under
    DDP that needs `find_unused_parameters=True` (config.find_unused_parameters, trainer_torchrun.py:120), whose graph walk
    starts at the outputs of the custom Functions."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    torch.backends.cudnn.benchmark = False
    want, _, noise = _plain_reference("ACVNet", TOY_D, attn_weights_only=True, bn_beta_shift=1.0)
    m = _filled_model("ACVNet", TOY_D, attn_weights_only=True, bn_beta_shift=1.0).cuda().train()
    ddp = DDP(m, device_ids=[0], output_device=0, find_unused_parameters=True)
    _gpu_step(ddp)
    torch.cuda.synchronize()
    _, used = _same_grads(ddp.module.named_parameters(), want, noise, "ddp_world1_acv_attention_only", parity_log)
    assert 0 < used < len(want)


@pytest.mark.gpu
def test_flat_grad_sync_overlap_runs_on_rccl_world1(nccl_world1, parity_log):
    """The bench's gradient exchange on a real stream: autograd hooks launch asynchronous RCCL AVG all-reduces of the two
    ranges while backward() is still running, finish() waits for them.  In a 1-rank group the average is the identity, so
    the flat buffer must equal the plain gradients (bit for bit behind the 2-D CNN) -- and every range must really have gone
    through RCCL."""
    from stereo_toolbox_amd.distributed import FlatGradSync
    torch.backends.cudnn.benchmark = False
    want, _, noise = _plain_reference("GwcNet_GC", TOY_D, bn_beta_shift=1.0)
    from stereo_toolbox_amd.distributed import broadcast_parameters
    m = _filled_model("GwcNet_GC", TOY_D, bn_beta_shift=1.0).cuda().train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    broadcast_parameters(m)                            # the flat per-dtype broadcasts (fp32 and int64 buffers) over RCCL
    torch.cuda.synchronize()
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k            # (a 1-rank broadcast is the identity, layouts included)
    gs = FlatGradSync(m, buckets=2, overlap=True, collective_at_world_1=True)
    assert gs.overlap and gs.exchange and gs.nb == 2
    calls = []
    orig = dist.all_reduce

    def counting(t, *a, **k):
        calls.append((t.numel(), k.get("async_op", False), k.get("op")))
        return orig(t, *a, **k)
    dist.all_reduce = counting
    try:
        for it in range(2):
            gs.detach_grads() if it == 0 else gs.zero_grad()
            _gpu_step(m)
            assert any(gs._launched), "no range was launched from a hook during backward()"
            gs.finish()
            torch.cuda.synchronize()
            assert gs.views_intact() and all(gs._launched)
            _same_grads(m.named_parameters(), want, noise, f"flat_grad_sync_overlap_world1[step{it}]", parity_log)
    finally:
        dist.all_reduce = orig
    assert len(calls) == 4 and all(c[1] for c in calls) and all(c[2] == dist.ReduceOp.AVG for c in calls)
    assert sum(c[0] for c in calls[:2]) == gs.flat.numel()


class _BehindTheFeatures(nn.Module):
    """GwcNet_GC from its 1/4-resolution features on (`aggregate`), as a module DDP / FlatGradSync can wrap: the features are
    fixed buffers, so nothing of the stock 2-D CNN (MIOpen: not run-to-run reproducible) is in the graph and every gradient
    behind them is a deterministic function of the inputs."""

    def __init__(self, model, feats, H, W):
        super().__init__()
        self.model = model
        for p in self.model.feature_extraction.parameters():
            p.requires_grad_(False)
        for i, f in enumerate(feats):
            self.register_buffer(f"f{i}", f)
        self.hw = (H, W)

    def forward(self, _unused):          # (DDP with device_ids scatters its positional inputs: it needs at least one)
        return self.model.aggregate({"gwc_feature": self.f0, "concat_feature": self.f2},
                                    {"gwc_feature": self.f1, "concat_feature": self.f3}, *self.hw)


@pytest.mark.gpu
def test_ddp_and_flat_sync_are_exact_behind_fixed_features_rccl_world1(nccl_world1, parity_log):
    """the wrapped-vs-plain checks above accept max(5 x run-to-run noise, 10 %) because the stock 2-D CNN makes two
    plain steps differ.  Here the graph starts at FIXED feature maps: the hand-written path is bit-for-bit reproducible, a 1-rank
    RCCL AVG is the identity, so torch DDP's reducer and FlatGradSync's hook -> asynchronous all-reduce -> finish() sequence must
    hand back EXACTLY the plain module's gradients -- a bucket-ordering error, a stale view or a partially reduced range would
    show as a non-zero difference, not as a few per cent."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    from stereo_toolbox_amd.distributed import FlatGradSync
    from stereo_toolbox_amd.losses import masked_smooth_l1_multi
    from stereo_toolbox_amd.utils import synthetic_tensor
    Hh, Ww, Dd, B = 64, 128, 64, 1
    feats = [synthetic_tensor((B, 320, Hh // 4, Ww // 4), 21, lo=-1.0, hi=1.0).cuda(),
             synthetic_tensor((B, 320, Hh // 4, Ww // 4), 22, lo=-1.0, hi=1.0).cuda(),
             synthetic_tensor((B, 12, Hh // 4, Ww // 4), 23, lo=-1.0, hi=1.0).cuda(),
             synthetic_tensor((B, 12, Hh // 4, Ww // 4), 24, lo=-1.0, hi=1.0).cuda()]
    gt = synthetic_tensor((B, Hh, Ww), 3, lo=0.0, hi=float(Dd - 2)).cuda()

    def make():
        return _BehindTheFeatures(_filled_model("GwcNet_GC", Dd).cuda().train(), feats, Hh, Ww)

    def step(mod):
        preds = mod(gt)
        masked_smooth_l1_multi(preds, gt, Dd, LOSS_W[-len(preds):]).backward()
        torch.cuda.synchronize()

    plain = make()
    step(plain)
    want = {k: p.grad.clone() for k, p in plain.named_parameters() if p.grad is not None}
    assert len(want) >= 100          # every parameter behind the feature extractor
    again = make()
    step(again)
    assert all(torch.equal(p.grad, want[k]) for k, p in again.named_parameters() if p.grad is not None), "the plain step itself is not reproducible"

    ddp = DDP(make(), device_ids=[0], output_device=0)
    step(ddp)
    bad = [k for k, p in ddp.module.named_parameters() if k in want and not torch.equal(p.grad, want[k])]
    assert not bad, ("DDP", bad[:5])

    m = make()
    gs = FlatGradSync(m, buckets=3, overlap=True, collective_at_world_1=True)
    for it in range(2):
        gs.detach_grads() if it == 0 else gs.zero_grad()
        step(m)
        gs.finish()
        torch.cuda.synchronize()
        assert gs.views_intact() and all(gs._launched)
        bad = [k for k, p in m.named_parameters() if k in want and not torch.equal(p.grad, want[k])]
        assert not bad, (f"FlatGradSync step {it}", bad[:5])
    parity_log("ddp_and_flat_sync_exact_behind_fixed_features", tensors=len(want), not_bitwise_equal=0)
