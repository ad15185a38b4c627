"""Helpers of tests/test_gpu_apply_optimizer.py: DistributedOptimizer(batch="apply") — the
compressed tensors stepped from the gathered entries — against the recorded reference runs
(W = 2 over gloo, the replay of tests/gpu_dist_helpers.py) and against batch=True (W = 1)."""
import contextlib
import copy
import io
import json
import os
import random

import numpy as np
import torch

import gpu_dist_helpers as G


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def apply_replay_worker(rank, world, port, label, queue):
    """``G.optimizer_replay_worker``'s steps with batch="apply": the weights after every step
    equal the goldens, and every step with a compressed tensor was an apply step — counted,
    the compressed parameters left without a ``.grad`` (looked at between ``step()`` and
    ``zero_grad()``), the batch's accumulator all-zero bits; a ratio-1 epoch's step counts as
    a dense one."""
    import torch.distributed as dist
    G._init(rank, world, port)
    problems = []
    try:
        dev = torch.device("cuda:0")
        meta = json.load(open(os.path.join(G.GOLDEN, "optimizer_trace.json")))
        trace = np.load(os.path.join(G.GOLDEN, "optimizer_trace.npz"))
        cfg, schedule = G._load_cfg(label)
        want = G._want(label)
        run = G._setup(label, "apply", dev, cfg)
        dopt = run["dopt"]
        bs = dopt._batched
        seen = {}
        zero_grad = dopt.zero_grad

        def spy(*args, **kwargs):   # what step() left, before zero_grad() drops every gradient
            plan = bs._plan
            seen["comp"] = [n for n, p, _, _ in plan["comp"] if p.grad is not None]
            seen["dense"] = [n for n, p, _, _ in plan["dense"] if p.grad is None]
            return zero_grad(*args, **kwargs)

        dopt.zero_grad = spy
        random.seed(cfg["random_seed"])
        layouts = set()
        for epoch, s in schedule:
            before = (bs.apply_steps, bs.dense_steps)
            G._replay_step(run, label, "apply", rank, epoch, s, meta, trace, dev, problems)
            G._check_weights(run, label, cfg, want, s, rank, problems)
            b = bs._plan["batch"]
            layouts.add(id(b))
            took = (bs.apply_steps - before[0], bs.dense_steps - before[1])
            if run["comp"].compress_ratio < 1.0:
                if took != (1, 0):
                    problems.append(("not an apply step", s, took))
                if seen["comp"]:
                    problems.append(("compressed parameters with a .grad", s, seen["comp"]))
                if b._acc is None or int(b._acc.view(torch.int32).count_nonzero()):
                    problems.append(("accumulator not all-zero bits", s))
            elif took != (0, 1):
                problems.append(("a ratio-1 step not counted as dense", s, took))
            if seen["dense"]:
                problems.append(("dense parameters without a .grad", s, seen["dense"]))
        if label == "resnet20" and len(layouts) < 2:
            problems.append(("the warmup did not rebuild the layout", len(layouts)))
        G._check_final(run, label, want, problems)
        queue.put((rank, problems))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback
        queue.put((rank, [("error", repr(e), traceback.format_exc())]))
    finally:
        dist.destroy_process_group()


SETTINGS = ("wd0", "wd_mom_damp", "two_groups")
# the script of a W = 1 run, per step: how it steps, then how it zeroes the gradients
SCRIPT = [("step", True), ("step", False), ("synchronize", False), ("step", True), ("closure", True), ("step", False)]
APPLIED = [how == "step" for how, _ in SCRIPT]


def tiny_setup(batch, setting, dev, dtype=torch.float32, optimizer=None):
    """TinyNet, DGCSGDMemory + DGCCompressor(0.05) on its two weights, DGCSGD in ``setting``
    (or ``optimizer(params)``) under DistributedOptimizer(batch=batch). HOROVOD_ELASTIC=1
    must be set: W = 1 registers the hooks only then."""
    from dgc.compression import DGCCompressor
    from dgc.horovod import DistributedOptimizer
    from dgc.memory import DGCSGDMemory
    from dgc.optim import DGCSGD
    from models import TinyNet
    torch.manual_seed(0)
    random.seed(0)   # the sample starts: the reference's Python-global random.randint draws
    model = TinyNet().to(dev).to(dtype)
    if optimizer is not None:
        opt = optimizer(model.parameters())
    elif setting == "wd0":
        opt = DGCSGD(model.parameters(), lr=0.1)
    elif setting == "wd_mom_damp":
        opt = DGCSGD(model.parameters(), lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    else:   # two groups, both holding a compressed tensor, with different lr and weight decay
        opt = DGCSGD([dict(params=list(model.fc1.parameters()), lr=0.1, weight_decay=0.0),
                      dict(params=list(model.fc2.parameters()), lr=0.05, weight_decay=1e-4)],
                     lr=0.1, momentum=0.9, dampening=0.1)
    mem = DGCSGDMemory(momentum=0.9)
    with contextlib.redirect_stdout(io.StringIO()):
        comp = DGCCompressor(0.05, memory=mem)
        mem.initialize(model.named_parameters())
        comp.initialize([(n, p) for n, p in model.named_parameters() if p.dim() > 1])
    dopt = DistributedOptimizer(opt, named_parameters=model.named_parameters(), compression=comp, batch=batch)
    return model, dopt


def tiny_run(batch, setting, dev):
    """SCRIPT on TinyNet with fresh per-step gradients; returns, per step, the weights' and the
    momentum buffers' bits, which compressed parameters have a ``.grad`` after the step, and
    BatchedStep's (apply_steps, dense_steps) where it counts them."""
    model, dopt = tiny_setup(batch, setting, dev)
    names = [n for n, _ in model.named_parameters()]
    compressed = [n for n, p in model.named_parameters() if p.dim() > 1]
    gen = torch.Generator().manual_seed(1234)
    trail = []
    for s, (how, set_to_none) in enumerate(SCRIPT):
        for p in model.parameters():
            g = torch.randn(p.shape, generator=gen).to(dev)
            if p.grad is None:
                p.grad = g
            else:
                p.grad.add_(g)   # zeroed in place by zero_grad(set_to_none=False)
        for _, hook in reversed(dopt._hook_fns):
            hook()
        if how == "step":
            dopt.step()
        elif how == "synchronize":   # whoever calls it wants the gradients
            dopt.synchronize()
            assert all(p.grad is not None for p in model.parameters())
            with dopt.skip_synchronize():
                dopt.step()
        else:
            dopt.step(lambda: torch.zeros((), device=dev))
        params = dict(model.named_parameters())
        state = {n: dopt.state[params[n]].get("momentum_buffer") if params[n] in dopt.state else None for n in names}
        bs = dopt._batched
        acc = getattr(bs._plan["batch"], "_acc", None)
        trail.append(dict(weights={n: _bits(params[n]) for n in names},
                          state={n: None if b is None else _bits(b) for n, b in state.items()},
                          with_grad=[n for n in compressed if params[n].grad is not None],
                          counts=(getattr(bs, "apply_steps", None), getattr(bs, "dense_steps", None)),
                          acc_nonzero=None if acc is None else int(acc.view(torch.int32).count_nonzero())))
        dopt.zero_grad(set_to_none=set_to_none)
        if s == 2:   # the hyper-parameters are read at every step
            for group in dopt.param_groups:
                group["lr"] *= 0.5
        if s == 3:   # a checkpoint's state: new tensors in state[p]
            dopt.load_state_dict(copy.deepcopy(dopt.state_dict()))
    torch.cuda.synchronize()
    return trail, compressed
