"""Workers of the W = 2 gradient-clipping tests (tests/test_gpu_clip.py): two processes on
cuda:0 over gloo, in the manner of tests/gpu_dist_helpers.py (whose process-group setup
and recorded-backward replay they use), running the product path with
``DGCSGDMemory(gradient_clipping=...)`` against tests/golden/clip.* recorded from the
reference."""
import contextlib
import functools
import io
import json
import math
import os
import random

import numpy as np
import torch

import gpu_dist_helpers as G
from gpu_dist_helpers import GOLDEN

from oracle import synth


def _clip_fn(mode, param, name=None):
    from dgc import clip_grad as K
    if mode == "norminf":
        return functools.partial(K.clip_grad_norm_, max_norm=param, norm_type=math.inf)
    if mode == "norm2":
        return functools.partial(K.clip_grad_norm_, max_norm=param)
    if mode == "value":
        return functools.partial(K.clip_grad_value_, clip_value=param)
    if mode == "global_value":
        return functools.partial(K.clip_grad_value_by_global_norm_, name=name)
    return functools.partial(K.clip_grad_norm_2_by_global_, max_norm=param, name=name)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clip_optimizer_worker(rank, world, port, label, batch, queue):
    """The reference's TinyNet run with a clipping memory (clip.json ``label``), replayed
    from its recorded gradients and hook order: the weights after every step must be the
    reference's. batch "default": the drop-in default must take the batched step."""
    import torch.distributed as dist
    G._init(rank, world, port)
    problems = []
    try:
        from dgc.comm import Average
        from dgc.compression import DGCCompressor
        from dgc.horovod import DistributedOptimizer
        from dgc.memory import DGCSGDMemory
        from dgc.optim import DGCSGD
        from models import TinyNet
        dev = torch.device("cuda:0")
        cfg = json.load(open(os.path.join(GOLDEN, "clip.json")))["cases"][label]
        arr = np.load(os.path.join(GOLDEN, "clip.npz"))
        torch.manual_seed(cfg["model_seed"])
        model = TinyNet().to(dev)
        opt = DGCSGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                     nesterov=cfg["nesterov_sgd"])
        mem = DGCSGDMemory(momentum=cfg["momentum"], gradient_clipping=_clip_fn(cfg["mode"], cfg["param"]))
        with contextlib.redirect_stdout(io.StringIO()):
            comp = DGCCompressor(cfg["ratio"], memory=mem, fp16_values=cfg["fp16_values"],
                                 int32_indices=cfg["int32_indices"], warmup_epochs=-1)
            mem.initialize(model.named_parameters())
            comp.initialize([(n, p) for n, p in model.named_parameters() if p.dim() > 1])
        kw = {} if batch == "default" else dict(batch=batch)
        dopt = DistributedOptimizer(opt, named_parameters=model.named_parameters(), compression=comp,
                                    backward_passes_per_step=1, op=Average, **kw)
        if batch and dopt._batched is None:
            problems.append(("not batched",))
        params = dict(model.named_parameters())
        random.seed(cfg["random_seed"])
        for s in range(cfg["steps"]):
            key = f"{label}/s{s}/r{rank}"
            order = cfg["trace"][key]
            grads = [arr[f"{key}/{j}"] for j in range(len(order))]
            G.replay_backward(params, order, grads, dev)
            dopt.step()
            dopt.zero_grad()
            torch.cuda.synchronize()
            for n, p in model.named_parameters():
                got = p.detach().cpu().numpy()
                if synth.digest(got) != cfg["weight_sha"][s][n]:
                    problems.append(("weights", s, n))
                if s == cfg["steps"] - 1 and not np.array_equal(_bits(got), _bits(arr[f"{label}/s{s}/{n}"])):
                    problems.append(("final", n, float(np.abs(got - arr[f"{label}/s{s}/{n}"]).max())))
        queue.put((rank, problems))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback
        queue.put((rank, [("error", repr(e), traceback.format_exc())]))
    finally:
        dist.destroy_process_group()


def clip_global_worker(rank, world, port, label, queue):
    """A global variant (clip.json ``label``) on the per-tensor path: one compressed
    tensor per rank, the statistic Averaged between the ranks. The sum of squares has no
    fixed order in the reference, so the device coefficient is read back and checked
    against the recorded one to the sums' accuracy; state and payload must then be the
    oracle's on the gradient clipped with the device coefficient, bit for bit."""
    import torch.distributed as dist
    G._init(rank, world, port)
    problems = []
    try:
        from dgc.compression import DGCCompressor
        from dgc.memory import DGCSGDMemory
        from oracle import dgc_oracle as O
        dev = torch.device("cuda:0")
        case = json.load(open(os.path.join(GOLDEN, "clip.json")))["cases"][label]
        arr = np.load(os.path.join(GOLDEN, "clip.npz"))
        N = case["N"]
        mem = DGCSGDMemory(momentum=0.9, nesterov=True, gradient_clipping=_clip_fn(case["mode"], case["param"], "w"))
        p = torch.zeros(N, device=dev)
        with contextlib.redirect_stdout(io.StringIO()):
            comp = DGCCompressor(case["ratio"], memory=mem)
            mem.initialize([("w", p)])
            comp.initialize([("w", p)])
        random.seed(42)
        m_o, v_o = np.zeros(N, np.float32), np.zeros(N, np.float32)
        for s, step in enumerate(case["per_step"]):
            r = step["ranks"][rank]
            g = synth.gradient(r["seed"], N, "normal", r["scale"])
            (vals, idx), _ = comp.compress(torch.from_numpy(g).to(dev), "w")
            torch.cuda.synchronize()
            c = mem.last_clip_coef.cpu().numpy()[0]
            want = np.array([r["coef_bits"]], np.uint32).view(np.float32)[0]
            # both are fp32 roundings of nearly the same real number: the reference's fp32
            # sums of squares carry up to ~log2(N) * 2^-24, halved by the root
            if abs(float(c) - float(want)) > 2e-6 * abs(float(want)):
                problems.append(("coef", s, float(c), float(want)))
            if case["mode"] == "global_value":
                gc = np.minimum(np.maximum(g, -c), c).astype(np.float32)
            else:
                gc = (g * c).astype(np.float32) if c < 1 else g
            ov, oi, _ = O.compress_step(gc, m_o, v_o, tuple(case["attrs"]), step["start"], nesterov=True)
            if not np.array_equal(idx.view(-1).cpu().numpy(), oi):
                problems.append(("indices", s))
            elif not np.array_equal(_bits(vals.view(-1).cpu().numpy()), _bits(ov)):
                problems.append(("values", s))
            if not np.array_equal(_bits(mem.velocities["w"].cpu().numpy()), _bits(v_o)):
                problems.append(("velocity", s))
            if np.array_equal(oi, arr[f"{label}/s{s}/r{rank}/indices"]) is False:
                problems.append(("golden indices", s))   # the coefficient's last bits cannot move the selection here
        queue.put((rank, problems))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback
        queue.put((rank, [("error", repr(e), traceback.format_exc())]))
    finally:
        dist.destroy_process_group()
