#!/usr/bin/env python3
"""Generate ``tests/golden/clip.json`` / ``clip.npz``: the REFERENCE's local gradient
clipping (dgc/clip_grad.py) run through its own DGCSGDMemory, DGCCompressor and
DistributedOptimizer.

Like ``make_goldens.py`` (whose Horovod stub and helpers it reuses) it runs only where
the reference is mounted at ``/root/reference``, on CPU PyTorch with one thread. Two more
stubs: ``torch._six`` (gone from torch >= 2; the reference imports ``inf`` from it) and
``horovod.torch.allreduce_(tensor, average=True, name=...)`` for the global variants,
restated as the rank-order sum divided by the size.

Inputs come from ``oracle/synth.py`` seeds (only their SHA-256 is stored). Stored per
step: the ``total_norm`` and coefficient the reference computed, the transmitted indices
and values, and the memory state (in full for the smallest tensor, as SHA-256 otherwise).

``clip_grad_value_`` and ``clip_grad_value_by_global_norm_`` return None in the
reference, which its own ``DGCSGDMemory.compensate`` cannot take; they are wrapped to
return the tensor they clipped (the one deviation dgc/clip_grad.py documents).

N = 1000 runs at ratio 0.001, the unsampled ``numel <= ceil(2 / ratio)`` path (one
element transmitted); the sampled tensors run at ratios that select at least 10.

Usage:  python tests/golden/make_goldens_clip.py
"""
import json
import math
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as G  # noqa: E402
from make_goldens import _World, _quiet, synth  # noqa: E402
from models import TinyNet  # noqa: E402


class _Global:
    """The per-rank sums of squares of the step being run (global variants)."""
    sums = None


def _import_reference():
    six = types.ModuleType("torch._six")
    six.inf = math.inf
    sys.modules["torch._six"] = six
    torch._six = six
    C, M, H, O = G._import_reference()

    def allreduce_(tensor, average=True, name=None):
        sums = _Global.sums
        assert sums is not None and torch.equal(tensor, sums[_World.rank]), "unexpected allreduce_ input"
        acc = sums[0].clone()
        for q in range(1, _World.size):
            acc.add_(sums[q])
        if average:
            acc.div_(_World.size)
        return acc

    sys.modules["horovod.torch"].allreduce_ = allreduce_
    import dgc.clip_grad as K
    return C, M, H, O, K


class _Spy:
    """Records what the reference's clip computed: every 0-dim ``total_norm`` and
    coefficient it formed, read off the function's own arithmetic."""

    def __init__(self, K, mode, param):
        self.mode, self.param, self.K = mode, param, K
        self.norms, self.coefs = [], []

    def __call__(self, grad):
        K, p = self.K, self.param
        g0 = grad.detach().clone()
        if self.mode == "norm2":
            out = K.clip_grad_norm_(grad, p)
            total = g0.norm(2.0)
        elif self.mode == "norminf":
            out = K.clip_grad_norm_(grad, p, norm_type=math.inf)
            total = g0.abs().max()
        elif self.mode == "value":
            K.clip_grad_value_(grad, p)
            out, total = grad, None
        elif self.mode == "global_value":
            K.clip_grad_value_by_global_norm_(grad, name="w")
            out = grad
            total = torch.sqrt(_Global.reduced())
        else:
            out = K.clip_grad_norm_2_by_global_(grad, p, name="w")
            total = torch.sqrt(_Global.reduced())
        if total is None:
            self.norms.append(None)
            self.coefs.append(np.float32(p))
        else:
            self.norms.append(np.float32(total.item()))
            coef = total if self.mode == "global_value" else p / (total + 1e-6)
            self.coefs.append(np.float32(coef.item()))
        return out


def _reduced():
    acc = _Global.sums[0].clone()
    for q in range(1, _World.size):
        acc.add_(_Global.sums[q])
    return acc.div_(_World.size)


_Global.reduced = staticmethod(_reduced)

# (N, ratio, nesterov): the unsampled path, a sampled odd size, more than one K1 block row
SIZES = [(1000, 0.001, True), (4097, 0.01, False), (70001, 0.001, True)]
# per-step gradient scales: with max_norm = sqrt(N) / 2 the 2-norm coefficient is about
# 0.5, 5 and 0.25 — below and above 1 within a case
SCALES = [1.0, 0.1, 2.0]
FULL_STATE_MAX = 1000
POISON = dict(nan=17, inf=100)   # positions of the NaN and +inf of the poisoned inputs (step 0)


def _param(mode, N):
    if mode == "norm2":
        return round(math.sqrt(N) / 2, 3)
    if mode == "norminf":
        return 2.5
    return 1.5   # value clamp


def _bits(x):
    return None if x is None else int(np.float32(x).view(np.uint32))


def gen_tensor_cases(C, M, K, meta, arrays):
    cases = []
    for mode in ("norm2", "norminf", "value"):
        for N, r, nest in SIZES:
            cases.append((f"{mode}_n{N}", mode, N, r, nest, False, 3))
        cases.append((f"{mode}_n4097_poison", mode, 4097, 0.01, True, True, 2))
    for ci, (name, mode, N, r, nest, poison, steps) in enumerate(cases):
        _World.size, _World.rank = 1, 0
        spy = _Spy(K, mode, _param(mode, N))
        mem = M.DGCSGDMemory(momentum=0.9, nesterov=nest, gradient_clipping=spy)
        comp = _quiet(C.DGCCompressor, r, memory=mem)
        p = torch.zeros(N)
        _quiet(mem.initialize, [("w", p)])
        _quiet(comp.initialize, [("w", p)])
        random.seed(42)
        numel, shape, k, S, ks, stride = comp.attributes["w"]
        case = dict(kind="tensor", mode=mode, param=spy.param, N=N, ratio=r, nesterov=nest, poison=poison,
                    steps=steps, attrs=[numel, k, S, ks, stride], per_step=[])
        for s in range(steps):
            seed = 90000 + 100 * ci + s
            g = synth.gradient(seed, N, "normal", SCALES[s])
            sha = synth.digest(g)
            if poison and s == 0:
                g[POISON["nan"]], g[POISON["inf"]] = np.nan, np.inf
            rstate = random.getstate()
            (vals, idx), ctx = comp.compress(torch.from_numpy(g.copy()), "w")
            start = None
            if numel != S:
                st = random.getstate()
                random.setstate(rstate)
                start = random.randint(0, stride - 1)
                random.setstate(st)
            key = f"{name}/s{s}"
            arrays[key + "/indices"] = idx.view(-1).numpy().copy()
            arrays[key + "/values"] = vals.view(-1).numpy().copy()
            if N <= FULL_STATE_MAX:
                arrays[key + "/mmt"] = mem.momentums["w"].numpy().copy()
                arrays[key + "/vec"] = mem.velocities["w"].numpy().copy()
            case["per_step"].append(dict(seed=seed, scale=SCALES[s], input_sha=sha, start=start,
                                         total_norm_bits=_bits(spy.norms[-1]), coef_bits=_bits(spy.coefs[-1]),
                                         coef=float(spy.coefs[-1]), n=int(idx.numel()),
                                         mmt_sha=synth.digest(mem.momentums["w"].numpy()),
                                         vec_sha=synth.digest(mem.velocities["w"].numpy())))
        meta[name] = case
        print(f"clip {name}: coefs " + ", ".join(f"{p['coef']:.4g}" for p in case["per_step"]))


def gen_dense_cases(M, K, meta, arrays):
    """compensate(accumulate=False), the dense branch of decompress, 2 steps per mode."""
    N = 1027   # not a multiple of 4, more than one 1024-element block of the multi-tensor K1
    for ci, mode in enumerate(("norm2", "norminf", "value")):
        spy = _Spy(K, mode, _param(mode, N))
        mem = M.DGCSGDMemory(momentum=0.9, nesterov=bool(ci % 2), gradient_clipping=spy)
        _quiet(mem.initialize, [("b", torch.zeros(N))])
        name = f"dense_{mode}"
        case = dict(kind="dense", mode=mode, param=spy.param, N=N, nesterov=bool(ci % 2), steps=2, per_step=[])
        for s in range(2):
            seed = 95000 + 100 * ci + s
            g = synth.gradient(seed, N, "normal", SCALES[s])
            out = mem.compensate(torch.from_numpy(g.copy()), "b", accumulate=False)
            arrays[f"{name}/s{s}/out"] = out.numpy().copy()
            arrays[f"{name}/s{s}/mmt"] = mem.momentums["b"].numpy().copy()
            case["per_step"].append(dict(seed=seed, scale=SCALES[s], input_sha=synth.digest(g),
                                         total_norm_bits=_bits(spy.norms[-1]), coef_bits=_bits(spy.coefs[-1]),
                                         coef=float(spy.coefs[-1])))
        meta[name] = case
        print(f"clip {name}")


def gen_global_cases(C, M, K, meta, arrays):
    """The global variants: W = 2 emulated in process, one compressed tensor, 2 steps."""
    N, r, W = 4097, 0.01, 2
    for ci, mode in enumerate(("global_value", "global_norm2")):
        _World.size = W
        spies, comps, mems = [], [], []
        for q in range(W):
            _World.rank = q
            spy = _Spy(K, mode, 20.0)
            mem = M.DGCSGDMemory(momentum=0.9, nesterov=True, gradient_clipping=spy)
            comp = _quiet(C.DGCCompressor, r, memory=mem)
            p = torch.zeros(N)
            _quiet(mem.initialize, [("w", p)])
            _quiet(comp.initialize, [("w", p)])
            spies.append(spy), comps.append(comp), mems.append(mem)
        random.seed(42)
        numel, shape, k, S, ks, stride = comps[0].attributes["w"]
        name = mode
        case = dict(kind="global", mode=mode, param=20.0, N=N, ratio=r, W=W, nesterov=True, steps=2,
                    attrs=[numel, k, S, ks, stride], per_step=[])
        for s in range(2):
            seeds = [97000 + 100 * ci + 10 * s + q for q in range(W)]
            grads = [synth.gradient(sd, N, "normal", SCALES[s] * (1 + q)) for q, sd in enumerate(seeds)]
            _Global.sums = [torch.sum(torch.from_numpy(g).square()) for g in grads]
            rstate = random.getstate()
            ranks = []
            for q in range(W):
                random.setstate(rstate)
                _World.rank = q
                (vals, idx), ctx = comps[q].compress(torch.from_numpy(grads[q].copy()), "w")
                arrays[f"{name}/s{s}/r{q}/indices"] = idx.view(-1).numpy().copy()
                arrays[f"{name}/s{s}/r{q}/values"] = vals.view(-1).numpy().copy()
                ranks.append(dict(seed=seeds[q], scale=SCALES[s] * (1 + q), input_sha=synth.digest(grads[q]),
                                  coef_bits=_bits(spies[q].coefs[-1]), coef=float(spies[q].coefs[-1]),
                                  n=int(idx.numel()), mmt_sha=synth.digest(mems[q].momentums["w"].numpy()),
                                  vec_sha=synth.digest(mems[q].velocities["w"].numpy())))
            st = random.getstate()
            random.setstate(rstate)
            start = random.randint(0, stride - 1)
            random.setstate(st)
            case["per_step"].append(dict(start=start, ranks=ranks))
        _Global.sums = None
        meta[name] = case
        print(f"clip {name}: coefs " + ", ".join(f"{p['ranks'][0]['coef']:.4g}" for p in case["per_step"]))


# (label, mode, param, fp16_values, int32_indices): the bit-exact modes on both wires
OPT_CASES = [("opt_norminf_fp32", "norminf", 0.02, False, False), ("opt_value_fp16", "value", 0.004, True, True)]


def gen_optimizer_cases(C, M, H, O, K, meta, arrays):
    """The reference's DistributedOptimizer + DGCSGD on TinyNet with a clipping memory, 2
    ranks emulated in one process as make_goldens.gen_optimizer does, 3 steps: the SHA-256
    of rank 0's weights after every step and the weights themselves after the last (the
    replicas are checked bit-identical here), and every rank's compress-call order and
    gradients, which the GPU tests replay."""
    W, steps = 2, 3
    for label, mode, param, fp16, i32 in OPT_CASES:
        _World.size = W
        ranks = []
        for q in range(W):
            _World.rank = q
            torch.manual_seed(7)
            model = TinyNet()
            opt = O.DGCSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
            mem = M.DGCSGDMemory(momentum=0.9, gradient_clipping=_Spy(K, mode, param))
            comp = _quiet(C.DGCCompressor, 0.01, memory=mem, fp16_values=fp16, int32_indices=i32, warmup_epochs=-1)
            _quiet(mem.initialize, model.named_parameters())
            _quiet(comp.initialize, [(n, p) for n, p in model.named_parameters() if p.dim() > 1])
            dopt = H.DistributedOptimizer(opt, named_parameters=model.named_parameters(), compression=comp,
                                          backward_passes_per_step=1, op="Average")
            ranks.append((model, dopt, comp, mem))
        trace, step_ref = {}, [0]
        for q, (_, _, comp, _) in enumerate(ranks):
            G._trace_compress(comp, q, trace, step_ref)
        random.seed(42)
        digests = []
        for s in range(steps):
            step_ref[0] = s
            _World.registry.clear()
            _World.reduced.clear()
            rstate = random.getstate()
            for q, (model, dopt, comp, mem) in enumerate(ranks):
                _World.rank = q
                random.setstate(rstate)
                gen = torch.Generator().manual_seed(5000 + 10 * s + q)
                x = torch.randn(32, 64, generator=gen)
                y = torch.randint(0, 10, (32,), generator=gen)
                torch.nn.functional.cross_entropy(model(x), y).backward()
            for q, (model, dopt, comp, mem) in enumerate(ranks):
                _World.rank = q
                dopt.step()
                dopt.zero_grad()
            digests.append({n: synth.digest(p.detach().numpy()) for n, p in ranks[0][0].named_parameters()})
            for n, p in ranks[0][0].named_parameters():
                if s == steps - 1:
                    arrays[f"{label}/s{s}/{n}"] = p.detach().numpy().copy()
                if not np.array_equal(p.detach().numpy(), dict(ranks[1][0].named_parameters())[n].detach().numpy()):
                    raise SystemExit(f"clip {label}: the reference's replicas diverged")
        spy = ranks[0][3].gradient_clipping
        clipped = sum(1 for c in spy.coefs if mode == "value" or c < 1)
        tmeta = {}
        G._save_trace(label, trace, arrays, tmeta)
        meta[label] = dict(kind="optimizer", mode=mode, param=param, W=W, steps=steps, fp16_values=fp16,
                           int32_indices=i32, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov_sgd=True,
                           memory_nesterov=False, ratio=0.01, batch=32, data_seed="5000 + 10*step + rank",
                           model_seed=7, random_seed=42, clip_calls=len(spy.coefs), clipped_calls=clipped,
                           weight_sha=digests, trace=tmeta)
        print(f"clip {label}: {steps} steps, {clipped} / {len(spy.coefs)} rank-0 calls clipped")


def main():
    C, M, H, O, K = _import_reference()
    torch.set_num_threads(1)
    meta, arrays = {}, {}
    gen_tensor_cases(C, M, K, meta, arrays)
    gen_dense_cases(M, K, meta, arrays)
    gen_global_cases(C, M, K, meta, arrays)
    gen_optimizer_cases(C, M, H, O, K, meta, arrays)
    np.savez_compressed(os.path.join(HERE, "clip.npz"), **arrays)
    with open(os.path.join(HERE, "clip.json"), "w") as f:
        json.dump(dict(poison=POISON, cases=meta), f, indent=1)
    print(f"clip.npz: {os.path.getsize(os.path.join(HERE, 'clip.npz')) // 1024} KB")


if __name__ == "__main__":
    main()
