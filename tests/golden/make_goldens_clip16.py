#!/usr/bin/env python3
"""Generate ``tests/golden/clip16.json`` / ``clip16.npz``: the REFERENCE's local gradient
clipping (dgc/clip_grad.py) on bf16 / fp16 parameters, run through its own DGCSGDMemory
and DGCCompressor.

``make_goldens_clip.py``'s reference import, ``_Spy`` and layout are reused; like it this
runs only where the reference is mounted at ``/root/reference``, on CPU PyTorch with one
thread. Every ATen op of the reference then computes in fp32 and rounds to the dtype.

Tensor cases: dtype {bf16, fp16} x mode {norm2, norminf, value} x ``make_goldens_clip.SIZES``,
three steps at scales 1.0 / 0.1 / 2.0 (the coefficient on both sides of 1); fp16 gradients
and clip parameters are scaled by 0.01. One poison case per dtype and mode (NaN at 17, +inf
at 100 in step 0) and one fp16 case whose norm exceeds 65504: the norm is inf in fp16, the
coefficient 0 and the clip zeroes the gradient — the reference's own hazard, kept. Dense
cases: N = 1027 through ``compensate(accumulate=False)``.

Stored per step: the reference's ``total_norm`` and coefficient (bits of their fp32 images),
the transmitted indices and values, and the 16-bit state (fp32 images: in full for N = 1000,
as SHA-256 otherwise), every NaN stored as the quiet NaN 0x7FC00000 (``_f32``).

Condition on the inputs: for every norm-2 step the reference's ``total_norm`` must equal the
dtype rounding of fl32(sqrt(sum x^2)) with the sum taken in float64. Torch accumulates in
fp32 in an order of its own, so the two can differ where the root lies on a rounding boundary
of the dtype; such a seed is refused here (the script stops and names it) and another one is
chosen, so that "equal to the reference" has one meaning.

Usage:  python tests/golden/make_goldens_clip16.py
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens_clip as GC  # noqa: E402
from make_goldens_clip import POISON, SCALES, SIZES, _bits, _param, _Spy  # noqa: E402
from make_goldens import _World, _quiet, synth  # noqa: E402

DTYPES = [("bf16", torch.bfloat16, 1.0), ("fp16", torch.float16, 0.01)]
MODES = ("norm2", "norminf", "value")
FULL_STATE_MAX = 1000
SEED0 = 120000


def _f32(t):
    """The fp32 image of a 16-bit tensor, every NaN as the quiet NaN 0x7FC00000: which NaN
    pattern a CPU kernel leaves (0xFFFF from ATen's vectorised bf16 narrowing, 0x7FC0 from its
    scalar tail) depends on the element's position in the vector loop, not on the reference."""
    a = t.float().numpy().copy()
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def _check_norm(g, spy, what):
    """The condition on a norm-2 step (module docstring)."""
    x = g.double().numpy()
    want = torch.tensor(np.float32(np.sqrt(np.sum(x * x)))).to(g.dtype)
    got = torch.tensor(spy.norms[-1]).to(g.dtype)
    if _bits(want.float().item()) != _bits(got.float().item()):
        raise SystemExit(f"clip16 {what}: the reference's total_norm {got.item()!r} is not the {g.dtype} rounding of "
                         f"the float64 norm ({want.item()!r}); choose another seed")


def _grad(seed, N, scale, dt, poison):
    g = synth.gradient(seed, N, "normal", scale)
    sha = synth.digest(g)
    g = torch.from_numpy(g.copy()).to(dt)
    if poison:
        g[POISON["nan"]], g[POISON["inf"]] = float("nan"), float("inf")
    return g, sha


def gen_tensor_cases(C, M, K, meta, arrays):
    cases = []
    for dname, dt, dscale in DTYPES:
        for mode in MODES:
            for N, r, nest in SIZES:
                cases.append((f"{dname}_{mode}_n{N}", dname, dt, dscale, mode, N, r, nest, False, SCALES))
            cases.append((f"{dname}_{mode}_n4097_poison", dname, dt, dscale, mode, 4097, 0.01, True, True, SCALES[:2]))
    # the norm of step 0 (about 2000 * sqrt(4097)) is above fp16's largest finite value
    cases.append(("fp16_norm2_n4097_overflow", "fp16", torch.float16, 1.0, "norm2", 4097, 0.01, True, False,
                  [2000.0, 1.0]))
    for ci, (name, dname, dt, dscale, mode, N, r, nest, poison, scales) in enumerate(cases):
        _World.size, _World.rank = 1, 0
        spy = _Spy(K, mode, _param(mode, N) * dscale)
        mem = M.DGCSGDMemory(momentum=0.9, nesterov=nest, gradient_clipping=spy)
        comp = _quiet(C.DGCCompressor, r, memory=mem)
        p = torch.zeros(N, dtype=dt)
        _quiet(mem.initialize, [("w", p)])
        _quiet(comp.initialize, [("w", p)])
        random.seed(42)
        numel, shape, k, S, ks, stride = comp.attributes["w"]
        case = dict(kind="tensor", dtype=dname, mode=mode, param=spy.param, N=N, ratio=r, nesterov=nest, poison=poison,
                    steps=len(scales), attrs=[numel, k, S, ks, stride], per_step=[])
        for s, sc in enumerate(scales):
            seed = SEED0 + 100 * ci + s
            g, sha = _grad(seed, N, sc * dscale, dt, poison and s == 0)
            rstate = random.getstate()
            (vals, idx), ctx = comp.compress(g.clone(), "w")
            if mode == "norm2" and not (poison and s == 0):
                _check_norm(g, spy, f"{name} step {s} (seed {seed})")
            start = None
            if numel != S:
                st = random.getstate()
                random.setstate(rstate)
                start = random.randint(0, stride - 1)
                random.setstate(st)
            key = f"{name}/s{s}"
            arrays[key + "/indices"] = idx.view(-1).numpy().copy()
            arrays[key + "/values"] = _f32(vals.view(-1))
            if N <= FULL_STATE_MAX:
                arrays[key + "/mmt"] = _f32(mem.momentums["w"])
                arrays[key + "/vec"] = _f32(mem.velocities["w"])
            case["per_step"].append(dict(seed=seed, scale=sc * dscale, input_sha=sha, start=start,
                                         total_norm_bits=_bits(spy.norms[-1]), coef_bits=_bits(spy.coefs[-1]),
                                         coef=float(spy.coefs[-1]), n=int(idx.numel()),
                                         mmt_sha=synth.digest(_f32(mem.momentums["w"])),
                                         vec_sha=synth.digest(_f32(mem.velocities["w"]))))
        meta[name] = case
        print(f"clip16 {name}: coefs " + ", ".join(f"{p['coef']:.4g}" for p in case["per_step"]))


def gen_dense_cases(M, K, meta, arrays):
    """compensate(accumulate=False), 2 steps per dtype and mode."""
    N = 1027
    ci = 0
    for dname, dt, dscale in DTYPES:
        for mode in MODES:
            spy = _Spy(K, mode, _param(mode, N) * dscale)
            nest = bool(ci % 2)
            mem = M.DGCSGDMemory(momentum=0.9, nesterov=nest, gradient_clipping=spy)
            _quiet(mem.initialize, [("b", torch.zeros(N, dtype=dt))])
            name = f"{dname}_dense_{mode}"
            case = dict(kind="dense", dtype=dname, mode=mode, param=spy.param, N=N, nesterov=nest, steps=2, per_step=[])
            for s in range(2):
                seed = SEED0 + 5000 + 100 * ci + s
                g, sha = _grad(seed, N, SCALES[s] * dscale, dt, False)
                out = mem.compensate(g.clone(), "b", accumulate=False)
                if mode == "norm2":
                    _check_norm(g, spy, f"{name} step {s} (seed {seed})")
                arrays[f"{name}/s{s}/out"] = _f32(out)
                arrays[f"{name}/s{s}/mmt"] = _f32(mem.momentums["b"])
                case["per_step"].append(dict(seed=seed, scale=SCALES[s] * dscale, input_sha=sha,
                                             total_norm_bits=_bits(spy.norms[-1]), coef_bits=_bits(spy.coefs[-1]),
                                             coef=float(spy.coefs[-1])))
            meta[name] = case
            ci += 1
            print(f"clip16 {name}")


def main():
    C, M, H, O, K = GC._import_reference()
    torch.set_num_threads(1)
    meta, arrays = {}, {}
    gen_tensor_cases(C, M, K, meta, arrays)
    gen_dense_cases(M, K, meta, arrays)
    np.savez_compressed(os.path.join(HERE, "clip16.npz"), **arrays)
    with open(os.path.join(HERE, "clip16.json"), "w") as f:
        json.dump(dict(poison=POISON, cases=meta), f, indent=1)
    print(f"clip16.npz: {os.path.getsize(os.path.join(HERE, 'clip16.npz')) // 1024} KB")


if __name__ == "__main__":
    main()
