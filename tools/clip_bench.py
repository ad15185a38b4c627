"""What local gradient clipping costs per step on one MI355X: `python tools/clip_bench.py`.

The ResNet-50 gradient set (dgc/workloads.py) through dgc.horovod.DistributedOptimizer,
as bench.py's drop-in leg drives it (fresh p.grad tensors, the hooks in backward order,
synchronize(), zero_grad()), in one session on one box:

  (a) native     DGCSGDMemory(gradient_clipping=partial(dgc.clip_grad.clip_grad_norm_, ...)):
                 batch="auto" takes the batched step, the clip fused into K1
  (b) callable   the same clipping as a torch-op callable with the reference's formula
                 (dgc/clip_grad.py:10-20) — all a tree without dgc/clip_grad.py can run, and
                 what an opaque callable still runs here: the per-tensor hook path, the
                 `if clip_coef < 1` a host synchronisation per tensor
  (c) unclipped  the batched step without clipping

then dgc_hbm_probe's streaming rate (K1's 3R2W shape) to set (a) - (c) against the 4
B/element the statistics pass re-reads, and dgc_grad_stats on a 1e9-element tensor
against 8 TB/s. Every leg that touches the GPU is a child process under a time limit of
its own; the parent never initialises HIP. Prints one JSON line.

`--tree DIR` runs leg (b) with DIR's dgc package and library (a built checkout of a
revision without dgc/clip_grad.py) instead of this tree's.
"""
import argparse
import contextlib
import ctypes
import functools
import io
import json
import os
import random
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NORM = 0.05   # below most ResNet-50 tensors' N(0, 1e-3) norms: the scaling branch runs


def reference_clip_grad_norm_(grad, max_norm=MAX_NORM):
    """dgc/clip_grad.py:10-20 for norm_type 2, in torch ops."""
    total_norm = grad.data.norm(2.0)
    clip_coef = max_norm / (total_norm + 1e-6)
    if clip_coef < 1:
        grad.data.mul_(clip_coef)
    return grad


def _optimizer_leg(leg, steps, warmup):
    import torch
    from dgc import workloads
    from dgc.compression import DGCCompressor
    from dgc.horovod import DistributedOptimizer
    from dgc.memory import DGCSGDMemory
    os.environ.setdefault("HOROVOD_ELASTIC", "1")
    dev = torch.device("cuda:0")
    clipping = None
    if leg == "native":
        from dgc.clip_grad import clip_grad_norm_
        clipping = functools.partial(clip_grad_norm_, max_norm=MAX_NORM)
    elif leg == "callable":
        clipping = reference_clip_grad_norm_
    shapes = workloads.resnet50()
    comp_shapes, dense_shapes = workloads.split(shapes)
    named = [(n, torch.nn.Parameter(torch.zeros(s, device=dev))) for n, s in shapes]
    params = dict(named)
    compression = DGCCompressor(0.001, memory=DGCSGDMemory(momentum=0.9, nesterov=True, gradient_clipping=clipping))
    with contextlib.redirect_stdout(io.StringIO()):
        compression.memory.initialize(named)
        compression.initialize([(n, params[n]) for n, _ in comp_shapes])
    random.seed(42)
    opt = DistributedOptimizer(torch.optim.SGD([p for _, p in named], lr=0.0), named_parameters=named,
                               compression=compression)
    batched = opt._batched is not None
    n_steps = steps if batched else max(3, steps // 4)   # the per-tensor path syncs per tensor
    gen = torch.Generator(device=dev)
    sets = []
    for s in range(n_steps + warmup):
        gen.manual_seed(0xD6C + s)
        sets.append([torch.randn(p.shape, generator=gen, device=dev).mul_(1e-3) for _, p in named])
    hooks = list(reversed(opt._hook_fns))

    def step(i):
        for (_, p), g in zip(named, sets[i]):
            p.grad = g
        for _, hook in hooks:
            hook()
        opt.synchronize()
        opt.zero_grad()

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_steps):
        step(warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / n_steps
    return {"leg": leg, "ms_per_step": round(ms, 4), "batched": batched, "steps": n_steps,
            "compressed_elements": sum(workloads.numel(s) for _, s in comp_shapes),
            "elements": sum(workloads.numel(s) for _, s in shapes)}


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _probe_leg(reps=10):
    import torch
    from dgc import _lib
    dev = torch.device("cuda:0")
    L, st = _lib.lib(), _lib.stream_of(dev)
    n = 1 << 28
    a, b, c, d, e = (torch.zeros(n, device=dev) for _ in range(5))
    ms = _timed(lambda: _lib.check(L.dgc_hbm_probe(_lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(d), _lib.ptr(e), n,
                                                   st), "dgc_hbm_probe"), reps)
    return {"leg": "hbm_probe", "elements": n, "ms": round(ms, 4), "tb_per_s": round(20 * n / ms / 1e9, 3)}


def _stats_leg(reps=10):
    import torch
    from dgc import _lib
    dev = torch.device("cuda:0")
    L, st = _lib.lib(), _lib.stream_of(dev)
    n = 10 ** 9
    g = torch.randn(n, device=dev)
    ptrs, nums = (ctypes.c_void_p * 1)(g.data_ptr()), (ctypes.c_int64 * 1)(n)
    wsz = L.dgc_grad_stats_workspace(nums, 1)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    out = torch.empty(1, device=dev)
    ms = _timed(lambda: _lib.check(L.dgc_grad_stats(ptrs, nums, 1, 1, 0, _lib.ptr(out), _lib.ptr(ws), wsz, st),
                                   "dgc_grad_stats"), reps)
    want = float(g.double().square().sum().sqrt())
    return {"leg": "stats_1e9", "elements": n, "ms": round(ms, 4), "tb_per_s": round(4 * n / ms / 1e9, 3),
            "fraction_of_8_tb_per_s": round(4 * n / ms / 1e9 / 8, 3), "norm": float(out.item()), "norm_float64": want}


def child(leg, steps, warmup):
    if leg in ("native", "callable", "unclipped"):
        res = _optimizer_leg(leg, steps, warmup)
    elif leg == "hbm_probe":
        res = _probe_leg()
    else:
        res = _stats_leg()
    print(json.dumps(res), flush=True)


def run_leg(leg, tree, steps, warmup, limit):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(tree, "adam-compression_amd"), tree, env.get("PYTHONPATH", "")])
    env.pop("DGC_HIP_LIB", None)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps",
           str(steps), "--warmup", str(warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"clip_bench: leg {leg} ended with {p.returncode}; nothing further is run\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", default=None, help="run leg (b) from this checkout (built)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    other = os.path.abspath(a.tree) if a.tree else REPO
    legs = {}
    for leg, tree in (("native", REPO), ("callable", other), ("unclipped", REPO), ("native", REPO),
                      ("unclipped", REPO), ("hbm_probe", REPO), ("stats_1e9", REPO)):
        r = run_leg(leg, tree, a.steps, a.warmup, a.limit)
        legs.setdefault(leg, []).append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    nat = min(r["ms_per_step"] for r in legs["native"])
    unc = min(r["ms_per_step"] for r in legs["unclipped"])
    rate = legs["hbm_probe"][0]["tb_per_s"]
    n_comp, n_all = legs["native"][0]["compressed_elements"], legs["native"][0]["elements"]
    print(json.dumps({
        "native_ms": [r["ms_per_step"] for r in legs["native"]], "native_batched": legs["native"][0]["batched"],
        "callable_ms": legs["callable"][0]["ms_per_step"], "callable_batched": legs["callable"][0]["batched"],
        "unclipped_ms": [r["ms_per_step"] for r in legs["unclipped"]],
        "clip_cost_ms": round(nat - unc, 4), "hbm_probe_tb_per_s": rate,
        "stats_reread_floor_ms": round(4 * n_all / (rate * 1e9), 4), "compressed_elements": n_comp, "elements": n_all,
        "stats_1e9": legs["stats_1e9"][0], "tree_b": other}))


if __name__ == "__main__":
    main()
