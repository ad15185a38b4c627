"""DistributedOptimizer(batch="apply") against batch=True on the model sets, on one MI355X:
`python tools/apply_opt_bench.py`.

The parameter shapes of dgc.workloads.resnet50 and vgg16_bn (ratio 0.001, the dim > 1 tensors
compressed), W = 1 with HOROVOD_ELASTIC=1 (the hooks register), a fresh gradient set per step
generated before the timed region, 5 warm-up and 20 event-timed steps per leg. A step is what
a training loop runs after backward: the hooks fire, `optimizer.step()` (compress -> exchange
-> the update of every parameter), `zero_grad()`.

  (a) batched  DistributedOptimizer(DGCSGD, batch=True).step(): the dense decompress into the
               batch's output, p.grad rebound to its views, K7 (dgc_sgd_step) reading them
  (b) apply    DistributedOptimizer(DGCSGD, batch="apply").step(): the compressed tensors
               updated from the gathered entries (dgc_apply_packed_multi), K7 for the dense ones

for two optimizer settings: `wd0` (weight_decay = 0) and `wd` (weight_decay 1e-4, momentum
0.9, nesterov). A run is a child process under a time limit of its own that runs (a) then (b)
for each model and setting from identical state and compares the last step's weights bit for
bit; the parent repeats it `--repeats` times, never initialises HIP, and stops at the first
run that fails. Prints one JSON line per run, then a summary line: per model, setting and leg
the median over the repeats of the runs' median step (ms), its spread (max - min of the
repeats), and whether (b) is ahead of (a) by more than the larger spread.
"""
import argparse
import contextlib
import io
import json
import os
import random
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("resnet50", "vgg16_bn")
SETTINGS = {"wd0": dict(momentum=0.9, weight_decay=0.0, nesterov=True),
            "wd": dict(momentum=0.9, weight_decay=1e-4, nesterov=True)}
LR, RATIO = 0.1, 0.001


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _leg(torch, batch, shapes, sets, kw, steps, warmup, dev):
    """One leg from fresh state; returns (median step ms, the weights, BatchedStep's counts)."""
    from dgc import workloads
    from dgc.compression import DGCCompressor
    from dgc.horovod import DistributedOptimizer
    from dgc.memory import DGCSGDMemory
    from dgc.optim import DGCSGD
    gen = torch.Generator(device=dev).manual_seed(7)
    named = [(n, torch.nn.Parameter(torch.empty(s, device=dev).normal_(generator=gen))) for n, s in shapes]
    params = dict(named)
    comp_shapes, _ = workloads.split(shapes)
    compression = DGCCompressor(RATIO, memory=DGCSGDMemory(momentum=0.9, nesterov=True))
    with contextlib.redirect_stdout(io.StringIO()):
        compression.memory.initialize(named)
        compression.initialize([(n, params[n]) for n, _ in comp_shapes])
    random.seed(42)   # the sample starts: the same draws in both legs
    opt = DistributedOptimizer(DGCSGD([p for _, p in named], lr=LR, **kw), named_parameters=named,
                               compression=compression, batch=batch)
    hooks = list(reversed(opt._hook_fns))
    times = []

    def step(i, timed):
        for (_, p), g in zip(named, sets[i]):
            p.grad = g
        for _, hook in hooks:
            hook()
        if timed:
            times.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            times[-1][0].record()
        opt.step()
        opt.zero_grad()
        if timed:
            times[-1][1].record()

    for i in range(warmup):
        step(i, False)
    torch.cuda.synchronize()
    for i in range(steps):
        step(warmup + i, True)
    torch.cuda.synchronize()
    bs = opt._batched
    bs._plan["batch"].status.check(sync=True)   # raises what the status words hold
    return (_median([a.elapsed_time(b) for a, b in times]), [p.detach() for _, p in named],
            (bs.apply_steps, bs.dense_steps))


def _child(a):
    import torch
    from dgc import workloads
    os.environ["HOROVOD_ELASTIC"] = "1"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"ratio": RATIO, "steps": a.steps, "warmup": a.warmup}
    ok = True
    for model in a.models.split(","):
        shapes = getattr(workloads, model)()
        gen, sets = torch.Generator(device=dev), []
        for s in range(a.warmup + a.steps):   # a fresh gradient set per step, in HBM before the timed region
            gen.manual_seed(1234 + s)
            sets.append([torch.randn(sh, generator=gen, device=dev).mul_(1e-3) for _, sh in shapes])
        res[model] = {}
        for name, kw in SETTINGS.items():
            ms_a, w_a, n_a = _leg(torch, True, shapes, sets, kw, a.steps, a.warmup, dev)
            ms_b, w_b, n_b = _leg(torch, "apply", shapes, sets, kw, a.steps, a.warmup, dev)
            equal = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(w_a, w_b))
            counted = n_a == (0, a.warmup + a.steps) and n_b == (a.warmup + a.steps, 0)
            res[model][name] = {"batched_step_ms": round(ms_a, 4), "apply_step_ms": round(ms_b, 4),
                                "weights_bit_equal": bool(equal), "every_step_its_kind": counted}
            ok = ok and equal and counted
            del w_a, w_b
        del sets
        torch.cuda.empty_cache()
    res["gpu_mem_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    print(json.dumps(res), flush=True)
    if not ok:
        raise SystemExit("apply_opt_bench: the legs' weights differ, or a leg did not take its kind of step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        _child(a)
        return
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "adam-compression_amd"), REPO, env.get("PYTHONPATH", "")])
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--models",
           a.models, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    runs = []
    for _ in range(a.repeats):
        p = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if p.stdout.strip():
            print(p.stdout.strip().splitlines()[-1], flush=True)
        if p.returncode != 0:
            raise SystemExit(f"apply_opt_bench: a run ended with {p.returncode}; nothing further is run\n"
                             f"{p.stderr[-2000:]}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    summary = {"summary": True, "ratio": RATIO, "repeats": a.repeats}
    for model in a.models.split(","):
        summary[model] = {}
        for s in SETTINGS:
            row = {}
            for key in ("batched_step_ms", "apply_step_ms"):
                xs = [r[model][s][key] for r in runs]
                row[key] = {"median": _median(xs), "spread": round(max(xs) - min(xs), 4), "runs": xs}
            d, ap_ = row["batched_step_ms"], row["apply_step_ms"]
            row["apply_ahead"] = ap_["median"] < d["median"] - max(d["spread"], ap_["spread"])
            row["weights_bit_equal"] = all(r[model][s]["weights_bit_equal"] for r in runs)
            summary[model][s] = row
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
