"""The sparse optimizer step against what it replaces, on one MI355X: `python tools/apply_bench.py`.

One flat fp32 tensor of N elements (default 1e9, ratio 0.001), W = 1, two pre-generated
gradients rotated per step, 5 warm-up and 20 event-timed steps per leg:

  (a) dense   DGCBucket(fill="sparse").step(g, out), then dgc_sgd_step reading `out` (K7):
              only what a tree without dgc_apply_packed has
  (b) apply   DGCBucket.step_apply(g, DGCSGD): scatter into the bucket's accumulator, then
              dgc_apply_packed

for two optimizer settings: `wd0` (weight_decay = 0) and `wd` (weight_decay 1e-4, momentum
0.9, nesterov). A run is a child process under a time limit of its own that runs (a) then (b)
for each setting from identical state and compares the last step's parameter bit for bit;
the parent repeats it `--repeats` times, never initialises HIP, and stops at the first run
that fails. Prints one JSON line per run, then a summary line: per setting and leg the
medians of the phase after the exchange (`post`: decompress + K7, or apply) and of the whole
step over the repeats, their spread (max - min of the repeats), and whether (b) is no slower
than (a) by more than that spread.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {"wd0": dict(momentum=0.9, weight_decay=0.0, nesterov=True),
            "wd": dict(momentum=0.9, weight_decay=1e-4, nesterov=True)}
LR = 0.1


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _leg(torch, leg, n, ratio, steps, warmup, grads, kw, dev):
    """One leg from fresh state; returns (post ms median, step ms median, the parameter)."""
    from dgc import _lib
    from dgc.bucket import DGCBucket
    from dgc.optim import DGCSGD
    gen = torch.Generator(device=dev).manual_seed(7)
    p = torch.empty(n, device=dev).normal_(generator=gen)
    eng = DGCBucket(n, compress_ratio=ratio, momentum=0.9, nesterov=True, device=dev, world_size=1, seed=42,
                    fill="sparse" if leg == "dense" else "auto")
    post = []

    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    if leg == "dense":
        L, one = _lib.lib(), ctypes.c_void_p * 1
        out = torch.empty(n, device=dev)
        use_buf = kw["weight_decay"] != 0 and kw["momentum"] != 0
        buf = torch.empty(n, device=dev) if use_buf else None
        P, G, B = one(p.data_ptr()), one(out.data_ptr()), one(buf.data_ptr() if use_buf else 0)
        N1 = (ctypes.c_int64 * 1)(n)

        def step(i, timed):
            ev = {}
            if timed:
                post.append(pair())
                ev = {"decompress": (post[-1][0], torch.cuda.Event(enable_timing=True))}
            eng.step(grads[i % len(grads)], out, events=ev)
            _lib.check(L.dgc_sgd_step(P, G, B, N1, (ctypes.c_int32 * 1)(int(i == 0)), 1, LR, kw["momentum"], 0.0,
                                      kw["weight_decay"], int(kw["nesterov"]), _lib.stream_of(dev)), "dgc_sgd_step")
            if timed:
                post[-1][1].record()
    else:
        opt = DGCSGD([p], lr=LR, **kw)

        def step(i, timed):
            ev = {}
            if timed:
                post.append(pair())
                ev = {"apply": post[-1]}
            eng.step_apply(grads[i % len(grads)], opt, events=ev)

    for i in range(warmup):
        step(i, False)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        step(warmup + i, True)
        marks[i + 1].record()
    torch.cuda.synchronize()
    eng.last_info()   # raises what the status words hold
    return (_median([a.elapsed_time(b) for a, b in post]),
            _median([marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]), p)


def _child(a):
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev)
    grads = [torch.empty(a.numel, device=dev).normal_(generator=gen.manual_seed(1234 + i)) for i in range(2)]
    res = {"elements": a.numel, "ratio": a.ratio, "steps": a.steps}
    for name, kw in SETTINGS.items():
        post_a, step_a, p_a = _leg(torch, "dense", a.numel, a.ratio, a.steps, a.warmup, grads, kw, dev)
        post_b, step_b, p_b = _leg(torch, "apply", a.numel, a.ratio, a.steps, a.warmup, grads, kw, dev)
        res[name] = {"dense_post_ms": round(post_a, 4), "apply_post_ms": round(post_b, 4),
                     "dense_step_ms": round(step_a, 4), "apply_step_ms": round(step_b, 4),
                     "param_bit_equal": bool(torch.equal(p_a.view(torch.int32), p_b.view(torch.int32)))}
        del p_a, p_b
    res["gpu_mem_gb"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    print(json.dumps(res), flush=True)
    if not all(res[s]["param_bit_equal"] for s in SETTINGS):
        raise SystemExit("apply_bench: the legs' parameters differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=10 ** 9)
    ap.add_argument("--ratio", type=float, default=0.001)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        _child(a)
        return
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "adam-compression_amd"), REPO, env.get("PYTHONPATH", "")])
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--numel",
           str(a.numel), "--ratio", repr(a.ratio), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    runs = []
    for _ in range(a.repeats):
        p = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if p.stdout.strip():
            print(p.stdout.strip().splitlines()[-1], flush=True)
        if p.returncode != 0:
            raise SystemExit(f"apply_bench: a run ended with {p.returncode}; nothing further is run\n"
                             f"{p.stderr[-2000:]}")
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    summary = {"summary": True, "elements": a.numel, "ratio": a.ratio, "repeats": a.repeats}
    for s in SETTINGS:
        row = {}
        for key in ("dense_post_ms", "apply_post_ms", "dense_step_ms", "apply_step_ms"):
            xs = [r[s][key] for r in runs]
            row[key] = {"median": _median(xs), "spread": round(max(xs) - min(xs), 4), "runs": xs}
        for what in ("post", "step"):
            d, ap_ = row[f"dense_{what}_ms"], row[f"apply_{what}_ms"]
            row[f"apply_{what}_no_slower"] = ap_["median"] <= d["median"] + max(d["spread"], ap_["spread"])
        row["param_bit_equal"] = all(r[s]["param_bit_equal"] for r in runs)
        summary[s] = row
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
