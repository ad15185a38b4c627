"""The mixed flat bucket (fp32 state, bf16 gradient) against what it replaces, on one MI355X:
`python tools/mixed_bench.py`.

One flat tensor of N elements (default 1e9 at flat-1B's ratio 0.001), W = 1, nesterov, three
pre-generated bf16-origin gradients rotated per step (a fresh gradient every step, SURVEY.md
§8d), 5 warm-up and 20 event-timed steps, `--repeats` runs of each leg, the legs alternating:

  (a) fp32    DGCBucket on an fp32 gradient (bf16-origin values held in fp32): the fp32 path
  (b) widen   `grad.float()` then (a): what a caller with a bf16 gradient and fp32 state pays
              without (c); its K1 time runs from before the widening to the end of compensate
  (c) mixed   DGCBucket(grad_dtype=torch.bfloat16) on the bf16 gradient: K1 widens in its load

then dgc_hbm_probe's streaming rate (K1's 3R2W shape), to set the K1 rates against. HIP-event
times of K1 alone (`k1_ms_*`) and of the whole step. Every leg is a child process under a time
limit of its own; the parent never initialises HIP, and stops at the first leg that fails.
Prints one JSON line per run, then a summary line: per leg the K1 medians, their spread
between the repeats and the achieved bytes per second of K1 (20, 26 and 18 B/elem plus the
4 B samples).
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("fp32", "widen", "mixed")
K1_BYTES = {"fp32": 20, "widen": 26, "mixed": 18}   # per element; + 4 per sample
NGRADS = 3


def _gradients(torch, n, count, dtype, dev):
    """count gradients of n elements: N(0, 1) rounded to bf16, held in dtype."""
    gen = torch.Generator(device=dev)
    out = []
    for i in range(count):
        gen.manual_seed(1234 + i)
        g = torch.empty(n, dtype=torch.bfloat16, device=dev).normal_(generator=gen)
        out.append(g if dtype == torch.bfloat16 else g.to(dtype))
    return out


def _step_leg(leg, n, ratio, steps, warmup):
    import torch
    from dgc.bucket import DGCBucket
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    kw = {"grad_dtype": torch.bfloat16} if leg == "mixed" else {}
    eng = DGCBucket(n, compress_ratio=ratio, momentum=0.9, nesterov=True, device=dev, world_size=1, seed=42, **kw)
    grads = _gradients(torch, n, NGRADS, torch.float32 if leg == "fp32" else torch.bfloat16, dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    k1 = []   # (start, end) events around K1 (the widen leg: from before the widening)

    def event():
        return torch.cuda.Event(enable_timing=True)

    def step(i, timed):
        g = grads[i % NGRADS]
        first, pair = event(), (event(), event())
        if timed:
            first.record()
        if leg == "widen":
            g = g.float()
        eng.step(g, out, events={"compensate": pair} if timed else None)
        if timed:
            k1.append((first, pair[1]))

    for i in range(warmup):
        step(i, False)
    torch.cuda.synchronize()
    marks = [event() for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        step(warmup + i, True)
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    k1ms = sorted(a.elapsed_time(b) for a, b in k1)
    ms = marks[0].elapsed_time(marks[-1]) / steps
    info = eng.last_info()
    return {"leg": leg, "elements": n, "ratio": ratio, "k": eng.k, "num_samples": eng.num_samples, "steps": steps,
            "ms_per_step": round(ms, 4), "ms_median": round(per[len(per) // 2], 4), "ms_min": round(per[0], 4),
            "ms_max": round(per[-1], 4), "k1_ms_median": round(k1ms[len(k1ms) // 2], 4), "k1_ms_min": round(k1ms[0], 4),
            "k1_ms_max": round(k1ms[-1], 4), "last_branch": info["branch"], "last_full_passes": info["full_passes"],
            "gpu_mem_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}


def _probe_leg(reps=10):
    import torch
    from dgc import _lib
    dev = torch.device("cuda:0")
    L, st = _lib.lib(), _lib.stream_of(dev)
    n = 1 << 28
    a, b, c, d, e = (torch.zeros(n, device=dev) for _ in range(5))

    def fn():
        _lib.check(L.dgc_hbm_probe(_lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(d), _lib.ptr(e), n, st),
                   "dgc_hbm_probe")
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    return {"leg": "hbm_probe", "elements": n, "ms": round(ms, 4), "tb_per_s": round(20 * n / ms / 1e9, 3)}


def run_leg(leg, a):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "adam-compression_amd"), REPO, env.get("PYTHONPATH", "")])
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", leg, "--numel",
           str(a.numel), "--ratio", repr(a.ratio), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"mixed_bench: leg {leg} ended with {p.returncode}; nothing further is run\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=10 ** 9)
    ap.add_argument("--ratio", type=float, default=0.001)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of " + ",".join(LEGS))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        res = _probe_leg() if a.child == "hbm_probe" else _step_leg(a.child, a.numel, a.ratio, a.steps, a.warmup)
        print(json.dumps(res), flush=True)
        return
    runs = {}
    for _ in range(a.repeats):   # the legs alternate, so a drift of the box lands on all of them
        for leg in a.legs.split(","):
            r = run_leg(leg, a)
            runs.setdefault(leg, []).append(r)
            print(json.dumps(r), flush=True)
    probe = run_leg("hbm_probe", a)
    print(json.dumps(probe), flush=True)
    summary = {"summary": True, "elements": a.numel, "ratio": a.ratio, "hbm_probe_tb_per_s": probe["tb_per_s"]}
    for leg, rs in runs.items():
        ms, k1 = [r["ms_per_step"] for r in rs], [r["k1_ms_median"] for r in rs]
        nbytes = K1_BYTES[leg] * a.numel + 4 * rs[0]["num_samples"]
        summary[leg] = {"ms_per_step": ms, "step_spread": round(max(ms) - min(ms), 4), "k1_ms_median": k1,
                        "k1_spread": round(max(k1) - min(k1), 4),
                        "k1_tb_per_s": round(nbytes / min(k1) / 1e9, 3),
                        "k1_frac_of_probe": round(nbytes / min(k1) / 1e9 / probe["tb_per_s"], 3)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
