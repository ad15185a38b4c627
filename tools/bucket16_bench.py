"""The 16-bit flat bucket against what it replaces, on one MI355X: `python tools/bucket16_bench.py`.

One flat tensor of N elements (default 1e9, ratio 0.001; `--numel 7000000000 --ratio 1e-4`
for the 7B shape), W = 1, nesterov, a handful of pre-generated bf16 gradients rotated per
step, 5 warm-up and 20 event-timed steps, `--repeats` runs of each leg:

  (a) bucket16   DGCBucket(dtype=torch.bfloat16): K1-16 with the sample and the lists fused
  (b) batch16    DGCBatch([("w", (N,))], dtype=torch.bfloat16): the 16-bit engine a tree
                 without (a) has — a scalar K1-16, then the selection re-reads its image
  (c) bucket32   the fp32 DGCBucket on the same values widened to fp32

then dgc_hbm_probe's streaming rate (K1's 3R2W shape), to set (a)'s K1 against. Every leg
is a child process under a time limit of its own; the parent never initialises HIP, and
stops at the first leg that fails. Prints one JSON line per run, then a summary line.

`--tree DIR` runs legs (b) and (c) with DIR's dgc package and library (a built checkout of
the revision to compare against); they use nothing a tree without (a) lacks. The batch
takes its gradient from its own flat buffer: the rotation rebinds `grad_flat` to the next
pre-generated tensor (no copy), as the buckets are handed theirs.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("bucket16", "batch16", "bucket32")
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
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dt = torch.float32 if leg == "bucket32" else torch.bfloat16
    k1 = []   # (start, end) events around the compensate phase

    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    if leg == "batch16":
        from dgc.batch import DGCBatch
        eng = DGCBatch([("w", (n,))], compress_ratio=ratio, momentum=0.9, nesterov=True, device=dev, world_size=1,
                       seed=42, dtype=dt)
        grads = _gradients(torch, eng.flat_numel, NGRADS, dt, dev)
        k, num_samples = eng.attrs[0][0], eng.attrs[0][1]

        def step(i, timed):
            eng.grad_flat = grads[i % NGRADS]
            if timed:
                k1.append(pair())
                k1[-1][0].record()
            eng.compensate()
            if timed:
                k1[-1][1].record()
            eng.select()
            eng.exchange()
            eng.decompress()
    else:
        from dgc.bucket import DGCBucket
        kw = {} if leg == "bucket32" else {"dtype": dt}
        eng = DGCBucket(n, compress_ratio=ratio, momentum=0.9, nesterov=True, device=dev, world_size=1, seed=42, **kw)
        grads = _gradients(torch, n, NGRADS, dt, dev)
        out = torch.empty(n, dtype=dt, device=dev)
        k, num_samples = eng.k, eng.num_samples

        def step(i, timed):
            ev = {}
            if timed:
                k1.append(pair())
                ev = {"compensate": k1[-1]}
            eng.step(grads[i % NGRADS], out, events=ev)

    for i in range(warmup):
        step(i, False)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        step(warmup + i, True)
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    k1ms = sorted(a.elapsed_time(b) for a, b in k1)
    ms = marks[0].elapsed_time(marks[-1]) / steps
    info = eng.infos()[0] if leg == "batch16" else eng.last_info()
    return {"leg": leg, "elements": n, "ratio": ratio, "k": k, "num_samples": num_samples, "steps": steps,
            "ms_per_step": round(ms, 4),
            "ms_median": round(per[len(per) // 2], 4), "ms_min": round(per[0], 4), "ms_max": round(per[-1], 4),
            "elements_per_s": round(n / ms * 1e3, 1), "k1_ms_median": round(k1ms[len(k1ms) // 2], 4),
            "k1_ms_min": round(k1ms[0], 4), "last_branch": info["branch"], "last_full_passes": info["full_passes"],
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


def run_leg(leg, tree, a):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(tree, "adam-compression_amd"), tree, env.get("PYTHONPATH", "")])
    env.pop("DGC_HIP_LIB", None)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", leg, "--numel",
           str(a.numel), "--ratio", repr(a.ratio), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"bucket16_bench: leg {leg} ended with {p.returncode}; nothing further is run\n"
                         f"{p.stderr[-2000:]}")
    r = json.loads(p.stdout.strip().splitlines()[-1])
    r["tree"] = os.path.relpath(tree, REPO)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=10 ** 9)
    ap.add_argument("--ratio", type=float, default=0.001)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated subset of " + ",".join(LEGS))
    ap.add_argument("--tree", default=None, help="run legs (b) and (c) from this checkout (built)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        res = _probe_leg() if a.child == "hbm_probe" else _step_leg(a.child, a.numel, a.ratio, a.steps, a.warmup)
        print(json.dumps(res), flush=True)
        return
    other = os.path.abspath(a.tree) if a.tree else REPO
    runs = {}
    for _ in range(a.repeats):   # the legs alternate, so a drift of the box lands on all of them
        for leg in a.legs.split(","):
            r = run_leg(leg, REPO if leg == "bucket16" else other, a)
            runs.setdefault(leg, []).append(r)
            print(json.dumps(r), flush=True)
    probe = run_leg("hbm_probe", REPO, a)
    print(json.dumps(probe), flush=True)
    summary = {"summary": True, "elements": a.numel, "ratio": a.ratio, "hbm_probe_tb_per_s": probe["tb_per_s"]}
    for leg, rs in runs.items():
        ms = [r["ms_per_step"] for r in rs]
        summary[leg] = {"ms_per_step": ms, "min": min(ms), "max": max(ms), "spread": round(max(ms) - min(ms), 4),
                        "elements_per_s": round(a.numel / min(ms) * 1e3, 1),
                        "k1_ms_median": [r["k1_ms_median"] for r in rs]}
    if "bucket16" in runs:
        # K1-16's bytes: 3 x 2 B read, 2 x 2 B written, the 4 B image, 4 B per sample
        num_samples = runs["bucket16"][0]["num_samples"]
        k1 = min(r["k1_ms_median"] for r in runs["bucket16"])
        tbs = (14 * a.numel + 4 * num_samples) / k1 / 1e9
        summary["k1_16"] = {"ms": k1, "tb_per_s": round(tbs, 3), "frac_of_8_tb_per_s": round(tbs / 8, 3),
                            "frac_of_probe": round(tbs / probe["tb_per_s"], 3)}
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
