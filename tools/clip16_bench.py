"""What local gradient clipping costs the 16-bit flat bucket per step on one MI355X:
`python tools/clip16_bench.py`.

DGCBucket(dtype=bf16) at 1e9 elements, fresh gradients per step (a ring of distinct
tensors), clip_grad_norm_ with a coefficient below 1, in one session on one box, the legs
alternating:

  (a) fused     DGCBucket(clip=partial(dgc.clip_grad.clip_grad_norm_, max_norm=...)):
                dgc_grad_stats16 -> dgc_clip_coefs16 -> dgc_compress_begin16_clip
  (b) aten      the same bucket without `clip`, the reference's formula (dgc/clip_grad.py:10-20)
                in ATen ops on the bf16 gradient before `step` (the multiply by a coefficient
                >= 1 replaced by a multiply by 1, so no host synchronisation): what a tree
                without DGCBucket(clip=) has to do
  (c) none      no clipping

then dgc_hbm_probe's streaming rate, to set (a) - (c) against the 2 B/element the statistics
pass re-reads, and dgc_grad_stats16 alone on a tensor of the same size. Every leg is a child
process under a time limit of its own; the parent never initialises HIP and starts nothing
after a leg that failed. Prints one JSON line.
"""
import argparse
import functools
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 10 ** 9
RING = 3
MAX_NORM = 10.0   # N(0, 1e-3) at 1e9 elements has norm ~31.6: the coefficient is ~0.32


def _bucket_leg(leg, steps, warmup, numel):
    import torch
    from dgc.bucket import DGCBucket
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    clip = None
    if leg == "fused":
        from dgc.clip_grad import clip_grad_norm_
        clip = functools.partial(clip_grad_norm_, max_norm=MAX_NORM)
    kw = dict(compress_ratio=0.001, momentum=0.9, nesterov=True, device=dev, world_size=1, seed=42, dtype=dt)
    b = DGCBucket(numel, clip=clip, **kw) if clip is not None else DGCBucket(numel, **kw)
    gen = torch.Generator(device=dev)
    ring = []
    for s in range(RING):
        gen.manual_seed(0xC16 + s)
        ring.append(torch.randn(numel, generator=gen, device=dev, dtype=dt).mul_(1e-3))
    spare = torch.empty(numel, dtype=dt, device=dev)   # leg (b) clips a copy: the ring stays fresh
    out = torch.empty(numel, dtype=dt, device=dev)
    one = torch.ones((), dtype=dt, device=dev)

    def step(i):
        g = ring[i % RING]
        if leg == "aten":
            g = spare.copy_(g)
        return g

    def run(i, g, phases=None):
        if leg == "aten":
            total = g.norm(2.0)
            coef = MAX_NORM / (total + 1e-6)
            g.mul_(torch.where(coef < 1, coef, one))
        b.step(g, out, phases)

    for i in range(warmup):
        run(i, step(i))
    torch.cuda.synchronize()
    pair = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))   # noqa: E731
    ev = [pair() for _ in range(steps)]
    # the bucket's own phases (the statistics and the coefficient are part of "compensate")
    ph = [{"compensate": pair(), "select": pair()} for _ in range(steps)]
    for i in range(steps):
        g = step(warmup + i)   # (the copy that keeps leg (b)'s input fresh is not timed)
        ev[i][0].record()
        run(warmup + i, g, ph[i])
        ev[i][1].record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(z) for a, z in ev)
    med = lambda name: round(sorted(p[name][0].elapsed_time(p[name][1]) for p in ph)[steps // 2], 4)   # noqa: E731
    info = b.last_info()
    return {"leg": leg, "elements": numel, "ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4),
            "ms_max": round(ms[-1], 4), "compensate_ms": med("compensate"), "select_ms": med("select"), "steps": steps,
            "branch": info["branch"],
            "coef": None if b.clip_coef is None else float(b.clip_coef[0])}


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


def _stats_leg(numel, reps=10):
    """dgc_grad_stats16 (2-norm) alone on a bf16 tensor of numel elements."""
    import ctypes
    import torch
    from dgc import _lib
    dev = torch.device("cuda:0")
    L, st = _lib.lib(), _lib.stream_of(dev)
    g = torch.randn(numel, device=dev, dtype=torch.bfloat16)
    ptrs, nums = (ctypes.c_void_p * 1)(g.data_ptr()), (ctypes.c_int64 * 1)(numel)
    wsz = L.dgc_grad_stats_workspace(nums, 1)
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    out = torch.empty(1, device=dev)

    def fn():
        _lib.check(L.dgc_grad_stats16(ptrs, nums, 1, 1, _lib.VD[torch.bfloat16], _lib.ptr(out), _lib.ptr(ws), wsz, st),
                   "dgc_grad_stats16")
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / reps
    return {"leg": "stats16", "elements": numel, "ms": round(ms, 4), "tb_per_s": round(2 * numel / ms / 1e9, 3),
            "norm": float(out.item())}


def run_leg(leg, a):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "adam-compression_amd"), REPO, env.get("PYTHONPATH", "")])
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", leg, "--steps",
           str(a.steps), "--warmup", str(a.warmup), "--numel", str(a.numel)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"clip16_bench: leg {leg} ended with {p.returncode}; nothing further is run\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--numel", type=int, default=N)
    ap.add_argument("--rounds", type=int, default=2, help="times the three legs alternate")
    ap.add_argument("--limit", type=int, default=150, help="seconds per child")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        if a.child == "hbm_probe":
            res = _probe_leg()
        elif a.child == "stats16":
            res = _stats_leg(a.numel)
        else:
            res = _bucket_leg(a.child, a.steps, a.warmup, a.numel)
        print(json.dumps(res), flush=True)
        return
    legs = {}
    for leg in ["fused", "aten", "none"] * a.rounds + ["hbm_probe", "stats16"]:
        r = run_leg(leg, a)
        legs.setdefault(leg, []).append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    best = {leg: min(r["ms_median"] for r in legs[leg]) for leg in ("fused", "aten", "none")}
    rate = legs["hbm_probe"][0]["tb_per_s"]
    comp = {leg: min(r["compensate_ms"] for r in legs[leg]) for leg in ("fused", "aten", "none")}
    print(json.dumps({
        "compensate_ms": {leg: [r["compensate_ms"] for r in legs[leg]] for leg in comp},
        "select_ms": {leg: [r["select_ms"] for r in legs[leg]] for leg in comp},
        "branch": {leg: [r["branch"] for r in legs[leg]] for leg in comp},
        "clip_cost_compensate_ms": round(comp["fused"] - comp["none"], 4),
        "elements": a.numel, "fused_ms": [r["ms_median"] for r in legs["fused"]],
        "aten_ms": [r["ms_median"] for r in legs["aten"]], "none_ms": [r["ms_median"] for r in legs["none"]],
        "clip_cost_ms": round(best["fused"] - best["none"], 4), "aten_cost_ms": round(best["aten"] - best["none"], 4),
        "hbm_probe_tb_per_s": rate, "stats_reread_floor_ms": round(2 * a.numel / (rate * 1e9), 4),
        "coef": legs["fused"][0]["coef"], "stats16": legs["stats16"][0]}))


if __name__ == "__main__":
    main()
