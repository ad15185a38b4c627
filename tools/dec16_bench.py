"""The 16-bit receive side, timed on one MI355X: dgc_decompress_packed16 (one allgather's
decompress: a 2-byte zero fill, one read-modify-write launch per rank, a dense scale pass)
against dgc_fill_zero16 + the `parts` phases of dgc_scatter_split16 back to back (the split
exchange's decompress with nothing to wait for: one 16-B-store fill, every index written once).

  python tools/dec16_bench.py [--numel 1e9 7e9] [--W 2 4 8] [--parts P] [--reps 10] [--rounds 5]

bf16 gradient, bf16 wire, int64 indices, capacity ceil(0.001 n) per rank. No collective is
involved: every rank's payload is synthesised on the device (entry j of a rank at a random
offset inside the j-th stride of n / capacity elements: ascending, distinct, ~0.1 % of them
shared with any other rank), split with dgc_payload_split and laid out part-major as the
collectives would leave it. parts defaults to fp32's "auto" (2 at W <= 4, 4 at W = 8).

Each figure is the median over `rounds` rounds, the two paths alternating within a round,
`reps` calls per timing between HIP events after a warm-up call; before any timing the two
outputs are compared bit for bit on the device. One JSON line per (numel, W).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "adam-compression_amd"))

import torch  # noqa: E402

from dgc import _lib  # noqa: E402

BF16, I64 = _lib.VD[torch.bfloat16], _lib.ID[torch.int64]


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bench(L, N, W, P, reps, rounds, dev):
    k = (N + 999) // 1000
    stride, voff, ioff = _lib.payload_layout(k, torch.bfloat16, torch.int64)
    gen = torch.Generator(device=dev).manual_seed(3)
    step = N // k
    pay = torch.zeros(W * stride, dtype=torch.uint8, device=dev)
    for r in range(W):
        row = pay[r * stride:(r + 1) * stride]
        idx = torch.arange(k, device=dev, dtype=torch.int64) * step
        idx += torch.randint(0, step, (k,), device=dev, generator=gen)
        row[:8].view(torch.int64).fill_(k)
        row[voff:voff + 2 * k].view(torch.bfloat16).copy_(torch.randn(k, device=dev, generator=gen))
        row[ioff:ioff + 8 * k].view(torch.int64).copy_(idx)
        del idx
    pc = ctypes.c_int64(0)
    pb = L.dgc_payload_split_layout(k, P, BF16, I64, ctypes.byref(pc))
    split = torch.zeros(L.dgc_payload_split_bytes(k, P, BF16, I64), dtype=torch.uint8, device=dev)
    g = torch.zeros(P * W * pb, dtype=torch.uint8, device=dev)
    s = _lib.stream_of(dev)
    for r in range(W):
        _lib.check(L.dgc_payload_split(pay[r * stride:].data_ptr(), k, P, BF16, I64, split.data_ptr(), s),
                   "dgc_payload_split")
        for p in range(P):
            g[(p * W + r) * pb:(p * W + r + 1) * pb].copy_(split[p * pb:(p + 1) * pb])
    ws = torch.empty(L.dgc_decompress_split16_workspace(N, W, P, k), dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(N, dtype=torch.bfloat16, device=dev)

    def packed16(o=out):
        _lib.check(L.dgc_decompress_packed16(pay.data_ptr(), W, stride, k, BF16, I64, o.data_ptr(), BF16, N, 1.0 / W,
                                             bad.data_ptr(), s), "dgc_decompress_packed16")

    def fill():
        _lib.check(L.dgc_fill_zero16(out.data_ptr(), N, s), "dgc_fill_zero16")

    def phases():
        for p in range(P):
            _lib.check(L.dgc_scatter_split16(g.data_ptr(), W, P, p, k, BF16, I64, out.data_ptr(), BF16, N, 1.0 / W,
                                             ws.data_ptr(), ws.numel(), s), "dgc_scatter_split16")

    def split16():
        fill()
        phases()

    ref = torch.empty(N, dtype=torch.bfloat16, device=dev)   # the results agree before anything is timed
    packed16(ref)
    split16()
    torch.cuda.synchronize()
    st = ctypes.c_int32(-1)
    _lib.check(L.dgc_decompress_status(ws.data_ptr(), ctypes.byref(st), s), "dgc_decompress_status")
    if st.value != 0 or int(bad) != 0 or not torch.equal(ref.view(torch.int16), out.view(torch.int16)):
        raise RuntimeError(f"numel {N} W {W}: the split scatter's result differs from dgc_decompress_packed16's "
                           f"(status {st.value}, bad {int(bad)})")
    written = int(ref.view(torch.int16).count_nonzero())
    del ref
    t = {"packed16_ms": [], "split16_ms": [], "fill16_ms": [], "phases_ms": []}
    for _ in range(rounds):
        t["packed16_ms"].append(timeit(packed16, reps))
        t["split16_ms"].append(timeit(split16, reps))
        t["fill16_ms"].append(timeit(fill, reps))
        fill()
        t["phases_ms"].append(timeit(phases, reps))   # (every phase rewrites the same values)
    res = {"numel": N, "W": W, "parts": P, "capacity": k, "written": written, "reps": reps, "rounds": rounds}
    for name, xs in t.items():
        res[name] = round(statistics.median(xs), 4)
        res[name.replace("_ms", "_spread")] = [round(min(xs), 4), round(max(xs), 4)]
    res["ratio"] = round(res["packed16_ms"] / res["split16_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=float, nargs="*", default=[1e9, 7e9])
    ap.add_argument("--W", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--parts", type=int, default=0, help="0: 2 at W <= 4, 4 at W = 8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dec16_bench: needs the MI355X (nothing is timed on a CPU)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for n in args.numel:
        for W in args.W:
            P = args.parts or (2 if W <= 4 else 4)
            print(json.dumps(bench(L, int(n), W, P, args.reps, args.rounds, dev)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
