"""K6-16, the split exchange onto a bf16 / fp16 gradient (dgc_fill_zero16 +
dgc_scatter_split16): the decompress of dgc/compression.py:179-194 run on a 16-bit tensor,
scattered part by part as the `parts` collectives land.

Single process: W ranks' packed payloads are built in numpy, split on the device
(dgc_payload_split), laid out part-major as the collectives would leave them, and scattered
phase by phase onto a view that starts 2 bytes into a poisoned buffer. Everything is
compared as int16 bits against BOTH
  (a) dgc_decompress_packed16 over the same unsplit payloads (tests/test_gpu_half.py pins it
      to the reference's fixtures), and
  (b) the torch-CPU op sequence zeros(n, dtype).index_put_([idx], vals.to(dtype),
      accumulate=True).mul_(1 / W) in rank order (oracle/torch_cpu.py),
and after every phase but the last each index below the phase's bound already holds its
final value while every index at or above it still holds +0. Each case asserts in numpy, on
its inputs, the property that makes it reach its path.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import torch_cpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F16, BF16 = 0, 1, 2
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
I64MAX = np.iinfo(np.int64).max
POISON = 0x5A5A          # a finite, non-zero pattern in bf16 and fp16
CHUNK = 4096


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    return _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(L, rc):
    assert rc == 0, L.dgc_last_error().decode()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def wire(v, vd):
    """fp32 numpy values as the wire dtype's tensor (round to nearest even, as the selection emits them)."""
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(TORCH[vd])


def rank_payload(L, v, i, cap, vd, idt):
    """One rank's packed payload [count | values(cap) | indices(cap)] on the device."""
    vo, io = ctypes.c_int64(0), ctypes.c_int64(0)
    stride = L.dgc_payload_layout(cap, vd, idt, ctypes.byref(vo), ctypes.byref(io))
    p = np.zeros(stride, np.uint8)
    vb = wire(v, vd).view(torch.int32 if vd == F32 else torch.int16).numpy().view(np.uint8)
    ib = np.ascontiguousarray(i, np.int32 if idt else np.int64).view(np.uint8)
    assert len(i) <= cap
    p[:8] = np.frombuffer(np.int64(len(i)).tobytes(), np.uint8)
    p[vo.value: vo.value + vb.size] = vb
    p[io.value: io.value + ib.size] = ib
    return torch.from_numpy(p).to(DEV), stride


def make_runs(rng, N, W, cap, overlap, common=0, shuffled=(), counts=None, lo=0, hi=None):
    """W runs of exactly counts[r] (default cap) distinct ascending indices in [lo, hi):
    `common` indices are in every run, a share `overlap` of the rest comes from one shared
    pool; a few values are -0.0; the runs in `shuffled` come in a random order."""
    hi = N if hi is None else hi
    space = np.arange(lo, hi)
    pool = np.sort(rng.choice(space, min(cap, hi - lo), replace=False))
    everyone = pool[:: max(1, len(pool) // common)][:common] if common else pool[:0]
    runs = []
    for r in range(W):
        c = cap if counts is None else counts[r]
        assert c == 0 or c >= everyone.size
        own = rng.choice(space, c, replace=False)
        pick = rng.random(c) < overlap
        rest = np.setdiff1d(np.where(pick, pool[:c], own), everyone)[: max(c - everyone.size, 0)]
        idx = np.concatenate([everyone, rest]) if c else rest
        if idx.size < c:   # collisions between the pool's and the rank's own picks: top up
            idx = np.concatenate([idx, rng.choice(np.setdiff1d(space, idx), c - idx.size, replace=False)])
        idx = np.sort(idx).astype(np.int64)
        assert idx.size == c and np.unique(idx).size == c
        v = (rng.standard_normal(idx.size) * 0.25).astype(np.float32)
        v[rng.random(idx.size) < 0.02] = -0.0
        if r in shuffled:
            o = rng.permutation(idx.size)
            v, idx = v[o], idx[o]
        runs.append((v, idx))
    return runs


def occurrences(runs):
    """index -> in how many runs it occurs (indices are distinct within a run)."""
    idx, cnt = np.unique(np.concatenate([i for _, i in runs]), return_counts=True)
    return idx, cnt


def expect_torch(runs, N, W, vd, dt):
    """(b): the reference's op sequence on a CPU tensor of the gradient's dtype."""
    vals = torch.cat([wire(v, vd) for v, _ in runs]).to(TORCH[dt])
    idx = torch.from_numpy(np.concatenate([i for _, i in runs]).astype(np.int64))
    return bits(torch_cpu.decompress(vals, idx, torch.zeros(N, dtype=TORCH[dt]), W))


def expect_packed16(L, runs, N, W, cap, vd, idt, dt):
    """(a): dgc_decompress_packed16 over the unsplit payloads."""
    pays = [rank_payload(L, v, i, cap, vd, idt) for v, i in runs]
    stride = pays[0][1]
    g = torch.cat([p for p, _ in pays])
    out = torch.full((N,), POISON, dtype=torch.int16, device=DEV).view(TORCH[dt])
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    check(L, L.dgc_decompress_packed16(P(g), W, stride, cap, vd, idt, P(out), dt, N, 1.0 / W, P(bad), stream()))
    torch.cuda.synchronize()
    assert int(bad) == 0
    return bits(out)


class Split16:
    """The device side of one case: split, part-major gather, fill and phases onto
    buf[off : off + N] of a poisoned buffer."""

    def __init__(self, L, N, W, parts, cap, vd, idt, dt, off=1):
        self.L, self.N, self.W, self.parts, self.cap, self.vd, self.idt, self.dt = L, N, W, parts, cap, vd, idt, dt
        pc = ctypes.c_int64(0)
        self.pbytes = L.dgc_payload_split_layout(cap, parts, vd, idt, ctypes.byref(pc))
        self.pc = pc.value
        self.split = torch.zeros(L.dgc_payload_split_bytes(cap, parts, vd, idt), dtype=torch.uint8, device=DEV)
        wsz = L.dgc_decompress_split16_workspace(N, W, parts, cap)
        assert wsz > 0
        self.ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
        self.off, self.guard = off, 64
        self.buf = torch.full((off + N + self.guard,), POISON, dtype=torch.int16, device=DEV).view(TORCH[dt])
        self.out = self.buf[off: off + N]
        assert self.out.data_ptr() % 16 == (2 * off) % 16

    def gather(self, runs):
        """Every rank's payload split on the device and placed part-major; the part headers."""
        L, pb, W = self.L, self.pbytes, self.W
        g = torch.zeros(self.parts * W * pb, dtype=torch.uint8, device=DEV)
        heads = []
        for r, (v, i) in enumerate(runs):
            pay, _ = rank_payload(L, v, i, self.cap, self.vd, self.idt)
            check(L, L.dgc_payload_split(P(pay), self.cap, self.parts, self.vd, self.idt, P(self.split), stream()))
            for p in range(self.parts):
                g[(p * W + r) * pb: (p * W + r + 1) * pb].copy_(self.split[p * pb: (p + 1) * pb])
            heads.append(self.split[: self.parts * pb].view(self.parts, pb)[:, :16].clone().view(torch.int64)
                         .cpu().numpy())
        return g, heads

    def bounds(self, runs):
        """Phase p's bound from the inputs: min over ranks of the smallest index after part p."""
        b = []
        for p in range(self.parts - 1):
            later = [i[(p + 1) * self.pc:] for _, i in runs]
            b.append(min([int(x.min()) for x in later if x.size] or [I64MAX]))
        return b

    def fill(self):
        check(self.L, self.L.dgc_fill_zero16(P(self.out), self.N, stream()))

    def phase(self, g, p):
        check(self.L, self.L.dgc_scatter_split16(P(g), self.W, self.parts, p, self.cap, self.vd, self.idt, P(self.out),
                                                 self.dt, self.N, 1.0 / self.W, P(self.ws), self.ws.numel(), stream()))

    def run(self, g, want=None, bounds=None):
        """fill + the phases; with `want`, the per-phase check: final below the bound, +0 from it on."""
        self.fill()
        for p in range(self.parts):
            self.phase(g, p)
            if want is not None and p < self.parts - 1:
                torch.cuda.synchronize()
                o, b = bits(self.out), min(bounds[p], self.N)
                assert np.array_equal(o[:b], want[:b]), f"phase {p}: an index below its bound {b} is not final"
                assert not o[b:].any(), f"phase {p}: an index at or above its bound {b} was written"
        torch.cuda.synchronize()
        self.untouched_around()
        return bits(self.out)

    def untouched_around(self):
        o = self.buf.view(torch.int16).cpu().numpy()
        assert (o[: self.off] == POISON).all(), "wrote before out"
        assert (o[self.off + self.N:] == POISON).all(), "wrote past out"

    def status(self):
        st = ctypes.c_int32(-1)
        check(self.L, self.L.dgc_decompress_status(P(self.ws), ctypes.byref(st), stream()))
        return st.value


def run_case(L, runs, N, W, parts, cap, vd, idt, dt, status=0, off=1):
    """The whole check of one case; returns (Split16, gathered, bounds, expected bits)."""
    sp = Split16(L, N, W, parts, cap, vd, idt, dt, off)
    g, heads = sp.gather(runs)
    bounds = sp.bounds(runs)
    for p in range(parts - 1):   # the device's headers say the same
        assert min(int(h[p, 1]) for h in heads) == bounds[p]
    assert all(a <= b for a, b in zip(bounds, bounds[1:]))
    want = expect_torch(runs, N, W, vd, dt)
    assert np.array_equal(expect_packed16(L, runs, N, W, cap, vd, idt, dt), want), "the two references differ"
    got = sp.run(g, want, bounds)
    assert sp.status() == status
    assert np.array_equal(got, want)
    return sp, g, bounds, want


# ---------------------------------------------------------------- the phase scatter
def test_many_ranks_ragged_capacity_duplicates(L):
    """W = 8, 8 parts of a ragged capacity (1001 = 7 * 126 + 119), bf16 on a bf16 wire."""
    N, W, parts, cap = 1_000_003, 8, 8, 1001
    rng = np.random.default_rng(816)
    counts = [int(c) for c in rng.integers(cap // 2, cap + 1, W)]
    counts[-1] = cap
    runs = make_runs(rng, N, W, cap, 0.3, common=16, counts=counts)
    _, cnt = occurrences(runs)
    assert (cnt >= 2).any() and (cnt == W).any() and (cnt == 1).any()
    assert cap % parts and N % 2 and N % CHUNK
    run_case(L, runs, N, W, parts, cap, BF16, 0, BF16)


@pytest.mark.parametrize("parts", [2, 4])
@pytest.mark.parametrize("dt,vd,idt", [(F16, F16, 0), (BF16, F16, 1), (BF16, F32, 0)],
                         ids=["fp16-fp16wire", "bf16-fp16wire-int32", "bf16-fp32wire"])
def test_other_dtypes_and_wires(L, parts, dt, vd, idt):
    N, W, cap = 300_001, 4, 1500
    rng = np.random.default_rng(41 + parts + 7 * dt + vd)
    runs = make_runs(rng, N, W, cap, 0.4, common=8)
    _, cnt = occurrences(runs)
    assert (cnt == W).any() and (cnt == 1).any()
    if vd != dt:   # values.type(dtype) rounds: some wire value is not a value of the gradient's dtype
        v = torch.cat([wire(v, vd) for v, _ in runs])
        assert not torch.equal(v.to(TORCH[dt]).to(v.dtype), v)
    run_case(L, runs, N, W, parts, cap, vd, idt, dt)


def test_rounding_order_is_the_rank_order_fold(L):
    """W = 3, bf16, every rank the same indices. Index 0 holds 1.0, 2^-8, 2^-8 in rank
    order: rd(rd(1 + 2^-8) + 2^-8) = 1 but 1 + rd(2^-8 + 2^-8) = 1 + 2^-7. The other indices
    hold triples found on the host for which the fold, any other order of it, and a sum
    kept in fp32 and rounded once after the scale all differ in some way."""
    N, W, parts, bf = 10_007, 3, 2, torch.bfloat16
    a, b, c = (torch.tensor([x], dtype=bf) for x in (1.0, 2.0 ** -8, 2.0 ** -8))
    assert not torch.equal((a + b) + c, a + (b + c))
    rng = np.random.default_rng(3)
    t = torch.from_numpy(rng.standard_normal((3, 20000)).astype(np.float32)).to(bf)
    fold = (t[0] + t[1]) + t[2]                              # every add rounded to bf16, rank order
    other = t[0] + (t[1] + t[2])
    s = 1.0 / W
    once = ((t[0].float() + t[1].float() + t[2].float()) * s).to(bf)   # fp32 throughout, one rounding
    twice = fold.clone().mul_(s)
    order = (fold != other).nonzero().view(-1)[:40]
    scale = ((twice != once) & (fold == other)).nonzero().view(-1)[:40]
    assert order.numel() == 40 and scale.numel() == 40
    pick = torch.cat([order, scale])
    vals = torch.cat([torch.stack([a, b, c]).view(3, 1), t[:, pick]], 1).float().numpy()
    cap = vals.shape[1]
    idx = np.concatenate([[0], 1 + np.sort(rng.choice(N - 1, cap - 1, replace=False))]).astype(np.int64)
    runs = [(vals[r], idx) for r in range(W)]
    want = expect_torch(runs, N, W, BF16, BF16)
    # the expectation itself tells the orders apart: it is not what the reversed rank order gives
    assert not np.array_equal(want, expect_torch(runs[::-1], N, W, BF16, BF16))
    assert want[0] == bits(torch.tensor([1.0], dtype=bf).mul_(s))[0]
    run_case(L, runs, N, W, parts, cap, BF16, 0, BF16)


def test_crowded_chunk_takes_the_workgroup_path(L):
    """Every rank's 3000 entries inside one 4096-element chunk: whatever super-chunk size
    the host picks (1..64 chunks), the one holding that chunk has > 64 entries, so it is
    queued for the workgroup path — in both phases, the bound falling inside the chunk."""
    N, W, parts, cap = 200_000, 4, 2, 3000
    c0 = 17
    rng = np.random.default_rng(5)
    runs = make_runs(rng, N, W, cap, 0.5, common=8, lo=c0 * CHUNK, hi=(c0 + 1) * CHUNK)
    allidx = np.concatenate([i for _, i in runs])
    assert ((allidx // CHUNK) == c0).all() and allidx.size == W * cap > 64
    sp = Split16(L, N, W, parts, cap, BF16, 0, BF16)
    b = sp.bounds(runs)[0]
    assert c0 * CHUNK < b < (c0 + 1) * CHUNK                      # the window edge cuts the chunk
    assert min((i[: sp.pc] < b).sum() for _, i in runs) > 64      # > 64 entries on either side of it
    assert min((i >= b).sum() for _, i in runs) > 64
    run_case(L, runs, N, W, parts, cap, BF16, 0, BF16)


def test_unsorted_run_is_regrouped(L):
    """One rank's payload in a shuffled (topk) order: status bit 1, the same sums."""
    N, W, parts, cap = 300_001, 2, 2, 1000
    rng = np.random.default_rng(12)
    runs = make_runs(rng, N, W, cap, 0.5, common=8, shuffled=(1,))
    assert (np.diff(runs[0][1]) > 0).all() and (np.diff(runs[1][1]) < 0).any()
    run_case(L, runs, N, W, parts, cap, BF16, 0, BF16, status=2)


@pytest.mark.parametrize("counts", [(1, 5), (0, 7), (0, 0)], ids=["one-entry", "empty-rank", "all-empty"])
def test_fewer_entries_than_parts(L, counts):
    N, W, parts, cap = 50_000, 2, 2, 7
    rng = np.random.default_rng(sum(counts))
    runs = make_runs(rng, N, W, cap, 0.0, counts=list(counts))
    assert [len(i) for _, i in runs] == list(counts) and min(counts) < parts
    run_case(L, runs, N, W, parts, cap, F16, 0, F16)


def test_identical_runs_give_every_phase_a_window(L):
    """All ranks' indices ascending and identical: the bounds strictly increase, so each of
    the 8 phases has a non-empty window, and each writes entries into it."""
    N, W, parts, cap = 1_000_003, 8, 8, 1001
    rng = np.random.default_rng(88)
    idx = np.sort(rng.choice(N, cap, replace=False)).astype(np.int64)
    runs = [((rng.standard_normal(cap) * 0.25).astype(np.float32), idx) for _ in range(W)]
    sp, g, bounds, want = run_case(L, runs, N, W, parts, cap, BF16, 0, BF16)
    edges = [0] + bounds + [N]
    assert all(a < b for a, b in zip(edges, edges[1:]))
    for a, b in zip(edges, edges[1:]):
        assert ((idx >= a) & (idx < b)).sum() == (sp.pc if b < N else cap - (parts - 1) * sp.pc)


def test_empty_windows(L):
    """Rank 1 comes shuffled with its smallest index in its last part, so phases 0, 1 and 2
    share one bound: the windows of phases 1 and 2 are empty and everything above the bound
    waits for the last phase."""
    N, W, parts, cap = 300_001, 2, 4, 400
    rng = np.random.default_rng(21)
    runs = make_runs(rng, N, W, cap, 0.3, common=4, shuffled=(1,))
    v, i = runs[1]
    j = int(i.argmin())
    v[[j, -1]], i[[j, -1]] = v[[-1, j]], i[[-1, j]]
    sp = Split16(L, N, W, parts, cap, BF16, 0, BF16)
    b = sp.bounds(runs)
    assert b[0] == b[1] == b[2] == i.min() and (np.concatenate([x for _, x in runs]) > b[0]).sum() > W * cap // 2
    run_case(L, runs, N, W, parts, cap, BF16, 0, BF16, status=2)


@pytest.mark.parametrize("off", [0, 3, 7])
def test_out_view_offsets(L, off):
    """out at 0, 6 and 14 bytes past a 16-B boundary (the other cases run at 2), n odd."""
    N, W, parts, cap = 70_001, 2, 2, 700
    runs = make_runs(np.random.default_rng(off), N, W, cap, 0.3, common=4)
    assert N % 2 and N % 8 and N % CHUNK
    run_case(L, runs, N, W, parts, cap, BF16, 0, BF16, off=off)


def test_indices_past_2_31(L):
    """n = 2^31 + 4099: element offsets that do not fit an int32, entries on both sides of
    2^31 and at n - 1. The outputs stay on the device: compared whole against
    dgc_decompress_packed16's, at the entries against the torch-CPU sums of the compacted
    indices (the same entries in the same order, so the same folds)."""
    N, W, parts, cap = 2 ** 31 + 4099, 2, 2, 2000
    rng = np.random.default_rng(31)
    runs = []
    for r in range(W):
        idx = np.unique(np.concatenate([rng.integers(0, 1 << 20, 900), 2 ** 31 - 2000 + rng.integers(0, 6099, 900),
                                        [0, 2 ** 31 - 1, 2 ** 31, N - 1]]))[:cap].astype(np.int64)
        runs.append(((rng.standard_normal(idx.size) * 0.25).astype(np.float32), idx))
    every = np.unique(np.concatenate([i for _, i in runs]))
    assert every[-1] == N - 1 and (every >= 2 ** 31).sum() > 100 and (occurrences(runs)[1] == W).sum() >= 4
    compact = [(v, np.searchsorted(every, i)) for v, i in runs]
    want = torch.from_numpy(expect_torch(compact, every.size, W, BF16, BF16)).to(DEV)
    sp = Split16(L, N, W, parts, cap, BF16, 0, BF16)
    g, _ = sp.gather(runs)
    b = sp.bounds(runs)[0]
    assert 2 ** 31 - 2000 <= b < N          # phase 0 stops inside the high group, phase 1 writes past 2^31

    pays = [rank_payload(L, v, i, cap, BF16, 0) for v, i in runs]
    ref = torch.full((N,), POISON, dtype=torch.int16, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    check(L, L.dgc_decompress_packed16(P(torch.cat([p for p, _ in pays])), W, pays[0][1], cap, BF16, 0, P(ref), BF16, N,
                                       1.0 / W, P(bad), stream()))
    out = sp.out.view(torch.int16)
    sp.fill()
    sp.phase(g, 0)
    torch.cuda.synchronize()
    assert torch.equal(out[:b], ref[:b]) and not bool(out[b:].any())
    sp.phase(g, 1)
    torch.cuda.synchronize()
    assert int(bad) == 0 and sp.status() == 0
    assert torch.equal(out, ref)
    at = torch.from_numpy(every).to(DEV)
    assert torch.equal(out[at], want) and int(out.count_nonzero()) == int(want.count_nonzero())
    edge = sp.buf.view(torch.int16)
    assert bool((edge[: sp.off] == POISON).all()) and bool((edge[sp.off + N:] == POISON).all())


# ---------------------------------------------------------------- the fill
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 17, 4095, 4097, 1_000_003])
@pytest.mark.parametrize("off", [0, 1, 3, 7])
def test_fill_zero16(L, n, off):
    """+0 over exactly [0, n) of a view `off` elements past a 16-B boundary; the poisoned
    neighbours on both sides stay."""
    buf = torch.full((off + n + 64,), POISON, dtype=torch.int16, device=DEV)
    assert buf.data_ptr() % 16 == 0
    check(L, L.dgc_fill_zero16(P(buf[off:]), n, stream()))
    torch.cuda.synchronize()
    o = buf.cpu().numpy()
    assert (o[:off] == POISON).all() and (o[off + n:] == POISON).all()
    assert not o[off: off + n].any()


# ---------------------------------------------------------------- corruption
KINDS = ["index-past-n", "index-negative", "count-past-capacity", "count-negative"]


@pytest.mark.parametrize("kind", KINDS)
def test_corrupt_part_is_reported_and_dropped(L, kind):
    """Rank 1's part-0 buffer corrupted as it landed: a bad index is dropped (status bit 0,
    sink word 0), a bad count clamped (bit 2, sink word 1); the rest of the output is the
    expectation without the bad entry; a healthy call after the report is clean."""
    from dgc import _lib
    N, W, parts, cap = 300_001, 2, 2, 3000
    rng = np.random.default_rng(9)
    runs = make_runs(rng, N, W, cap, 0.3, common=8)
    sp = Split16(L, N, W, parts, cap, BF16, 0, BF16)
    assert len(runs[1][1]) == cap and sp.pc * parts == cap     # part 0 of rank 1 is full: a clamp keeps all of it
    g, _ = sp.gather(runs)
    sink = _lib.StatusSink("split16", DEV)
    sink.bind(sp.ws)
    want = expect_torch(runs, N, W, BF16, BF16)
    assert np.array_equal(sp.run(g), want) and sp.status() == 0
    sink.check()

    io = ctypes.c_int64(0)
    L.dgc_payload_layout(sp.pc, BF16, 0, None, ctypes.byref(io))
    part0 = g[sp.pbytes: 2 * sp.pbytes]                        # part 0 of rank 1
    bad, (v1, i1) = g.clone(), runs[1]
    part0_bad = bad[sp.pbytes: 2 * sp.pbytes]
    if kind.startswith("index"):                               # its first entry's index
        part0_bad[io.value: io.value + 8].view(torch.int64).fill_(N + 5 if kind == "index-past-n" else -3)
        left = [runs[0], (v1[1:], i1[1:])]
    elif kind == "count-past-capacity":
        part0_bad[:8].view(torch.int64).fill_(sp.pc + 3)
        left = runs
    else:
        part0_bad[:8].view(torch.int64).fill_(-2)
        left = [runs[0], (v1[sp.pc:], i1[sp.pc:])]
    assert not torch.equal(part0_bad, part0)
    want_bad = expect_torch(left, N, W, BF16, BF16)
    assert np.array_equal(expect_packed16(L, left, N, W, cap, BF16, 0, BF16), want_bad)
    got = sp.run(bad)
    assert sp.status() & 5 == (1 if kind.startswith("index") else 4)
    assert np.array_equal(got, want_bad)
    words = sink.word.numpy()
    assert (words[1] != 0, words[2] != 0) == (kind.startswith("index"), kind.startswith("count"))
    with pytest.raises(RuntimeError, match="outside the gradient" if kind.startswith("index") else "count outside"):
        sink.check()
    assert np.array_equal(sp.run(g), want) and sp.status() == 0   # the report cleared the words
    sink.check()
