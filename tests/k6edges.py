"""K6 design inputs: gathered payloads whose entries sit on an edge of the decompress
(csrc/decompress.hip), with the path every one of them takes stated as data (CPU only, numpy;
``arena`` alone touches torch).

K6 turns W rank-ordered runs of (value, index) into ``zero_().index_put_(accumulate=True)
.mul_(1/W)``. The host picks a super-chunk of ``m`` 4096-element chunks and the whole-granule
store from ``4096 * W * capacity / n``; ``k_bounds`` marks every run's first entry per chunk (a
thread per entry, the wave for an entry that owns more than 8 chunks, a grid-stride sweep per
262 144 entries); a wave takes a super-chunk of at most 64 entries (lane order = rank order, a
cross-rank duplicate summed by its first lane, an entry alone in its 64-B granule written as a
granule), the others go to ``tile_chunk`` in batches of 1024 staged entries; a run out of order
is regrouped by chunk first; one run alone takes ``k_scatter_single`` (four threads per entry,
whole granules behind the header's DGC_ORDER_ASCENDING word).

In the style of k5sets.py / k3edges.py:

``route(n, W, cap, runs, form)``
    ``run_scatter``'s host routing and the device's routing per super-chunk, restated so that
    they only classify; ``.status`` is the ``dgc_decompress_status`` word they leave.
``pack`` / ``arena``
    a packed gathered buffer with a canary (NaN values, index 0) past every count, and an
    output view ``lead`` floats past a 256-B boundary between NaN guards.
``ROWS``
    the table tests/test_k6_edges_cpu.py confirms and tests/test_gpu_k6_edges.py runs; every
    row states its route and the counts it was designed for. Expected outputs never come from
    here: they are ``oracle.dgc_oracle.decompress``'s.
"""
import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

from oracle import dgc_oracle as O

F32, F16, I64, I32, U32 = np.float32, np.float16, np.int64, np.int32, np.uint32

# Copies of the kernels' constants (test_k6_edges_cpu.py reads the constexpr lines and fails when
# one drifts).
K_CHUNK = 4096            # elements per chunk
K_MAX_RUNS = 64
K_SCB = 4                 # super-chunks per wave iteration
K_GRANULES = 256          # per-wave granule counters
K_TILE_STAGE = 1024       # entries staged per batch of the workgroup path
K_REGROUP_THREADS = 1024
K_BLOCK = 256
K_MAX_GRID = 2048
K_MAX_PARTS = 8
ORDER_ASCENDING = 0x444E454353413147   # include/dgc_hip.h: DGC_ORDER_ASCENDING

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "adam-compression_amd" / "csrc"
CONSTANTS = {   # name -> (file, our copy)
    "kChunk": ("decompress.hip", K_CHUNK),
    "kMaxRuns": ("decompress.hip", K_MAX_RUNS),
    "kSCB": ("decompress.hip", K_SCB),
    "kGranules": ("decompress.hip", K_GRANULES),
    "kTileStage": ("decompress.hip", K_TILE_STAGE),
    "kRegroupThreads": ("decompress.hip", K_REGROUP_THREADS),
    "kMaxParts": ("decompress.hip", K_MAX_PARTS),
    "kBlock": ("dgc_common.hpp", K_BLOCK),
}
BOUNDS_SWEEP = K_BLOCK * K_MAX_GRID // 2     # k_bounds: entries (and the sentinel) per sweep
CLEAR_SWEEP = K_BLOCK * K_MAX_GRID // 2 // 4  # k_clear_packed: entries per sweep (4 threads each)
DESCENT_SWEEP = K_BLOCK * K_MAX_GRID         # k_find_descents: positions per sweep
WS_WORDS = K_MAX_RUNS * 24                   # carve_dec: Run[64] at 24 B, then nruns, status, ndesc, ovf_cnt
INT64_MAX = np.iinfo(np.int64).max


def header_constant(name):
    """The value of ``name = <integer>`` on a constexpr line of the file CONSTANTS names."""
    text = (CSRC / CONSTANTS[name][0]).read_text()
    m = [v for line in text.splitlines() if re.match(r"\s*constexpr\b", line)
         for v in re.findall(r"\b%s\s*=\s*(\d+)\s*[,;]" % re.escape(name), line)]
    assert len(m) == 1, f"{name}: {len(m)} constexpr definitions in {CONSTANTS[name][0]}"
    return int(m[0])


def header_order_word():
    text = (ROOT / "include" / "dgc_hip.h").read_text()
    return int(re.search(r"#define\s+DGC_ORDER_ASCENDING\s+(0x[0-9A-Fa-f]+)LL", text).group(1), 16)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the route
class Route(tuple):
    """``("single", gran)`` or ``("waves", m, gran, nsc, overflowed, unsorted, sweeps)``; compares
    as the tuple, and carries the status word the call leaves."""
    status = 0


def descends(idx):
    idx = np.asarray(idx, I64)
    return bool(idx.size > 1 and np.any(idx[1:] < idx[:-1]))


def in_range(i, n):
    i = np.asarray(i, I64)
    return (i >= 0) & (i < n)


def super_totals(n, m, runs):
    """T per super-chunk: sum over the runs of min(entries in it, 65) (k_scatter_waves' clamp). An
    index outside [0, n) belongs to no chunk (k_bounds ranks it before the first / after the last)."""
    nsc = ceil_div(ceil_div(n, K_CHUNK), m)
    T = np.zeros(nsc, I64)
    for _, i in runs:
        i = np.asarray(i, I64)
        i = i[in_range(i, n)]
        T += np.minimum(np.bincount(i // (K_CHUNK * m), minlength=nsc), 65)
    return T


def route(n, W, cap, runs, form="packed"):
    """What K6 does with ``runs`` = [(values, indices)] of W ranks at capacity ``cap``.
    form: ``packed`` (header word 1 = 0), ``ascending`` (header word 1 = DGC_ORDER_ASCENDING) or
    ``table`` (dgc_decompress with run offsets: the schedule is sized by the total, not W * cap)."""
    assert len(runs) == W and 1 <= W <= K_MAX_RUNS
    unsorted = tuple(int(descends(i)) for _, i in runs)
    bad = 0 if all(in_range(i, n).all() for _, i in runs) else 1   # status bit 0: an index outside [0, n)
    if W == 1:
        r = Route(("single", form == "ascending"))
        r.status = (2 if unsorted[0] else 0) | bad
        return r
    total = sum(len(i) for _, i in runs)
    entries, run_cap = (total, total) if form == "table" else (W * cap, cap)
    per_chunk = float(K_CHUNK) * float(entries) / float(n)
    m = 1
    while m < 64 and per_chunk * (2 * m) <= 32.0:
        m *= 2
    gran = per_chunk >= 24.0
    T = super_totals(n, m, runs)
    r = Route(("waves", m, gran, int(T.size), tuple(int(s) for s in np.flatnonzero(T > 64)), unsorted,
               ceil_div(run_cap + 1, BOUNDS_SWEEP)))
    r.status = (2 if any(unsorted) else 0) | bad
    return r


def waves(m, gran, nsc, ovf=(), unsorted=None, sweeps=1, W=2):
    """A stated multi-run route."""
    return ("waves", m, bool(gran), nsc, tuple(ovf), tuple(unsorted) if unsorted is not None else (0,) * W, sweeps)


# ------------------------------------------------------------------ payloads and outputs
def layout(cap, vd, idt):
    """dgc_payload_layout restated: (rank stride, values offset, indices offset)."""
    vb, ib = (2 if vd else 4), (4 if idt else 8)
    ioff = (16 + cap * vb + 15) // 16 * 16
    return (ioff + cap * ib + 255) // 256 * 256, 16, ioff


def pack(runs, cap, vd, idt, ascending=False, tail=True):
    """The gathered buffer of ``runs`` as uint8: per rank [count, word 1 | values(cap) |
    indices(cap)]. word 1 is DGC_ORDER_ASCENDING when ``ascending``. tail: the slots past each
    count hold a canary — NaN values, index 0 — so a kernel that reads past ``count`` shows in
    out[0]."""
    stride, vo, io = layout(cap, vd, idt)
    vt, it = (F16 if vd else F32), (I32 if idt else I64)
    buf = np.zeros(len(runs) * stride, np.uint8)
    for r, (v, i) in enumerate(runs):
        c = len(i)
        assert c <= cap and len(v) == c
        vv = np.full(cap, np.nan if tail else 0.0, vt)
        ii = np.zeros(cap, it)
        vv[:c] = np.asarray(v).astype(vt)
        ii[:c] = np.asarray(i).astype(it)
        base = r * stride
        head = np.array([c, ORDER_ASCENDING if ascending else 0], I64)
        buf[base: base + 16] = head.view(np.uint8)
        buf[base + vo: base + vo + vv.nbytes] = vv.view(np.uint8)
        buf[base + io: base + io + ii.nbytes] = ii.view(np.uint8)
    return buf


def carve(n, max_runs, sort_cap=0):
    """carve_dec restated: the byte offset of every area of the decompress workspace (each take
    starts on a 256-B boundary) and the workspace's size. ``words``: nruns, status, ndesc, ovf_cnt."""
    nch = ceil_div(n, K_CHUNK)
    takes = (("runs", K_MAX_RUNS * 24), ("words", 16), ("desc", K_MAX_RUNS * 8), ("bnd", max_runs * (nch + 1) * 8),
             ("ovf_list", nch * 4), ("unsorted", K_MAX_RUNS * 4), ("sorted", K_MAX_RUNS * 24),
             ("cursor", max_runs * nch * 4 if sort_cap else 0), ("sort_buf", max_runs * sort_cap * 12 if sort_cap else 0))
    off, at = {}, 0
    for name, size in takes:
        at = (at + 255) // 256 * 256
        off[name] = at
        at += size
    off["bytes"] = (at + 255) // 256 * 256
    return off


GUARD = 64


class Arena:
    """``out``: n floats starting ``lead`` floats past a 256-B boundary of a NaN-filled buffer,
    at least GUARD floats of guard on each side."""

    def __init__(self, n, lead, device=None):
        import torch
        self.torch = torch
        self.buf = torch.full((n + lead + 2 * GUARD + 128,), float("nan"), dtype=torch.float32, device=device)
        first = self.buf.data_ptr() + 4 * GUARD
        base = (first + 255) // 256 * 256
        self.start = (base - self.buf.data_ptr()) // 4 + lead
        self.n, self.lead = n, lead
        self.out = self.buf[self.start: self.start + n]
        assert (self.out.data_ptr() - 4 * lead) % 256 == 0 and self.start >= GUARD
        assert self.buf.numel() - (self.start + n) >= GUARD

    def guards_intact(self):
        t = self.torch
        return bool(t.isnan(self.buf[: self.start]).all()) and bool(t.isnan(self.buf[self.start + self.n:]).all())


def arena(n, lead, device=None):
    return Arena(n, lead, device)


def same_bits(got, want):
    """Bit patterns equal; where the reference holds a NaN, any NaN (IEEE 754 leaves the sign and
    payload of a generated NaN to the implementation: inf + -inf is 0xFFC00000 on the x86 host
    that computes the reference and 0x7FC00000 on the device)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(got.view(U32)[~nan], want.view(U32)[~nan]) and np.all(np.isnan(got[nan])))


# ------------------------------------------------------------------ rows
Row = namedtuple("Row", "name group n W cap form runs route status claims fp16 int32 scale leads prev order parts")
ROWS = []
LEADS3 = (0, 1, 3)
LEADS5 = (0, 1, 3, 4, 15)


def _row(name, group, n, W, cap, runs, rt, *, form="packed", status=0, claims=None, fp16=False, int32=False,
         scale=None, leads=(0,), prev=None, order=False, parts=0):
    assert name not in {r.name for r in ROWS}, name
    ROWS.append(Row(name, group, n, W, cap, form, runs, rt, status, claims or {}, fp16, int32,
                    (1.0 / W) if scale is None else scale, leads, prev, order, parts))


def seeded(idx, r, salt=0):
    """Values for the indices of run r: seeded normals (every sum's order shows in fp32)."""
    return np.random.default_rng([r, salt, len(idx)]).standard_normal(len(idx)).astype(F32)


def _norm(runs, salt=0):
    out = []
    for r, x in enumerate(runs):
        if isinstance(x, tuple):
            v, i = x
            out.append((np.asarray(v, F32), np.asarray(i, I64)))
        else:
            i = np.asarray(x, I64)
            out.append((seeded(i, r, salt), i))
    return out


@functools.lru_cache(maxsize=None)
def build(name):
    """The row's runs: [(values fp32, indices int64)] in rank order (values already on the wire's
    grid for fp16 rows)."""
    r = ROW_BY_NAME[name]
    runs = _norm(r.runs())
    if r.fp16:
        with np.errstate(over="ignore"):
            runs = [(v.astype(F16).astype(F32), i) for v, i in runs]
    for v, i in runs:
        v.setflags(write=False)
        i.setflags(write=False)
    return tuple(runs)


def oracle_of(runs, n, scale):
    """oracle.dgc_oracle.decompress at this scale (1: the Sum op; 1/k: Average over k ranks)."""
    keep = [in_range(i, n) for _, i in runs]   # an index outside [0, n) is dropped from the sum (and flagged)
    vals, idxs = [v[k] for (v, _), k in zip(runs, keep)], [i[k] for (_, i), k in zip(runs, keep)]
    k = 1 if scale == 1.0 else int(round(1.0 / scale))
    assert F32(1.0 / k) == F32(scale)
    with np.errstate(over="ignore", invalid="ignore"):   # the rows with inf and NaN entries
        return O.decompress(vals, idxs, n, k, average=scale != 1.0)


@functools.lru_cache(maxsize=None)
def want(name):
    r = ROW_BY_NAME[name]
    w = oracle_of(build(name), r.n, r.scale)
    w.setflags(write=False)
    return w


def default_prev(name):
    """A previous step's payload for the re-zero forms: per rank every other index of the row, the
    others moved by 17, and both ends of the buffer — ascending, below capacity."""
    r = ROW_BY_NAME[name]
    out = []
    for q, (_, i) in enumerate(build(name)):
        i = np.sort(i[in_range(i, r.n)])
        p = np.unique(np.concatenate([i[::2], (i[1::2] + 17) % r.n, np.array([0, r.n - 1] if q == 0 else [], I64)]))
        p = p[: max(0, r.cap - 1)].astype(I64)
        out.append((seeded(p, q, 7) + F32(3.0), p))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def prev_of(name):
    r = ROW_BY_NAME[name]
    prev = tuple(_norm(r.prev(), 7)) if r.prev else default_prev(name)
    return tuple((v.astype(F16).astype(F32), i) for v, i in prev) if r.fp16 else prev


def spread(lo, hi, k, seed):
    """k distinct indices of [lo, hi), both ends among them from k = 2 on."""
    if k == 0:
        return np.zeros(0, I64)
    if k == 1:
        return np.array([lo + (hi - lo) // 3], I64)
    inner = np.random.default_rng(seed).choice(hi - lo - 2, k - 2, replace=False) + lo + 1
    return np.sort(np.concatenate([[lo, hi - 1], inner])).astype(I64)


def occupy(n, m, W, per_sc, seed=1):
    """Runs with per_sc[s] = (entries of run 0, of run 1, ...) in super-chunk s, all indices
    distinct, the first and last element of every occupied super-chunk among them."""
    span = K_CHUNK * m
    parts = [[] for _ in range(W)]
    for s, counts in sorted(per_sc.items()):
        counts = tuple(counts) + (0,) * (W - len(counts))
        lo, hi = s * span, min((s + 1) * span, n)
        pts = spread(lo, hi, sum(counts), seed + s)
        pts = pts[np.random.default_rng(seed + 1000 + s).permutation(pts.size)]
        at = 0
        for r, c in enumerate(counts):
            parts[r].append(np.sort(pts[at: at + c]))
            at += c
    return [np.concatenate(p).astype(I64) if p else np.zeros(0, I64) for p in parts]


def rand_idx(n, k, seed):
    """k distinct seeded indices of [0, n), ascending."""
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False)).astype(I64)


def cat(*a):
    return np.concatenate([np.asarray(x, I64).reshape(-1) for x in a]).astype(I64)


N100 = K_CHUNK * 100

# --- 1. host thresholds: W = 2, n = 4096 * 100, per_chunk = cap / 50 -------------------------
# m: 40 + 40 entries in the two halves of a would-be super-chunk overflow it (T = 80) at the
# larger m and fit two waves (T = 40 each) at the smaller: the overflow count tells m.
def _halves(m_big):
    return lambda: occupy(N100, m_big // 2, 2, {0: (20, 20), 1: (20, 20)})


_row("thr_pc0.5_m64", 1, N100, 2, 25, lambda: occupy(N100, 32, 2, {0: (12, 12), 1: (13, 13)}), waves(64, 0, 2),
     claims={"T": {0: 50}})
_row("thr_pc0.52_m32", 1, N100, 2, 26, lambda: occupy(N100, 32, 2, {0: (12, 12), 1: (13, 13)}), waves(32, 0, 4),
     claims={"T": {0: 24, 1: 26}})
# capacity 25 cannot hold 40 + 40: the pair at the capacities next to the m = 64 edge of a larger n
N800 = K_CHUNK * 800
_row("thr_pc0.5_m64_ovf", 1, N800, 2, 200, lambda: occupy(N800, 32, 2, {0: (20, 20), 1: (20, 20)}),
     waves(64, 0, 13, ovf=(0,)), claims={"T": {0: 80}})
_row("thr_pc0.5025_m32", 1, N800, 2, 201, lambda: occupy(N800, 32, 2, {0: (20, 20), 1: (20, 20)}),
     waves(32, 0, 25), claims={"T": {0: 40, 1: 40}})
_row("thr_pc16_m2", 1, N100, 2, 800, _halves(2), waves(2, 0, 50, ovf=(0,)), claims={"T": {0: 80}})
_row("thr_pc16.02_m1", 1, N100, 2, 801, _halves(2), waves(1, 0, 100), claims={"T": {0: 40, 1: 40}})
_row("thr_pc23.98_gran_off", 1, N100, 2, 1199, lambda: occupy(N100, 1, 2, {0: (20, 20), 5: (1, 0), 99: (3, 2)}),
     waves(1, 0, 100))
_row("thr_pc24_gran_on", 1, N100, 2, 1200, lambda: occupy(N100, 1, 2, {0: (20, 20), 5: (1, 0), 99: (3, 2)}),
     waves(1, 1, 100))

# --- 2. super-chunk occupancy at m = 1, 4, 64 --------------------------------------------------
SHAPES = {1: (N100, 1000, 100), 4: (N100, 300, 25), 64: (N800, 200, 13)}   # m -> (n, cap, nsc)
for _m, (_n, _cap, _nsc) in SHAPES.items():
    # T = 1, 63, 64, 65, 0: the overflowed super-chunk 3 shares its wave's group of kSCB with 0-2
    _row(f"occ_T_m{_m}", 2, _n, 2, _cap, functools.partial(occupy, _n, _m, 2, {0: (1, 0), 1: (32, 31), 2: (32, 32),
                                                                                3: (33, 32), 5: (0, 1)}),
         waves(_m, 0, _nsc, ovf=(3,)), claims={"T": {0: 1, 1: 63, 2: 64, 3: 65, 4: 0, 5: 1}}, leads=LEADS3)
    # 64 of one run; 66 of one run (the clamp at 65); 40 + 40; 64 of the other run
    _row(f"occ_one_run_m{_m}", 2, _n, 2, _cap,
         functools.partial(occupy, _n, _m, 2, {0: (64, 0), 1: (66, 0), 2: (40, 40), 3: (0, 64)}),
         waves(_m, 0, _nsc, ovf=(1, 2)), claims={"T": {0: 64, 1: 65, 2: 80, 3: 64}}, leads=LEADS3)
# nsc % 4 = 0, 1, 2, 3: the last group of kSCB partial, its last super-chunks occupied
for _k in (100, 101, 102, 103):
    _n = K_CHUNK * _k
    _row(f"occ_nsc{_k}", 2, _n, 2, 1000,
         functools.partial(occupy, _n, 1, 2, {0: (3, 3), _k - 4: (5, 4), _k - 3: (40, 30), _k - 2: (2, 1),
                                              _k - 1: (31, 33)}),
         waves(1, 0, _k, ovf=(_k - 3,)), claims={"T": {_k - 3: 70, _k - 1: 64}}, leads=LEADS3)
# the last super-chunk partial: 99 chunks at m = 4 (3 chunks in super-chunk 24), n = 3 mod 4096,
# entries at n - 1 and at 4096c - 1 / 4096c
N_ODD = K_CHUNK * 98 + 3
_row("occ_partial_last", 2, N_ODD, 2, 300,
     lambda: [cat(4095, 4096, K_CHUNK * 96 - 1, K_CHUNK * 96, K_CHUNK * 98 - 1, N_ODD - 1),
              cat(4096, 8191, 8192, K_CHUNK * 98, K_CHUNK * 98 + 1, N_ODD - 1)],
     waves(4, 0, 25), claims={"T": {0: 5, 23: 1, 24: 6}}, leads=LEADS3)
_row("occ_partial_last_ovf", 2, N_ODD, 2, 300,
     lambda: [cat(K_CHUNK * 96 + np.arange(0, 4096 * 2, 128), N_ODD - 3, N_ODD - 1), cat(N_ODD - 2, N_ODD - 1)],
     waves(4, 0, 25, ovf=(24,)), claims={"T": {24: 67}}, leads=LEADS3)
# W = 64, one entry per run: one index in every run (a 64-term rank-order sum on one lane), and
# 64 distinct ones
_row("occ_w64_same", 2, N100, 64, 1, lambda: [cat(12345)] * 64, waves(32, 0, 4, W=64), claims={"T": {0: 64}},
     leads=LEADS3, order=True)
_row("occ_w64_distinct", 2, N100, 64, 1, lambda: [cat(97 * q + 5 if q % 2 else K_CHUNK * 32 - 1 - 97 * q)
                                                   for q in range(64)],
     waves(32, 0, 4, W=64), claims={"T": {0: 64}}, leads=LEADS3)

# --- 3. duplicates and arithmetic -------------------------------------------------------------
# W = 4, cap = 300 at n = 4096 * 100: per_chunk 12, m = 2 (8192-element super-chunks)
def _dup_runs(shared, counts=(30, 30, 2, 2), sc=3, tail_unique=True):
    """Super-chunk `sc` filled to exactly 64 lanes: `shared` = {index: runs that send it}; every
    other entry distinct. The smallest index of run 0 is the span's first element (lane 0)."""
    lo = sc * 8192
    pool = iter(lo + 5 + 61 * np.arange(400))
    runs = []
    for r, c in enumerate(counts):
        mine = [i for i, rs in shared.items() if r in rs]
        own = [int(next(pool)) for _ in range(c - len(mine))]
        runs.append(np.sort(np.array(mine + own, I64)))
    return runs


_D0 = 3 * 8192   # lane 0: the smallest index of run 0
_row("dup_2_runs_lane0", 3, N100, 4, 300, lambda: _dup_runs({_D0: (0, 1)}), waves(2, 0, 50, W=4),
     claims={"T": {3: 64}, "dups": {_D0: 2}})
_row("dup_3_runs_lane0", 3, N100, 4, 300, lambda: _dup_runs({_D0: (0, 2, 3)}), waves(2, 0, 50, W=4),
     claims={"T": {3: 64}, "dups": {_D0: 3}})
_row("dup_all_runs_lane0", 3, N100, 4, 300, lambda: _dup_runs({_D0: (0, 1, 2, 3)}), waves(2, 0, 50, W=4),
     claims={"T": {3: 64}, "dups": {_D0: 4}}, order=True)
# the slow path with an entry that occurs once, in lane 63 (the largest index of the last run)
_row("dup_lone_lane63", 3, N100, 4, 300, lambda: _dup_runs({_D0 + 9: (0, 1), 4 * 8192 - 1: (3,)}),
     waves(2, 0, 50, W=4), claims={"T": {3: 64}, "dups": {_D0 + 9: 2}})
_row("dup_two_indices", 3, N100, 4, 300, lambda: _dup_runs({_D0 + 9: (0, 1, 3), _D0 + 4097: (1, 2, 3)}),
     waves(2, 0, 50, W=4), claims={"T": {3: 64}, "dups": {_D0 + 9: 3, _D0 + 4097: 3}})
# 4096 apart in one super-chunk: the duplicate bitmap (offset mod 4096) aliases them
_row("dup_alias_4096", 3, N100, 4, 300, lambda: [cat(_D0 + 77), cat(_D0 + 77 + 4096), cat(_D0 + 78), cat(_D0 + 79)],
     waves(2, 0, 50, W=4), claims={"T": {3: 4}, "no_dups": True})
_row("dup_alias_4096_and_dup", 3, N100, 4, 300,
     lambda: [cat(_D0 + 77, _D0 + 300), cat(_D0 + 300, _D0 + 77 + 4096), cat(_D0 + 77 + 4096), cat(_D0 + 77)],
     waves(2, 0, 50, W=4), claims={"T": {3: 6}, "dups": {_D0 + 77: 2, _D0 + 300: 2, _D0 + 77 + 4096: 2}})
# rank order in fp32: W = 3 (the rounding of 1/3), per_chunk 6 at cap 200 -> m = 4
for _tag, _vals in (("2p24", (16777216.0, 1.0, 1.0)), ("1e8", (1e8, 1.0, -1e8))):
    for _p, _perm in enumerate(((0, 1, 2), (1, 0, 2), (1, 2, 0))):
        _v = [_vals[q] for q in _perm]
        _row(f"order_{_tag}_perm{_p}", 3, N100, 3, 200,
             functools.partial(lambda v: [(np.array([v[q], 0.5 + q], F32), cat(5000, 5001 + q)) for q in range(3)], _v),
             waves(4, 0, 25, W=3), claims={"dups": {5000: 3}}, order=True)
# -0.0: alone (the fast path's 0 + a), in two runs, and alone beside a duplicate (the slow path)
_NZ = F32(-0.0)
_row("negzero_lone", 3, N100, 2, 1000, lambda: [(np.array([_NZ, 1.5], F32), cat(100, 9000)), (np.array([_NZ], F32), cat(20000))],
     waves(1, 0, 100), claims={"negzero": (100, 20000), "no_dups": True}, leads=LEADS3)
_row("negzero_lone_m4", 3, N100, 2, 300, lambda: [(np.array([_NZ], F32), cat(70000)), (np.array([_NZ, 2.5], F32), cat(70001, 70002))],
     waves(4, 0, 25), claims={"negzero": (70000, 70001), "no_dups": True}, leads=LEADS3)
# gran on, no duplicate in the super-chunk: -0.0 alone in its granule (a whole-granule store) and beside another entry
_row("negzero_lone_gran", 3, N100, 2, 1500,
     lambda: [(np.array([_NZ, _NZ, 1.0], F32), cat(64, 200, 201)), (np.array([_NZ], F32), cat(9000))],
     waves(1, 1, 100), claims={"negzero": (64, 200, 9000), "no_dups": True, "granule": {4: 1, 12: 2, 562: 1}}, leads=LEADS3)
_row("negzero_two_runs", 3, N100, 2, 1000, lambda: [(np.array([_NZ], F32), cat(100)), (np.array([_NZ], F32), cat(100))],
     waves(1, 0, 100), claims={"negzero": (100,), "dups": {100: 2}})
_row("negzero_beside_dup", 3, N100, 2, 1000,
     lambda: [(np.array([_NZ, 2.0], F32), cat(100, 200)), (np.array([3.0, _NZ], F32), cat(200, 300))],
     waves(1, 0, 100), claims={"negzero": (100, 300), "dups": {200: 2}})
_row("negzero_gran", 3, N100, 2, 1500, lambda: [(np.array([_NZ], F32), cat(100)), (np.array([_NZ, _NZ], F32), cat(64, 100))],
     waves(1, 1, 100), claims={"negzero": (64, 100), "dups": {100: 2}})
_SPECIAL = np.array([np.nan, np.inf, -np.inf, np.inf, 1e-45, -1e-45, 1e-40, 3e38, 1.0], F32)
_row("specials", 3, N100, 3, 200,
     lambda: [(_SPECIAL, cat(10 + np.arange(9))),
              (np.array([1.0, 1.0, 1.0, -np.inf, 1e-45, 1e-45, -1e-40, 3e38, np.nan], F32), cat(10 + np.arange(9))),
              (np.array([2e-45, 1.1754942e-38], F32), cat(14, 30))],
     waves(4, 0, 25, W=3), claims={"dups": {10: 2, 13: 2, 14: 3}})
_row("w3_seeded", 3, N100, 3, 200, lambda: [spread(0, N100, 150, 5), spread(0, N100, 160, 5), spread(7, N100 - 7, 150, 6)],
     waves(4, 0, 25, W=3))
_row("w2_scale1", 3, N100, 2, 1000, lambda: [spread(0, N100, 700, 8), spread(0, N100, 700, 8)[::2]], waves(1, 0, 100),
     scale=1.0)
# fp16 wire values (subnormals, the largest finite, inf) and int32 indices
_H = np.array([6e-8, -6e-8, 6.1e-5, 65504.0, np.inf, -np.inf, 1.0009765625, -0.0], F32)
_row("fp16_i32", 3, N100, 2, 1000, lambda: [(_H, cat(3, 4, 5, 4095, 4096, 9000, N100 - 2, N100 - 1)),
                                              (_H[::-1].copy(), cat(3, 4, 5, 4095, 4096, 9000, N100 - 2, N100 - 1))],
     waves(1, 0, 100), fp16=True, int32=True, claims={"dups": {3: 2, N100 - 1: 2}})
_row("fp16_i64_seeded", 3, N100, 4, 300, lambda: [spread(0, N100, 250, 20 + q % 2) for q in range(4)],
     waves(2, 0, 50, W=4), fp16=True)
_row("fp32_i32_seeded", 3, N100, 4, 300, lambda: [spread(0, N100, 250, 30 + q % 3) for q in range(4)],
     waves(2, 0, 50, W=4), int32=True)

# --- 4. granule stores: per_chunk 30 at cap 1500 -> gran on, m = 1 ------------------------------
_row("gran_positions", 4, N100, 2, 1500, lambda: [cat([16 * (10 + 3 * k) + k for k in range(0, 16, 2)]),
                                                   cat([16 * (10 + 3 * k) + k for k in range(1, 16, 2)])],
     waves(1, 1, 100), claims={"granule": {10 + 3 * k: 1 for k in range(16)}}, leads=LEADS5)
_row("gran_shared", 4, N100, 2, 1500,
     lambda: [cat(16 * 50 + 2, 16 * 50 + 9, 16 * 60 + 5, 16 * 70 + 7, 16 * 80 + 0),
              cat(16 * 60 + 6, 16 * 70 + 7, 16 * 80 + 15, 16 * 90 + 3)],
     waves(1, 1, 100), claims={"granule": {50: 2, 60: 2, 70: 1, 80: 2, 90: 1}, "dups": {16 * 70 + 7: 2}}, leads=LEADS5)
# the first and last granule of a chunk and of the buffer: with a lead the granules straddle the
# chunk edges and the buffer's ends, and the entry falls back to its word
_row("gran_edges", 4, N100, 2, 1500,
     lambda: [cat(0, 4080, 4096 + 15, 8191, K_CHUNK * 50, N100 - 16), cat(15, 4095, 4096, 8192 - 16, K_CHUNK * 50 - 1, N100 - 1)],
     waves(1, 1, 100), claims={"granule": {0: 2, 255: 2, 256: 2, 511: 2, 12799: 1, 12800: 1, N100 // 16 - 1: 2}}, leads=LEADS5)
_row("gran_edges_lone", 4, N100, 2, 1500,
     lambda: [cat(0, 4096 + 15, K_CHUNK * 50, N100 - 16 + 7), cat(4095, 8192 - 16, K_CHUNK * 70 - 1)],
     waves(1, 1, 100), claims={"granule": {0: 1, 255: 1, 256: 1, 511: 1, 12800: 1, 17919: 1, N100 // 16 - 1: 1}}, leads=LEADS5)
_row("gran_seeded_30_per_chunk", 4, N100, 2, 1500, lambda: [spread(0, N100, 1500, 41), spread(0, N100, 1400, 42)],
     waves(1, 1, 100), leads=LEADS3)

# the single-run path. ascending: the payload's header word 1 is DGC_ORDER_ASCENDING
_SG = cat([16 * 3 * k + (k % 16) for k in range(63)],        # payload positions 0-62: one entry per granule
          16 * 200 + 4, 16 * 200 + 5,                          # positions 63 and 64 (two workgroups) in one granule
          16 * 300 + np.arange(16),                            # a whole granule
          16 * 400 + np.array([1, 6, 11, 12]),                 # one entry in each 16-B quarter
          16 * 500 + 9, N100 - 1)
_row("single_asc_granules", 4, N100, 1, 200, lambda: [_SG], ("single", True), form="ascending", leads=LEADS3,
     claims={"granule": {0: 1, 200: 2, 300: 16, 400: 4, 500: 1, N100 // 16 - 1: 1}, "positions": {63: 16 * 200 + 4, 64: 16 * 200 + 5}})
_row("single_asc_ends", 4, N100, 1, 200, lambda: [cat(0, 1, 14, 15, 16, N100 - 17, N100 - 16, N100 - 2, N100 - 1)],
     ("single", True), form="ascending", leads=LEADS5, claims={"granule": {0: 4, 1: 1, N100 // 16 - 2: 1, N100 // 16 - 1: 3}})
_row("single_asc_scale_half", 4, N100, 1, 200, lambda: [_SG], ("single", True), form="ascending", scale=0.5, leads=LEADS3)
_row("single_asc_negzero", 4, N100, 1, 200,
     lambda: [(np.array([_NZ, _NZ, 1.0, _NZ], F32), cat(5, 16 * 9 + 3, 16 * 9 + 4, N100 - 1))], ("single", True),
     form="ascending", leads=LEADS3, claims={"negzero": (5, 16 * 9 + 3, N100 - 1)})
_row("single_asc_fp16_i32", 4, N100, 1, 200, lambda: [_SG], ("single", True), form="ascending", fp16=True, int32=True,
     leads=LEADS3)
_row("single_asc_full", 4, N100, 1, 200, lambda: [spread(0, N100, 200, 43)], ("single", True), form="ascending",
     claims={"count_is_cap": True}, leads=LEADS3)
_row("single_asc_empty", 4, N100, 1, 200, lambda: [np.zeros(0, I64)], ("single", True), form="ascending", leads=LEADS3)
# the word path: header word 1 = 0, a topk-order run, scale 1 and 0.5, -0.0
_row("single_word", 4, N100, 1, 200, lambda: [_SG], ("single", False), leads=LEADS3)
_row("single_word_scale_half", 4, N100, 1, 200, lambda: [_SG], ("single", False), scale=0.5)
_row("single_word_negzero", 4, N100, 1, 200, lambda: [(np.array([_NZ, 1.0], F32), cat(5, 6))], ("single", False),
     claims={"negzero": (5,)})
_row("single_word_topk_order", 4, N100, 1, 200,
     lambda: [_SG[np.random.default_rng(44).permutation(_SG.size)]], ("single", False), status=2, leads=LEADS3)
_row("single_word_full", 4, N100, 1, 200, lambda: [spread(0, N100, 200, 43)], ("single", False),
     claims={"count_is_cap": True})
_row("single_word_empty", 4, N100, 1, 200, lambda: [np.zeros(0, I64)], ("single", False))

# --- 5. the workgroup path (tile_chunk): cap 4096 at W = 2 -> per_chunk 80, m = 1 ---------------
_row("tile_totals", 5, N100, 2, 4096,
     lambda: occupy(N100, 1, 2, {1: (33, 32), 2: (512, 511), 3: (512, 512), 4: (513, 512), 5: (1025, 1024), 7: (30, 30)}),
     waves(1, 1, 100, ovf=(1, 2, 3, 4, 5)), claims={"staged": {1: 65, 2: 1023, 3: 1024, 4: 1025, 5: 2049, 7: 60}},
     leads=LEADS3)
_row("tile_full_chunk", 5, N100, 2, 4096, lambda: [K_CHUNK * 7 + np.arange(4096), K_CHUNK * 7 + np.arange(4096)],
     waves(1, 1, 100, ovf=(7,)), claims={"staged": {7: 8192}, "count_is_cap": True}, leads=LEADS3)
# every entry in thread 5's 16 slots (elements 20-23 of each 1024-element quarter): W = 8 x 16
_T5 = cat([1024 * u + 20 + j for u in range(4) for j in range(4)])
_row("tile_one_thread", 5, N100, 8, 16, lambda: [K_CHUNK * 17 + _T5] * 8, waves(16, 0, 7, ovf=(1,), W=8),
     claims={"staged": {17: 128}, "T": {1: 128}}, leads=LEADS3, order=True)
# every entry in wave 2's share (offsets with bits 8-9 = 2)
_W2 = cat([1024 * u + 512 + 3 * j for u in range(4) for j in range(10)])
_row("tile_one_wave", 5, N100, 2, 4096, lambda: [K_CHUNK * 9 + _W2, K_CHUNK * 9 + _W2 + 1],
     waves(1, 1, 100, ovf=(9,)), claims={"staged": {9: 80}}, leads=LEADS3)
_row("tile_run_absent", 5, N100, 3, 2731, lambda: [spread(K_CHUNK * 4, K_CHUNK * 5, 50, 51), cat(K_CHUNK * 3 + 5, K_CHUNK * 5 + 5),
                                                     spread(K_CHUNK * 4, K_CHUNK * 5, 50, 52)],
     waves(1, 1, 100, ovf=(4,), W=3), claims={"staged": {4: 100}}, leads=LEADS3)
_row("tile_64_runs", 5, N100, 64, 2, lambda: [cat(K_CHUNK * 20 + 7 * (q % 16), K_CHUNK * 20 + 1000 + q) for q in range(64)],
     waves(16, 0, 7, ovf=(1,), W=64), claims={"staged": {20: 128}, "T": {1: 128}}, leads=LEADS3)
_row("tile_negzero", 5, N100, 2, 4096,
     lambda: [(np.concatenate([[_NZ, _NZ], seeded(np.arange(40), 0)]).astype(F32), cat(K_CHUNK * 2 + np.arange(2), K_CHUNK * 2 + 10 + np.arange(40))),
              (np.concatenate([[_NZ], seeded(np.arange(40), 1)]).astype(F32), cat(K_CHUNK * 2 + 1, K_CHUNK * 2 + 30 + np.arange(40)))],
     waves(1, 1, 100, ovf=(2,)), claims={"staged": {2: 83}, "negzero": (K_CHUNK * 2, K_CHUNK * 2 + 1)}, leads=LEADS3)
_row("tile_partial_last", 5, N_ODD, 2, 4096, lambda: [cat(K_CHUNK * 97 + 4000 + np.arange(60), K_CHUNK * 98 + np.arange(3)),
                                                       cat(K_CHUNK * 97 + 4030 + np.arange(66), N_ODD - 1)],
     waves(1, 1, 99, ovf=(97,)), claims={"staged": {97: 126, 98: 4}}, leads=LEADS3)
_row("tile_partial_last_ovf", 5, K_CHUNK * 98 + 100, 2, 4096,
     lambda: [K_CHUNK * 98 + np.arange(0, 100, 2), K_CHUNK * 98 + np.arange(50, 100)],
     waves(1, 1, 99, ovf=(98,)), claims={"staged": {98: 100}}, leads=LEADS3)
# m = 2 (cap 600: per_chunk 12): a super-chunk overflowed by one chunk, the other empty; the same
# at the end of a 99-chunk buffer, where the second chunk does not exist
N99 = K_CHUNK * 99
_row("tile_m2_other_empty", 5, N99, 2, 600,
     lambda: [cat(spread(K_CHUNK * 6, K_CHUNK * 7, 35, 53), spread(K_CHUNK * 98, N99, 35, 54)),
              cat(spread(K_CHUNK * 6, K_CHUNK * 7, 35, 55), spread(K_CHUNK * 98, N99, 35, 56))],
     waves(2, 0, 50, ovf=(3, 49)), claims={"staged": {6: 70, 7: 0, 98: 70}, "T": {3: 70, 49: 70}}, leads=LEADS3)

# --- 6. bounds --------------------------------------------------------------------------------
_row("bnd_gap_8_9", 6, N100, 2, 1000, lambda: [cat(100, 100 + 8 * K_CHUNK, 100 + 17 * K_CHUNK, 100 + 17 * K_CHUNK + 1),
                                               cat(K_CHUNK * 9 + 1, K_CHUNK * 18 + 1, K_CHUNK * 26 + 4095, K_CHUNK * 99)],
     waves(1, 0, 100), claims={"gaps": {0: (1, 8, 9, 0, 83), 1: (10, 9, 8, 73, 1)}})
_row("bnd_first_chunk9", 6, N100, 2, 1000, lambda: [cat(K_CHUNK * 9), cat(K_CHUNK * 8, K_CHUNK * 8 + 1)],
     waves(1, 0, 100), claims={"gaps": {0: (10, 91), 1: (9, 0, 92)}})
for _w, _e in (("first", 0), ("middle", 1), ("last", 2)):
    _row(f"bnd_empty_{_w}", 6, N100, 3, 667,
         functools.partial(lambda e: [np.zeros(0, I64) if q == e else spread(0, N100, 300, 60 + q) for q in range(3)], _e),
         waves(1, 0, 100, W=3), claims={"empty": (_e,)})
_row("bnd_one_entry_ends", 6, N100, 2, 1000, lambda: [cat(0), cat(N100 - 1)], waves(1, 0, 100),
     claims={"gaps": {0: (1, 100), 1: (100, 1)}})
_row("bnd_one_entry_ends_odd", 6, N_ODD, 2, 1000, lambda: [cat(N_ODD - 1), cat(0)], waves(1, 0, 99))
for _c in (255, 256, 257):
    _row(f"bnd_count_{_c}", 6, N100, 2, 1000, functools.partial(lambda c: [spread(0, N100, c, 61), spread(0, N100, c, 62)], _c),
         waves(1, 0, 100), claims={"counts": (_c, _c)})
_row("bnd_below_cap", 6, N100, 2, 1000, lambda: [spread(0, N100, 1, 63), spread(0, N100, 999, 64)], waves(1, 0, 100),
     claims={"counts": (1, 999)})
# indices outside [0, n): dropped and flagged (status bit 0), below 0, at n, inside the last chunk's
# 4096 but past n, past it, and far past 2^32 — on the wave path, the workgroup path and the single run
N_TAIL = K_CHUNK * 98 + 100
_row("bad_index_waves", 6, N_ODD, 2, 1000,
     lambda: [cat(-7, 3, N_ODD - 1, N_ODD, N_ODD + 1, K_CHUNK * 99 - 1, K_CHUNK * 99, 1 << 40), cat(3, N_ODD - 1)],
     waves(1, 0, 99), status=1, claims={"bad": 6, "T": {0: 2, 98: 2}}, leads=LEADS3)
_row("bad_index_tile", 6, N_TAIL, 2, 4096,
     lambda: [cat(K_CHUNK * 98 + np.arange(0, 100, 2), N_TAIL, N_TAIL + 1, K_CHUNK * 99 - 1, K_CHUNK * 99),
              cat(-(1 << 40), -1, K_CHUNK * 98 + np.arange(50, 100))],
     waves(1, 1, 99, ovf=(98,)), status=1, claims={"bad": 6, "staged": {98: 100}}, leads=LEADS3)
_row("bad_index_regroup", 6, N_ODD, 2, 1000,
     lambda: [cat(N_ODD, 9, N_ODD - 1, -1, 3, K_CHUNK * 99 - 1), cat(3, N_ODD - 1)],
     waves(1, 0, 99, unsorted=(1, 0)), status=3, claims={"bad": 3}, leads=LEADS3)
_row("bad_index_single_asc", 6, N_ODD, 1, 200, lambda: [cat(-1, 5, 6, N_ODD - 1, N_ODD, N_ODD + 16)], ("single", True),
     form="ascending", status=1, claims={"bad": 3}, leads=LEADS3)
_row("bad_index_single_word", 6, N_ODD, 1, 200, lambda: [cat(-1, 5, 6, N_ODD - 1, N_ODD, 1 << 40)], ("single", False),
     status=1, claims={"bad": 3}, leads=LEADS3)

# the second sweep of k_bounds: more than 262 143 entries per run (W = 2, n = 4096 * 2048: 128
# entries of each run per chunk, every super-chunk on the workgroup path)
N2048 = K_CHUNK * 2048


def _every32(count, shift):
    i = 32 * np.arange(262144, dtype=I64) + shift
    return i if count <= 262144 else np.sort(np.concatenate([i, [N2048 - 1]]))[:count]


for _c, _sw in ((262143, 1), (262144, 2), (262145, 2)):
    _row(f"bnd_sweep_{_c}", 6, N2048, 2, _c,
         functools.partial(lambda c: [_every32(c, 0)[:c], _every32(c, 7)[:c]], _c),
         waves(1, 1, 2048, ovf=range(2048), sweeps=_sw), claims={"counts": (_c, _c), "count_is_cap": True})
_row("bnd_sweep_sparse_second", 6, N2048, 2, 262145,
     lambda: [spread(0, N2048, 300, 65), cat(5, N2048 - 1)], waves(1, 1, 2048, sweeps=2), claims={"counts": (300, 2)})

# --- 7. regroup (runs in topk order) -----------------------------------------------------------
N1023, N1024P = K_CHUNK * 1023, K_CHUNK * 1024 + 1


def _shuffled(i, seed):
    i = np.asarray(i, I64)
    return i[np.random.default_rng(seed).permutation(i.size)]


for _tag, _n in (("1023", N1023), ("1024p1", N1024P)):
    _nsc = ceil_div(ceil_div(_n, K_CHUNK), 8)
    _row(f"regroup_one_run_{_tag}", 7, _n, 2, 2000,
         functools.partial(lambda n: [_shuffled(spread(0, n, 1500, 70), 71), spread(0, n, 1800, 72)], _n),
         waves(8, 0, _nsc, unsorted=(1, 0)), status=2)
    _row(f"regroup_all_runs_{_tag}", 7, _n, 2, 2000,
         functools.partial(lambda n: [_shuffled(spread(0, n, 2000, 70), 73), _shuffled(spread(0, n, 1999, 70), 74)], _n),
         waves(8, 0, _nsc, unsorted=(1, 1)), status=2, claims={"counts": (2000, 1999)})
_row("regroup_w64", 7, N100, 64, 4, lambda: [_shuffled(rand_idx(N100, 4, 140 + q % 9), q) if q % 3 else rand_idx(N100, 3, 150 + q)
                                                for q in range(64)],
     waves(8, 0, 13, W=64, unsorted=[int(q % 3 != 0 and descends(_shuffled(rand_idx(N100, 4, 140 + q % 9), q))) for q in range(64)]),
     status=2)
_row("regroup_inside_one_chunk", 7, N100, 2, 300, lambda: [_shuffled(K_CHUNK * 40 + 3 * np.arange(20), 75), cat(K_CHUNK * 40 + 3, K_CHUNK * 41)],
     waves(4, 0, 25, unsorted=(1, 0)), status=2, claims={"staged": {40: 21}})
_row("regroup_empty_chunks_between", 7, N100, 2, 300,
     lambda: [cat(K_CHUNK * 90 + 1, K_CHUNK * 3 + 2, K_CHUNK * 50, K_CHUNK * 3 + 1, N100 - 1, 0), cat(K_CHUNK * 50, K_CHUNK * 60)],
     waves(4, 0, 25, unsorted=(1, 0)), status=2)
_row("regroup_beside_ascending", 7, N100, 4, 300,
     lambda: [spread(0, N100, 200, 76), _shuffled(spread(0, N100, 200, 76), 77), spread(0, N100, 200, 76)[::3], _shuffled(spread(0, N100, 100, 78), 79)],
     waves(2, 0, 50, W=4, unsorted=(0, 1, 0, 1)), status=2)
_row("regroup_crowded", 7, N100, 2, 300,
     lambda: [_shuffled(np.unique(cat(K_CHUNK * 12 + 5 * np.arange(100), spread(0, N100, 100, 80)[1:-1])), 81), K_CHUNK * 12 + 5 * np.arange(0, 100, 2)],
     waves(4, 0, 25, ovf=(3,), unsorted=(1, 0)), status=2, claims={"T": {3: 115}})

# --- 8. re-zero (the row's `prev` is designed; the other rows get default_prev) -----------------
N512 = K_CHUNK * 512
for _c in (65536, 65537):
    _row(f"rezero_prev_cap_{_c}", 8, N512, 2, _c,
         lambda: [spread(0, N512, 200, 82), spread(0, N512, 100, 83)],
         waves(1, 1, 512),
         prev=functools.partial(lambda c: [32 * np.arange(c, dtype=I64) % N512 + np.arange(c) // 65536, 32 * np.arange(c, dtype=I64) % N512 + 5 + np.arange(c) // 65536], _c),
         claims={"prev_counts": (_c, _c)}, leads=LEADS3)
_ENDS = cat(0, 1, 2, 15, 16, N100 - 17, N100 - 16, N100 - 3, N100 - 2, N100 - 1)
_row("rezero_prev_at_ends", 8, N100, 2, 1000, lambda: [cat(7, 5000), cat(N100 - 8)], waves(1, 0, 100),
     prev=lambda: [_ENDS, _ENDS[::2]], leads=LEADS5)
_row("rezero_disjoint", 8, N100, 2, 1000, lambda: [np.unique(spread(0, N100, 500, 84) | 1), np.unique(spread(0, N100, 400, 85) | 1)], waves(1, 0, 100),
     prev=lambda: [np.unique(spread(0, N100, 500, 86) & ~1), np.unique(spread(0, N100, 300, 87) & ~1)], leads=LEADS3,
     claims={"prev_relation": "disjoint"})
_row("rezero_identical", 8, N100, 2, 1000, lambda: [np.unique(spread(0, N100, 500, 84)), spread(0, N100, 400, 85)], waves(1, 0, 100),
     prev=lambda: [np.unique(spread(0, N100, 500, 84)), spread(0, N100, 400, 85)], leads=LEADS3,
     claims={"prev_relation": "identical"})
_row("rezero_subset", 8, N100, 2, 1000, lambda: [spread(0, N100, 500, 84)[::3], spread(0, N100, 400, 85)[::5]], waves(1, 0, 100),
     prev=lambda: [spread(0, N100, 500, 84), spread(0, N100, 400, 85)], leads=LEADS3,
     claims={"prev_relation": "subset"})
_row("rezero_prev_below_cap", 8, N100, 2, 1500, lambda: [spread(0, N100, 1500, 88), spread(0, N100, 3, 89)], waves(1, 1, 100),
     prev=lambda: [spread(0, N100, 2, 90), spread(0, N100, 700, 91)], leads=LEADS3, claims={"prev_counts": (2, 700)})

# --- 9. the run-table form (dgc_decompress): `table` with run offsets, `detect` without ---------
def _table(name, n, runs, rt, **kw):
    W = len(runs())
    _row(name, 9, n, W, 0, runs, rt, form="table", **kw)


_table("table_1_run_repeats", 5000, lambda: [np.sort(np.random.default_rng(92).integers(0, 5000, 3000))], ("single", False))
_table("table_1_run_empty", 5000, lambda: [np.zeros(0, I64)], ("single", False))
_table("table_1_run_one", 5000, lambda: [cat(4999)], ("single", False))
_table("table_2_runs", N100, lambda: [spread(0, N100, 300, 93), spread(0, N100, 200, 94)], waves(4, 0, 25))
for _w, _e, _m, _nsc in (("first", (0,), 8, 13), ("middle", (1, 2), 16, 7), ("last", (3,), 8, 13)):   # totals 300, 200, 300
    _table(f"table_empty_{_w}", N100,
           functools.partial(lambda e: [np.zeros(0, I64) if q in e else spread(0, N100, 100, 95 + q) for q in range(4)], _e),
           waves(_m, 0, _nsc, W=4), claims={"empty": _e})
_table("table_64_runs", N100, lambda: [rand_idx(N100, 1 + q % 5, 100 + q % 7) for q in range(64)], waves(16, 0, 7, W=64),
       claims={"total": 190})
_table("table_64_runs_empty_ends", N100,
       lambda: [np.zeros(0, I64) if q in (0, 31, 63) else cat(777, 1000 + q) for q in range(64)],
       waves(16, 0, 7, W=64, ovf=(0,)), claims={"empty": (0, 31, 63), "T": {0: 122}, "total": 122}, order=True)
# detection: `descents` runs boundaries found on the device
DETECT = {   # name -> (n, runs builder, descents or None for DGC_ERR_UNSORTED)
    "detect_0_descents": (N100, lambda: [spread(0, N100, 500, 110)], 0),
    "detect_1_descent": (N100, lambda: [spread(0, N100, 500, 110), spread(0, N100, 400, 111)], 1),
    "detect_63_descents": (N100, lambda: [cat(50000 + q, 60000 - q) if q % 2 else cat(40000, 50000 + q, 70000 + q) for q in range(64)], 63),
    "detect_64_descents": (N100, lambda: [cat(40000, 50000 + q) for q in range(65)], None),
    "detect_total_0": (N100, lambda: [np.zeros(0, I64)], 0),
    "detect_total_1": (N100, lambda: [cat(N100 - 1)], 0),
    # more than one sweep of k_find_descents, the one descent exactly at position 524 288
    "detect_descent_at_524288": (K_CHUNK * 256, lambda: [2 * np.arange(524288, dtype=I64), cat(1, 3, K_CHUNK * 256 - 1)], 1),
    # ... and at 524 289: the pair (524 288, 524 289) is the first one only the second sweep compares
    "detect_descent_at_524289": (K_CHUNK * 256, lambda: [cat(2 * np.arange(524288, dtype=I64), K_CHUNK * 256 - 1), cat(1, 3)], 1),
}

# --- 10. split phases, fp32 (dgc_scatter_split): W = 2, parts = 2, cap 20 -> part capacity 10, --
# 40 slots at n = 4096 * 100: per_chunk 0.4, m = 64, super-chunks of 262 144 elements
_SPAN = 64 * K_CHUNK


def _split_runs(bound, other):
    """Rank 0's entry 10 (the first of its part 1) is `bound`; rank 1's is `other`."""
    a = cat(spread(0, min(bound, _SPAN) - 1, 10, 120), bound, spread(bound + 1, N100, 5, 121))
    b = cat(spread(0, min(other, _SPAN) - 1, 10, 122), other, spread(other + 1, N100, 4, 123))
    return [a, b]


for _tag, _b in (("on", _SPAN), ("below", _SPAN - 1), ("above", _SPAN + 1)):
    _row(f"split_bound_{_tag}_edge", 10, N100, 2, 20, functools.partial(_split_runs, _b, _SPAN + 500),
         waves(64, 0, 2, W=4), parts=2, claims={"bounds": ((_b, INT64_MAX), (_SPAN + 500, INT64_MAX))})
_row("split_no_later_parts", 10, N100, 2, 20, lambda: [spread(0, N100, 10, 124), cat(spread(0, _SPAN, 10, 125), _SPAN + 9, N100 - 1)],
     waves(64, 0, 2, W=4), parts=2, claims={"bounds": ((INT64_MAX, INT64_MAX), (_SPAN + 9, INT64_MAX))})
_row("split_w8_parts8", 10, N100, 8, 64, lambda: [spread(q, N100 - q, 64 - q, 126 + q % 3) for q in range(8)],
     waves(4, 0, 25, W=64), parts=8)
_row("split_crowded", 10, N100, 2, 400, lambda: [cat(spread(0, K_CHUNK, 150, 127), spread(K_CHUNK, N100, 250, 128)), spread(0, N100, 390, 129)],
     waves(4, 0, 25, W=4, ovf=(0,)), parts=2)

ROW_BY_NAME = {r.name: r for r in ROWS}
PACKED = [r for r in ROWS if r.form != "table" and not r.parts]
MULTI = [r for r in PACKED if r.W > 1]
SINGLE = [r for r in PACKED if r.W == 1]
TABLE = [r for r in ROWS if r.form == "table"]
SPLIT = [r for r in ROWS if r.parts]


def split_parts(runs, parts, cap):
    """The runs of a split exchange in the scatter's order (run q = rank * parts + part): part p of
    a rank is entries [p * pc, (p + 1) * pc) of its payload, pc = ceil(cap / parts)."""
    pc = ceil_div(cap, parts)
    return [(v[p * pc: (p + 1) * pc], i[p * pc: (p + 1) * pc]) for v, i in runs for p in range(parts)], pc
