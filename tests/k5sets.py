"""K5s design inputs: resample candidate sets whose k-th largest key sits on an edge of the
index-order set path (CPU only, numpy).

K5s (csrc/select_set.hpp: resample_set_block, resample_set_body) serves a resample under
``resample_order = 1``: a two-pass radix select over ``key - key(t_cur)`` (4096 bins of bits
13-24, clamped; 8192 bins of bits 0-12 under the pass-0 prefix) finds the k-th largest
candidate key; untied across the k boundary, the set ``key >= kth`` is emitted in index order by
G co-resident workgroups, each over a stretch of ``per`` rounds of 1024 candidates. A k-th key
in the top bin, a tie across the boundary, and a stretch of more than kSetRoundsMax rounds leave
the tensor to the exact replay (K5), whose payload is in torch.topk's order.

In the style of killer.py / k3edges.py:

``route(keys, t, k, cand_cap)``
    resample_set_block and resample_set_body restated so that they only classify.
``design`` / ``place``
    a candidate key multiset relative to ``mn = key(t)`` with the k-th key planted (every other
    key seeded), and its order along the candidate queue (ascending element index).
``embed``
    the candidates inside a gradient whose other elements lie below the threshold, in three
    layouts of the gather.
``ROWS``
    the table tests/test_k5s_sets_cpu.py confirms and tests/test_gpu_k5s_sets.py runs; every
    row states its route. Expected payloads never come from here: they are torch.topk's.
"""
import functools
import re
import zlib
from collections import namedtuple
from pathlib import Path

import numpy as np

from oracle import dgc_oracle as O

F32, U32 = np.float32, np.uint32

# Copies of the kernels' constants (test_k5s_sets_cpu.py reads the constexpr lines and fails
# when one drifts).
K_SET_REG_C = 16          # rounds of a stretch kept in registers
K_SET_ROUNDS_MAX = 64     # rounds of a stretch at most (the rest from L2); past it: the replay
K_SET_G_DEFAULT = 4       # a cooperative set's fewest workgroups
K_SET_G_BIG = 128         # ... and most
K_SET_SPAN = 25           # key bits above key(t_cur) the two passes cover
K_SET_LO0 = 13            # pass 1's bits
K_CAP = 64                # list slots per segment
K_SEG = 1024              # elements per segment
K_GROUP_SEGS = 1024       # segments per group
K_SCAN_THREADS = 1024     # candidates per round
K_NTH_LDS = 12288         # introselect.hpp: larger replays start in global memory

CSRC = Path(__file__).resolve().parents[1] / "adam-compression_amd" / "csrc"
CONSTANTS = {   # name -> (file, our copy)
    "kSetRegC": ("select_types.hpp", K_SET_REG_C),
    "kSetRoundsMax": ("select_types.hpp", K_SET_ROUNDS_MAX),
    "kSetGDefault": ("select_types.hpp", K_SET_G_DEFAULT),
    "kSetGBig": ("select_types.hpp", K_SET_G_BIG),
    "kSetSpan": ("select_types.hpp", K_SET_SPAN),
    "kSetLo0": ("select_types.hpp", K_SET_LO0),
    "kCap": ("select_types.hpp", K_CAP),
    "kSeg": ("select_types.hpp", K_SEG),
    "kGroupSegs": ("select_types.hpp", K_GROUP_SEGS),
    "kScanThreads": ("radix_select.hpp", K_SCAN_THREADS),
    "kNthLds": ("introselect.hpp", K_NTH_LDS),
}
BINS0 = 1 << (K_SET_SPAN - K_SET_LO0)
BINS1 = 1 << K_SET_LO0
COOP_MIN = K_SET_REG_C * K_SCAN_THREADS      # kSetCoopMin = kSetOneMax
TOP = (BINS0 - 1) << K_SET_LO0               # the first offset of pass 0's top bin


def header_constant(name):
    """The value of ``name = <integer>`` on a constexpr line of the file CONSTANTS names (a line
    may define several: ``constexpr int kSetSpan = 25, kSetLo0 = 13;``)."""
    text = (CSRC / CONSTANTS[name][0]).read_text()
    m = [v for line in text.splitlines() if re.match(r"\s*constexpr\b", line)
         for v in re.findall(r"\b%s\s*=\s*(\d+)\s*[,;]" % re.escape(name), line)]
    assert len(m) == 1, f"{name}: {len(m)} constexpr definitions in {CONSTANTS[name][0]}"
    return int(m[0])


def key_of(t):
    return int(np.array([t], F32).view(U32)[0] & U32(0x7FFFFFFF))


def keys_of(x):
    """|x| bit patterns."""
    return np.ascontiguousarray(np.asarray(x, F32)).view(U32) & U32(0x7FFFFFFF)


def f32_of(keys):
    return np.asarray(keys, dtype=np.uint64).astype(U32).view(F32)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ the route
def set_workgroups(k, cand_cap):
    """select_layout.hpp, BT_SET: the workgroups the host launches for a tensor."""
    if k < 1 or cand_cap <= k:
        return 0
    if cand_cap <= COOP_MIN:
        return 1
    return min(K_SET_G_BIG, max(K_SET_G_DEFAULT, ceil_div(cand_cap, COOP_MIN)))


def _pick(hist, k_rem):
    """The bin of the k_rem-th largest and the count above it (pick_bin_small)."""
    above = np.cumsum(hist[::-1])[::-1]          # above[b] = sum(hist[b:])
    b = int(np.flatnonzero(above >= k_rem)[-1])
    return b, int(above[b] - hist[b]), int(hist[b])


def route(keys, t, k, cand_cap):
    """What K5s does with the candidate keys ``keys`` (every one >= key(t)) of a resample for
    k: ``("set", Gt, G, per, ovf, bin0, bin1, eq)`` or ``("replay", reason)``, reason one of
    ``tied``, ``span``, ``rounds``."""
    keys = np.asarray(keys, np.int64)
    n, mn = keys.size, key_of(t)
    assert keys.min() >= mn
    Gt = set_workgroups(k, cand_cap)
    assert Gt > 0 and n > k and n <= cand_cap, (n, k, cand_cap)
    rounds = ceil_div(n, K_SCAN_THREADS)
    G = 1
    if n > COOP_MIN and Gt > 1:
        want = ceil_div(rounds, K_SET_REG_C)
        G = min(max(want, K_SET_G_DEFAULT), Gt)
    per = ceil_div(rounds, G)
    if per > K_SET_ROUNDS_MAX:
        return ("replay", "rounds")
    x = keys - mn
    hi = x >> K_SET_LO0
    bin0, above0, _ = _pick(np.bincount(np.minimum(hi, BINS0 - 1), minlength=BINS0), k)
    if bin0 == BINS0 - 1:
        return ("replay", "span")
    k_rem = k - above0
    bin1, above1, eq = _pick(np.bincount(x[hi == bin0] & (BINS1 - 1), minlength=BINS1), k_rem)
    k_rem -= above1
    if eq != k_rem:
        return ("replay", "tied")
    return ("set", Gt, G, per, per > K_SET_REG_C, bin0, bin1, eq)


# ------------------------------------------------------------------ key multisets
Keys = namedtuple("Keys", "above run below")   # offsets from mn: > the k-th, == it, < it
NEAR = 1 << 18                                 # seeded keys lie within this many units of the k-th


def design(c, k, D, eq=1, ka=None, above=(), below=(), seed=0):
    """c candidate key offsets (from mn) whose k-th largest is D: ``eq`` keys at D, ``ka`` of them
    inside the top k (eq: untied), k - ka above and the rest below; ``above`` / ``below`` are
    planted, the others seeded within NEAR of D and at least two units from it (D - 1 and D + 1
    are present only when planted). One key is mn itself (offset 0) whenever D > 0; D = 0 has
    no room below, so every key that is not above is the k-th (``eq`` is ignored)."""
    rng = np.random.default_rng(seed)
    ka = eq if ka is None else ka
    na = k - ka
    if D == 0:
        eq, below = c - na, ()
    nb = c - na - eq
    floor = 1 if D > 0 and nb > 0 else 0      # mn itself
    assert 1 <= ka <= eq and na >= len(above) and nb >= len(below) + floor and all(a > D for a in above) \
        and all(0 <= b < D for b in below), (c, k, D, eq, ka)
    up = np.concatenate([np.asarray(above, np.int64), rng.integers(D + 2, D + 2 + NEAR, na - len(above))])
    lo = np.asarray(below, np.int64)
    if floor:
        room = max(0, D - 2 - NEAR), max(1, D - 1)      # [lo, hi): D - 2 at most
        lo = np.concatenate([lo, [0], rng.integers(room[0], room[1], nb - len(below) - 1)])
    return Keys(up.astype(np.int64), np.full(eq, D, np.int64), lo.astype(np.int64))


def stretches(c, G):
    """(per, the candidate slots [lo, hi) of the last non-empty stretch) of a G-workgroup set."""
    rounds = ceil_div(c, K_SCAN_THREADS)
    per = ceil_div(rounds, G)
    last = (rounds - 1) // per
    return per, last * per * K_SCAN_THREADS, c


def place(keys, how, G=1, run_at=None, seed=0):
    """The offsets in candidate-queue order (ascending element index). ``how``: ``random``;
    ``first`` / ``last`` — the top k (above + run) at seeded slots of the first / the last
    non-empty stretch (of the first / last 2k slots when a stretch holds fewer than k);
    ``waves`` — one of the top k in every wave of 64 slots, the rest of them anywhere.
    ``run_at``: the run of equal keys occupies the slots around that one, half before it."""
    rng = np.random.default_rng(seed)
    top = np.concatenate([keys.above, keys.run])
    c, k = top.size + keys.below.size, top.size
    out = np.empty(c, np.int64)
    if run_at is not None:
        assert how == "random"
        lo = run_at - keys.run.size // 2
        assert 0 <= lo and lo + keys.run.size <= c
        rest = rng.permutation(np.concatenate([keys.above, keys.below]))
        out[:lo], out[lo:lo + keys.run.size], out[lo + keys.run.size:] = rest[:lo], keys.run, rest[lo:]
        return out
    if how == "random":
        return rng.permutation(np.concatenate([top, keys.below]))
    per, last_lo, _ = stretches(c, G)
    if how == "first":
        hi = min(c, per * K_SCAN_THREADS if per * K_SCAN_THREADS >= k else 2 * k)
        slots = rng.choice(hi, k, replace=False)
    elif how == "last":
        lo = last_lo if c - last_lo >= k else c - min(c, 2 * k)
        slots = lo + rng.choice(c - lo, k, replace=False)
    else:
        assert how == "waves"
        waves = ceil_div(c, 64)
        assert waves <= k
        width = np.minimum(64, c - 64 * np.arange(waves))
        one = 64 * np.arange(waves) + (rng.random(waves) * width).astype(np.int64)
        free = np.setdiff1d(np.arange(c), one)
        slots = np.concatenate([one, rng.choice(free, k - waves, replace=False)])
    mask = np.zeros(c, bool)
    mask[slots] = True
    assert mask.sum() == k
    out[mask] = rng.permutation(top)
    out[~mask] = rng.permutation(keys.below)
    return out


# ------------------------------------------------------------------ embedding
Embedded = namedtuple("Embedded", "vec mmt pos attrs thr")
QUARTER = K_SEG * K_GROUP_SEGS // 4    # element 262144: the first boundary between two emit workgroups
GROUP = K_SEG * K_GROUP_SEGS           # element 1048576: the first group boundary
STRIDE = 8


def numel(c, layout, N=None):
    """The gradient's size: ``N`` when given, else the layout's own for c candidates."""
    if N:
        return N
    if layout in ("edges0", "edges3"):
        return GROUP + 4096 + int(layout[-1])
    return (40 if layout == "scattered" else 3) * c + 1031 + c % 7


def _positions(c, layout, N, rng):
    N = numel(c, layout, N)
    if layout == "scattered":     # lists serve: at most kCap candidates per segment, one segment exactly full
        nseg = N // K_SEG
        if c > 2 * K_CAP and nseg > 2:
            s = int(rng.integers(1, nseg - 1))
            full = s * K_SEG + rng.choice(K_SEG, K_CAP, replace=False)
            others = np.setdiff1d(np.arange(N), np.arange(s * K_SEG, (s + 1) * K_SEG))
            pos = np.concatenate([full, rng.choice(others, c - K_CAP, replace=False)])
        else:
            pos = rng.choice(N, c, replace=False)
        assert np.bincount(pos // K_SEG).max() <= K_CAP, "scattered: a segment spills"
    elif layout == "dense":       # more than kCap candidates per segment, one whole segment of them
        assert c >= 2 * K_SEG
        s = int(rng.integers(1, N // K_SEG - 1))
        whole = np.arange(s * K_SEG, (s + 1) * K_SEG)
        others = rng.choice(N - K_SEG, c - K_SEG, replace=False)      # of the elements outside that segment
        pos = np.concatenate([whole, np.where(others >= s * K_SEG, others + K_SEG, others)])
        assert np.bincount(pos // K_SEG).max() == K_SEG and np.median(np.bincount(pos // K_SEG)) > K_CAP
    else:
        assert layout in ("edges0", "edges3")   # N = 0 / 3 mod 4
        assert N % 4 == int(layout[-1]) and N > GROUP + 2
        forced = np.array([0, 1, N - 2, N - 1, QUARTER - 2, QUARTER - 1, QUARTER, QUARTER + 1,
                           GROUP - 2, GROUP - 1, GROUP, GROUP + 1])
        others = np.setdiff1d(np.arange(N), forced)
        pos = np.concatenate([forced, rng.choice(others, c - forced.size, replace=False)])
    assert c <= N and np.unique(pos).size == c
    return N, np.sort(pos)


def embed(values, k, layout, N=None, t=1.0, seed=0):
    """The candidates ``values`` (|x| >= t, queue order) at increasing positions of a gradient of N
    elements whose other elements are nonzero, of either sign and below t. ``attrs`` =
    (N, k, S, ks, stride) as oracle.attributes lays them out, with N > S so that the selection
    adapts, and ``floor(1.3 k) < c < 64 k`` so that it resamples through nth_element. Layouts:
    ``scattered`` (the gather reads the segments' lists), ``dense`` (it re-reads spilled segments),
    ``edges0`` / ``edges3`` (candidates at elements 0 and N - 1 and on both sides of the first
    quarter-group and group boundaries; N = 0 / 3 mod 4)."""
    c = values.size
    assert O.adapt_bounds(k)[0] < c < 64 * k, (c, k)
    assert np.abs(values).min() >= F32(t)
    rng = np.random.default_rng(seed)
    N, pos = _positions(c, layout, N, rng)
    assert c <= min(N, 64 * k - 1)
    vec = (rng.uniform(0.01, 0.9, N) * t).astype(F32) * np.where(rng.random(N) < 0.5, F32(-1), F32(1))
    assert 0 < np.abs(vec).min() and np.abs(vec).max() < F32(t)
    vec[pos] = values
    mmt = (rng.standard_normal(N).astype(F32) + F32(3.0)).astype(F32)
    return Embedded(vec.astype(F32), mmt, pos, (N, k, N // STRIDE, max(1, k // STRIDE), STRIDE), F32(t))


# ------------------------------------------------------------------ the rows
# name; c, k; t; the design (D, eq, ka, planted above / below); the placement (how, G, run_at);
# the layout and N; the route the row was designed for.
Row = namedtuple("Row", "name c k t D eq ka above below how G run_at layout N route")
ROWS = []
ROW_BY_NAME = {}
LAYOUTS = ("scattered", "dense", "edges0", "edges3")
INF_KEY, BIG_KEY = 0x7F800000, key_of(3e38)


def _add(name, c, k, t, D, route_, eq=1, ka=None, above=(), below=(), how="random", G=1, run_at=None,
         layout="scattered", N=None):
    assert floor13(k) < c < 64 * k, (name, c, k)       # the count resamples through nth_element
    ka = eq if ka is None else ka
    if D == 0:      # no room below mn: every key that is not above is the k-th
        eq = c - (k - ka)
    r = Row(name, c, k, t, D, eq, ka, tuple(above), tuple(below), how, G, run_at, layout, N,
            route_)
    assert name not in ROW_BY_NAME, name
    ROWS.append(r)
    ROW_BY_NAME[name] = r


def floor13(k):
    return O.adapt_bounds(k)[0]


def _set(shape, D, eq=1):
    return ("set",) + shape + (D >> K_SET_LO0, D & (BINS1 - 1), eq)


def _key_rows():
    P = 50 << K_SET_LO0     # an inner pass-0 prefix
    # (tag, c, k, (Gt, G, per, ovf), the slot of a stretch boundary or None)
    sizes = (("one", 3001, 100, (1, 1, 3, False), None), ("coop", 40003, 1000, (4, 4, 10, False), 10 * 1024))
    for tag, c, k, shape, stretch in sizes:
        for t in (1.0, 0.75):
            mn = key_of(t)
            n = [0]

            def add(name, D, route_, **kw):
                lay = LAYOUTS[n[0] % 4]
                if lay == "dense" and c < 2 * K_SEG:
                    lay = "scattered"
                n[0] += 1
                _add(f"{name}_{tag}_t{t}", c, k, t, D, route_, G=shape[1], layout=lay, **kw)
            # pass 0
            add("p0_bin0", 5000, _set(shape, 5000))
            add("p0_kth_is_mn", 0, ("replay", "tied"))
            add("p0_inner_below", (7 << K_SET_LO0) - 1, _set(shape, (7 << K_SET_LO0) - 1))   # low bits all one
            add("p0_inner_above", 7 << K_SET_LO0, _set(shape, 7 << K_SET_LO0))             # low bits all zero
            add("p0_bin4094", TOP - 1, _set(shape, TOP - 1))      # every key above it is clamped into the top bin
            add("p0_bin4095", TOP, ("replay", "span"))
            add("p0_clamped_above", (100 << K_SET_LO0) + 77, _set(shape, (100 << K_SET_LO0) + 77),
                above=(INF_KEY - mn, INF_KEY - mn, BIG_KEY - mn, 1 << K_SET_SPAN, (1 << K_SET_SPAN) + 5, TOP, TOP + 1))
            # pass 1
            add("p1_zero_neighbours", P, _set(shape, P), above=(P + 1,), below=(P - 1,))
            add("p1_zero_alone", P, _set(shape, P))
            add("p1_ones_neighbours", P + 8191, _set(shape, P + 8191), above=(P + 8192,), below=(P + 8190,))
            add("p1_ones_alone", P + 8191, _set(shape, P + 8191))
            alias = [(j << K_SET_LO0) + 1234 for j in (0, 1, 49, 49, 49, 51, 51, 51, 52, 4000, 4094)]
            add("p1_alias", P + 1234, _set(shape, P + 1234), above=[a for a in alias if a > P + 1234],
                below=[a for a in alias if a < P + 1234])
            # ties: a run of equal keys with k on its last, first and a middle member
            add("tie_last", P + 300, _set(shape, P + 300, 5), eq=5, ka=5)
            add("tie_first", P + 300, ("replay", "tied"), eq=5, ka=1)
            add("tie_mid", P + 300, ("replay", "tied"), eq=5, ka=3)
            add("tie_all_equal", (3 << K_SET_LO0) + 9, ("replay", "tied"), eq=c, ka=k)
            for where, slot in (("wave", 64 * 7), ("round", 2 * 1024), ("stretch", stretch)):
                if slot is None:
                    continue
                add(f"tie_last_at_{where}", P + 300, _set(shape, P + 300, 6), eq=6, ka=6, run_at=slot)
                add(f"tie_first_at_{where}", P + 300, ("replay", "tied"), eq=6, ka=1, run_at=slot)
                add(f"tie_mid_at_{where}", P + 300, ("replay", "tied"), eq=6, ka=3, run_at=slot)
    # the smallest count that resamples: floor(1.3 k) + 1
    _add("min_count", floor13(100) + 1, 100, 1.0, 5000, _set((1, 1, 1, False), 5000))


D_COUNT = (9 << K_SET_LO0) + 17


def _count_rows():
    def one(c, k, shape, layout, N=None):
        _add(f"count_{c}_k{k}", c, k, 1.0, D_COUNT, _set(shape, D_COUNT), layout=layout, N=N)

    def coop(c, k, shape, layout, hows=("first", "last", "waves")):
        for how in hows:
            _add(f"count_{c}_k{k}_{how}", c, k, 1.0, D_COUNT, _set(shape, D_COUNT), how=how, G=shape[1], layout=layout)
    # capacity 12799: one workgroup launched
    one(1023, 200, (1, 1, 1, False), "scattered")
    one(1024, 200, (1, 1, 1, False), "scattered")
    one(1025, 200, (1, 1, 2, False), "edges3")
    # capacity 19199: four launched, one runs (workgroups 1-3 return at b >= G)
    one(1023, 300, (4, 1, 1, False), "scattered")
    one(1024, 300, (4, 1, 1, False), "edges0")
    one(1025, 300, (4, 1, 2, False), "scattered")
    one(16383, 300, (4, 1, 16, False), "dense", N=19199)        # N == the capacity
    one(16384, 300, (4, 1, 16, False), "scattered")
    coop(16385, 300, (4, 4, 5, False), "dense")                 # 17 rounds: the last stretch holds 2, the last round one key
    coop(65536, 2000, (8, 4, 16, False), "scattered")
    coop(65537, 2000, (8, 5, 13, False), "dense")
    coop(262144, 8000, (32, 16, 16, False), "dense")
    coop(262145, 8000, (32, 17, 16, False), "dense")
    coop(2097152, 100000, (128, 128, 16, False), "dense")       # the largest set that stays in registers
    coop(2097153, 100000, (128, 128, 17, True), "dense")        # OVF; stretches 121.. are empty
    coop(8388608, 1000000, (128, 128, 64, True), "dense")       # 48 rounds per stretch from L2
    _add("count_8388609_k1000000", 8388609, 1000000, 1.0, D_COUNT, ("replay", "rounds"), layout="dense")


_key_rows()
_count_rows()


def make(c, k, t, D, eq=1, ka=None, above=(), below=(), how="random", G=1, run_at=None, seed=0):
    """Candidate values in queue order (float32, seeded signs) from ``design`` and ``place``."""
    keys = design(c, k, D, eq, ka, above, below, seed)
    off = place(keys, how, G, run_at, seed + 1)
    rng = np.random.default_rng(seed + 2)
    v = f32_of(key_of(t) + off)
    return np.where(rng.random(c) < 0.5, -v, v).astype(F32)


@functools.lru_cache(maxsize=4)
def candidates(name):
    """The row's candidate values in queue order."""
    r = ROW_BY_NAME[name]
    v = make(r.c, r.k, r.t, r.D, r.eq, r.ka, r.above, r.below, r.how, r.G, r.run_at, zlib.crc32(name.encode()) % 100000)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=2)
def build(name):
    """(row, candidate values, the embedded gradient) of a row of ROWS."""
    r = ROW_BY_NAME[name]
    v = candidates(name)
    e = embed(v, r.k, r.layout, r.N, r.t, zlib.crc32(name.encode()) % 1000)
    for a in (e.vec, e.mmt, e.pos):
        a.setflags(write=False)
    return r, v, e


def on_lattice(values, numel, attrs, start, seed=0):
    """The candidates ``values`` (queue order) in a gradient of ``numel`` elements whose strided
    sample ``start::stride`` holds exactly ks = top_k_samples of them, the smallest among these:
    the sampled threshold is that value, and every candidate and nothing else counts at it. The
    smallest candidate changes places with another one below the k-th key, so the top k stay
    where ``place`` put them. Returns (gradient, the candidates' positions, their values in queue order)."""
    _, k, _, ks, stride = attrs
    c = values.size
    rng = np.random.default_rng(seed)
    lattice = np.arange(start, numel, stride)
    off = np.setdiff1d(np.arange(numel), lattice)
    pos = np.sort(np.concatenate([rng.choice(lattice, ks, replace=False), rng.choice(off, c - ks, replace=False)]))
    values = values.copy()
    mag = np.abs(values)
    low, kth = mag.min(), np.sort(mag)[-k]
    if low < kth:
        sampled = np.flatnonzero(((pos - start) % stride == 0) & (mag < kth))
        a, b = int(np.argmin(mag)), int(sampled[rng.integers(sampled.size)])
        values[[a, b]] = values[[b, a]]
    t = float(low)
    g = (rng.uniform(0.01, 0.9, numel) * t).astype(F32) * np.where(rng.random(numel) < 0.5, F32(-1), F32(1))
    g[pos] = values
    on = np.abs(g[lattice])
    assert np.count_nonzero(on >= low) == ks and low in on and np.count_nonzero(np.abs(g) >= low) == c
    return g, pos, values


def cand_cap(N, k):
    """select_types.hpp nth_cand_cap."""
    return min(N, 64 * k - 1)
