"""Median-of-3 killer candidate sets: inputs that drive libstdc++'s introselect to its
depth limit (CPU only, numpy).

torch's CPU topk runs ``std::nth_element`` over the resample's candidates, and K5
(csrc/introselect.hpp) replays it. ``std::__introselect`` counts a depth limit of
``2 * lg(n)`` down and at zero leaves its partition loop for ``__heap_select`` +
``iter_swap(first, nth)``. On seeded normal, tied or bf16 data the Hoare partitions halve
the range and the limit is never reached, so none of the kernel's five copies of that exit
(one per phase of the replay) runs. This module builds the inputs that reach them:

``scalar_nth_element``
    libstdc++'s ``nth_element`` restated element by element and driven by a comparator
    callback (``__introselect``, ``__move_median_to_first``, ``__unguarded_partition``,
    ``__heap_select``, ``__insertion_sort``), recording the trace oracle/introselect.py's
    ``nth_element(trace=...)`` records from its data-parallel form.
``killer``
    a McIlroy "antiquicksort" adversary (M. D. McIlroy, A Killer Adversary for Quicksort,
    1999) run against that restatement: an element's value is decided only when a
    comparison needs it ("gas" until then), and the element the partition is about to use
    as its pivot is frozen to the extreme value still free, so every step strips about
    two elements off the front of the range. ``block``: the block-lexicographic variant —
    elements outside a target block have fixed ranks above or below it and partition well,
    the block that holds the nth is gas — which reaches the limit after the range has
    shrunk into a later phase.
``embed``
    the candidates at increasing positions of a gradient whose other elements lie below
    the threshold, with the attributes that take ``dgc_select`` to the replay.
``phases``
    the device phase (csrc/introselect.hpp's, by the size of the range) of every step of a
    trace and of its exit.
``CASES``
    the table tests/test_killer_cpu.py confirms and tests/test_gpu_killer.py runs.
"""
import functools
import re
import zlib
from collections import namedtuple
from pathlib import Path

import numpy as np

from oracle import dgc_oracle as O
from oracle import introselect as I

F32 = np.float32

# Copies of the kernels' phase bounds (test_killer_cpu.py reads the constexpr lines and
# fails when one drifts).
K_NTH_LDS = 12288          # introselect.hpp kNthLds: larger ranges are partitioned in global memory
K_NTH_WAVE = 1024          # introselect.hpp kNthWave: ranges up to it are finished by one wave
K_WAVE = 64                # dgc_common.hpp kWave: ranges up to it are finished in registers
K_NTH_G_MIN_CAND = 98304   # select.hip kNthGMinCand: more candidates start on several workgroups

CSRC = Path(__file__).resolve().parents[1] / "adam-compression_amd" / "csrc"
CONSTANTS = {   # name -> (file, our copy)
    "kNthLds": ("introselect.hpp", K_NTH_LDS),
    "kNthWave": ("introselect.hpp", K_NTH_WAVE),
    "kWave": ("dgc_common.hpp", K_WAVE),
    "kNthGMinCand": ("select.hip", K_NTH_G_MIN_CAND),
}


def header_constant(name):
    """The value of ``constexpr <type> name = <integer>;`` in the file CONSTANTS names."""
    text = (CSRC / CONSTANTS[name][0]).read_text()
    m = re.findall(r"^\s*constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), text, re.M)
    assert len(m) == 1, f"{name}: {len(m)} constexpr definitions in {CONSTANTS[name][0]}"
    return int(m[0])


def _lg(n):
    return int(n).bit_length() - 1


# ------------------------------------------------------------------ libstdc++, scalar
def _swap(q, a, b):
    q[a], q[b] = q[b], q[a]


def _move_median_to_first(q, result, a, b, c, comp):
    if comp(q[a], q[b]):
        if comp(q[b], q[c]):
            _swap(q, result, b)
        elif comp(q[a], q[c]):
            _swap(q, result, c)
        else:
            _swap(q, result, a)
    elif comp(q[a], q[c]):
        _swap(q, result, a)
    elif comp(q[b], q[c]):
        _swap(q, result, c)
    else:
        _swap(q, result, b)


def _unguarded_partition(q, first, last, pivot, comp):
    while True:
        while comp(q[first], q[pivot]):
            first += 1
        last -= 1
        while comp(q[pivot], q[last]):
            last -= 1
        if not first < last:
            return first
        _swap(q, first, last)
        first += 1


def _adjust_heap(q, first, hole, n, value, comp):
    top = hole
    second = hole
    while second < (n - 1) // 2:
        second = 2 * (second + 1)
        if comp(q[first + second], q[first + second - 1]):
            second -= 1
        q[first + hole] = q[first + second]
        hole = second
    if (n & 1) == 0 and second == (n - 2) // 2:
        second = 2 * (second + 1)
        q[first + hole] = q[first + second - 1]
        hole = second - 1
    parent = (hole - 1) // 2
    while hole > top and comp(q[first + parent], value):
        q[first + hole] = q[first + parent]
        hole = parent
        parent = (hole - 1) // 2
    q[first + hole] = value


def _heap_select(q, first, middle, last, comp):
    n = middle - first
    if n >= 2:
        parent = (n - 2) // 2
        while True:
            _adjust_heap(q, first, parent, n, q[first + parent], comp)
            if parent == 0:
                break
            parent -= 1
    for i in range(middle, last):
        if comp(q[i], q[first]):
            value = q[i]
            q[i] = q[first]
            _adjust_heap(q, first, 0, n, value, comp)


def _insertion_sort(q, first, last, comp):
    for i in range(first + 1, last):
        value = q[i]
        if comp(value, q[first]):
            q[first + 1:i + 1] = q[first:i]
            q[first] = value
        else:
            j = i
            while comp(value, q[j - 1]):
                q[j] = q[j - 1]
                j -= 1
            q[j] = value


def scalar_nth_element(q, nth, comp, trace=None, finish=True):
    """``std::nth_element(q, q + nth, q + len(q), comp)`` on the list ``q``, in place.

    ``trace`` receives what oracle/introselect.py's records: ``(f, l, depth)`` per step, then
    ``("heap", f, l)`` or ``("insertion", f, l)``. ``finish=False`` stops at the exit (the
    adversary's use: the heap select would only freeze more elements)."""
    first, last = 0, len(q)
    if first == last or nth == last:
        return
    depth = 2 * _lg(last - first)
    while last - first > 3:
        if depth == 0:
            if trace is not None:
                trace.append(("heap", first, last))
            if finish:
                _heap_select(q, first, nth + 1, last, comp)
                _swap(q, first, nth)
            return
        if trace is not None:
            trace.append((first, last, depth))
        depth -= 1
        mid = first + (last - first) // 2
        _move_median_to_first(q, first, first + 1, mid, last - 1, comp)
        cut = _unguarded_partition(q, first + 1, last, first, comp)
        if cut <= nth:
            first = cut
        else:
            last = cut
    if trace is not None:
        trace.append(("insertion", first, last))
    if finish:
        _insertion_sort(q, first, last, comp)


def scalar_topk_order(values, k, trace=None):
    """The nth_element path of torch's CPU topk through the scalar restatement: the first
    k queue indices (``comp`` = key greater, oracle/introselect.py's keys)."""
    key = I.keys_of(values).tolist()
    q = list(range(len(key)))
    scalar_nth_element(q, k - 1, lambda a, b: key[a] > key[b], trace)
    return np.array(q[:k], np.int64)


def oracle_trace(values, k):
    """The trace of oracle/introselect.py's nth_element on the same queue."""
    key = I.keys_of(values).astype(np.int64)
    trace = []
    I.nth_element(key, np.arange(key.size, dtype=np.int64), k - 1, trace)
    return trace


# ------------------------------------------------------------------ the adversary
class _Adversary:
    """Ranks in the comparator's order (rank 0 = the largest magnitude). ``cls``: 0 an
    element above the block, 1 of the block, 2 below it; ``rank`` is fixed outside the
    block and, inside it, None (gas) until a comparison between two gas elements freezes
    one of them to the next free rank — the one the last comparison touched (the pivot
    candidate), as in McIlroy's aqsort. Gas comes after every frozen block element."""

    def __init__(self, cls, rank):
        self.cls, self.rank = cls, rank
        self.nsolid = 0
        self.candidate = -1

    def _freeze(self, x):
        self.rank[x] = self.nsolid
        self.nsolid += 1

    def comp(self, x, y):
        cls, rank = self.cls, self.rank
        gx = cls[x] == 1 and rank[x] is None
        gy = cls[y] == 1 and rank[y] is None
        if gx and gy:
            self._freeze(x if x == self.candidate else y)
            gx, gy = rank[x] is None, rank[y] is None
        if gx:
            self.candidate = x
        elif gy:
            self.candidate = y
        if cls[x] != cls[y]:
            return cls[x] < cls[y]
        if gx or gy:
            return gy           # the frozen one comes first
        return rank[x] < rank[y]


def killer(n, k, block=None, back=0, tie_gas=False, seed=0):
    """float32 values of n candidates in queue order on which ``nth_element(k - 1)`` under
    "magnitude greater" reaches its depth limit; magnitudes in (1, 2], distinct except for
    the tied gas, signs mixed.

    ``block=None``: the adversary decides every element. Otherwise ``block`` elements are
    the adversary's, at seeded queue positions, and the rest have seeded fixed ranks above
    and below them, with the nth (rank k - 1) ``back`` ranks before the block's last:
    ``k - block + back`` elements rank above the block. ``tie_gas``: the elements still
    gas at the exit — compared with frozen elements only, so any values below those keep
    every comparison made — all get one value; otherwise distinct seeded ones."""
    assert n < 65536, "ranks are spaced 2^-16 apart in (1, 2]"
    rng = np.random.default_rng(seed)
    if block is None:
        block, high = n, 0
        assert back == 0
    else:
        high = k - block + back
    low = n - high - block
    assert high >= 0 and low >= 0 and high <= k - 1 < high + block, (n, k, block, back)
    cls = np.full(n, 1, np.int64)
    rank = [None] * n
    if high or low:
        where = rng.permutation(n)
        for r, j in enumerate(where[:high]):
            cls[j], rank[j] = 0, r
        for r, j in enumerate(where[high:high + low]):
            cls[j], rank[j] = 2, r
    adv = _Adversary(cls.tolist(), rank)
    q = list(range(n))
    scalar_nth_element(q, k - 1, adv.comp, finish=False)
    gas = [j for j in range(n) if adv.cls[j] == 1 and rank[j] is None]
    final = np.empty(n, np.int64)
    for j in range(n):
        if rank[j] is not None:
            final[j] = rank[j] + (0, high, high + block)[adv.cls[j]]
    if gas:
        base = high + adv.nsolid
        final[gas] = base if tie_gas else base + rng.permutation(len(gas))
    mag = (F32(2.0) - final.astype(F32) / F32(65536.0)).astype(F32)
    assert np.unique(mag).size == n - (len(gas) - 1 if tie_gas and gas else 0)
    sign = np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    return (mag * sign).astype(F32)


def shuffled(values, seed=1):
    """The control: the same values in a seeded order (ends in the insertion sort)."""
    return np.random.default_rng(seed).permutation(values)


# ------------------------------------------------------------------ phases
def phase_of(size, n, mode="default"):
    """The device phase that partitions (or heap-selects) a range of ``size`` entries of an
    ``n``-candidate replay. ``mode``: DGC_K5_GLOBAL — "multi", "wg" or "default" (several
    workgroups only above kNthGMinCand candidates)."""
    if size > K_NTH_LDS:
        return "multi" if mode == "multi" or (mode == "default" and n > K_NTH_G_MIN_CAND) else "wg"
    if size > K_NTH_WAVE:
        return "lds"
    if size > K_WAVE:
        return "wave"
    return "regs"


def phases(trace, n, mode="default"):
    """(phase of every step, phase of the exit) of a trace."""
    steps = [phase_of(l - f, n, mode) for f, l, _ in trace[:-1]]
    _, f, l = trace[-1]
    return steps, phase_of(l - f, n, mode)


def path_of(trace, n, mode="default"):
    """The phases a trace passes through, in order, the exit's last: "lds>wave>regs"."""
    steps, last = phases(trace, n, mode)
    out = []
    for p in steps + [last]:
        if not out or out[-1] != p:
            out.append(p)
    return ">".join(out)


# ------------------------------------------------------------------ embedding
Embedded = namedtuple("Embedded", "vec mmt pos attrs thr")


def embed(values, k, seed=0):
    """The candidates ``values`` at increasing, scattered positions of a gradient of N
    elements; every other element is nonzero, of either sign and below the threshold 1.0
    (the candidates' magnitudes are above it). ``attrs`` = (N, k, S, ks, stride) as
    oracle.attributes lays them out, with N > S so that the selection adapts, and
    ``floor(1.3 k) < c < 64 k`` so that it resamples through nth_element."""
    c = values.size
    assert O.adapt_bounds(k)[0] < c < 64 * k, (c, k)
    rng = np.random.default_rng(seed)
    N = 3 * c + 1031 + int(rng.integers(0, 7))
    pos = np.sort(rng.choice(N, c, replace=False))
    assert np.any(np.diff(pos) > 1)
    vec = rng.uniform(0.01, 0.9, N).astype(F32) * np.where(rng.random(N) < 0.5, F32(-1), F32(1))
    vec[pos] = values
    mmt = (rng.standard_normal(N).astype(F32) + F32(3.0)).astype(F32)
    stride = 8
    return Embedded(vec.astype(F32), mmt, pos, (N, k, N // stride, max(1, k // stride), stride), F32(1.0))


# ------------------------------------------------------------------ the cases
# name, n, k, block, back, the phases (with the global phase on one workgroup) the
# classifier must confirm, the exit's last. The seed of a case is derived from its name.
Case = namedtuple("Case", "name n k block back path")


@functools.lru_cache(maxsize=None)
def build(name, tie_gas):
    """(values, trace) of a case of CASES, distinct or with tied gas."""
    c = CASE_BY_NAME[name]
    values = killer(c.n, c.k, c.block, c.back, tie_gas=tie_gas, seed=zlib.crc32(name.encode()) % 1000)
    values.setflags(write=False)
    return values, oracle_trace(values, c.k)


def heap_mid(trace, k):
    """The heap size of the exit's heap select: nth + 1 - f."""
    return k - trace[-1][1]


CASES = []   # filled below
CASE_BY_NAME = {}


def _add(*rows):
    for r in rows:
        c = Case(*r)
        CASES.append(c)
        CASE_BY_NAME[c.name] = c


_add(
    # the adversary over all n: the exit range is n minus two per step
    ("regs_only", 56, 30, None, 0, "regs"),
    ("wave_regs", 80, 41, None, 0, "wave>regs"),
    ("wave_65", 90, 50, None, 0, "wave"),
    ("wave_1024", 1024, 300, None, 0, "wave"),
    ("lds_1025_low", 1070, 41, None, 0, "lds"),        # heap of one entry (mid = 1)
    ("lds_1025_high", 1070, 823, None, 0, "lds"),      # the largest k with floor(1.3 k) < c
    ("lds_12288_low", 12288, 193, None, 0, "lds"),     # the smallest k with c < 64 k
    ("lds_12288_high", 12288, 9452, None, 0, "lds"),
    ("wg_13000", 13000, 300, None, 0, "wg"),
    ("wg_40000", 40000, 700, None, 0, "wg"),
    # block-lexicographic: the limit is reached after the range has shrunk
    ("lds_wave_regs_26", 5000, 100, 65, 10, "lds>wave>regs"),
    ("lds_wave_regs_mid1", 5000, 100, 60, 28, "lds>wave>regs"),
    ("lds_wave_regs_mid2", 5000, 101, 60, 29, "lds>wave>regs"),
    ("lds_wave_regs_mid3", 5000, 101, 86, 44, "lds>wave>regs"),
    ("lds_wave_65", 5000, 101, 100, 41, "lds>wave"),
    ("lds_wave_1024", 5000, 300, 1050, 815, "lds>wave"),            # exit range 1018
    ("wg_lds_12288_low", 40000, 701, 12292, 12239, "wg>lds"),       # exit range 12249, mid 1
    ("wg_lds_12288_high", 40000, 12700, 12264, 116, "wg>lds"),      # exit range 12253, mid 12100
    ("wg_lds_wave_65", 13000, 301, 100, 36, "wg>lds>wave"),
    ("wg_lds_wave_1024", 13000, 300, 1040, 795, "wg>lds>wave"),
    ("wg_lds_1025_low", 13000, 302, 1055, 1010, "wg>lds"),
    ("wg_lds_1025_high", 13000, 1200, 1065, 3, "wg>lds"),
    ("wg_lds_5000", 40000, 700, 4888, 4284, "wg>lds"),
)
