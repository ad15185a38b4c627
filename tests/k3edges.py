"""K3 edge inputs: key sets and sample windows whose sampled threshold
``t0 = min(topk(|samples|, ks))`` sits on an edge of the radix select (CPU only, numpy).

K3 (csrc/radix_select.hpp, select_thresholds.hpp) picks one of six paths by data: the
one-workgroup select of <= 32768 keys (``rs_small_wg``, two register layouts, pass 0 floored
by the per-thread maxima), the three multi-block passes (11 + 11 + 10-bit digits), and — for a
tensor of more than 32768 samples — K1's sample window: its 4096-bin histogram plus one
gathered bin (``rs_window_hist_wg``), the span-relative digits of ``rs_window_wg`` when the
histogram refuses, the passes over the window when that has more than 65536 keys, and the
passes over the samples when the window is short, overflowed or absent.

Three parts, in the style of staircase.py / killer.py:

(a) ``key_sets()``: float32 arrays plus the k values to ask ``dgc_kth_largest`` for — digit
    edges, floor adversaries for both register layouts, sizes around every loop bound;
(b) ``window_cases()``: whole sample lattices for the compress engines, every ``start::stride``
    element designed relative to a window key ``wk``, the off-lattice bulk far below it, so
    the count at ``t0`` is exactly ``num_selects`` (the ``ok`` branch: K4 / K5 are not the subject);
(c) ``route(case)``: k_rs_small_multi's routing restated. It classifies only — every expected
    value comes from the oracle on the same arrays.
"""
import functools
from collections import namedtuple

import numpy as np

F32, U32 = np.float32, np.uint32
INF_KEY = 0x7F800000
NAN_KEY = 0x7FC00000

# csrc constants (radix_select.hpp, select_layout.hpp)
SMALL_N = 32768           # kSmallN: keys of a one-workgroup select
THREADS = 1024            # kScanThreads
WIN_BINS = 4096           # kWinBins: K1's histogram of the window
WIN_SHIFT = 10            # kWinShift: key units per bin = 1 << 10
WIN_BIN_CAP = 4096        # kWinBinCap: keys of the k-th key's bin gathered on chip
WIN_MAX = 65536           # kWinMax: keys rs_window_wg holds in registers
BIN = 1 << WIN_SHIFT


def f32_of(keys):
    return np.asarray(keys, dtype=np.uint64).astype(U32).view(F32)


def keys_of(x):
    """|x| bit patterns."""
    return np.ascontiguousarray(np.asarray(x, F32)).view(U32) & U32(0x7FFFFFFF)


def signed(x, rng):
    """Random signs: the kernels take |x|."""
    x = np.asarray(x, F32).copy()
    neg = rng.random(x.size) < 0.5
    return np.where(neg, (x.view(U32) | U32(0x80000000)).view(F32), x)


# ================================================================== (a) key sets
KeySet = namedtuple("KeySet", "name x ks")


def _ks(n, *more):
    return tuple(sorted({k for k in (1, 2, n - 1, n, (n + 1) // 2) + more if 1 <= k <= n}))


def _around(target, n, rng, lo_only=False, hi_only=False):
    """n keys: ``target`` once, the rest on both sides of it (half of them within 2048 units,
    sharing its upper digits; half anywhere finite). Returns (keys, rank of target, 1-based)."""
    t = int(target)
    hi_room, lo_room = INF_KEY - 1 - t, t        # finite keys above / keys below
    n_hi = 0 if (hi_room <= 0 or lo_only) else ((n - 1) if (lo_room <= 0 or hi_only) else (n - 1) // 2)
    n_lo = 0 if lo_room <= 0 or hi_only else n - 1 - n_hi
    n_hi = n - 1 - n_lo
    assert n_hi == 0 or hi_room > 0

    def side(m, room, sign):
        near = rng.integers(1, min(room, 2048) + 1, m // 2)
        far = rng.integers(1, room + 1, m - m // 2)
        return t + sign * np.concatenate([near, far])
    keys = np.concatenate([[t], side(n_hi, hi_room, 1) if n_hi else [], side(n_lo, lo_room, -1) if n_lo else []])
    keys = keys.astype(np.int64)
    rng.shuffle(keys)
    return keys, int((keys > t).sum()) + 1


def _digit_sets(rng):
    out = []
    for n in (3001, 40003):   # one workgroup / the multi-block passes
        tag = "wg" if n <= SMALL_N else "mb"
        # the k-th key's digits all-zero / all-one in each pass
        for t in (0x3F800000, 0x3F7FFFFF, 0x00000000, 0x00000001, 0x7F7FFFFF, 0x7F800000):
            keys, r = _around(t, n, rng, lo_only=(t == INF_KEY))
            out.append(KeySet(f"digit_{t:08x}_{tag}", f32_of(keys), _ks(n, r - 1, r, r + 1)))
        # one key on each side of a pass-0 (bit 21), pass-1 (bit 10) and pass-2 (bit 0) boundary
        for p, b in (("p0", 0x3FA00000), ("p1", 0x3F800400), ("p2", 0x3F800401)):
            above, _ = _around(b, n // 2, rng, hi_only=True)
            below, _ = _around(b - 1, n - n // 2, rng, lo_only=True)
            keys = np.concatenate([above, below])
            rng.shuffle(keys)
            r = int((keys > b).sum()) + 1
            assert int((keys == b).sum()) == 1 and int((keys == b - 1).sum()) == 1
            out.append(KeySet(f"boundary_{p}_{tag}", f32_of(keys), _ks(n, r, r + 1)))
        # a run of equal keys: k on its first, a middle and its last member
        a, run = n // 3, n // 5
        v = 0x3E99999A
        keys = np.concatenate([v + rng.integers(1, 1 << 22, a), np.full(run, v),
                               v - rng.integers(1, 1 << 22, n - a - run)])
        rng.shuffle(keys)
        out.append(KeySet(f"run_{tag}", f32_of(keys), _ks(n, a, a + 1, a + run // 2, a + run, a + run + 1)))
        # +-0 mixed with denormals and small keys
        nz = n // 4
        keys = np.concatenate([np.zeros(n - nz, np.int64), rng.integers(1, 0x00800010, nz)])
        rng.shuffle(keys)
        out.append(KeySet(f"zeros_{tag}", f32_of(keys), _ks(n, nz, nz + 1)))
        # NaN present: k = 1 and k = n (and every k between) give NaN
        keys, _ = _around(0x3F000000, n, rng)
        keys[n // 2] = 0x7FC00001
        out.append(KeySet(f"nan_{tag}", f32_of(keys), (1, n)))
    return out


def owner_slots(layout, t, n):
    """Element indices thread t of rs_small_wg holds, for n keys: ``vec`` (16-B loads,
    load_keys4) 4 (t + 1024 j4) + e, ``scalar`` t + 1024 j."""
    if layout == "vec":
        idx = [4 * (t + THREADS * j4) + e for j4 in range(SMALL_N // THREADS // 4) for e in range(4)]
    else:
        idx = [t + THREADS * j for j in range(SMALL_N // THREADS)]
    return np.array([i for i in idx if i < n], np.int64)


def _floor_sets(rng):
    """rs_small_wg floors pass 0 at the bin of the k-th largest per-thread maximum."""
    out = []
    small = lambda m: 0x3A800000 + rng.integers(0, 1 << 22, m)   # ~1e-3: many pass-0 bins below # noqa: E731
    big = lambda m: 0x44800000 + rng.integers(0, 1 << 22, m)     # ~1e3 # noqa: E731
    for layout in ("vec", "scalar"):
        # all k largest keys in ONE thread's slots: the maxima's k-th largest is a small key
        for n in (SMALL_N, 20003):
            keys = small(n)
            mine = owner_slots(layout, 5, n)
            top = mine[:20]
            keys[top] = big(top.size)
            out.append(KeySet(f"floor_one_thread_{layout}_{n}", f32_of(keys), _ks(n, 19, 20, 21, mine.size)))
        # exactly one large key in each of the 1024 threads: the floor applies at k = 1023 and
        # 1024 and not at 1025
        n = SMALL_N
        keys = small(n)
        for t in range(THREADS):   # ... all in one pass-0 bin, the smallest of them that bin's first key:
            mine = owner_slots(layout, t, n)   # at k = 1024 the k-th key IS the floor
            keys[mine[rng.integers(0, mine.size)]] = 0x44800000 + (0 if t == 777 else rng.integers(1, 1 << 21))
        out.append(KeySet(f"floor_one_each_{layout}", f32_of(keys), (1, 1023, 1024, 1025, n)))
    # k greater than the number of threads that hold a key (no floor): n < 1024 in the 16-B
    # layout (n / 4 threads hold keys); the scalar layout holds one per thread up to 1024
    keys = np.concatenate([small(350), big(350)])
    rng.shuffle(keys)
    out.append(KeySet("floor_none_vec_700", f32_of(keys), (1, 175, 176, 177, 350, 351, 700)))
    keys = np.concatenate([small(750), big(750)])
    rng.shuffle(keys)
    out.append(KeySet("floor_none_scalar_1500", f32_of(keys), (1, 750, 751, 1024, 1025, 1500)))
    return out


ONE_WG_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 32765, 32766, 32767, 32768)
MULTI_SIZES = (32769, 32771, 4096 * 9 - 1, 4096 * 9 + 1, 4096 * 512 - 1, 4096 * 512 + 1, 4096 * 512 * 8 + 3)


def _size_sets(rng):
    out = []
    for n in ONE_WG_SIZES + MULTI_SIZES:
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(F32)
        coarse = rng.random(n) < 0.125           # ties: an eighth of the keys keep 6 mantissa bits
        x[coarse] = (x[coarse].view(U32) & U32(0xFFFE0000)).view(F32)
        x[n - 1] = F32(37.5) if n > 1 else x[n - 1]   # the largest key is the last element
        out.append(KeySet(f"size_{n}", x, _ks(n)))
    return out


@functools.lru_cache(maxsize=None)
def key_sets():
    """Every key set of part (a), generated once (treat the arrays as read-only)."""
    rng = np.random.default_rng(20240521)
    sets = _digit_sets(rng) + _floor_sets(rng) + _size_sets(rng)
    out = {}
    for s in sets:
        x = signed(s.x, rng)
        x.setflags(write=False)
        assert s.name not in out
        out[s.name] = KeySet(s.name, x, s.ks)
    return out


# ================================================================== (b) window cases
N_W = 140_000             # stride 4: S = 35000, win_cap 6283
N_WBIG = 4_000_000        # stride 4: S = 1e6, win_cap 66596 > kWinMax
STRIDE = 4
K_W, K_WBIG = 300, 5500   # num_selects of the rows at N_W / N_WBIG (one workspace layout per size)
WK = 0x3F800000           # the window key: 1.0f; bins 0 .. 4093 end below 1.5f
OVER = WK + (WIN_BINS - 2) * BIN   # the first key past the binned range (bin kWinBins - 2)


def win_cap_of(S):
    """select_layout.hpp: a window for S + 1 > kSmallN samples, min(S + 1, (S + 1) / 16 + 4096) slots."""
    return min(S + 1, (S + 1) // 16 + 4096) if S + 1 > SMALL_N else 0


WinCase = namedtuple("WinCase", "name N start stride ks k grad spec0 spec2 route window_keys t0_key expect")


def _lattice_case(name, N, ks, win, *, route, seed, below=(), wk=WK, start=1, k=None, spec_from=2, expect=None,
                  stride=STRIDE, dtype="float32", fill_to=None, padded=False):
    """A gradient of N elements whose sample lattice ``start::stride`` holds exactly the keys
    ``win`` (all >= wk) and ``below`` (< wk) as designed samples, every other element bulk in
    [wk / 64, wk / 32) (rounded to ``dtype``). The first and the last sample are designed ones.
    ``fill_to``: off-lattice elements above the k-th key bring the count at t0 up to it."""
    rng = np.random.default_rng(seed)
    win, below = np.asarray(win, np.int64), np.asarray(below, np.int64)
    assert (win >= wk).all() and (below < wk).all()
    S_act = -(-(N - start) // stride)
    designed = np.concatenate([win, below])
    rng.shuffle(designed)
    pos = rng.permutation(np.arange(1, S_act - 1))[:designed.size - 2]
    pos = np.concatenate([[0, S_act - 1], pos])[:designed.size]
    wkf = float(f32_of([wk])[0])
    g = rng.uniform(wkf / 64, wkf / 32, N).astype(F32)
    if dtype != "float32":
        from oracle import dgc_oracle as O
        g = O.round16(g, dtype)
    g[start + stride * pos] = f32_of(designed)
    keys = np.sort(designed)[::-1]
    has_nan = bool((designed > INF_KEY).any())
    t0_key = NAN_KEY if has_nan else int(keys[ks - 1])
    n_at = 0 if has_nan else int((designed >= t0_key).sum())
    if fill_to is not None and fill_to > n_at:   # off the lattice, at twice the k-th key's value
        off = rng.permutation(N)[:2 * (fill_to - n_at) + 8]
        off = off[(off - start) % stride != 0][:fill_to - n_at]
        g[off] = F32(2) * f32_of([t0_key])[0]
        n_at = fill_to
    g = signed(g, rng)
    g.setflags(write=False)
    k = k if k is not None else n_at
    cnt = int(win.size)
    S = N // stride
    windowed = win_cap_of(S) > 0 and (N % 4 == 0 or padded)
    complete = windowed and ks <= cnt <= win_cap_of(S)
    spec = (F32(np.inf), f32_of([wk])[0]) if spec_from == 2 else (f32_of([wk])[0], F32(np.inf))
    e = dict(cnt=cnt, count_at_t0=n_at, S=S, samples=S_act, win_cap=win_cap_of(S))
    e.update(expect or {})
    return WinCase(name, N, start, stride, ks, k, g, spec[0], spec[1], route, cnt if complete else 0, t0_key, e)


def _spread(rng, lo, hi, m):
    """m keys in [lo, hi)."""
    return rng.integers(lo, hi, m) if m > 0 else np.empty(0, np.int64)


def _bin_full(rng, b, total, n_top, tie_at):
    """``total`` keys of bin b: the top ``n_top`` are >= sub-bin ``tie_at`` — one per sub-bin
    above it and a tied pair on it —, the rest fall below it with every sub-bin used."""
    lo = WK + b * BIN
    top = np.concatenate([lo + np.arange(tie_at + 1, tie_at + n_top - 1), [lo + tie_at] * 2])
    assert top.size == n_top and top.max() < lo + BIN
    rest = np.concatenate([lo + np.arange(tie_at), lo + rng.integers(0, tie_at, total - n_top - tie_at)])
    return np.concatenate([top, rest])


def _n_w_cases():
    S = N_W // STRIDE
    cap = win_cap_of(S)
    assert S + 1 > SMALL_N and 4097 + 600 < cap < WIN_MAX, cap
    rng = np.random.default_rng(7)
    ks = K_W
    in_range = lambda m: _spread(rng, WK + BIN, OVER - BIN, m)   # noqa: E731
    C = []

    def add(name, ks_, win, **kw):
        C.append(_lattice_case(name, kw.pop("N", N_W), ks_, win, seed=1000 + len(C), **kw))

    kth = WK + 700 * BIN + 123
    top = _spread(rng, kth + 1, OVER, ks - 1)
    # exactly ks keys >= wk, the k-th the smallest of the window
    add("eq_ks", ks, np.concatenate([top, [kth]]), route="hist", below=[WK - 1, WK - 2])
    # the same window, its key read from spec[0] (spec[2] still inf: before the first prediction)
    add("eq_ks_spec0", ks, np.concatenate([top, [kth]]), route="hist", below=[WK - 1], spec_from=0)
    # ks - 1 keys >= wk and a sample one ulp below it: the window is short
    add("short", ks, top, route="samples", below=[WK - 1, WK - 5000])
    # the k-th key IS wk: bin 0, sub-bin 0
    add("at_wk", ks, np.concatenate([top, [WK]]), route="hist", below=[WK - 1])
    # cnt == win_cap / win_cap + 1
    for name, cnt, r in (("cap", cap, "hist"), ("cap+1", cap + 1, "samples")):
        add(name, ks, np.concatenate([top, [kth], _spread(rng, WK, kth, cnt - ks)]), route=r, below=[WK - 1])
    # the k-th key in the last served bin / the first refused one
    for name, key, r in (("bin_4093", OVER - 1, "hist"), ("bin_4094", OVER, "window_wg")):
        win = np.concatenate([_spread(rng, OVER + 1, OVER + 40 * BIN, ks - 1), [key], in_range(900)])
        add(name, ks, win, route=r, below=[WK - 1], expect=dict(kth_bin=min((key - WK) >> WIN_SHIFT, WIN_BINS - 2)))
    # the k-th key's bin holds 4096 / 4097 keys, distinct sub-bins and ties in it; the k-th key
    # is the first of a tied pair on sub-bin 925
    b = 2000
    above = _spread(rng, WK + (b + 1) * BIN, OVER, 200)
    for name, total, r in (("bin_4096", WIN_BIN_CAP, "hist"), ("bin_4097", WIN_BIN_CAP + 1, "window_wg")):
        win = np.concatenate([above, _bin_full(rng, b, total, 100, 925), _spread(rng, WK, WK + b * BIN, 400)])
        add(name, ks - 1, win, route=r, below=[WK - 1], expect=dict(kth_bin=b, kth_bin_count=total, ties_at_t0=2))
    # k on the first / a middle / the last member of a run of equal keys inside one bin
    run, v = 60, WK + 1500 * BIN + 511
    a = ks - run
    win = np.concatenate([_spread(rng, v + 1, OVER, a), np.full(run, v), _spread(rng, WK, v, 500)])
    for name, ks_ in (("ties_first", a + 1), ("ties_mid", a + run // 2), ("ties_last", a + run)):
        add(name, ks_, win, route="hist", below=[WK - 1], expect=dict(ties_at_t0=run))
    # infinite samples: fewer than ks of them (the k-th key is in range) / at least ks
    n_inf = 40
    win = np.concatenate([np.full(n_inf, INF_KEY), _spread(rng, kth + 1, OVER, ks - 1 - n_inf), [kth], in_range(0)])
    add("inf_few", ks, win, route="hist", below=[WK - 1])
    win = np.concatenate([np.full(ks, INF_KEY), in_range(700), [WK + 3]])
    add("inf_many", ks - 50, win, route="window_wg", below=[WK - 1], expect=dict(span=INF_KEY - (WK + 3)))
    # one NaN sample in the window: t0 is NaN
    add("nan", ks, np.concatenate([top, [kth, 0x7FC00001]]), route="hist", below=[WK - 1], k=K_W)
    # rs_window_wg by the span of its keys: zero, one, two, two and three digit passes
    eq = WK + 7 * BIN + 5
    add("span_0", 1234, np.full(WIN_BIN_CAP + 1, eq), route="window_wg", below=[WK - 1],
        expect=dict(span=0, passes=0, kth_bin=7, kth_bin_count=WIN_BIN_CAP + 1))
    mn = OVER + 17
    for span, passes in ((4095, 1), (4096, 2), ((1 << 24) - 1, 2), (1 << 24, 3)):
        body = mn + np.minimum(rng.integers(0, span + 1, 1500), rng.integers(0, span + 1, 1500))
        body[:40] = body[40:80]                     # ties
        win = np.concatenate([[mn, mn + span], body])
        name = {4095: "span_4095", 4096: "span_4096", (1 << 24) - 1: "span_2p24m1", 1 << 24: "span_2p24"}[span]
        add(name, ks, win, route="window_wg", below=[WK - 1],
            expect=dict(span=span, passes=passes, kth_bin=WIN_BINS - 2))
    # N_W + 1 elements, unpadded: the scalar tail's samples are written outside K1, no window
    add("tail", ks, np.concatenate([top, [kth]]), route="samples", below=[WK - 1], N=N_W + 1)
    # S + 1 == 32768: rs_small_wg with every register slot used (start 0: 32768 samples);
    # S + 1 == 32769: the smallest windowed tensor
    add("edge_S_32768", ks, np.concatenate([top, [kth]]), route="small", below=[WK - 1], N=4 * 32768 - 1, start=0)
    add("edge_S_32769", ks, np.concatenate([top, [kth]]), route="hist", below=[WK - 1], N=4 * 32768)
    return C


def _n_wbig_cases():
    S = N_WBIG // STRIDE
    cap = win_cap_of(S)
    assert cap > WIN_MAX + 1, cap
    rng = np.random.default_rng(11)
    ks = K_WBIG
    C = []

    def add(name, ks_, win, **kw):
        C.append(_lattice_case(name, N_WBIG, ks_, win, seed=2000 + len(C), below=[WK - 1], **kw))

    kth = WK + 3000 * BIN + 77
    # more than 65536 keys, the k-th key in range: the histogram serves what rs_window_wg could not hold
    win = np.concatenate([_spread(rng, kth + 1, OVER + 9 * BIN, ks - 1), [kth], _spread(rng, WK, kth, 66000 - ks)])
    add("big_hist", ks, win, route="hist")
    # cnt == 65536 with the k-th key in a bin of 5000 ties: rs_window_wg at its full 64 keys per thread
    v = WK + 2500 * BIN + 300
    win = np.concatenate([_spread(rng, v + BIN, OVER, 500), np.full(5000, v),
                          _spread(rng, WK, v - BIN, WIN_MAX - 5500)])
    add("big_wg", 3000, win, route="window_wg", expect=dict(kth_bin=2500, kth_bin_count=5000, ties_at_t0=5000))
    # cnt == 65537 with the k-th key past the binned range: the passes over the window, 17 workgroups
    win = np.concatenate([_spread(rng, OVER + 1, OVER + 3000 * BIN, ks - 1), [OVER],
                          _spread(rng, WK, OVER, WIN_MAX + 1 - ks)])
    add("big_passes", ks, win, route="window_passes", expect=dict(kth_bin=WIN_BINS - 2, blocks=17))
    # ... and with the k-th key in a crowded bin of distinct keys and ties
    b = 1000
    win = np.concatenate([_spread(rng, WK + (b + 1) * BIN, OVER, ks - 100), _bin_full(rng, b, 4500, 100, 800),
                          _spread(rng, WK, WK + b * BIN, WIN_MAX + 1 - (ks - 100) - 4500)])
    add("big_passes_bin", ks - 1, win, route="window_passes",
        expect=dict(kth_bin=b, kth_bin_count=4500, ties_at_t0=2, blocks=17))
    return C


@functools.lru_cache(maxsize=None)
def window_cases(which="all"):
    """The table's rows by name, generated once per process. ``which``: "w" (N_W and the edge
    sizes), "big" (N_WBIG) or "all"."""
    rows = (_n_w_cases() if which in ("w", "all") else []) + (_n_wbig_cases() if which in ("big", "all") else [])
    assert len({c.name for c in rows}) == len(rows)
    return {c.name: c for c in rows}


# ------------------------------------------------------------------ rows for the other engines
KEY_STEP = {"float32": 1, "float16": 1 << 13, "bfloat16": 1 << 16}   # key units between values in [1, 2)
ENGINE_ROWS = {"eq_ks": "hist", "bin_4094": "window_wg", "bin_4097": "window_wg", "cap+1": "samples"}


@functools.lru_cache(maxsize=None)
def smallest_windowed_numel(ratio=0.001):
    """The smallest N whose reference attributes (1 % sample) give S + 1 > kSmallN samples
    (3178496 at 0.001: stride 97, S = 32768; S does not fall again above it)."""
    from oracle import dgc_oracle as O
    n = 90 * SMALL_N
    while O.attributes(n, ratio)[2] + 1 <= SMALL_N:
        n += 1
    return n


@functools.lru_cache(maxsize=32)
def engine_row(kind, attrs, start, wk, dtype="float32", seed=0):
    """A row of ENGINE_ROWS for a tensor with the reference's own attributes (its stride, its
    top_k_samples) and any window key, keys representable in ``dtype``: a 16-bit format's keys
    are ``KEY_STEP`` units apart, so a 1024-unit bin holds one value and ``bin_4097`` is 4097
    equal samples. Off-lattice elements bring the count at t0 up to num_selects where the
    lattice holds fewer (the ``ok`` branch). ``eq_ks`` also serves a tensor too small for a
    window (route "small")."""
    N, k, S, ks, stride = attrs
    u = KEY_STEP[dtype]
    assert wk % u == 0 and (win_cap_of(S) > 0 or kind == "eq_ks")
    rng = np.random.default_rng(seed)
    over = wk + -(-((WIN_BINS - 2) * BIN) // u) * u      # the first representable key past the binned range
    grid = lambda lo, hi, m: lo + u * rng.integers(0, max(1, (hi - lo) // u), m)   # noqa: E731
    kth = wk + 16 * u if u > 1 else wk + 700 * BIN + 123
    below = [wk - u]
    expect = {}
    if kind == "eq_ks":
        win = np.concatenate([grid(kth + u, over, ks - 1), [kth]])
    elif kind == "cap+1":
        win = np.concatenate([grid(kth + u, over, ks - 1), [kth], grid(wk, kth, win_cap_of(S) + 1 - ks)])
    elif kind == "bin_4094":
        win = np.concatenate([grid(over + u, over + 40 * u * (1 if u > 1 else BIN), ks - 1), [over],
                              grid(wk, over, 900)])
        expect = dict(kth_bin=WIN_BINS - 2)
    elif kind == "bin_4097":
        a = ks // 3
        if u == 1:
            b = 2000
            body = _bin_full(rng, b, WIN_BIN_CAP + 1, ks - a + 1, 925) - WK + wk
            win = np.concatenate([grid(wk + (b + 1) * BIN, over, a), body, grid(wk, wk + b * BIN, 400)])
            expect = dict(kth_bin=b, kth_bin_count=WIN_BIN_CAP + 1, ties_at_t0=2)
        else:
            v = wk + 24 * u
            win = np.concatenate([grid(v + u, over, a), np.full(WIN_BIN_CAP + 1, v), grid(wk, v, 400)])
            expect = dict(kth_bin=(v - wk) >> WIN_SHIFT, kth_bin_count=WIN_BIN_CAP + 1, ties_at_t0=WIN_BIN_CAP + 1)
    else:
        raise KeyError(kind)
    route = ENGINE_ROWS[kind] if win_cap_of(S) else "small"
    return _lattice_case(kind, N, ks, win, route=route, seed=seed + 1, below=below, wk=wk, start=start,
                         stride=stride, dtype=dtype, fill_to=k, k=k, expect=expect, padded=True)


def window_key(case):
    """K1's window key (k1_segment_begin): spec[2] when finite, else the list threshold spec[0]."""
    tw = case.spec2 if np.isfinite(case.spec2) else case.spec0
    return int(keys_of([tw])[0])


def lattice_keys(case):
    return keys_of(case.grad[case.start::case.stride]).astype(np.int64)


# ================================================================== (c) the route
def route(case, padded=False):
    """(route, window_keys) of a case, as k_rs_small_multi / k_rs_reset_samples decide it:
    "small" (rs_small_wg), "samples" (the passes over the samples), "hist"
    (rs_window_hist_wg), "window_wg" (rs_window_wg), "window_passes" (the passes over the
    window). ``padded``: a batch's or a bucket's tensor (whole float4 groups: no scalar tail).
    Classifies only: no expected threshold comes from here."""
    S = case.N // case.stride                  # num_samples the call is given
    if S + 1 <= SMALL_N:
        return "small", 0
    cap = win_cap_of(S)
    if cap == 0 or (case.N % 4 and not padded):   # no window: TDesc::tail
        return "samples", 0
    keys, wk = lattice_keys(case), window_key(case)
    win = keys[keys >= wk]
    cnt = win.size
    if not (case.ks <= cnt <= cap):            # complete?
        return "samples", 0
    if (win > INF_KEY).any():                  # the histogram's NaN bin: NaN at once
        return "hist", cnt
    bins = np.minimum((win - wk) >> WIN_SHIFT, WIN_BINS - 2)
    h = np.bincount(bins, minlength=WIN_BINS)
    above = np.cumsum(h[::-1])                 # keys in bins >= b, from the top
    b = WIN_BINS - 1 - int(np.searchsorted(above, case.ks))
    if b < WIN_BINS - 2 and h[b] <= WIN_BIN_CAP:
        return "hist", cnt
    return ("window_wg" if cnt <= WIN_MAX else "window_passes"), cnt


def window_passes_of(span):
    """rs_window_wg's digit passes over a window of key span ``span``: 12 bits at a time from the top."""
    hi, n = int(span).bit_length(), 0
    while hi > 0:
        hi = hi - 12 if hi > 12 else 0
        n += 1
    return n
