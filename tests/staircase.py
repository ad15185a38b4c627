"""Staircase gradients: inputs whose count at every rung of the selection's
threshold-adaptation ladder is a number the test chose (CPU only, numpy).

The reference's loop (dgc/compression.py:128-149) multiplies the sampled threshold by the
lower bound until the count reaches lower * k. Which rung it stops at, and which branch it
then takes, depends on the counts alone, so a gradient that fixes the counts fixes the
decision. ``staircase`` builds one; ``CASES`` is the table of decisions the GPU tests pin
(tests/test_gpu_adapt_lattice.py); ``assert_case_is_what_it_says`` has the oracle confirm
that a generated case is the one its row names (tests/test_staircase_cpu.py runs it for
every row, the GPU tests before they compare).

With zero momentum / velocity state and ``nesterov=False`` the velocity after compensate
IS the gradient, bit for bit (0 * m + g, then 0 + that), so the selection sees exactly
what was designed.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import dgc_oracle as O

F32 = np.float32
SEG = 1024                # the kernels' segment (select_types.hpp kSeg)
GROUP = 1 << 20           # 1024 segments (kGroupSegs * kSeg)
KCAP = 64                 # list slots per segment (kCap)
SPILL_DIV = 32            # lists dropped when more than nseg / 32 segments spill (kSpillDiv)
LOWER_LISTS = 4           # rungs k_lower_lists serves (kLowerLists)
MAX_LOWER = 16            # rungs of the one multi-threshold pass (kMaxLower)
SPILL_FILL = KCAP + 6     # fillers of a spilled segment

# A sampled threshold whose iterated fp32 ladder lies below fl32(t0 * powf(fl32(0.8), j)) at
# every rung from 2 to 16 (test_staircase_cpu.py checks that it still does): a kernel that
# computed the closed form would miss the element that sits on the rung, one count short of
# what the reference sees there.
T0 = 0.3084999918937683

Stair = namedtuple("Stair", "grad th rungs marks spill_segs t_list")


# ------------------------------------------------------------------ number formats
def round_dtype(x, dtype):
    """fp32 value(s) rounded to ``dtype`` ("float32", "bfloat16", "float16"), as fp32."""
    x = np.asarray(x, F32)
    return x if dtype == "float32" else O.round16(x, dtype)


def pred(x, dtype):
    """The largest value of ``dtype`` below the positive, representable ``x``."""
    x = F32(x)
    if dtype == "float32":
        return np.nextafter(x, F32(0))
    if dtype == "float16":
        return F32(np.nextafter(np.float16(x), np.float16(0)))
    return (x.view(np.uint32) - np.uint32(0x10000)).view(F32)   # bf16: one step of the top 16 bits


def ladder(t0, factor, n, dtype="float32"):
    """th[0] = t0, th[j] = round_dtype(fl32(th[j-1] * fl32(factor))): the reference's iterated
    product (``threshold *= bound`` on a 0-dim tensor of the dtype; csrc thr_mul)."""
    th = [F32(round_dtype(t0, dtype))]
    for _ in range(n):
        th.append(F32(round_dtype(F32(th[-1] * F32(factor)), dtype)))
    return np.array(th, F32)


def _band(rng, lo, hi, n, dtype):
    """n representable magnitudes in [lo, hi)."""
    if n <= 0:
        return np.empty(0, F32)
    v = round_dtype(rng.uniform(float(lo), float(hi), n).astype(F32), dtype)
    return np.clip(v, F32(lo), pred(hi, dtype)).astype(F32)


def layout_marks(N):
    """The positions every staircase puts a designed element at: index 0, the last two
    elements (the last partial segment and the scalar tail), both sides of a segment
    boundary and of every group boundary N has."""
    marks = [0, N - 2, N - 1, SEG - 1, SEG]
    g = GROUP
    while g + 1 < N - 2:
        marks += [g - 1, g]
        g += GROUP
    return marks


# ------------------------------------------------------------------ the generator
def staircase(attrs, start, t0, counts, *, lower=0.8, upper=1.3, max_iters=10, dtype="float32", layout=None,
              seed=0, up=False, zero_bulk=False, bulk_max=None):
    """A gradient of ``attrs[0]`` elements (fp32 array of values representable in ``dtype``)
    with ``#{|x| >= th[j]} == counts[j]`` for every j given.

    ``th`` is the downward ladder from ``t0`` (``lower``; at least ``max_iters`` rungs), or
    with ``up`` the upward one (``upper``, for ``resample=False``: counts then fall).
    The sampled lattice ``start::stride`` holds exactly ``top_k_samples`` elements >= t0 whose
    minimum is t0 — the sampled threshold must come out as t0 — and every other designed
    element sits off it. In each band [th[j], th[j-1]) one element is exactly th[j] and (when
    the band has two) one exactly the value below th[j-1]; one further element is one step
    below the lowest designed rung. The bulk is random, non-zero and below half the lowest
    rung of the ladder (``zero_bulk``: +0.0, and no element below the rungs; ``bulk_max``: also below that). Signs are random.

    ``layout``: ``spill=s`` puts more than kCap fillers in [t_list, lowest rung) — counted by
    no rung — into each of s segments (``t_list`` must be given, below the ladder);
    ``cut_in_spill=j`` makes the first of them the segment that holds the k-th element, in
    index order, of those >= th[j]. ``layout_marks(N)`` always carry designed elements.
    """
    N, k, S, ks, stride = attrs
    lay = dict(layout or {})
    spill, cut, t_list = int(lay.pop("spill", 0)), lay.pop("cut_in_spill", None), lay.pop("t_list", None)
    assert not lay, f"unknown layout keys {sorted(lay)}"
    rng = np.random.default_rng(seed)
    m = len(counts) - 1
    if up:
        th = ladder(t0, upper, m, dtype)
        T, C = th[::-1], list(counts)[::-1]           # descending thresholds, rising counts
        floor_t = th[0]
    else:
        th = ladder(t0, lower, max(m, max_iters), dtype)
        T, C = th[:m + 1], list(counts)
        floor_t = th[max(m, max_iters)]
    t0 = th[0]
    assert all(a <= b for a, b in zip(C, C[1:])), f"counts must not fall along the ladder: {counts}"
    assert all(float(a) > float(b) for a, b in zip(T, T[1:])), "the ladder collapsed in this dtype"
    home = len(T) - 1 if up else 0                     # the band whose lower edge is t0
    in_home = C[home] - (C[home - 1] if home else 0)
    assert in_home >= ks, f"the band above t0 needs the {ks} sampled elements (has {in_home})"

    # --- magnitudes, band by band; per band the exact-rung and the just-below elements first
    lattice_vals, special_vals, free_vals, rungs = None, [], [], {}
    for j in range(len(T)):
        n_j = C[j] - (C[j - 1] if j else 0)
        hi = T[j - 1] if j else F32(4) * T[0]
        vals = []
        if n_j >= 1:
            vals.append(T[j])
        if n_j >= 2 and j:
            vals.append(pred(hi, dtype))
        rest = _band(rng, T[j], hi, n_j - len(vals), dtype)
        if j == home:   # the sampled elements: t0 itself and ks - 1 more of its band
            lattice_vals = np.concatenate([[T[j]], rest[:ks - 1]]).astype(F32)
            special_vals += vals[1:]
            free_vals += list(rest[ks - 1:])
        else:
            special_vals += vals
            free_vals += list(rest)
        rungs[len(T) - 1 - j if up else j] = dict(count=int(C[j]), in_band=int(n_j))
    below = pred(T[-1], dtype)
    if not zero_bulk:   # (a zero-bulk staircase is selected whole: nothing below its rungs)
        special_vals.append(below)
    assert below >= floor_t / F32(2) or up, "one step below the last rung fell into the bulk"

    # --- positions
    on_lattice = lambda p: p >= start and (p - start) % stride == 0   # noqa: E731
    marks = layout_marks(N)
    n_lat = (N - start + stride - 1) // stride
    lat_q = [(p - start) // stride for p in marks if on_lattice(p)]
    pool = np.setdiff1d(rng.permutation(n_lat)[:ks + len(lat_q)], lat_q, assume_unique=False)
    rng.shuffle(pool)
    lat_pos = start + stride * np.concatenate([np.array(lat_q, np.int64), pool[:ks - len(lat_q)]]).astype(np.int64)
    assert lat_pos.size == ks
    off_marks = [p for p in marks if not on_lattice(p)]
    designed = np.array(special_vals + free_vals, F32)          # specials first: they take the marks
    assert designed.size >= len(off_marks), "fewer designed elements than layout marks"

    nseg = -(-N // SEG)
    mark_segs = {p // SEG for p in marks} | {nseg - 1, nseg - 2}
    n_rand = spill - (cut is not None)
    eligible = np.array([s for s in range(2, nseg - 2) if s not in mark_segs])
    spill_segs = list(rng.choice(eligible, n_rand, replace=False)) if n_rand > 0 else []
    taken = np.zeros(N, bool)
    taken[lat_pos] = True
    taken[off_marks] = True
    for s in spill_segs:
        taken[s * SEG:(s + 1) * SEG] = True
    need = designed.size - len(off_marks)
    cand = rng.choice(N, size=min(N, 2 * need + 4096), replace=False)
    cand = cand[~taken[cand] & ((cand - start) % stride != 0)]
    assert cand.size >= need
    pos = np.concatenate([np.array(off_marks, np.int64), cand[:need].astype(np.int64)])

    g = np.zeros(N, F32)
    if not zero_bulk:
        top = floor_t / F32(2) if bulk_max is None else min(floor_t / F32(2), F32(bulk_max))
        g[:] = _band(rng, top / F32(32), top, N, dtype)
        assert float(g.min()) > 0 and float(g.max()) < float(floor_t) / 2
    g[lat_pos] = lattice_vals
    g[pos] = designed
    if cut is not None:   # the segment of the k-th element >= th[cut], in index order, spills
        assert spill >= 1 and not up
        at = np.flatnonzero(g >= th[cut])
        assert at.size > k, "cut_in_spill needs more than k elements at the landed rung"
        spill_segs.insert(0, int(at[k - 1] // SEG))
        assert spill_segs[0] not in mark_segs and spill_segs[0] not in spill_segs[1:], "cut segment collides: reseed"
    if spill:
        assert t_list is not None and float(t_list) < float(floor_t) and float(t_list) > float(floor_t) / 2
        for s in spill_segs:
            free = s * SEG + np.flatnonzero(g[s * SEG:(s + 1) * SEG] < floor_t / F32(2))
            g[rng.choice(free, SPILL_FILL, replace=False)] = _band(rng, t_list, floor_t, SPILL_FILL, dtype)
    g *= rng.choice(np.array([-1, 1], F32), N)
    g += F32(0)   # a zero bulk stays +0.0
    return Stair(g, th, rungs, marks, sorted(int(s) for s in spill_segs), t_list)


# ------------------------------------------------------------------ the cases
# name, counts (an expression in k, L = ceil(0.8 k), U = floor(1.3 k) and pre(n): n counts
# rising from just above top_k_samples, all far below L), selection knobs, then what the
# reference must do on it: the branch and the number of threshold moves (= recounts).
Case = namedtuple("Case", "name counts kw branch moves")


def _cases():
    rows = [
        # no lowering: the first count decides
        Case("ok_L", "[L]", {}, "ok", 0),
        Case("ok_k", "[k]", {}, "ok", 0),
        Case("trunc_k1", "[k + 1]", {}, "trunc", 0),
        Case("trunc_U", "[U]", {}, "trunc", 0),
        Case("resample_U1", "[U + 1]", {}, "resample", 0),
    ]
    # j*: the rung before stays one short of L, the rung itself lands on the edge of a branch
    for j in (1, 2, 4, 5, 9):
        for end, cnt, branch in (("ok", "L", "ok"), ("trunc", "U", "trunc"), ("resample", "U + 1", "resample")):
            rows.append(Case(f"j{j}_{end}", f"pre({j - 1}) + [L - 1, {cnt}]", {}, branch, j))
    rows += [
        Case("j2_ok_k", "pre(1) + [L - 1, k]", {}, "ok", 2),
        Case("j2_trunc_k1", "pre(1) + [L - 1, k + 1]", {}, "trunc", 2),
        # exhausted: ten lowerings, the count at th[10] is never checked
        Case("ex_short", "pre(11)", {}, "exhausted", 10),
        Case("ex_trunc", "pre(10) + [U]", {}, "exhausted", 10),
        Case("ex_over", "pre(10) + [U + 7]", {}, "exhausted", 10),
        # max_iters
        Case("mi0_low", "[L - 1]", dict(max_iters=0), "exhausted", 0),
        Case("mi0_over", "[U + 1]", dict(max_iters=0), "exhausted", 0),
        Case("mi2_ex", "pre(2) + [U + 1]", dict(max_iters=2), "exhausted", 2),
        Case("mi2_j1", "[L - 1, L]", dict(max_iters=2), "ok", 1),
        Case("mi4_none", "pre(5)", dict(max_iters=4), "exhausted", 4),       # no rung reaches L: js = ms
        Case("mi4_last", "pre(3) + [L - 1, U + 1]", dict(max_iters=4), "exhausted", 4),
        Case("mi16_j16", "pre(16) + [U]", dict(max_iters=16), "exhausted", 16),
        Case("mi16_j15", "pre(14) + [L - 1, L]", dict(max_iters=16), "ok", 15),
        Case("mi17_j3", "pre(2) + [L - 1, U]", dict(max_iters=17), "trunc", 3),   # iterative: a recount per step
        Case("mi17_j1_res", "[L - 1, U + 1]", dict(max_iters=17), "resample", 1),
        # resample=False: twice above U, the threshold raised by 1.3 twice, then it lands
        Case("up2_trunc", "[U + 200, U + 100, k + 1]", dict(resample=False, up=True), "trunc", 2),
    ]
    return rows


CASES = {c.name: c for c in _cases()}
ZERO_BULK = Case("warmup", "[k - 3]", {}, "ok", 0)   # every designed element >= t0, count in [L, k]


def case_counts(case, attrs):
    N, k, S, ks, stride = attrs
    U, L = O.adapt_bounds(k)
    counts = eval(case.counts, {"k": k, "L": L, "U": U, "pre": lambda n: [ks + 9 + 10 * i for i in range(n)]})
    assert all(c < L for c in counts[:case.moves]) or case.kw.get("up"), (case.name, counts)
    return counts


def below_ladder(t0, case, dtype="float32"):
    """A list threshold below every rung the case's ladder has (three quarters of the
    lowest; the bulk stays under half of it)."""
    n = 0 if case.kw.get("up") else max(case.moves, case.kw.get("max_iters", 10))
    return F32(F32(0.75) * ladder(t0, 0.8, n, dtype)[-1])


def sample_start(attrs, seed=7):
    """A sample start that keeps index 0 off the lattice (so the mark at 0 is an off-lattice
    element and the lattice begins inside the tensor)."""
    return 1 + (seed * 31) % (attrs[4] - 1)


@functools.lru_cache(maxsize=64)
def generate(name, N, dtype="float32", spill=0, cut=False, ratio=0.001, start=None, t0=T0, zero_bulk=False,
             bulk_max=None):
    """The staircase of a case at N, cached: the GPU tests and the CPU check share one copy
    (treat ``grad`` as read-only). Returns (Stair, attrs, start, counts)."""
    case = ZERO_BULK if name == ZERO_BULK.name else CASES[name]
    attrs = O.attributes(N, ratio)
    start = sample_start(attrs) if start is None else start
    counts = case_counts(case, attrs)
    mi = case.kw.get("max_iters", 10)
    up = case.kw.get("up", False)
    layout = {}
    if spill:
        layout = dict(spill=spill, t_list=below_ladder(t0, case, dtype))
        if cut:
            layout["cut_in_spill"] = case.moves
    seed = (sum(map(ord, name)) * 7919 + N + 13 * spill) % (2 ** 31)
    st = staircase(attrs, start, t0, counts, max_iters=mi, dtype=dtype, layout=layout, seed=seed, up=up,
                   zero_bulk=zero_bulk or case is ZERO_BULK, bulk_max=bulk_max)
    st.grad.setflags(write=False)
    return st, attrs, start, counts


# ------------------------------------------------------------------ the oracle's confirmation
def oracle_run(st, attrs, start, case, dtype="float32"):
    """The reference's decision on the staircase: (thresholds, counts, branch, values,
    indices). fp32: oracle.dgc_oracle.sparsify. 16-bit: oracle.torch_cpu.sparsify on a tensor
    of the dtype with test_gpu_bucket16's oracle_branch for the path, the counts taken at
    the thresholds that path visits."""
    mi, resample = case.kw.get("max_iters", 10), case.kw.get("resample", True)
    if dtype == "float32":
        v, i, info = O.sparsify(st.grad.copy(), attrs, start, max_iters=mi, resample=resample)
        return info["thresholds"], [int(c) for c in info["counts"]], info["branch"], v, i
    import torch
    from oracle import torch_cpu as TC
    from test_gpu_bucket16 import oracle_branch
    assert resample, "the 16-bit oracle path has no resample=False form"
    vec = torch.from_numpy(st.grad.copy()).to(getattr(torch, dtype))
    thr0, trace = oracle_branch(vec, attrs, start, max_iters=mi)
    thr, ths = thr0.clone(), [F32(thr0.float().item())]
    for step in trace:
        if step == "lower":
            thr = thr * 0.8
            ths.append(F32(thr.float().item()))
    cnts = [int(torch.ge(vec.abs(), torch.tensor(float(t), dtype=vec.dtype)).sum()) for t in ths]
    v, i = TC.sparsify(vec, *attrs, start, max_iters=mi)
    return np.array(ths, F32), cnts, trace[-1], v.clone(), i.clone()


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def assert_case_is_what_it_says(name, N, dtype="float32", spill=0, cut=False, start=None, t0=T0, bulk_max=None):
    """The generated case is the one its row names — no case silently degenerates: the
    oracle's thresholds are the ladder from t0, its counts the designed ones, its moves and
    branch the row's; the exact-rung and the one-step-below elements exist; the lattice holds
    exactly top_k_samples elements >= t0 with minimum t0; the layout marks carry designed
    elements; the designed number of segments (and, with ``cut``, the one holding the k-th
    landed element) hold more than kCap elements >= the list threshold. Returns the
    oracle's run."""
    case = ZERO_BULK if name == ZERO_BULK.name else CASES[name]
    st, attrs, start, counts = generate(name, N, dtype, spill, cut, start=start, t0=t0, bulk_max=bulk_max)
    Nn, k, S, ks, stride = attrs
    g, th = st.grad, st.th
    mag = np.abs(g)
    ths, cnts, branch, v, i = oracle_run(st, attrs, start, case, dtype)
    key = (name, N, dtype, spill, cut)
    assert branch == case.branch, (key, branch, cnts)
    assert len(cnts) - 1 == case.moves, (key, cnts)
    assert cnts == counts[:len(cnts)] and len(counts) == len(cnts), (key, cnts, counts)
    assert np.array_equal(bits32(ths), bits32(th[:len(ths)])), (key, ths, th)
    assert bits32(ths[0]) == bits32(round_dtype(t0, dtype)), key
    # the sampled lattice
    lat = mag[start::stride]
    assert int((lat >= th[0]).sum()) == ks and bits32(lat[lat >= th[0]].min()) == bits32(th[0]), key
    # every count, the element on every rung and the element just below the rung above
    up = case.kw.get("up", False)
    for j, want in enumerate(counts):
        assert int((mag >= th[j]).sum()) == want, (key, j)
        assert (mag == th[j]).any(), (key, j, "no element on the rung")
        above = j + 1 if up else j - 1
        if 0 <= above < len(counts) and st.rungs[j]["in_band"] >= 2:
            assert (mag == pred(th[above], dtype)).any(), (key, j, "no element one step below the rung above")
    lowest = th[0] if up else th[len(counts) - 1]
    assert (mag == pred(lowest, dtype)).any() != (case is ZERO_BULK), (key, "one step below the last rung")
    floor_t = th[0] if up else th[-1]
    designed = mag >= pred(lowest, dtype)
    if st.t_list is not None:
        designed |= mag >= st.t_list
    bulk = mag[~designed]
    assert float(bulk.max()) < float(floor_t) / 2, key
    assert (bulk == 0).all() if case is ZERO_BULK else (bulk > 0).all(), key
    for p in st.marks:
        assert designed[p], (key, p, "layout mark without a designed element")
    assert 0 < int((g < 0).sum()) < Nn, key
    # the spilled segments
    if spill:
        nseg = -(-Nn // SEG)
        per_seg = np.add.reduceat(mag >= st.t_list, np.arange(0, Nn, SEG))
        assert per_seg.size == nseg and int((per_seg > KCAP).sum()) == spill, (key, int((per_seg > KCAP).sum()))
        assert sorted(np.flatnonzero(per_seg > KCAP)) == st.spill_segs, key
        assert not (mag[(mag >= st.t_list) & (mag < floor_t)] >= th[len(counts) - 1]).any(), key
        if cut:
            landed = np.flatnonzero(mag >= th[case.moves])
            assert landed.size > k and int(landed[k - 1] // SEG) in st.spill_segs, key
            assert per_seg[landed[k - 1] // SEG] > KCAP, key
    return ths, cnts, branch, v, i


def lists_dropped(N, spill):
    """sel_init_tensor: the K1 lists are not served when spills * kSpillDiv > nseg."""
    return spill * SPILL_DIV > -(-N // SEG)


def closed_form_ladder(t0, n, lower=0.8):
    """fl32(t0 * powf(fl32(lower), j)): the ladder a kernel must NOT compute."""
    return np.array([F32(F32(t0) * F32(F32(lower) ** F32(j))) for j in range(n + 1)], F32)


# ------------------------------------------------------------------ the routing a list threshold implies
SPEC_KINDS = ("inf", "above_t0", "mid23", "at_landed", "below", "spill1", "spill_max", "spill_drop")


def spec_of(kind, case, N, dtype="float32", t0=T0):
    """(spec[0], spill, cut) of a list-threshold setting: no lists; just above t0 (the first
    count misses the lists); between th[2] and th[3]; exactly the threshold the case lands
    at; below the whole ladder, with no / one / the most kept / one too many spilled
    segments (one: the k-th landed element inside it where the branch emits the first k)."""
    lad = ladder(t0, 0.8, MAX_LOWER + 1, dtype)
    nseg = -(-N // SEG)
    if kind == "inf":
        return F32(np.inf), 0, False
    if kind == "above_t0":
        return np.nextafter(lad[0], F32(np.inf)), 0, False
    if kind == "mid23":
        return F32((lad[2] + lad[3]) / F32(2)), 0, False
    if kind == "at_landed":
        return (lad[0] if case.kw.get("up") else lad[case.moves]), 0, False
    spill = {"below": 0, "spill1": 1, "spill_max": nseg // SPILL_DIV, "spill_drop": nseg // SPILL_DIV + 1}[kind]
    attrs = O.attributes(N, 0.001)
    return below_ladder(t0, case, dtype), spill, kind == "spill1" and cuttable(case, case_counts(case, attrs), attrs[1], N)


def cuttable(case, counts, k, N):
    """A first-k branch whose k-th landed element can lie in a spilled segment: more landed
    elements past the k-th than layout marks (the marks at the tensor's end carry landed
    elements, and their segments do not spill)."""
    return (case.branch in ("trunc", "exhausted") and not case.kw.get("up")
            and counts[case.moves] > k + len(layout_marks(N)))


def route(case, counts, spec0, spill, N, k, dtype="float32", t0=T0):
    """The path select_core takes for a case under a list threshold — what csrc/select.hip,
    select_state.hpp (decide_tensor) and select_count.hpp (k_lower_lists) say:
    (full_passes, lowering, landed, spill), lowering one of "-" (none), "lists" (k_lower_lists
    decided), "lists_js_ms" (it served every rung, none reached: js = ms = max_iters), "mixed"
    (it served some rungs, k_lower_counts decided), "vec" (k_lower_counts alone), "steps" (the
    iterative path: a count pass per move); landed "lists" or "full"; spill "" / "reread" /
    "reread+cut" / "dropped"."""
    mi, resample, up = case.kw.get("max_iters", 10), case.kw.get("resample", True), case.kw.get("up", False)
    U, L = O.adapt_bounds(k)
    lad = ladder(t0, 1.3 if up else 0.8, max(MAX_LOWER + 1, mi), dtype)
    dropped = lists_dropped(N, spill)
    built = np.isfinite(spec0)
    tl = F32(np.inf) if (dropped or not built) else F32(spec0)
    fp, used_lists = 0, False
    if lad[0] < tl:
        fp, tl, land = 1, lad[0], "full"
    else:
        land, used_lists = "lists", True
    lowering = "-"
    if case.moves and resample and mi <= MAX_LOWER:
        ms = max([j for j in range(1, min(LOWER_LISTS, mi) + 1) if lad[j] >= tl], default=0)
        reach = next((j for j in range(1, len(counts)) if counts[j] >= L), None)
        if ms and reach is not None and reach <= ms:
            lowering = "lists"
        elif ms and ms == mi:
            lowering = "lists_js_ms"
        else:
            lowering = "mixed" if ms else "vec"
        used_lists |= ms > 0
        if lad[case.moves] < tl:
            fp, tl, land = fp + 1, lad[case.moves], "full"
        else:
            land, used_lists = "lists", True
    elif case.moves:
        lowering = "steps"
        for j in range(1, case.moves + 1):
            if lad[j] < tl:
                fp, tl, land = fp + 1, lad[j], "full"
            else:
                land, used_lists = "lists", True
    sp = ""
    if spill:
        sp = "dropped" if dropped else ("reread" if used_lists and built else "")
        if sp == "reread" and spill == 1 and land == "lists" and cuttable(case, counts, k, N):
            sp = "reread+cut"
    return fp, lowering, land, sp
