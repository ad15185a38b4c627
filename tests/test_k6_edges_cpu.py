"""tests/k6edges.py's rows take the K6 path they were designed for (CPU only): ``route()`` — the
host's and the device's routing restated — gives the route every row states, field by field; the
counts a row claims (entries per super-chunk, per chunk, per granule, the chunk gaps between
consecutive indices) hold; the oracle's output is torch's ``index_put_`` on the CPU bit for bit;
and on every rank-order row some permutation of the ranks changes the result. Expected outputs
are the oracle's, never the designer's; tests/test_gpu_k6_edges.py compares the kernels with them."""
import itertools

import numpy as np
import pytest
import torch

import k6edges as K

I64, F32 = np.int64, np.float32


@pytest.mark.parametrize("name", list(K.CONSTANTS))
def test_constants_match_the_sources(name):
    assert K.header_constant(name) == K.CONSTANTS[name][1]


def test_derived_constants():
    assert K.header_order_word() == K.ORDER_ASCENDING
    assert K.header_constant("kBlock") * 8 == K.K_MAX_GRID          # dgc_common.hpp: kMaxGrid = 256 * 8
    assert "constexpr int kMaxGrid = 256 * 8;" in (K.CSRC / "dgc_common.hpp").read_text()
    assert (K.BOUNDS_SWEEP, K.CLEAR_SWEEP, K.DESCENT_SWEEP, K.WS_WORDS) == (262144, 65536, 524288, 1536)
    assert K.WS_WORDS % 256 == 0                                    # the carve's next take starts right after Run[64]


def scatter_runs(r):
    """The runs as the scatter sees them and their capacity (a split row: one run per part)."""
    runs = K.build(r.name)
    if r.parts:
        return K.split_parts(runs, r.parts, r.cap) + (r.W * r.parts,)
    return list(runs), r.cap, r.W


def chunk_gaps(idx, n):
    """hi - lo of k_bounds for e = 0 .. count: the chunks each entry (and the sentinel) owns."""
    nch = K.ceil_div(n, K.K_CHUNK)
    rank = [min(int(v) >> 12, nch - 1) + 1 + (1 if v >= n else 0) for v in idx]
    edges = [0] + rank + [nch + 1]
    return tuple(max(0, b - a) for a, b in zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("name", [r.name for r in K.ROWS])
def test_row_takes_its_route(name):
    r = K.ROW_BY_NAME[name]
    runs, cap, W = scatter_runs(r)
    assert len(K.build(name)) == r.W
    for q, (v, i) in enumerate(runs):
        assert v.dtype == F32 and i.dtype == I64 and v.size == i.size
        assert "bad" in r.claims or bool(K.in_range(i, r.n).all())
        if r.form != "table":
            assert i.size <= cap and np.unique(i).size == i.size           # a DGC payload: unique per rank
        if r.int32:
            assert r.n < 2 ** 31
    got = K.route(r.n, W, cap, runs, r.form)
    assert got == r.route, (got, r.route)
    assert got.status == r.status
    assert type(r.route[1]) is bool if r.route[0] == "single" else type(r.route[2]) is bool
    c = r.claims
    counts = tuple(len(i) for _, i in runs)
    allidx = np.concatenate([i for _, i in runs]) if counts else np.zeros(0, I64)
    assert int(np.count_nonzero(~K.in_range(allidx, r.n))) == c.get("bad", 0)   # dropped, flagged in the status
    allidx = allidx[K.in_range(allidx, r.n)]
    if r.route[0] == "waves":
        m, nsc, ovf = r.route[1], r.route[3], r.route[4]
        assert nsc == K.ceil_div(K.ceil_div(r.n, K.K_CHUNK), m)
        T = K.super_totals(r.n, m, runs)
        for s, t in c.get("T", {}).items():
            raw = sum(int(np.count_nonzero(i[K.in_range(i, r.n)] // (K.K_CHUNK * m) == s)) for _, i in runs)
            assert raw == t or (T[s] == t and raw > t), (s, raw, int(T[s]), t)   # a claim at the clamp states T
        assert set(ovf) == {s for s in range(nsc) if T[s] > 64}
    for ch, t in c.get("staged", {}).items():
        assert int(np.count_nonzero(allidx // K.K_CHUNK == ch)) == t, ch
    for g, t in c.get("granule", {}).items():      # distinct indices per 64-B granule of an aligned output
        assert np.unique(allidx[allidx // 16 == g]).size == t, g
    for q, gaps in c.get("gaps", {}).items():
        assert chunk_gaps(runs[q][1], r.n) == tuple(gaps), (q, chunk_gaps(runs[q][1], r.n))
    u, cnt = np.unique(allidx, return_counts=True)
    for i, t in c.get("dups", {}).items():
        assert sum(int(i in set(x.tolist())) for _, x in runs) == t, i
    if c.get("no_dups"):
        assert cnt.size == 0 or cnt.max() == 1
    if "counts" in c:
        assert counts == tuple(c["counts"])
    if c.get("count_is_cap"):
        assert max(counts) == cap
    for q in c.get("empty", ()):
        assert counts[q] == 0
    if "total" in c:
        assert sum(counts) == c["total"]
    for p, i in c.get("positions", {}).items():
        assert runs[0][1][p] == i
    w = K.want(name)
    for i in c.get("negzero", ()):                 # entries of -0.0 only: index_put_ onto +0.0 gives +0.0
        vs = np.concatenate([v[x == i] for v, x in runs])
        assert vs.size and np.all(vs.view(np.uint32) == 0x80000000) and w.view(np.uint32)[i] == 0
    if "bounds" in c:                              # dgc_payload_split's header word 1 per (rank, part)
        pc = cap
        for (v, i), b in zip(K.build(name), c["bounds"]):
            for p in range(r.parts):
                later = i[(p + 1) * pc:]
                assert b[p] == (int(later.min()) if later.size else K.INT64_MAX)
    if r.form != "table" and not r.parts:
        prev = K.prev_of(name)
        assert len(prev) == r.W
        for q, (v, i) in enumerate(prev):
            assert i.size <= r.cap and np.unique(i).size == i.size and (i.size == 0 or (0 <= i.min() and i.max() < r.n))
            assert not np.any(np.isnan(v))
        if "prev_counts" in c:
            assert tuple(len(i) for _, i in prev) == tuple(c["prev_counts"])
        pall = np.concatenate([i for _, i in prev])
        rel = c.get("prev_relation")
        if rel == "disjoint":
            assert np.intersect1d(pall, allidx).size == 0
        elif rel == "identical":
            assert all(np.array_equal(a[1], b[1]) for a, b in zip(prev, runs))
        elif rel == "subset":
            assert all(np.isin(b[1], a[1]).all() and b[1].size < a[1].size for a, b in zip(prev, runs))


def torch_reference(runs, n, scale):
    runs = [(v[K.in_range(i, n)], i[K.in_range(i, n)]) for v, i in runs]   # index_put_ raises on the others
    idx = torch.from_numpy(np.concatenate([i for _, i in runs]).astype(I64))
    val = torch.from_numpy(np.concatenate([v for v, _ in runs]).astype(F32))
    out = torch.zeros(n).index_put_([idx], val, accumulate=True)
    return (out.mul_(scale) if scale != 1.0 else out).numpy()


@pytest.mark.parametrize("name", [r.name for r in K.ROWS])
def test_oracle_is_sequential_index_put(name):
    r = K.ROW_BY_NAME[name]
    with torch.no_grad():
        torch.set_num_threads(1)
        ref = torch_reference(K.build(name), r.n, r.scale)
    w = K.want(name)
    assert K.same_bits(w, ref)
    nan = np.isnan(w)
    assert np.array_equal(nan, np.isnan(ref))
    if r.parts:   # the phases' runs, concatenated in the scatter's order, are the same sum
        pr, _ = K.split_parts(K.build(name), r.parts, r.cap)
        assert K.same_bits(K.oracle_of(pr, r.n, r.scale), w)
    if r.form != "table" and not r.parts and r.W > 1:
        assert K.same_bits(K.oracle_of(K.prev_of(name), r.n, r.scale),
                           torch_reference(K.prev_of(name), r.n, r.scale))


@pytest.mark.parametrize("name", [r.name for r in K.ROWS if r.order])
def test_rank_order_rows_show_the_order(name):
    r = K.ROW_BY_NAME[name]
    runs = list(K.build(name))
    w = K.want(name)
    perms = itertools.permutations(range(r.W)) if r.W <= 4 else \
        [list(range(r.W))[::-1], list(range(1, r.W)) + [0], list(np.random.default_rng(1).permutation(r.W))]
    assert any(not K.same_bits(K.oracle_of([runs[q] for q in p], r.n, r.scale), w) for p in perms)


@pytest.mark.parametrize("name", list(K.DETECT))
def test_detect_rows_hold_their_descents(name):
    n, runs, desc = K.DETECT[name]
    idx = np.concatenate([np.asarray(i, I64) for i in runs()])
    found = int(np.count_nonzero(idx[1:] < idx[:-1])) if idx.size > 1 else 0
    assert found == (64 if desc is None else desc)
    assert all(not K.descends(i) for i in runs()) and len(runs()) == found + 1
    if name.startswith("detect_descent_at_"):
        at = int(name.rsplit("_", 1)[1])                # 524 288: the first sweep's last pair; 524 289: the second's first
        assert idx.size > K.DESCENT_SWEEP and idx[at] < idx[at - 1] and at - K.DESCENT_SWEEP in (0, 1)


def test_pack_layout_and_canary():
    runs = [(np.array([1.5, -2.0], F32), np.array([3, 9], I64)), (np.zeros(0, F32), np.zeros(0, I64))]
    for vd, idt in itertools.product((0, 1), (0, 1)):
        stride, vo, io = K.layout(5, vd, idt)
        assert stride % 256 == 0 and vo == 16 and io % 16 == 0 and io >= 16 + 5 * (2 if vd else 4)
        for asc in (False, True):
            b = K.pack(runs, 5, vd, idt, ascending=asc)
            assert b.size == 2 * stride
            for q, (v, i) in enumerate(runs):
                p = b[q * stride: (q + 1) * stride]
                head = p[:16].view(I64)
                assert head[0] == len(i) and head[1] == (K.ORDER_ASCENDING if asc else 0)
                vals = p[vo: vo + 5 * (2 if vd else 4)].view(np.float16 if vd else F32)
                idx = p[io: io + 5 * (4 if idt else 8)].view(np.int32 if idt else I64)
                assert np.array_equal(vals[: len(i)].astype(F32), v) and np.array_equal(idx[: len(i)], i)
                assert np.all(np.isnan(vals[len(i):])) and np.all(idx[len(i):] == 0)   # the canary
    assert not np.isnan(K.pack(runs, 5, 0, 0, tail=False)[16:36].view(F32)).any()


@pytest.mark.parametrize("lead", K.LEADS5)
def test_arena_places_the_view(lead):
    a = K.arena(1000, lead)
    assert a.out.numel() == 1000 and (a.out.data_ptr() - 4 * lead) % 256 == 0
    assert a.start >= K.GUARD and a.buf.numel() - a.start - 1000 >= K.GUARD and a.guards_intact()
    a.out.zero_()
    assert a.guards_intact() and int(torch.isnan(a.buf).sum()) == a.buf.numel() - 1000
    a.buf[a.start - 1] = 0.0
    assert not a.guards_intact()


def test_same_bits_tells_zero_signs_and_accepts_any_nan():
    a = np.array([0.0, 1.0, np.nan], F32)
    b = np.array([-0.0, 1.0, np.nan], F32)
    assert not K.same_bits(a, b) and K.same_bits(a, a.copy())
    c = a.copy()
    c.view(np.uint32)[2] = 0xFFC00000
    assert K.same_bits(c, a) and not K.same_bits(np.array([0.0, 1.0, 2.0], F32), a)
