"""tests/k5sets.py's rows take the K5s path they were designed for (CPU only): ``route()`` — the
kernel's classification restated — gives the route every row states, field by field; the oracle
resamples over exactly the row's candidates; and the expected payloads (torch.topk's, never the
designer's) are what tests/test_gpu_k5s_sets.py compares the kernels with."""
import numpy as np
import pytest
import torch

import k5sets as K
from oracle import dgc_oracle as O

ORACLE_MAX = 13000     # (test_gpu_killer.ORACLE_MAX) the pure-Python oracle's comfortable candidate count
EMBED_MAX = 300_000    # larger rows: the route from the candidates alone (the embedding only places them)


@pytest.mark.parametrize("name", list(K.CONSTANTS))
def test_constants_match_the_headers(name):
    assert K.header_constant(name) == K.CONSTANTS[name][1]
    assert K.BINS0 == 4096 and K.BINS1 == 8192 and K.COOP_MIN == 16384


def topk_order(values, k):
    return torch.topk(torch.from_numpy(np.abs(values)), k, 0, largest=True, sorted=False)[1].numpy()


@pytest.mark.parametrize("name", [r.name for r in K.ROWS])
def test_row_takes_its_route(name):
    r = K.ROW_BY_NAME[name]
    v = K.candidates(name)
    N = K.numel(r.c, r.layout, r.N)
    assert v.size == r.c and O.adapt_bounds(r.k)[0] < r.c < 64 * r.k and r.c <= min(N, 64 * r.k - 1)
    keys = K.keys_of(v).astype(np.int64)
    mn = K.key_of(r.t)
    assert keys.min() >= mn
    got = K.route(keys, r.t, r.k, K.cand_cap(N, r.k))
    assert got == r.route, (name, got, r.route)
    order = topk_order(v, r.k)
    kth = np.sort(keys)[-r.k]
    assert kth == mn + r.D and np.count_nonzero(keys == kth) == r.eq
    assert np.count_nonzero(keys > kth) == r.k - r.ka
    chosen = np.sort(order)
    if r.route[0] == "set":
        assert np.array_equal(chosen, np.flatnonzero(keys >= kth)) and chosen.size == r.k
        assert r.route[-1] == r.eq == r.ka
    else:
        assert r.route[1] != "tied" or np.count_nonzero(keys >= kth) > r.k
    if r.c > EMBED_MAX:
        return
    _, _, e = K.build(name)
    assert e.attrs[0] == N and np.array_equal(e.vec[e.pos], v) and np.all(np.diff(e.pos) > 0)
    assert np.array_equal(np.flatnonzero(np.abs(e.vec) >= e.thr), e.pos)
    per_seg = np.bincount(e.pos // K.K_SEG)
    if r.layout == "scattered":
        assert per_seg.max() <= K.K_CAP
    elif r.layout == "dense":
        assert per_seg.max() == K.K_SEG and np.count_nonzero(per_seg > K.K_CAP) > 1
    else:
        assert {0, N - 1, K.QUARTER - 1, K.QUARTER, K.GROUP - 1, K.GROUP} <= set(e.pos.tolist())
        assert N % 4 == int(r.layout[-1])
    want = np.sort(e.pos[order]) if r.route[0] == "set" else e.pos[order]
    if r.route[0] == "set":
        assert np.array_equal(want, e.pos[np.abs(v) >= K.f32_of([kth])[0]]) and want.size == r.k
    if r.c <= ORACLE_MAX:
        _, oi, info = O.sparsify(e.vec, e.attrs, threshold=e.thr)
        assert info["branch"] == "resample" and info["counts"] == [r.c], (name, info["branch"], info["counts"])
        assert np.array_equal(oi, e.pos[order]), name      # the oracle's payload: torch.topk's, in its order


def test_placements_reach_their_stretches():
    """``first`` / ``last`` / ``waves`` put the selected keys where they say."""
    for r in K.ROWS:
        if r.how == "random" or r.c > EMBED_MAX:
            continue
        v = K.candidates(r.name)
        sel = np.flatnonzero(K.keys_of(v).astype(np.int64) >= K.key_of(r.t) + r.D)
        per, last_lo, _ = K.stretches(r.c, r.G)
        assert sel.size == r.k
        if r.how == "first":
            assert sel.max() < per * K.K_SCAN_THREADS, r.name      # (rows past EMBED_MAX: the first 2k slots)
        elif r.how == "last":      # the last non-empty stretch, or the last 2k slots when it holds fewer than k
            assert last_lo < r.c and sel.min() >= (last_lo if r.c - last_lo >= r.k else r.c - 2 * r.k), r.name
        else:
            assert np.unique(sel // 64).size == K.ceil_div(r.c, 64), r.name


def test_tie_runs_straddle_their_boundaries():
    for r in K.ROWS:
        if r.run_at is None:
            continue
        v = K.candidates(r.name)
        at = np.flatnonzero(K.keys_of(v).astype(np.int64) == K.key_of(r.t) + r.D)
        assert at.size == r.eq and at.min() < r.run_at <= at.max() and at.max() - at.min() == r.eq - 1, r.name
