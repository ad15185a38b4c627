"""tests/killer.py's candidate sets are what their rows say (CPU only): every case leaves
the introselect through the depth-limit heap select, at depth 0, in the phase named; the
scalar restatement and oracle/introselect.py record the same trace; and the oracle's
depth-limit branch equals torch.topk(sorted=False) in order."""
import numpy as np
import pytest
import torch

import killer as K
from oracle import introselect as I

NAMES = [c.name for c in K.CASES]


def test_phase_constants_match_the_headers():
    for name, (_, ours) in K.CONSTANTS.items():
        assert K.header_constant(name) == ours, name


@pytest.mark.parametrize("tie_gas", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_the_heap_exit(name, tie_gas):
    c = K.CASE_BY_NAME[name]
    values, trace = K.build(name, tie_gas)
    assert values.size == c.n and values.dtype == np.float32
    kind, f, l = trace[-1]
    steps = trace[:-1]
    assert kind == "heap" and len(steps) == 2 * K._lg(c.n) and steps[-1][2] == 1, trace[-3:]
    assert [d for _, _, d in steps] == list(range(2 * K._lg(c.n), 0, -1))
    assert f <= c.k - 1 < l
    assert K.path_of(trace, c.n, "wg") == c.path
    assert K.phase_of(c.n, c.n, "wg") == c.path.split(">")[0]
    mag = np.abs(values)
    kth = np.sort(mag)[::-1][c.k - 1]
    ties = int(np.count_nonzero(mag == kth))
    if not tie_gas:
        assert np.unique(mag).size == c.n and (values < 0).any() and (values > 0).any()
    else:
        assert ties > 1, (name, ties)
    want = torch.topk(torch.from_numpy(mag), c.k, 0, largest=True, sorted=False)[1].numpy()
    assert np.array_equal(I.topk_order(values, c.k), want)


@pytest.mark.parametrize("name", NAMES)
def test_scalar_restatement_equals_oracle(name):
    c = K.CASE_BY_NAME[name]
    for tie_gas in (False, True):
        values, trace = K.build(name, tie_gas)
        for v in (values, K.shuffled(values)):
            st = []
            got = K.scalar_topk_order(v, c.k, st)
            assert st == K.oracle_trace(v, c.k)
            assert np.array_equal(got, I.topk_order(v, c.k))


@pytest.mark.parametrize("name", ["regs_only", "wave_1024", "lds_12288_low", "wg_13000", "wg_lds_wave_65"])
def test_control_permutation_ends_in_insertion(name):
    c = K.CASE_BY_NAME[name]
    values, _ = K.build(name, False)
    v = K.shuffled(values)
    trace = K.oracle_trace(v, c.k)
    assert trace[-1][0] == "insertion" and len(trace) - 1 < 2 * K._lg(c.n)
    want = torch.topk(torch.from_numpy(np.abs(v)), c.k, 0, largest=True, sorted=False)[1].numpy()
    assert np.array_equal(I.topk_order(v, c.k), want)


def test_heap_sizes_cover_the_lone_child_and_the_guard():
    mids = {K.heap_mid(K.build(n, False)[1], K.CASE_BY_NAME[n].k) for n in NAMES}
    assert 1 in mids and 2 in mids and any(m > 2 and m % 2 for m in mids) and any(m > 2 and m % 2 == 0 for m in mids)


def test_register_exits_have_moved_the_inner_front():
    """Every register-exit case takes steps inside the register phase before the limit, so
    the heap select's base there is q + f + F with F > 0 (f: where the phase began)."""
    for n in NAMES:
        c = K.CASE_BY_NAME[n]
        if c.path.endswith("regs"):
            trace = K.build(n, False)[1]
            entry = next(f for f, l, _ in trace[:-1] if l - f <= K.K_WAVE)
            assert trace[-1][1] > entry, n


def test_embedding_takes_the_nth_path():
    c = K.CASE_BY_NAME["lds_wave_65"]
    values, _ = K.build(c.name, True)
    e = K.embed(values, c.k)
    N, k, S, _, _ = e.attrs
    assert N > S and np.array_equal(np.flatnonzero(np.abs(e.vec) >= e.thr), e.pos)
    assert np.count_nonzero(e.vec) == N and (e.vec[np.abs(e.vec) < e.thr] < 0).any()
    assert np.array_equal(e.vec[e.pos], values)
