"""The staircase generator (tests/staircase.py) against the oracle, on the CPU: every case
the GPU tests of tests/test_gpu_adapt_lattice.py run is confirmed to be what its row says —
the sampled threshold, the count at every rung, the number of threshold moves, the branch,
the elements on and just below the rungs, the layout — so that no GPU case silently
degenerates; and the table of expected paths is held to the restated routing."""
import random

import numpy as np
import pytest

import staircase as S
import test_gpu_adapt_lattice as G
from oracle import dgc_oracle as O
from oracle import torch_cpu as TC


def _settings(rows, N, dtype="float32"):
    """The distinct generated gradients (case, spill, cut) a list of rows needs at N."""
    return sorted({(r[0],) + S.spec_of(r[1], S.CASES[r[0]], N, dtype)[1:] for r in rows})


@pytest.mark.parametrize("name", list(S.CASES))
def test_every_case_is_what_it_says(name):
    """Engine (a): every row of the case at N_ODD, with the spill layouts its rows use."""
    rows = [r for r in G.PAIRS if r[0] == name]
    for _, spill, cut in _settings(rows, G.N_ODD):
        S.assert_case_is_what_it_says(name, G.N_ODD, "float32", spill, cut)


def test_three_group_cases_are_what_they_say():
    for name, spill, cut in _settings(G.BIG_ROWS + G.QUARTER_ROWS, G.N_BIG):
        st = S.generate(name, G.N_BIG, "float32", spill, cut)[0]
        assert {S.GROUP - 1, S.GROUP, 2 * S.GROUP - 1, 2 * S.GROUP} <= set(st.marks)
        S.assert_case_is_what_it_says(name, G.N_BIG, "float32", spill, cut)


@pytest.mark.parametrize("dname", ["bfloat16", "float16"])
def test_half_cases_are_what_they_say(dname):
    """Engine (b): the generator in the dtype (ladder products rounded to it), at the sample
    start the bucket will draw; confirmed by the torch-CPU port on tensors of the dtype."""
    N = G.N_ODD
    start = random.Random(11).randint(0, TC.attributes(N, 0.001)[4] - 1)
    lad16, lad32 = S.ladder(S.T0, 0.8, 10, dname), S.ladder(S.round_dtype(S.T0, dname), 0.8, 10)
    assert (lad16 != lad32).any()   # rounding the products to the dtype matters on this ladder
    for name, spill, cut in _settings(G.HALF_ROWS, N, dname):
        st = S.generate(name, N, dname, spill, cut, start=start)[0]
        assert np.array_equal(S.round_dtype(st.grad, dname).view(np.uint32), st.grad.view(np.uint32))
        S.assert_case_is_what_it_says(name, N, dname, spill, cut, start=start)


def test_batch_cases_are_what_they_say():
    """Engine (c): the warm-up staircase (zero bulk, everything selected) and the cases at
    the batch's tensor sizes, with the bulk held under the warmed-up list threshold."""
    for lists in ("reach", "miss"):
        t0_warm = np.float32(S.T0 / 40 if lists == "reach" else S.T0 * 2)
        bulk_max = np.float32(0.8 * 0.95) * t0_warm if lists == "reach" else None
        for tname, numel, cname in G.BATCH:
            if cname is None:
                assert O.attributes(numel, 0.001)[2] == numel   # direct
                continue
            _, cnts, branch, v, i = S.assert_case_is_what_it_says("warmup", numel, t0=float(t0_warm))
            assert branch == "ok" and len(i) == cnts[0]   # all of it selected: the state returns to zero
            assert np.count_nonzero(S.generate("warmup", numel, t0=float(t0_warm))[0].grad) == cnts[0]
            S.assert_case_is_what_it_says(cname, numel, bulk_max=bulk_max)
            if bulk_max is not None:   # nothing but designed elements at or above the lists' threshold
                g = np.abs(S.generate(cname, numel, bulk_max=bulk_max)[0].grad)
                th = S.ladder(S.T0, 0.8, 10)
                assert int((g >= np.float32(0.8) * t0_warm).sum()) == int((g >= S.pred(th[S.CASES[cname].moves],
                                                                                       "float32")).sum())


def test_ladder_is_not_the_closed_form():
    """T0 keeps the iterated product apart from fl32(t0 * powf(0.8, j)) at every rung from 2
    on, the closed form above it: an element on the rung is then not counted by it."""
    it, cf = S.ladder(S.T0, 0.8, S.MAX_LOWER), S.closed_form_ladder(S.T0, S.MAX_LOWER)
    assert it[0] == cf[0] and it[1] == cf[1]
    assert all(cf[j] > it[j] for j in range(2, S.MAX_LOWER + 1)), (it, cf)


def test_table_of_paths_follows_the_routing():
    """PAIRS is data; staircase.route restates the routing of csrc/select.hip. They must
    agree at both sizes (spill settings scale with the segment count), every case must have
    rows, and the census of paths must be complete."""
    for N in (G.N_ODD, G.N_BIG):
        attrs = O.attributes(N, 0.001)
        for row in G.PAIRS:
            case = S.CASES[row[0]]
            spec0, spill, cut = S.spec_of(row[1], case, N)
            got = S.route(case, S.case_counts(case, attrs), spec0, spill, N, attrs[1])
            assert got == tuple(row[2:]), (N, row, got)
            assert cut == (row[5] == "reread+cut"), (N, row)
    nseg = -(-G.N_ODD // S.SEG)
    assert not S.lists_dropped(G.N_ODD, nseg // S.SPILL_DIV) and S.lists_dropped(G.N_ODD, nseg // S.SPILL_DIV + 1)
    G.test_census_of_paths()


def test_generator_rejects_what_it_cannot_build():
    attrs = O.attributes(100_003, 0.001)
    with pytest.raises(AssertionError, match="must not fall"):
        S.staircase(attrs, 3, 0.3, [50, 40])
    with pytest.raises(AssertionError, match="sampled elements"):
        S.staircase(attrs, 3, 0.3, [attrs[3] - 1, 60])
