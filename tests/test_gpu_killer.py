"""K5's depth-limit exits on tests/killer.py's candidate sets: dgc_select on the embedded
gradient returns torch.topk's indices over the candidates, in order, bit for bit, in
every phase the exit is taken in (tests/test_killer_cpu.py confirms each case's path);
one DGCBatch step over two killers and an ordinary tensor; and the phase bounds on
ordinary data."""
import random
import time

import numpy as np
import pytest
import torch

import killer as K
from oracle import dgc_oracle as O
from test_gpu_parity import DEV, L, bits, select_dev  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu

K5_FALLBACK, K5_BROKEN = 1, 2
ORACLE_MAX = 13000   # O.sparsify's pure-Python heap select takes tens of seconds on the 40,000-candidate cases


def _check(L, values, k, key, **kw):
    """dgc_select (sync 1 and 0) on the embedded candidates against torch.topk over them."""
    c = values.size
    e = K.embed(values, k)
    order = torch.topk(torch.from_numpy(np.abs(values)), k, 0, largest=True, sorted=False)[1].numpy()
    want = e.pos[order]
    if c <= ORACLE_MAX:
        _, oi, info = O.sparsify(e.vec, e.attrs, threshold=e.thr)
        assert info["branch"] == "resample" and np.array_equal(oi, want), key
    for sync in (1, 0):
        t0 = time.perf_counter()
        gv, gi, gvec, gmmt, branch, inf = select_dev(L, e.vec, e.mmt, float(e.thr), e.attrs, sync=sync, **kw)
        # K5_FALLBACK (the workgroups were not co-resident) is the machine's: reported, not failed on
        msg = (key, f"sync={sync}", f"{time.perf_counter() - t0:.3f}s",
               "K5_FALLBACK" if inf.k5_status & K5_FALLBACK else "no fallback")
        print("killer", *msg)
        assert not inf.k5_status & K5_BROKEN, msg
        assert branch == "resample" and inf.tie_rule == 1 and inf.candidates == c, msg
        assert np.array_equal(gi.astype(np.int64), want), msg
        wv = e.vec[want].astype(np.float16) if kw.get("fp16") else e.vec[want]
        assert np.array_equal(bits(gv), bits(wv)), msg
        ev, em = e.vec.copy(), e.mmt.copy()
        O.update(em, ev, want, True)
        assert np.array_equal(bits(gvec), bits(ev)) and np.array_equal(bits(gmmt), bits(em)), msg


def _run(L, name, tie_gas, **kw):
    c = K.CASE_BY_NAME[name]
    values, trace = K.build(name, tie_gas)
    assert trace[-1][0] == "heap" and K.path_of(trace, c.n, "wg") == c.path
    _check(L, values, c.k, (name, "tied" if tie_gas else "distinct"), **kw)


@pytest.mark.parametrize("tie_gas", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("name", [c.name for c in K.CASES if "wg" not in c.path])
def test_heap_exit_below_the_global_phase(L, name, tie_gas):
    _run(L, name, tie_gas)


@pytest.mark.parametrize("mode", ["wg", "multi"])
@pytest.mark.parametrize("tie_gas", [False, True], ids=["distinct", "tied"])
@pytest.mark.parametrize("name", [c.name for c in K.CASES if "wg" in c.path])
def test_heap_exit_from_the_global_phase(L, name, tie_gas, mode, monkeypatch):
    """``multi``: the global steps (and, for the plain cases, the heap select itself, by the
    last arriver of a barrier) on several workgroups; the depth counter and heap_exit are
    handed to the one-workgroup replay."""
    monkeypatch.setenv("DGC_K5_GLOBAL", mode)
    _run(L, name, tie_gas)


@pytest.mark.parametrize("name", ["wg_13000", "wg_lds_1025_low", "lds_12288_low"])
def test_heap_exit_in_the_recovery_replay(L, name, monkeypatch):
    monkeypatch.setenv("DGC_K5_GLOBAL", "multi")
    monkeypatch.setenv("DGC_K5_FORCE_BROKEN", "1")
    _run(L, name, True)


def test_heap_exit_fp16_values_int32_indices(L):
    _run(L, "lds_1025_high", True, fp16=True, int32=True)


# ------------------------------------------------------------------ the phase bounds on ordinary data
def _sweep_ks(c):
    """The smallest and the largest k with floor(1.3 k) < c < 64 k, and one between."""
    lo = c // 64 + 1
    hi = max(k for k in range(1, c) if O.adapt_bounds(k)[0] < c)
    return sorted({lo, (lo + hi) // 2, hi})


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("c", [4, 63, 64, 65, 1023, 1024, 1025, 12287, 12288, 12289])
def test_phase_boundary_sweep(L, c, kind, monkeypatch):
    """Candidate counts on both sides of every bound between two phases (registers / wave /
    LDS / global; 12289 under DGC_K5_GLOBAL=multi as well)."""
    rng = np.random.default_rng(c)
    if kind == "normal":
        v = (1.0 + np.abs(rng.standard_normal(c))).astype(np.float32)
    else:
        v = rng.integers(1, 6, c).astype(np.float32)
    v *= np.where(rng.random(c) < 0.5, np.float32(-1), np.float32(1))
    for k in _sweep_ks(c):
        assert O.adapt_bounds(k)[0] < c < 64 * k
        _check(L, v, k, ("sweep", kind, c, k))
        if c > K.K_NTH_LDS:
            monkeypatch.setenv("DGC_K5_GLOBAL", "multi")
            _check(L, v, k, ("sweep-multi", kind, c, k))
            monkeypatch.delenv("DGC_K5_GLOBAL")


# ------------------------------------------------------------------ the batch engine
BATCH = [("t_lds", 192_501, "lds_12288_low"), ("t_global", 299_501, "wg_13000"), ("t_normal", 200_003, None)]


@pytest.mark.parametrize("mode", ["default", "multi"])
def test_batch_step_over_two_killers(L, mode, monkeypatch):
    """One DGCBatch step (resample_order="index": an untied k-th key would go to K5s) over a
    tied LDS-exit killer, a tied global-exit killer and a seeded normal tensor. The killers'
    candidates are laid so that the sampled lattice start::stride holds exactly top_k_samples
    of them, the tied (lowest) value among these: the sampled threshold is that value and
    every candidate, nothing else, counts. Zero state and nesterov=False: the velocity is
    the gradient."""
    from dgc.batch import DGCBatch
    from oracle import synth
    from test_gpu_batch import _assert_sent
    if mode == "multi":
        monkeypatch.setenv("DGC_K5_GLOBAL", "multi")
    b = DGCBatch([(n, (numel,)) for n, numel, _ in BATCH], compress_ratio=0.001, momentum=0.9, nesterov=False,
                 device=DEV, seed=11, resample_order="index")
    starts = b.draw_starts()
    want = {}
    for t, (tname, numel, cname) in enumerate(BATCH):
        attrs = O.attributes(numel, 0.001)
        _, k, S, ks, stride = attrs
        rng = np.random.default_rng(t)
        if cname is None:
            g = synth.gradient(321, numel, "normal", 1e-3)
        else:
            case = K.CASE_BY_NAME[cname]
            values, trace = K.build(cname, True)
            assert case.k == k and trace[-1][0] == "heap", (cname, k)
            c = values.size
            lattice = np.arange(starts[t], numel, stride)
            off = np.setdiff1d(np.arange(numel), lattice)
            pos = np.sort(np.concatenate([rng.choice(lattice, ks, replace=False), rng.choice(off, c - ks, replace=False)]))
            g = rng.uniform(0.01, 0.9, numel).astype(np.float32) * np.where(rng.random(numel) < 0.5, -1, 1).astype(np.float32)
            g[pos] = values
            low = np.abs(values).min()
            assert np.count_nonzero(np.abs(values) == low) > 1 and low in np.abs(g[lattice])
        ov, oi, oinfo = O.compress_step(g, np.zeros(numel, np.float32), np.zeros(numel, np.float32), attrs,
                                        starts[t], nesterov=False)
        if cname is not None:
            assert oinfo["branch"] == "resample" and oinfo["counts"][-1] == c and len(oinfo["counts"]) == 1, oinfo
            order = torch.topk(torch.from_numpy(np.abs(values)), k, 0, largest=True, sorted=False)[1].numpy()
            assert np.array_equal(oi, pos[order])
        want[tname] = (g, ov, oi, oinfo)
        b.grad(tname).copy_(torch.from_numpy(g))
    b.compress(starts)
    b.decompress()
    torch.cuda.synchronize()
    sent, infos = b.transmitted(), b.infos()
    for t, (tname, numel, cname) in enumerate(BATCH):
        g, ov, oi, oinfo = want[tname]
        inf, key = infos[t], (mode, tname, cname)
        print("killer-batch", key, inf)
        assert inf["branch"] == oinfo["branch"] and inf["candidates"] == oinfo["counts"][-1], (key, inf)
        if cname is not None:   # the replay, not K5s
            assert inf["tie_rule"] == "exact", (key, inf)
        gv, gi = sent[tname]
        _assert_sent(gi, gv, oi, ov, inf, key)
        ref = g.copy()
        ref[oi] = 0
        assert np.array_equal(bits(b.velocity_of(tname).cpu().numpy()), bits(ref)), key
        assert np.array_equal(bits(b.momentum_of(tname).cpu().numpy()), bits(ref)), key
        assert np.array_equal(bits(b.out(tname).cpu().numpy()), bits(O.decompress([ov], [oi], numel, 1))), key
