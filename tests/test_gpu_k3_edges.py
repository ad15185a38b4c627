"""K3's sampled threshold t0 = min(topk(|samples|, ks)) at its digit, floor and window edges
(tests/k3edges.py): every path of the radix select is reached by designed data, and every
result is compared bit for bit with the oracle on the same arrays — no tolerances.

(1) ``dgc_kth_largest`` over the key sets, from 16-B-aligned pointers and from pointers 1, 2
and 3 floats into a NaN-guarded arena (a guard read as a key would turn the result NaN), all
k of a set back to back on one workspace. (2) The window rows through ``dgc_compress`` in
three modes, then sequences of rows on ONE workspace (K1's window histogram and k_rs_passes'
chain words must be zero at rest). (3) ``DGCBucket`` on bf16 / fp16 state. (4) ``DGCBatch``:
three windowed tensors whose rows swap between steps, beside a small one.
tests/test_k3_edges_cpu.py confirms every row's route; here the record's ``window_keys``
shows which keys K3 read.
"""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import k3edges as K
from oracle import dgc_oracle as O
from oracle import torch_cpu as TC
from test_gpu_parity import DEV, L, P, bits, check, stream, to_dev  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
# mode -> (sync mode, update_memory): device decisions with the deferred masking, with the
# immediate one, and the host loop (test_gpu_adapt_lattice.MODES)
MODES = {"dev2": (0, 2), "dev1": (0, 1), "host": (1, 1)}


def same_bits(got, want):
    """Bit-equal, NaN matching NaN."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ------------------------------------------------------------------ (1) dgc_kth_largest
@pytest.mark.parametrize("name", list(K.key_sets()))
def test_kth_largest_key_set(L, name):
    s = K.key_sets()[name]
    n = s.x.size
    mag = np.abs(s.x)
    want = np.array([O.kth_largest(mag, k) for k in s.ks], F32)
    x = to_dev(s.x.copy())
    wsz = L.dgc_kth_largest_workspace(n)
    ws = torch.empty(max(wsz, 256), dtype=torch.uint8, device=DEV)
    for off in (0, 1, 2, 3):   # floats past a 16-B boundary
        lo = 4 + off
        arena = torch.full((n + 12,), NAN, device=DEV)
        arena[lo:lo + n] = x
        out = torch.full((len(s.ks) + 2,), -1.0, device=DEV)
        for j, k in enumerate(s.ks):   # back to back on one workspace
            check(L, L.dgc_kth_largest(arena.data_ptr() + 4 * lo, n, k, out.data_ptr() + 4 * (j + 1), P(ws), wsz,
                                       stream()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert same_bits(got[1:-1], want), (name, off, s.ks, got, want)
        assert got[0] == -1.0 and got[-1] == -1.0, (name, off)
        a = arena.cpu().numpy()
        assert np.isnan(a[:lo]).all() and np.isnan(a[lo + n:]).all(), (name, off)
        assert np.array_equal(bits(a[lo:lo + n]), bits(s.x)), (name, off)


# ------------------------------------------------------------------ (2) the window rows, dgc_compress
@functools.lru_cache(maxsize=None)
def oracle_of(name):
    c = K.window_cases()[name]
    attrs = (c.N, c.k, c.N // c.stride, c.ks, c.stride)
    v, i, info = O.sparsify(c.grad.copy(), attrs, c.start)
    assert same_bits(info["thresholds"][0], K.f32_of([c.t0_key])[0]), name
    return v, i, info


def compress_rows(L, names, mode):
    """The rows ``names`` (one N, one num_selects) through dgc_compress, one after the other on
    ONE workspace — zero-filled before the first only — with vec / mmt reset and spec[0] /
    spec[2] written before each; every row against the oracle."""
    from dgc import _lib
    cases = [K.window_cases()[n] for n in names]
    N, k, stride = cases[0].N, cases[0].k, cases[0].stride
    assert all((c.N, c.k, c.stride) == (N, k, stride) for c in cases)
    Sn = N // stride
    sync, um = MODES[mode]
    p = _lib.select_params(N, k, Sn, 1.3, 0.8, 10, True, True, um, torch.float32, torch.int64)
    wsz = L.dgc_compress_workspace(N, k, Sn)
    ws = torch.zeros(wsz, dtype=torch.uint8, device=DEV)
    g, mmt, vec = (torch.zeros(N + 4, device=DEV) for _ in range(3))
    vals = torch.empty(k, device=DEV)
    idx = torch.empty(k, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    info = torch.zeros(_lib.INFO_BYTES, dtype=torch.uint8, device=DEV)
    for pos, c in enumerate(cases):
        key = (names, pos, c.name, mode)
        g[:N].copy_(torch.from_numpy(c.grad.copy()))
        mmt.zero_()
        vec.zero_()
        spec = torch.full((8,), float("inf"), device=DEV)
        spec[2] = float(c.spec2)
        spec[0] = float(c.spec0)
        check(L, L.dgc_compress(P(g), P(mmt), P(vec), 0.9, 0, c.start, stride, c.ks, ctypes.byref(p), P(spec),
                                _lib.SPEC_MARGIN, P(vals), P(idx), P(cnt), P(info), P(ws), wsz, sync, stream()))
        if um == 2:
            check(L, L.dgc_compress_flush(P(vec), P(mmt), stride, ctypes.byref(p), P(ws), wsz, stream()))
        torch.cuda.synchronize()
        n = int(cnt.item())
        inf = _lib.info_dict(_lib.SelectInfo.from_buffer_copy(info.cpu().numpy().tobytes()), "dgc_compress")
        ov, oi, oinfo = oracle_of(c.name)
        print(key, inf)
        assert same_bits(inf["threshold0"], oinfo["thresholds"][0]), (key, inf)
        assert inf["window_keys"] == c.window_keys, (key, inf)
        assert same_bits(inf["threshold"], oinfo["threshold"]), (key, inf)
        assert inf["branch"] == oinfo["branch"] and inf["recounts"] == len(oinfo["counts"]) - 1, (key, inf, oinfo)
        assert inf["candidates"] == oinfo["counts"][-1] and inf["count"] == len(oi) == n, (key, inf, oinfo)
        assert np.array_equal(idx.cpu().numpy()[:n], oi), key
        assert np.array_equal(bits(vals.cpu().numpy()[:n]), bits(ov)), key
        want = c.grad.copy()
        want[oi] = 0
        for buf in (vec, mmt):
            got = buf.cpu().numpy()
            assert same_bits(got[:N], want), key
            assert not got[N:].any(), key   # nothing written past the tensor


ROWS_W = [n for n, c in K.window_cases("w").items()]
ROWS_BIG = list(K.window_cases("big"))


@pytest.mark.parametrize("name", ROWS_W)
def test_window_row(L, name):
    """Every row at N_W (and the edge sizes) from a fresh zeroed workspace, in the three modes."""
    for mode in MODES:
        compress_rows(L, (name,), mode)


@pytest.mark.parametrize("name", ROWS_BIG)
def test_window_row_big(L, name):
    """The rows of more than 65536 window keys (N_WBIG)."""
    for mode in ("dev2", "host"):
        compress_rows(L, (name,), mode)


# a row, then different rows on the same workspace without re-zeroing it: after the passes over
# the samples (cap+1, short), after rs_window_wg (bin_4094), after the passes over a window
SEQUENCES = [("cap+1", "eq_ks", "short", "bin_4093", "bin_4094", "cap", "bin_4097", "at_wk"),
             ("short", "ties_mid", "cap+1", "inf_many", "eq_ks"),
             ("bin_4094", "bin_4096", "nan", "eq_ks")]
SEQUENCES_BIG = [("big_passes", "big_hist", "big_passes_bin", "big_wg", "big_passes", "big_hist")]


@pytest.mark.parametrize("names", SEQUENCES + SEQUENCES_BIG, ids=lambda n: n[0] + "...")
def test_window_rows_on_one_workspace(L, names):
    """Zero at rest: K1's window histogram (re-zeroed by whichever path served or refused the
    window) and k_rs_passes' chain words (re-zeroed by the last workgroup out)."""
    for mode in MODES:
        compress_rows(L, names, mode)


# ------------------------------------------------------------------ (3) the 16-bit bucket
def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


@pytest.mark.parametrize("dname", ["bfloat16", "float16"])
@pytest.mark.parametrize("kind", ["eq_ks", "bin_4094", "bin_4097"])
def test_bucket16_window_row(L, kind, dname):
    """DGCBucket(dtype=bf16 / fp16) at the smallest N whose 1 % sample is windowed, the window
    key written to ``spec[2]``; against the torch-CPU port on tensors of the dtype."""
    from dgc.bucket import DGCBucket
    from test_gpu_bucket16 import oracle_branch, payload_of
    dt, N = getattr(torch, dname), K.smallest_windowed_numel()
    b = DGCBucket(N, compress_ratio=0.001, momentum=0.9, nesterov=False, device=DEV, world_size=1, seed=11, dtype=dt)
    attrs = TC.attributes(N, 0.001)
    assert attrs == (N, b.k, b.num_samples, b.top_k_samples, b.stride) and attrs[2] + 1 > K.SMALL_N
    start = random.Random(11).randint(0, attrs[4] - 1)
    c = K.engine_row(kind, attrs, start, K.WK, dname, seed=17)
    g = torch.from_numpy(c.grad.copy()).to(dt)
    assert np.array_equal(bits(g.float().numpy()), bits(c.grad))   # representable: nothing rounded
    thr0, trace = oracle_branch(g, attrs, start)
    want_v, want_i = TC.sparsify(g, *attrs, start, max_iters=10)
    assert same_bits(thr0.float().item(), K.f32_of([c.t0_key])[0])
    b.spec[2] = float(K.f32_of([K.WK])[0])
    out = torch.full((N,), NAN, dtype=dt, device=DEV)
    b.step(g.to(DEV), out)
    torch.cuda.synchronize()
    assert b.start == start
    inf, key = b.last_info(), (kind, dname)
    print(key, inf, trace)
    assert same_bits(inf["threshold0"], thr0.float().item()), (key, inf)
    assert inf["window_keys"] == c.window_keys and c.window_keys > 0, (key, inf)
    assert inf["branch"] == trace[-1] and inf["recounts"] == trace.count("lower"), (key, inf, trace)
    assert inf["count"] == want_i.numel(), (key, inf)
    vals, idx = payload_of(b)
    assert np.array_equal(idx.cpu().numpy(), want_i.numpy()), key
    assert np.array_equal(bits16(vals), bits16(want_v)), key
    ref = g.clone()
    ref[want_i] = 0
    assert np.array_equal(bits16(b.vec), bits16(ref)), key
    assert np.array_equal(bits16(b.mmt), bits16(ref)), key
    assert np.array_equal(bits16(out), bits16(TC.decompress(want_v, want_i, torch.empty(N, dtype=dt), 1))), key


# ------------------------------------------------------------------ (4) the batch
N0 = K.smallest_windowed_numel()
BATCH = [("t_small", 200_003), ("t_a", N0), ("t_b", N0 + 1029), ("t_c", N0 + 2 * 4096 + 3)]
# step -> the row of t_small, t_a, t_b, t_c: a hist row, a rs_window_wg row and a cap+1 row (the
# passes run one active task beside two finished ones), then the rows swapped
BATCH_ROWS = {1: ("eq_ks", "eq_ks", "bin_4094", "cap+1"), 2: ("eq_ks", "cap+1", "bin_4097", "eq_ks")}


def next_window_key(t0, prev_t0, cnt, window_keys):
    """k_sel_finish's spec[2] after a call: fl32(fl32(t0 * mw) * g0), mw = 0.985 after a window
    of more than kWinMax keys, 0.97 after one K3 read, 0.9 after one it could not; g0 = 2 -
    spec[3] / t0 within [1, 1.5], spec[3] the sampled threshold before (inf at first)."""
    t0 = F32(t0)
    with np.errstate(over="ignore", invalid="ignore"):
        g0 = np.minimum(np.maximum(F32(2) - F32(F32(prev_t0) / t0), F32(1)), F32(1.5))
    mw = F32(0.985) if cnt > K.WIN_MAX else (F32(0.97) if window_keys > 0 else F32(0.9))
    return F32(F32(t0 * mw) * F32(g0))


@pytest.mark.parametrize("order", ["index", "topk"])
def test_batch_window_rows(L, order):
    """DGCBatch keeps spec[2] in its workspace: step 0 (test_batch_decisions_match_oracle's
    warm-up, no window yet: the passes over the samples) leaves fl32(fl32(t0_warm * 0.9f) *
    1.0f) there, steps 1 and 2 are designed against the key that the step before left — the
    record's window_keys confirms it: a key one ulp lower takes the sample designed one step
    below it into the window, a higher one drops the k-th key's ties at it."""
    import staircase as S
    from dgc.batch import DGCBatch
    from test_gpu_batch import _assert_sent
    b = DGCBatch([(n, (numel,)) for n, numel in BATCH], compress_ratio=0.001, momentum=0.9, nesterov=False,
                 device=DEV, seed=5, resample_order=order)
    T = len(BATCH)
    t0_warm = F32(S.T0)
    spec2 = [None] * T
    prev_t0 = [F32(np.inf)] * T
    for step in (0, 1, 2):
        starts = b.draw_starts()
        want = {}
        for t, (tname, numel) in enumerate(BATCH):
            attrs = O.attributes(numel, 0.001)
            assert attrs[1:] == tuple(b.attrs[t])
            if step == 0:
                g, case = S.generate("warmup", numel, start=starts[t], t0=float(t0_warm))[0].grad, None
            else:
                wk = int(K.keys_of([spec2[t]])[0])
                case = K.engine_row(BATCH_ROWS[step][t], attrs, starts[t], wk, seed=100 * step + t)
                assert K.route(case, padded=True) == (case.route, case.window_keys)
                g = case.grad
            ov, oi, oinfo = O.compress_step(g, np.zeros(numel, F32), np.zeros(numel, F32), attrs, starts[t],
                                            nesterov=False)
            assert oinfo["branch"] == "ok" and len(oinfo["counts"]) == 1, (step, tname, oinfo["branch"])
            want[tname] = (g, ov, oi, oinfo, case)
            b.grad(tname).copy_(torch.from_numpy(g.copy()))
        b.compress(starts)
        b.decompress()
        torch.cuda.synchronize()
        sent, infos = b.transmitted(), b.infos()
        for t, (tname, numel) in enumerate(BATCH):
            g, ov, oi, oinfo, case = want[tname]
            inf, key = infos[t], (order, step, tname, case and case.name)
            print(key, inf)
            assert bits(F32(inf["threshold0"])) == bits(oinfo["thresholds"][0]), (key, inf)
            assert bits(F32(inf["threshold"])) == bits(oinfo["threshold"]), (key, inf)
            assert inf["branch"] == "ok" and inf["recounts"] == 0, (key, inf)
            assert inf["candidates"] == oinfo["counts"][-1] and inf["count"] == len(oi), (key, inf)
            cnt = 0
            if case is not None:
                assert bits(F32(inf["threshold0"])) == case.t0_key, (key, inf)
                assert inf["window_keys"] == case.window_keys, (key, inf, case.expect)
                cnt = case.expect["cnt"]
            else:
                assert inf["window_keys"] == 0, (key, inf)   # spec[2] still inf: an empty window, the samples
            gv, gi = sent[tname]
            _assert_sent(gi, gv, oi, ov, inf, key)
            ref = g.copy()
            ref[oi] = 0
            assert np.array_equal(bits(b.velocity_of(tname).cpu().numpy()), bits(ref)), key
            assert np.array_equal(bits(b.momentum_of(tname).cpu().numpy()), bits(ref)), key
            assert np.array_equal(bits(b.out(tname).cpu().numpy()), bits(O.decompress([ov], [oi], numel, 1))), key
            spec2[t] = next_window_key(oinfo["thresholds"][0], prev_t0[t], cnt, inf["window_keys"])
            prev_t0[t] = oinfo["thresholds"][0]
        if step == 0:
            assert all(bits(s2) == bits(F32(F32(t0_warm * F32(0.9)) * F32(1.0))) for s2 in spec2)
        b.vec_flat.zero_()   # (flushes the deferred masking first) every step starts from zero state
        b.mmt_flat.zero_()
