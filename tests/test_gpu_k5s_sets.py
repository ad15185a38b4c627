"""K5s — the index-order resample set (csrc/select_set.hpp) — on tests/k5sets.py's rows: the
k-th key at the bin edges of both radix passes, ties inside and across the k boundary, every
candidate count at which the workgroup count, the stretch length or the register / L2 split
changes, and the selected keys laid over the stretches three ways. A set row's payload is
torch.topk's set in ascending index order, a replay row's is torch.topk's order; indices, values
(by bit pattern), vec and mmt are compared exactly — no tolerances. tests/test_k5s_sets_cpu.py
confirms every row's route.

(1) ``dgc_select(resample_order = 1)`` on every row, sync 1 and 0, fused into the wide emit and as
k_emit + k_resample_set (DGC_EMIT_SHAPE=quarter), all four calls on one zero-filled workspace
whose merged histograms must be zero again after each. (2) Sequences of different rows on ONE
workspace (zero at rest). (3) DGCBatch and DGCBucket(resample_order="index") on sampled lattices
that reproduce the rows.
"""
import random
import time

import numpy as np
import pytest
import torch

import k5sets as K
from oracle import dgc_oracle as O
from test_gpu_parity import DEV, L, bits, select_dev  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
FLAGS = {"K5_BROKEN": 2, "k5s_fallback": 8, "k5s_broken": 16}   # dgc/_lib.py; K5_FALLBACK = 1 is the machine's
TIES_EXACT, TIES_SET = 1, 2
SHAPES = ("wide", "quarter")   # the set fused into k_emit_wide_t<true> | k_emit, then k_resample_set


def topk_order(values, k):
    return torch.topk(torch.from_numpy(np.abs(values)), k, 0, largest=True, sorted=False)[1].numpy()


# ------------------------------------------------------------------ the workspace
SETG_HEAD = 8                                          # arrive .. mx
SETG_WORDS = SETG_HEAD + K.K_SET_G_BIG + K.BINS0 + K.BINS1
TAIL_BYTES = 256 + 384 * 4                             # fin_ticket (16 words, padded), chain (kChainWords)


def setg_words(ws, T=1):
    """SetG[T] of a selection workspace as uint32 [T, words]. carve_select (select_layout.hpp)
    takes setg, fin_ticket and chain last, each from a 256-B boundary."""
    size = -(-T * SETG_WORDS * 4 // 256) * 256
    lo = ws.numel() - TAIL_BYTES - size
    return ws[lo: lo + T * SETG_WORDS * 4].view(torch.int32).cpu().numpy().view(np.uint32).reshape(T, SETG_WORDS)


def assert_hists_at_rest(ws, key, T=1):
    g = setg_words(ws, T)
    # the reset's own words show that this is where SetG lies: mn = 0xFFFFFFFF, mx = 0
    assert np.all(g[:, 6] == 0xFFFFFFFF) and np.all(g[:, 7] == 0), (key, g[:, :SETG_HEAD])
    hist = g[:, SETG_HEAD + K.K_SET_G_BIG:]
    t, q = np.nonzero(hist)
    assert t.size == 0, (key, "merged histogram words not re-zeroed (tensor, word, value):",
                         list(zip(t[:8], q[:8], hist[t[:8], q[:8]])))


# ------------------------------------------------------------------ (1) dgc_select
def check_select(L, e, values, k, route, key, ws, sync, **kw):
    """One dgc_select(resample_order = 1) call on the embedded candidates against torch.topk."""
    order = topk_order(values, k)
    is_set = route[0] == "set"
    want = np.sort(e.pos[order]) if is_set else e.pos[order]
    t0 = time.perf_counter()
    gv, gi, gvec, gmmt, branch, inf = select_dev(L, e.vec, e.mmt, float(e.thr), e.attrs, sync=sync, resample_order=1,
                                                 ws=ws, **kw)
    msg = (key, f"sync={sync}", f"{time.perf_counter() - t0:.3f}s", f"k5_status={inf.k5_status}",
           f"spilled={inf.overflow_segments}")
    print("k5s", *msg)
    for flag, bit in FLAGS.items():
        if is_set or flag == "K5_BROKEN":
            assert not inf.k5_status & bit, (flag, msg)
    assert branch == "resample" and inf.candidates == values.size, (msg, branch, inf.candidates)
    assert inf.tie_rule == (TIES_SET if is_set else TIES_EXACT), (msg, inf.tie_rule)
    assert gi.size == k and np.array_equal(gi.astype(np.int64), want), msg
    assert gi.dtype == (np.int32 if kw.get("int32") else np.int64)
    wv = e.vec[want].astype(np.float16) if kw.get("fp16") else e.vec[want]
    assert np.array_equal(bits(gv), bits(wv)), msg
    ev, em = e.vec.copy(), e.mmt.copy()
    if kw.get("update_memory", True):
        O.update(em, ev, want, kw.get("masking", True))
    assert np.array_equal(bits(gvec), bits(ev)) and np.array_equal(bits(gmmt), bits(em)), msg
    return inf


def run_row(L, name, monkeypatch, shapes=SHAPES, **kw):
    r, v, e = K.build(name)
    ws = torch.zeros(L.dgc_select_workspace(e.attrs[0], r.k), dtype=torch.uint8, device=DEV)
    for shape in shapes:
        monkeypatch.setenv("DGC_EMIT_SHAPE", shape)
        for sync in (1, 0):
            inf = check_select(L, e, v, r.k, r.route, (name, shape), ws, sync, **kw)
            assert_hists_at_rest(ws, (name, shape, sync))
            if r.layout == "scattered":
                assert inf.overflow_segments == 0, name      # the gather read the lists
            elif r.layout == "dense":
                assert inf.overflow_segments > 0, name       # ... re-read spilled segments


KEY_ROWS = [r.name for r in K.ROWS if not r.name.startswith("count_")]
COUNT_ROWS = [r.name for r in K.ROWS if r.name.startswith("count_") and r.route[0] == "set"]
BIG_REPLAY = "count_8388609_k1000000"


@pytest.mark.parametrize("name", KEY_ROWS)
def test_key_row(L, name, monkeypatch):
    run_row(L, name, monkeypatch)


@pytest.mark.parametrize("name", COUNT_ROWS)
def test_count_row(L, name, monkeypatch):
    run_row(L, name, monkeypatch)


def test_count_row_past_rounds_max(L, monkeypatch):
    """8388609 candidates: 8193 rounds over 128 workgroups are 65 per stretch, past
    kSetRoundsMax — every K5s workgroup returns and the exact replay serves 8.4M candidates."""
    run_row(L, BIG_REPLAY, monkeypatch)


@pytest.mark.parametrize("name", [r.name for r in K.ROWS if r.route[0] == "replay" and r.c > K.K_NTH_LDS
                                  and r.name != BIG_REPLAY])
def test_replay_row_with_gathered_queue(L, name, monkeypatch):
    """DGC_K5_GLOBAL=multi: the replay's global phase runs on several workgroups, so the gather
    writes the queue itself; by default (above) k_nth_select rebuilds it from cand_key."""
    monkeypatch.setenv("DGC_K5_GLOBAL", "multi")
    run_row(L, name, monkeypatch)


def test_replay_row_past_rounds_max_with_gathered_queue(L, monkeypatch):
    monkeypatch.setenv("DGC_K5_GLOBAL", "multi")
    run_row(L, BIG_REPLAY, monkeypatch, shapes=("wide",))


@pytest.mark.parametrize("name,kw", [
    ("count_16385_k300_waves", dict(fp16=True, int32=True)),
    ("p1_alias_coop_t1.0", dict(masking=False)),
    ("tie_last_one_t0.75", dict(update_memory=False)),
    ("count_65537_k2000_last", dict(fp16=True, int32=True, masking=False)),
], ids=["fp16_int32", "no_masking", "no_update", "fp16_int32_no_masking"])
def test_wire_and_memory_flags(L, name, kw, monkeypatch):
    assert K.ROW_BY_NAME[name].route[0] == "set"
    run_row(L, name, monkeypatch, **kw)


# ------------------------------------------------------------------ (2) zero at rest
P = 50 << K.K_SET_LO0
# (k, N, the members: (c, D, design / placement arguments, the route's first fields)). Later
# members' k-th keys lie in LOWER bins than what the members before them counted: a bin left
# behind would sit above the k-th key and shift it.
SEQUENCES = {
    "top_bin_break_then_set": (1000, 130_003, [
        (40003, K.TOP + 5, {}, ("replay", "span")),                    # pass 1 never ran: only hist0 is re-zeroed
        (40003, P + 1234, {}, ("set", 4, 4, 10, False)),
        (30011, (3 << K.K_SET_LO0) + 1, {}, ("set", 4, 4, 8, False))]),
    "tied_then_set": (1000, 130_003, [
        (40003, P + 300, dict(eq=7, ka=3), ("replay", "tied")),
        (40003, (7 << K.K_SET_LO0) - 1, {}, ("set", 4, 4, 10, False)),
        (40003, 0, {}, ("replay", "tied")),
        (20480, 4097, dict(eq=3, ka=3), ("set", 4, 4, 5, False))]),
    "G5_G4_G1": (2000, 200_003, [
        # G = 5 divides neither 4096 nor 8192: the last bins of both histograms (a key past the span
        # in hist0's 4095, the k-th key's low bits all one in hist1's 8191) lie in the last share
        (65537, (9 << K.K_SET_LO0) + 8191, dict(how="waves", G=5, above=(1 << K.K_SET_SPAN,)), ("set", 8, 5, 13, False)),
        (65536, (5 << K.K_SET_LO0) + 100, dict(how="last", G=4), ("set", 8, 4, 16, False)),
        (16384, (2 << K.K_SET_LO0) + 5, {}, ("set", 8, 1, 16, False)),
        (65537, 77, dict(how="first", G=5), ("set", 8, 5, 13, False))]),
    "OVF_then_registers": (100_000, 6_300_007, [
        (2097153, (9 << K.K_SET_LO0) + 17, dict(how="waves", G=128), ("set", 128, 128, 17, True)),
        (2097152, (4 << K.K_SET_LO0) + 8191, dict(how="waves", G=128), ("set", 128, 128, 16, False)),
        (1048577, 12, {}, ("set", 128, 65, 16, False))]),
}


@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_rows_back_to_back_on_one_workspace(L, seq, monkeypatch):
    """Zero at rest: each workgroup re-zeroes its share of the merged histograms of the passes
    it ran — a share that depends on G, and one pass fewer after the top-bin break."""
    k, N, members = SEQUENCES[seq]
    built = []
    for j, (c, D, kw, head) in enumerate(members):
        v = K.make(c, k, 1.0, D, seed=1000 + j, **kw)
        got = K.route(K.keys_of(v).astype(np.int64), 1.0, k, K.cand_cap(N, k))
        assert got[:len(head)] == head, (seq, j, got)
        built.append((v, K.embed(v, k, "dense", N, 1.0, seed=j), got))
    ws = torch.zeros(L.dgc_select_workspace(N, k), dtype=torch.uint8, device=DEV)
    for shape in SHAPES:
        monkeypatch.setenv("DGC_EMIT_SHAPE", shape)
        for sync in (0, 1):
            for j, (v, e, got) in enumerate(built):
                check_select(L, e, v, k, got, (seq, j, shape), ws, sync)
                assert_hists_at_rest(ws, (seq, j, shape, sync))


# ------------------------------------------------------------------ (3) the engines
# tensor, numel, then per designed step (c, D, design arguments, the route's first fields); None:
# a seeded normal gradient. Every tensor's route changes from step to step.
INNER = (100 << K.K_SET_LO0) + 4097
BATCH = [
    ("t_one", 200_003, [(3001, INNER, {}, ("set", 1, 1, 3)), (3001, INNER, dict(eq=4, ka=2), ("replay", "tied")),
                        (2900, 8191, dict(eq=3, ka=3), ("set", 1, 1, 3))]),
    ("t_g4", 500_000, [(20000, INNER, dict(how="waves", G=4), ("set", 4, 4, 5)), (20000, K.TOP, {}, ("replay", "span")),
                       (16385, 8192, dict(how="last", G=4), ("set", 4, 4, 5))]),
    ("t_g7", 2_000_000, [(100_000, INNER, dict(how="waves", G=7), ("set", 8, 7, 14)),
                         (100_000, INNER, dict(eq=9, ka=1), ("replay", "tied")),
                         (127_999, 5, dict(how="first", G=8), ("set", 8, 8, 16))]),
    ("t_tied", 300_001, [(3001, INNER, dict(eq=5, ka=3), ("replay", "tied")), (3001, INNER, {}, ("set", 4, 1, 3)),
                         (3001, 0, {}, ("replay", "tied"))]),
    ("t_span", 250_007, [(3001, K.TOP + 9, {}, ("replay", "span")), (3001, K.TOP - 1, {}, ("set", 1, 1, 3)),
                         (3001, 1 << K.K_SET_SPAN, {}, ("replay", "span"))]),
    ("t_normal", 200_003, None),
]


@pytest.mark.parametrize("shape", SHAPES)
def test_batch_steps_over_designed_sets(L, shape, monkeypatch):
    """One fp32 DGCBatch (resample_order="index") over a one-workgroup set, a G = 4 set, a G = 7
    set, a tied tensor, a wide-span tensor and an ordinary one, three steps in which every
    designed tensor changes its route (set -> replay -> set, or the reverse). The candidates lie
    on the sampled lattice as in test_batch_step_over_two_killers (k5sets.on_lattice); zero
    state and nesterov=False before every step: the velocity is the gradient."""
    from dgc.batch import DGCBatch
    from oracle import synth
    from test_gpu_batch import _assert_sent
    monkeypatch.setenv("DGC_EMIT_SHAPE", shape)
    b = DGCBatch([(n, (numel,)) for n, numel, _ in BATCH], compress_ratio=0.001, momentum=0.9, nesterov=False,
                 device=DEV, seed=23, resample_order="index")
    T = len(BATCH)
    for step in range(3):
        starts = b.draw_starts()
        want = {}
        for t, (tname, numel, plan) in enumerate(BATCH):
            attrs = O.attributes(numel, 0.001)
            k = attrs[1]
            if plan is None:
                g, got = synth.gradient(321 + step, numel, "normal", 1e-3), None
            else:
                c, D, kw, head = plan[step]
                v = K.make(c, k, 1.0, D, seed=50 * t + step, **kw)
                g, pos, v = K.on_lattice(v, numel, attrs, starts[t], seed=7 * t + step)
                got = K.route(K.keys_of(v).astype(np.int64), float(np.abs(v).min()), k, K.cand_cap(numel, k))
                assert got[:len(head)] == head, (step, tname, got)
            ov, oi, oinfo = O.compress_step(g, np.zeros(numel, F32), np.zeros(numel, F32), attrs, starts[t],
                                            nesterov=False)
            if plan is not None:
                assert oinfo["branch"] == "resample" and oinfo["counts"] == [c], (step, tname, oinfo["counts"])
                assert np.array_equal(oi, pos[topk_order(v, k)])
            want[tname] = (g, ov, oi, oinfo, got)
            b.grad(tname).copy_(torch.from_numpy(g))
        b.compress(starts)
        b.decompress()
        torch.cuda.synchronize()
        sent, infos = b.transmitted(), b.infos()
        for t, (tname, numel, plan) in enumerate(BATCH):
            g, ov, oi, oinfo, got = want[tname]
            inf, key = infos[t], (shape, step, tname, got)
            print("k5s-batch", key, inf)
            assert inf["branch"] == oinfo["branch"] and inf["candidates"] == oinfo["counts"][-1], (key, inf)
            if got is not None:
                assert inf["tie_rule"] == ("set" if got[0] == "set" else "exact"), (key, inf)
                if got[0] == "set":
                    assert not inf["k5s_fallback"] and not inf["k5s_broken"], (key, inf)
            gv, gi = sent[tname]
            _assert_sent(gi, gv, oi, ov, inf, key)
            ref = g.copy()
            ref[oi] = 0
            assert np.array_equal(bits(b.velocity_of(tname).cpu().numpy()), bits(ref)), key
            assert np.array_equal(bits(b.momentum_of(tname).cpu().numpy()), bits(ref)), key
            assert np.array_equal(bits(b.out(tname).cpu().numpy()), bits(O.decompress([ov], [oi], numel, 1))), key
        assert_hists_at_rest(b.ws, (shape, step), T)
        b.vec_flat.zero_()   # (flushes the deferred masking first) every step starts from zero state
        b.mmt_flat.zero_()


def bf16_run_values(c, k, above, rng):
    """c candidates of four bf16 magnitudes: ``above`` at 3.0 and k - above at 2.0 (the k boundary
    lies between 2.0 and 1.5: eq = k_rem = k - above), the rest 1.5 and 1.0, in seeded order."""
    mag = np.concatenate([np.full(above, 3.0), np.full(k - above, 2.0), np.full((c - k) // 2, 1.5),
                          np.full(c - k - (c - k) // 2, 1.0)]).astype(F32)
    return rng.permutation(mag) * np.where(rng.random(c) < 0.5, F32(-1), F32(1))


@pytest.mark.parametrize("shape", SHAPES)
def test_batch16_set_between_two_runs(L, shape, monkeypatch):
    """One bf16 DGCBatch step: 20000 candidates of four bf16 magnitudes, the k boundary between
    the run at 2.0 (200 keys, all inside the top k = 500) and the run at 1.5 — a G = 4 set with
    eq = k_rem = 200. Against the torch-CPU port on bf16 tensors."""
    from dgc.batch import DGCBatch
    from oracle import torch_cpu as TC
    monkeypatch.setenv("DGC_EMIT_SHAPE", shape)
    N, c = 500_000, 20000
    b = DGCBatch([("t16", (N,)), ("small", (300, 1000))], compress_ratio=0.001, momentum=0.9, nesterov=False,
                 device=DEV, seed=31, resample_order="index", dtype=torch.bfloat16, world_size=1)
    attrs = TC.attributes(N, 0.001)
    k = attrs[1]
    assert attrs[1:] == tuple(b.attrs[0]) and k == 500
    starts = b.draw_starts()
    v = bf16_run_values(c, k, 300, np.random.default_rng(3))
    g32, pos, v = K.on_lattice(v, N, attrs, starts[0], seed=4)
    got = K.route(K.keys_of(v).astype(np.int64), 1.0, k, K.cand_cap(N, k))
    assert got == ("set", 4, 4, 5, False, (1 << 23) >> K.K_SET_LO0, 0, 200), got
    g = torch.from_numpy(g32).to(torch.bfloat16)
    assert np.array_equal(g.float().numpy()[pos], v) and int((g.float().abs() >= 1.0).sum()) == c   # nothing rounded up
    want_v, want_i = TC.sparsify(g.clone(), *attrs, starts[0])
    assert want_i.numel() == k and np.array_equal(np.sort(want_i.numpy()), pos[np.abs(v) >= 2.0])
    b.grad("t16").copy_(g.to(DEV))
    b.grad("small").copy_((torch.randn(300, 1000, generator=torch.Generator().manual_seed(5)) * 1e-3).to(torch.bfloat16))
    b.compress(starts)
    b.decompress()
    torch.cuda.synchronize()
    inf = b.infos()[0]
    print("k5s-batch16", shape, inf)
    assert inf["branch"] == "resample" and inf["candidates"] == c and inf["tie_rule"] == "set", inf
    assert not inf["k5s_fallback"] and not inf["k5s_broken"], inf
    gv, gi = b.transmitted()["t16"]
    o = torch.argsort(want_i)
    assert torch.equal(gi.cpu().long(), want_i[o])
    assert np.array_equal(bits16(gv), bits16(want_v[o]))
    ref = g.clone()
    ref[want_i] = 0
    assert np.array_equal(bits16(b.velocity_of("t16")), bits16(ref))
    assert np.array_equal(bits16(b.momentum_of("t16")), bits16(ref))
    assert np.array_equal(bits16(b.out("t16")), bits16(TC.decompress(want_v, want_i, torch.empty(N, dtype=torch.bfloat16), 1)))
    assert_hists_at_rest(b.ws, ("batch16", shape), 2)


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_bucket_index_order_set(L, shape, monkeypatch):
    """One DGCBucket(resample_order="index") step whose resample is a G = 4 set."""
    from dgc.bucket import DGCBucket
    from test_gpu_bucket16 import payload_of
    monkeypatch.setenv("DGC_EMIT_SHAPE", shape)
    N = 500_000
    b = DGCBucket(N, compress_ratio=0.001, momentum=0.9, nesterov=False, device=DEV, world_size=1, seed=11,
                  resample_order="index")
    attrs = O.attributes(N, 0.001)
    assert attrs == (N, b.k, b.num_samples, b.top_k_samples, b.stride)
    start = random.Random(11).randint(0, attrs[4] - 1)
    v = K.make(20000, b.k, 1.0, INNER, how="waves", G=4, seed=5)
    g, pos, v = K.on_lattice(v, N, attrs, start, seed=6)
    assert K.route(K.keys_of(v).astype(np.int64), 1.0, b.k, K.cand_cap(N, b.k))[:4] == ("set", 4, 4, 5)
    ov, oi, oinfo = O.compress_step(g, np.zeros(N, F32), np.zeros(N, F32), attrs, start, nesterov=False)
    assert oinfo["branch"] == "resample" and oinfo["counts"] == [20000]
    out = torch.full((N,), float("nan"), device=DEV)
    b.step(torch.from_numpy(g).to(DEV), out)
    torch.cuda.synchronize()
    assert b.start == start
    inf = b.last_info()
    print("k5s-bucket", shape, inf)
    assert inf["branch"] == "resample" and inf["candidates"] == 20000 and inf["tie_rule"] == "set", inf
    assert not inf["k5s_fallback"] and not inf["k5s_broken"], inf
    vals, idx = payload_of(b)
    o = np.argsort(oi, kind="stable")
    assert np.array_equal(idx.cpu().numpy(), oi[o]) and np.array_equal(bits(vals.cpu().numpy()), bits(ov[o]))
    ref = g.copy()
    ref[oi] = 0
    assert np.array_equal(bits(b.vec.cpu().numpy()), bits(ref)) and np.array_equal(bits(b.mmt.cpu().numpy()), bits(ref))
    assert np.array_equal(bits(out.cpu().numpy()), bits(O.decompress([ov], [oi], N, 1)))
