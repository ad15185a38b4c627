"""The selection's threshold-adaptation decisions, pinned with staircase gradients
(tests/staircase.py): the count at every rung of the ladder is designed, the K1 list
threshold (``spec[0]``) is chosen so that the path is, and every result is compared bit
for bit with the oracle, which first confirms that the case is what its row says.

Engines: (a) the C ABI, one tensor per ``dgc_compress`` call on a fresh workspace, in three
modes; (b) ``DGCBucket`` on bf16 / fp16 state; (c) ``DGCBatch``, several cases in one call.
What a row expects of ``dgc_select_info`` — the full passes over vec, how the lowering was
served, where the landed count came from, what the spilled segments did — stands in
``PAIRS`` as data: a rewrite that changes the routing has to edit it. ``staircase.route``
restates csrc/select.hip's routing and tests/test_staircase_cpu.py holds the table to it.

Not pinned here: N > 2^32, clipping, W > 1 (the sample window, S > 32768: test_gpu_k3_edges.py).
"""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import staircase as S
from oracle import dgc_oracle as O
from oracle import torch_cpu as TC
from test_gpu_parity import DEV, L, P, bits, check, stream  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu

N_ODD = 1_000_003   # 977 segments, one group, a 3-element scalar tail
N_BIG = 2_100_004   # three groups; a multiple of 4, so the first list count may carry the
#                     speculative first-k payload (select_core's `fuse` needs no scalar tail)

# mode -> (sync mode, update_memory): device decisions with the deferred masking (the fused
# count-emit, k_chain_one), with the immediate one (no fused emit), and the host loop
# (k_lower_lists + k_lower_counts as launches)
MODES = {"dev2": (0, 2), "dev1": (0, 1), "host": (1, 1)}

# case, spec[0] setting (staircase.spec_of), then what dgc_select_info and the routing must
# show: full passes over vec; the lowering ("-" none, "lists" k_lower_lists decided,
# "lists_js_ms" its js = ms = max_iters case, "mixed" it served rungs but k_lower_counts
# decided, "vec" k_lower_counts alone, "steps" a count pass per move); where the landed count
# came from; the spilled segments ("reread" kept, "+cut" the k-th landed element inside one,
# "dropped" the lists given up)
PAIRS = [
    ('ok_L',          'inf',        1, '-',           'full',  ''),
    ('ok_L',          'at_landed',  0, '-',           'lists', ''),
    ('ok_L',          'spill1',     0, '-',           'lists', 'reread'),
    ('ok_L',          'above_t0',   1, '-',           'full',  ''),
    ('ok_k',          'inf',        1, '-',           'full',  ''),
    ('ok_k',          'at_landed',  0, '-',           'lists', ''),
    ('ok_k',          'spill1',     0, '-',           'lists', 'reread'),
    ('trunc_k1',      'inf',        1, '-',           'full',  ''),
    ('trunc_k1',      'at_landed',  0, '-',           'lists', ''),
    ('trunc_k1',      'spill1',     0, '-',           'lists', 'reread'),
    ('trunc_U',       'inf',        1, '-',           'full',  ''),
    ('trunc_U',       'at_landed',  0, '-',           'lists', ''),
    ('trunc_U',       'spill1',     0, '-',           'lists', 'reread+cut'),
    ('trunc_U',       'spill_max',  0, '-',           'lists', 'reread'),
    ('trunc_U',       'spill_drop', 1, '-',           'full',  'dropped'),
    ('resample_U1',   'inf',        1, '-',           'full',  ''),
    ('resample_U1',   'at_landed',  0, '-',           'lists', ''),
    ('resample_U1',   'spill1',     0, '-',           'lists', 'reread'),
    ('j1_ok',         'above_t0',   2, 'vec',         'full',  ''),
    ('j1_ok',         'mid23',      0, 'lists',       'lists', ''),
    ('j1_ok',         'at_landed',  0, 'lists',       'lists', ''),
    ('j1_trunc',      'above_t0',   2, 'vec',         'full',  ''),
    ('j1_trunc',      'mid23',      0, 'lists',       'lists', ''),
    ('j1_trunc',      'at_landed',  0, 'lists',       'lists', ''),
    ('j1_resample',   'above_t0',   2, 'vec',         'full',  ''),
    ('j1_resample',   'mid23',      0, 'lists',       'lists', ''),
    ('j1_resample',   'at_landed',  0, 'lists',       'lists', ''),
    ('j2_ok',         'above_t0',   2, 'vec',         'full',  ''),
    ('j2_ok',         'mid23',      0, 'lists',       'lists', ''),
    ('j2_ok',         'at_landed',  0, 'lists',       'lists', ''),
    ('j2_trunc',      'above_t0',   2, 'vec',         'full',  ''),
    ('j2_trunc',      'mid23',      0, 'lists',       'lists', ''),
    ('j2_trunc',      'at_landed',  0, 'lists',       'lists', ''),
    ('j2_resample',   'above_t0',   2, 'vec',         'full',  ''),
    ('j2_resample',   'mid23',      0, 'lists',       'lists', ''),
    ('j2_resample',   'at_landed',  0, 'lists',       'lists', ''),
    ('j4_ok',         'inf',        2, 'vec',         'full',  ''),
    ('j4_ok',         'mid23',      1, 'mixed',       'full',  ''),
    ('j4_ok',         'at_landed',  0, 'lists',       'lists', ''),
    ('j4_ok',         'spill1',     0, 'lists',       'lists', 'reread'),
    ('j4_trunc',      'inf',        2, 'vec',         'full',  ''),
    ('j4_trunc',      'mid23',      1, 'mixed',       'full',  ''),
    ('j4_trunc',      'at_landed',  0, 'lists',       'lists', ''),
    ('j4_trunc',      'spill1',     0, 'lists',       'lists', 'reread+cut'),
    ('j4_resample',   'inf',        2, 'vec',         'full',  ''),
    ('j4_resample',   'mid23',      1, 'mixed',       'full',  ''),
    ('j4_resample',   'at_landed',  0, 'lists',       'lists', ''),
    ('j4_resample',   'spill1',     0, 'lists',       'lists', 'reread'),
    ('j5_ok',         'above_t0',   2, 'vec',         'full',  ''),
    ('j5_ok',         'mid23',      1, 'mixed',       'full',  ''),
    ('j5_ok',         'at_landed',  0, 'mixed',       'lists', ''),
    ('j5_ok',         'spill_max',  0, 'mixed',       'lists', 'reread'),
    ('j5_trunc',      'above_t0',   2, 'vec',         'full',  ''),
    ('j5_trunc',      'mid23',      1, 'mixed',       'full',  ''),
    ('j5_trunc',      'at_landed',  0, 'mixed',       'lists', ''),
    ('j5_trunc',      'spill_max',  0, 'mixed',       'lists', 'reread'),
    ('j5_resample',   'above_t0',   2, 'vec',         'full',  ''),
    ('j5_resample',   'mid23',      1, 'mixed',       'full',  ''),
    ('j5_resample',   'at_landed',  0, 'mixed',       'lists', ''),
    ('j5_resample',   'spill_max',  0, 'mixed',       'lists', 'reread'),
    ('j9_ok',         'inf',        2, 'vec',         'full',  ''),
    ('j9_ok',         'at_landed',  0, 'mixed',       'lists', ''),
    ('j9_ok',         'spill1',     0, 'mixed',       'lists', 'reread'),
    ('j9_ok',         'spill_drop', 2, 'vec',         'full',  'dropped'),
    ('j9_trunc',      'inf',        2, 'vec',         'full',  ''),
    ('j9_trunc',      'at_landed',  0, 'mixed',       'lists', ''),
    ('j9_trunc',      'spill1',     0, 'mixed',       'lists', 'reread+cut'),
    ('j9_resample',   'inf',        2, 'vec',         'full',  ''),
    ('j9_resample',   'at_landed',  0, 'mixed',       'lists', ''),
    ('j9_resample',   'spill1',     0, 'mixed',       'lists', 'reread'),
    ('j2_ok_k',       'above_t0',   2, 'vec',         'full',  ''),
    ('j2_ok_k',       'mid23',      0, 'lists',       'lists', ''),
    ('j2_ok_k',       'at_landed',  0, 'lists',       'lists', ''),
    ('j2_trunc_k1',   'above_t0',   2, 'vec',         'full',  ''),
    ('j2_trunc_k1',   'mid23',      0, 'lists',       'lists', ''),
    ('j2_trunc_k1',   'at_landed',  0, 'lists',       'lists', ''),
    ('ex_short',      'inf',        2, 'vec',         'full',  ''),
    ('ex_short',      'mid23',      1, 'mixed',       'full',  ''),
    ('ex_short',      'below',      0, 'mixed',       'lists', ''),
    ('ex_trunc',      'inf',        2, 'vec',         'full',  ''),
    ('ex_trunc',      'mid23',      1, 'mixed',       'full',  ''),
    ('ex_trunc',      'below',      0, 'mixed',       'lists', ''),
    ('ex_over',       'inf',        2, 'vec',         'full',  ''),
    ('ex_over',       'mid23',      1, 'mixed',       'full',  ''),
    ('ex_over',       'below',      0, 'mixed',       'lists', ''),
    ('ex_over',       'spill1',     0, 'mixed',       'lists', 'reread+cut'),
    ('mi0_low',       'inf',        1, '-',           'full',  ''),
    ('mi0_low',       'at_landed',  0, '-',           'lists', ''),
    ('mi0_low',       'spill1',     0, '-',           'lists', 'reread'),
    ('mi0_over',      'inf',        1, '-',           'full',  ''),
    ('mi0_over',      'at_landed',  0, '-',           'lists', ''),
    ('mi0_over',      'spill1',     0, '-',           'lists', 'reread+cut'),
    ('mi2_ex',        'mid23',      0, 'lists',       'lists', ''),
    ('mi2_ex',        'at_landed',  0, 'lists',       'lists', ''),
    ('mi2_ex',        'inf',        2, 'vec',         'full',  ''),
    ('mi2_j1',        'above_t0',   2, 'vec',         'full',  ''),
    ('mi2_j1',        'mid23',      0, 'lists',       'lists', ''),
    ('mi2_j1',        'at_landed',  0, 'lists',       'lists', ''),
    ('mi4_none',      'at_landed',  0, 'lists_js_ms', 'lists', ''),
    ('mi4_none',      'mid23',      1, 'mixed',       'full',  ''),
    ('mi4_none',      'below',      0, 'lists_js_ms', 'lists', ''),
    ('mi4_last',      'at_landed',  0, 'lists',       'lists', ''),
    ('mi4_last',      'inf',        2, 'vec',         'full',  ''),
    ('mi16_j16',      'inf',        2, 'vec',         'full',  ''),
    ('mi16_j16',      'below',      0, 'mixed',       'lists', ''),
    ('mi16_j15',      'above_t0',   2, 'vec',         'full',  ''),
    ('mi16_j15',      'at_landed',  0, 'mixed',       'lists', ''),
    ('mi17_j3',       'inf',        4, 'steps',       'full',  ''),
    ('mi17_j3',       'mid23',      1, 'steps',       'full',  ''),
    ('mi17_j3',       'at_landed',  0, 'steps',       'lists', ''),
    ('mi17_j1_res',   'above_t0',   2, 'steps',       'full',  ''),
    ('mi17_j1_res',   'mid23',      0, 'steps',       'lists', ''),
    ('mi17_j1_res',   'at_landed',  0, 'steps',       'lists', ''),
    ('up2_trunc',     'inf',        1, 'steps',       'lists', ''),
    ('up2_trunc',     'at_landed',  0, 'steps',       'lists', ''),
    ('up2_trunc',     'spill1',     0, 'steps',       'lists', 'reread'),
]
EXPECT = {(r[0], r[1]): r[2:] for r in PAIRS}

# the rows run again at the three-group size (modes dev2 and host)
BIG_ROWS = [('ok_L', 'at_landed'), ('trunc_U', 'spill1'), ('trunc_U', 'spill_max'), ('trunc_U', 'spill_drop'),
            ('resample_U1', 'at_landed'), ('j1_ok', 'mid23'), ('j2_trunc', 'above_t0'), ('j4_resample', 'at_landed'),
            ('j4_trunc', 'spill1'), ('j5_ok', 'at_landed'), ('j9_trunc', 'spill1'), ('ex_over', 'below'),
            ('mi4_none', 'at_landed'), ('mi17_j3', 'mid23'), ('up2_trunc', 'at_landed')]
# ... with grad / mmt / vec one element into their storage (4-B aligned only: dgc_compress
# then builds no lists and every kernel over vec takes its <false> form)
UNALIGNED_ROWS = [('trunc_U', 'at_landed'), ('j2_ok', 'mid23'), ('j5_resample', 'at_landed'), ('ex_trunc', 'below')]
# ... and under DGC_EMIT_SHAPE=quarter (k_emit)
QUARTER_ROWS = [('ok_k', 'inf'), ('trunc_U', 'spill1'), ('j4_trunc', 'spill1'), ('j9_ok', 'at_landed'),
                ('ex_over', 'spill1')]

# the 16-bit bucket's rows: j* in {0, 1, 4, 5} and exhausted
HALF_ROWS = [('ok_L', 'at_landed'), ('trunc_U', 'inf'), ('resample_U1', 'at_landed'), ('j1_ok', 'mid23'),
             ('j1_trunc', 'above_t0'), ('j4_ok', 'at_landed'), ('j4_resample', 'mid23'), ('j5_ok', 'at_landed'),
             ('j5_resample', 'above_t0'), ('ex_trunc', 'below'), ('ex_short', 'inf')]


@functools.lru_cache(maxsize=None)
def confirmed(name, N, dtype="float32", spill=0, cut=False):
    """The oracle's run of a case, after it confirmed that the case is what it says."""
    return S.assert_case_is_what_it_says(name, N, dtype, spill, cut)


def fused(case, row, mode, N):
    """What became of the speculative first-k payload of the first list count (select_core's
    `fuse`: device decisions, the deferred masking, no scalar tail): "accepted" when that
    count decided a first-k branch, "discarded" when a lowering or a resample followed, None
    where it was never written (no lists at t0, or not that mode)."""
    fp, lowering, landed, spill = EXPECT[row]
    spec0 = S.spec_of(row[1], case, N)[0]
    reach_t0 = np.isfinite(spec0) and spec0 <= S.ladder(S.T0, 0.8, 0)[0] and spill != "dropped"
    if mode != "dev2" or N % 4 or not reach_t0:
        return None
    return "accepted" if case.moves == 0 and case.branch != "resample" else "discarded"


# ------------------------------------------------------------------ engine (a): the C ABI
def compress_once(L, name, kind, mode, N, offset=0):
    """One dgc_compress call of a case on a fresh, zero-filled workspace and zero state, with
    spec[0] written first; returns what it produced, what the oracle says and the setting."""
    from dgc import _lib
    case = S.CASES[name]
    spec0, spill, cut = S.spec_of(kind, case, N)
    st, attrs, start, counts = S.generate(name, N, "float32", spill, cut)
    oracle = confirmed(name, N, "float32", spill, cut)
    _, k, Sn, ks, stride = attrs
    sync, um = MODES[mode]
    p = _lib.select_params(N, k, Sn, 1.3, 0.8, case.kw.get("max_iters", 10), case.kw.get("resample", True), True, um,
                           torch.float32, torch.int64)
    g = torch.zeros(N + 4, device=DEV)
    g[offset:offset + N].copy_(torch.from_numpy(st.grad))
    mmt, vec = torch.zeros(N + 4, device=DEV), torch.zeros(N + 4, device=DEV)
    wsz = L.dgc_compress_workspace(N, k, Sn)
    ws = torch.zeros(wsz, dtype=torch.uint8, device=DEV)
    spec = torch.full((8,), float("inf"), device=DEV)
    spec[0] = float(spec0)
    vals = torch.empty(k, device=DEV)
    idx = torch.empty(k, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    info = torch.zeros(_lib.INFO_BYTES, dtype=torch.uint8, device=DEV)
    ptrs = [t.data_ptr() + 4 * offset for t in (g, mmt, vec)]
    check(L, L.dgc_compress(*ptrs, 0.9, 0, start, stride, ks, ctypes.byref(p), P(spec), _lib.SPEC_MARGIN, P(vals),
                            P(idx), P(cnt), P(info), P(ws), wsz, sync, stream()))
    if um == 2:
        check(L, L.dgc_compress_flush(ptrs[2], ptrs[1], stride, ctypes.byref(p), P(ws), wsz, stream()))
    torch.cuda.synchronize()
    n = int(cnt.item())
    inf = _lib.info_dict(_lib.SelectInfo.from_buffer_copy(info.cpu().numpy().tobytes()), "dgc_compress")
    got = dict(values=vals.cpu().numpy()[:n], indices=idx.cpu().numpy()[:n], info=inf,
               vec=vec.cpu().numpy()[offset:offset + N], mmt=mmt.cpu().numpy()[offset:offset + N],
               guard=(vec.cpu().numpy(), mmt.cpu().numpy()))
    return got, oracle, dict(grad=st.grad, spec0=spec0, spill=spill, N=N, offset=offset)


def assert_matches_oracle(got, oracle, setting, key):
    """Bit for bit: threshold0, the final threshold, the branch, the counts, recounts = the
    number of threshold moves, indices in order, values, vec and mmt after the update."""
    ths, cnts, branch, ov, oi = oracle
    inf = got["info"]
    print(key, {f: inf[f] for f in ("branch", "recounts", "count", "candidates", "threshold0", "threshold",
                                    "full_passes", "list_threshold", "overflow_segments")})
    assert bits(np.float32(inf["threshold0"])) == bits(ths[0]), (key, inf)
    assert bits(np.float32(inf["threshold"])) == bits(ths[-1]), (key, inf)
    assert inf["branch"] == branch, (key, inf)
    assert inf["recounts"] == len(cnts) - 1, (key, inf)
    assert inf["candidates"] == cnts[-1] and inf["count"] == len(oi), (key, inf, cnts)
    assert np.array_equal(got["indices"], oi), (key, inf)
    assert np.array_equal(bits(got["values"]), bits(ov)), key
    want = setting["grad"].copy()
    want[oi] = 0
    assert np.array_equal(bits(got["vec"]), bits(want)), key
    assert np.array_equal(bits(got["mmt"]), bits(want)), key
    off, N = setting["offset"], setting["N"]
    for buf in got["guard"]:   # nothing written outside the tensor
        assert not buf[:off].any() and not buf[off + N:].any(), key


def assert_path_evidence(inf, row, setting, key, lists=True):
    """dgc_select_info's account of the path: the full passes the row states, the list
    threshold the call was given, and the designed spill count on a step served by kept lists."""
    fp, lowering, landed, spill = EXPECT[row]
    if not lists:   # no K1 lists at all: the row of the same case without them
        fp = 1 + (lowering != "-") if lowering != "steps" else None
    if fp is not None:
        assert inf["full_passes"] == fp, (key, inf)
    assert (inf["full_passes"] == 0) == (lists and landed == "lists" and fp == 0), (key, inf)
    assert bits(np.float32(inf["list_threshold"])) == bits(np.float32(setting["spec0"])), (key, inf)
    if lists and fp == 0:
        assert inf["overflow_segments"] == setting["spill"], (key, inf)
        assert not S.lists_dropped(setting["N"], setting["spill"]), key
    if spill == "dropped":
        assert S.lists_dropped(setting["N"], setting["spill"]) and inf["full_passes"] >= 1, (key, inf)
        assert inf["threshold"] >= inf["list_threshold"], (key, inf)   # they would have served it


@pytest.mark.parametrize("name", list(S.CASES))
def test_compress_decisions_match_oracle(L, name):
    """Every row of the case at N_ODD, in the three modes."""
    rows = [r[:2] for r in PAIRS if r[0] == name]
    assert len(rows) >= 2
    for row in rows:
        for mode in MODES:
            got, oracle, setting = compress_once(L, name, row[1], mode, N_ODD)
            key = (name, row[1], mode, N_ODD)
            assert_matches_oracle(got, oracle, setting, key)
            assert_path_evidence(got["info"], row, setting, key)


@pytest.mark.parametrize("row", BIG_ROWS, ids=["-".join(r) for r in BIG_ROWS])
def test_compress_decisions_three_groups(L, row):
    """Three groups (designed elements on both sides of both group boundaries), and the size
    at which the first list count carries the speculative first-k payload."""
    for mode in ("dev2", "host"):
        got, oracle, setting = compress_once(L, row[0], row[1], mode, N_BIG)
        key = (row, mode, N_BIG)
        assert_matches_oracle(got, oracle, setting, key)
        assert_path_evidence(got["info"], row, setting, key)


@pytest.mark.parametrize("row", UNALIGNED_ROWS, ids=["-".join(r) for r in UNALIGNED_ROWS])
def test_compress_decisions_unaligned(L, row):
    """grad, mmt and vec 4-B aligned only: dgc_compress accepts them, lists nothing (K1's
    scalar form) and runs the <false> forms of the count, lowering and chain kernels."""
    for mode in ("dev2", "host"):
        got, oracle, setting = compress_once(L, row[0], row[1], mode, N_ODD, offset=1)
        key = (row, mode, "unaligned")
        assert_matches_oracle(got, oracle, setting, key)
        assert_path_evidence(got["info"], row, setting, key, lists=False)


@pytest.mark.parametrize("row", QUARTER_ROWS, ids=["-".join(r) for r in QUARTER_ROWS])
def test_compress_decisions_quarter_emit(L, row, monkeypatch):
    """k_emit (the emit of >= 256 groups), forced at these sizes: the first-k cut inside a
    spilled segment goes through its re-read under the limit."""
    monkeypatch.setenv("DGC_EMIT_SHAPE", "quarter")
    for mode, N in (("dev2", N_ODD), ("dev1", N_BIG)):
        got, oracle, setting = compress_once(L, row[0], row[1], mode, N)
        key = (row, mode, N, "quarter")
        assert_matches_oracle(got, oracle, setting, key)
        assert_path_evidence(got["info"], row, setting, key)


# ------------------------------------------------------------------ engine (b): the 16-bit bucket
def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


@pytest.mark.parametrize("dname", ["bfloat16", "float16"])
@pytest.mark.parametrize("row", HALF_ROWS, ids=["-".join(r) for r in HALF_ROWS])
def test_bucket16_decisions_match_torch_cpu(L, row, dname):
    """DGCBucket(dtype=bf16 / fp16): the ladder's products round to the dtype. Against the
    torch-CPU port on tensors of the dtype, bit for bit."""
    from dgc.bucket import DGCBucket
    from test_gpu_bucket16 import payload_of
    name, kind = row
    case, dt, N = S.CASES[name], getattr(torch, dname), N_ODD
    b = DGCBucket(N, compress_ratio=0.001, momentum=0.9, nesterov=False, device=DEV, world_size=1, seed=11, dtype=dt)
    attrs = TC.attributes(N, 0.001)
    assert attrs == (N, b.k, b.num_samples, b.top_k_samples, b.stride)
    start = random.Random(11).randint(0, attrs[4] - 1)
    spec0, spill, cut = S.spec_of(kind, case, N, dname)
    st, attrs_g, start_g, counts = S.generate(name, N, dname, spill, cut, start=start)
    assert attrs_g == attrs
    ths, cnts, branch, want_v, want_i = S.assert_case_is_what_it_says(name, N, dname, spill, cut, start=start)
    g = torch.from_numpy(st.grad.copy()).to(dt)
    assert np.array_equal(bits(g.float().numpy()), bits(st.grad))   # representable: nothing rounded
    b.spec[0] = float(spec0)
    out = torch.full((N,), float("nan"), dtype=dt, device=DEV)
    b.step(g.to(DEV), out)
    torch.cuda.synchronize()
    assert b.start == start
    inf = b.last_info()
    key = (row, dname)
    print(key, inf)
    assert bits(np.float32(inf["threshold0"])) == bits(ths[0]), (key, inf)
    assert bits(np.float32(inf["threshold"])) == bits(ths[-1]), (key, inf)
    assert inf["branch"] == branch and inf["recounts"] == len(cnts) - 1, (key, inf)
    assert inf["candidates"] == cnts[-1] and inf["count"] == want_i.numel(), (key, inf, cnts)
    vals, idx = payload_of(b)
    assert np.array_equal(idx.cpu().numpy(), want_i.numpy()), key
    assert np.array_equal(bits16(vals), bits16(want_v)), key
    ref = g.clone()
    ref[want_i] = 0
    assert np.array_equal(bits16(b.vec), bits16(ref)), key
    assert np.array_equal(bits16(b.mmt), bits16(ref)), key
    assert np.array_equal(bits16(out), bits16(TC.decompress(want_v, want_i, torch.empty(N, dtype=dt), 1))), key
    fp = EXPECT[row][0]
    assert inf["full_passes"] == fp, (key, inf)
    assert bits(np.float32(inf["list_threshold"])) == bits(np.float32(spec0)), (key, inf)


# ------------------------------------------------------------------ engine (c): the batch
# one step of seven tensors, each its own case (and its own j*), one of them direct
BATCH = [("t_j0", 200_003, "trunc_U"), ("t_j1", 250_001, "j1_resample"), ("t_j4", 300_007, "j4_ok"),
         ("t_j5", 220_005, "j5_resample"), ("t_j9", 260_003, "j9_trunc"), ("t_ex", 240_001, "ex_trunc"),
         ("t_direct", 1500, None)]


@pytest.mark.parametrize("order", ["index", "topk"])
@pytest.mark.parametrize("lists", ["reach", "miss"])
def test_batch_decisions_match_oracle(L, lists, order):
    """DGCBatch keeps its list thresholds in its workspace, so step 0 warms them up: a
    zero-bulk staircase per tensor, all of it selected, after which the state is exactly
    zero again and step 1's velocity is its designed gradient. Step 1 runs the cases with t0
    40 x step 0's threshold (the lists, at 0.8 x that threshold, reach every rung: no full
    pass) or 0.5 x (they miss: a full pass)."""
    from dgc.batch import DGCBatch
    from test_gpu_batch import _assert_sent
    b = DGCBatch([(n, (numel,)) for n, numel, _ in BATCH], compress_ratio=0.001, momentum=0.9, nesterov=False,
                 device=DEV, seed=5, resample_order=order)
    t0_warm = np.float32(S.T0 / 40 if lists == "reach" else S.T0 * 2)
    bulk_max = np.float32(0.8 * 0.95) * t0_warm if lists == "reach" else None
    for step in (0, 1):
        starts = b.draw_starts()
        want = {}
        for t, (tname, numel, cname) in enumerate(BATCH):
            attrs = O.attributes(numel, 0.001)
            assert attrs[1:] == tuple(b.attrs[t])
            if cname is None:   # direct: numel == num_samples, no adaptation; step 0 sends all it has
                g = np.zeros(numel, np.float32)
                rng = np.random.default_rng(step)
                at = rng.choice(numel, attrs[1] if step == 0 else 200, replace=False)
                g[at] = rng.uniform(0.5, 1.0, at.size).astype(np.float32) * float(t0_warm)
                case = None
            elif step == 0:
                st = S.generate("warmup", numel, start=starts[t], t0=float(t0_warm))[0]
                S.assert_case_is_what_it_says("warmup", numel, start=starts[t], t0=float(t0_warm))
                g, case = st.grad, S.ZERO_BULK
            else:
                st = S.generate(cname, numel, start=starts[t], bulk_max=bulk_max)[0]
                g, case = st.grad, S.CASES[cname]
                S.assert_case_is_what_it_says(cname, numel, start=starts[t], bulk_max=bulk_max)
            ov, oi, oinfo = O.compress_step(g, np.zeros(numel, np.float32), np.zeros(numel, np.float32), attrs,
                                            starts[t], nesterov=False)
            if case is not None:
                assert oinfo["branch"] == case.branch and len(oinfo["counts"]) - 1 == case.moves, (tname, oinfo)
            else:
                assert oinfo["branch"] == "direct"
            want[tname] = (g, ov, oi, oinfo)
            b.grad(tname).copy_(torch.from_numpy(g))
        b.compress(starts)
        out = b.decompress()
        torch.cuda.synchronize()
        sent, infos = b.transmitted(), b.infos()
        for t, (tname, numel, cname) in enumerate(BATCH):
            g, ov, oi, oinfo = want[tname]
            inf, key = infos[t], (lists, order, step, tname, cname)
            print(key, inf)
            assert inf["branch"] == oinfo["branch"], (key, inf)
            assert bits(np.float32(inf["threshold0"])) == bits(oinfo["thresholds"][0]), (key, inf)
            assert bits(np.float32(inf["threshold"])) == bits(oinfo["threshold"]), (key, inf)
            assert inf["recounts"] == len(oinfo["counts"]) - 1, (key, inf)
            assert inf["candidates"] == oinfo["counts"][-1] and inf["count"] == len(oi), (key, inf)
            assert order == "index" or inf["tie_rule"] != "set", (key, inf)
            gv, gi = sent[tname]
            _assert_sent(gi, gv, oi, ov, inf, key)
            ref = g.copy()
            ref[oi] = 0
            assert np.array_equal(bits(b.velocity_of(tname).cpu().numpy()), bits(ref)), key
            assert np.array_equal(bits(b.momentum_of(tname).cpu().numpy()), bits(ref)), key
            assert np.array_equal(bits(b.out(tname).cpu().numpy()), bits(O.decompress([ov], [oi], numel, 1))), key
            if step == 1 and cname is not None:
                if lists == "reach":
                    assert np.isfinite(inf["list_threshold"]) and inf["full_passes"] == 0, (key, inf)
                    assert t0_warm / 2 < inf["list_threshold"] <= t0_warm, (key, inf)   # step 0's, by the margin
                else:
                    assert inf["full_passes"] >= 1, (key, inf)
        if step == 0:   # everything was selected: the state is all-zero bits again
            assert not bits(b.vec_flat.cpu().numpy()).any() and not bits(b.mmt_flat.cpu().numpy()).any()
    assert out is b.out_flat


# ------------------------------------------------------------------ the census
def test_census_of_paths():
    """Over engine (a)'s rows and modes each of these paths is taken at least once. The rows'
    own tests assert the evidence dgc_select_info gives for them; this one keeps a later edit
    of the tables from quietly dropping a path."""
    runs = [(r[:2], mode, N_ODD) for r in PAIRS for mode in MODES]
    runs += [(r, mode, N_BIG) for r in BIG_ROWS for mode in ("dev2", "host")]
    seen = set()
    for row, mode, N in runs:
        case = S.CASES[row[0]]
        fp, lowering, landed, spill = EXPECT[row]
        if lowering == "lists" and case.moves <= S.LOWER_LISTS:
            seen.add("lowering served by the lists")
        if lowering == "mixed":
            seen.add("lists served some rungs, k_lower_counts decided")
        if lowering == "vec":
            seen.add("lowering entirely over vec")
        if lowering == "lists_js_ms":
            seen.add("js = ms = max_iters")
        seen.add("landed count from lists" if landed == "lists" else "landed count by full pass")
        if spill.startswith("reread"):
            seen.add("spill re-read in a kept list")
        if spill == "reread+cut":
            seen.add("first-k cut inside a spilled segment")
        if spill == "dropped":
            seen.add("lists dropped by spill")
        f = fused(case, row, mode, N)
        if f:
            seen.add(f"fused speculative emit {f}")
    need = {"lowering served by the lists", "lists served some rungs, k_lower_counts decided",
            "lowering entirely over vec", "landed count from lists", "landed count by full pass",
            "js = ms = max_iters", "spill re-read in a kept list", "lists dropped by spill",
            "first-k cut inside a spilled segment", "fused speculative emit accepted",
            "fused speculative emit discarded"}
    assert need <= seen, sorted(need - seen)
    for rows in (BIG_ROWS, UNALIGNED_ROWS, QUARTER_ROWS, HALF_ROWS):
        assert all(r in EXPECT for r in rows)
    assert {r[0] for r in PAIRS} == set(S.CASES)
