"""K6 (csrc/decompress.hip) on tests/k6edges.py's designed rows: every packed row through
dgc_decompress_packed, dgc_fill_zero + dgc_scatter_packed, dgc_decompress_packed_over a designed
previous payload and dgc_clear_packed + dgc_scatter_packed_cleared; the run-table rows through
dgc_decompress (with run offsets and with descent detection); the split rows through
dgc_scatter_split's phases. The output is held to ``oracle.dgc_oracle.decompress`` by bit pattern
(no tolerance; a NaN of the reference must be a NaN), the NaN guards around the output view must
survive, and after every call the status word and the count of super-chunks queued for the
workgroup path — read from the workspace through a mirror of the carve — must be what the row's
route states (tests/test_k6_edges_cpu.py holds every row to that route)."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import k6edges as K
from gpu_split_helpers import DEV, P, Split, check, stream

pytestmark = pytest.mark.gpu
ERR_UNSORTED = 6   # dgc_hip.h: DGC_ERR_UNSORTED


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def workspace(nbytes):
    """Never zero: 0xA5 in every byte, so a read of an area no kernel of the call wrote shows."""
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)


def words(ws):
    """nruns, status, ndesc, ovf_cnt as the carve places them (after Run[64])."""
    return [int(x) for x in ws[K.WS_WORDS: K.WS_WORDS + 16].view(torch.int32).cpu()]


def flags(ws, n, W, cap):
    off = K.carve(n, W, cap)["unsorted"]
    return [int(x) for x in ws[off: off + 4 * W].view(torch.int32).cpu()]


def verify(L, ws, a, want, status, ovf, tag):
    torch.cuda.synchronize()
    assert K.same_bits(a.out.cpu().numpy(), want), tag
    assert a.guards_intact(), tag
    st = ctypes.c_int32(-1)
    check(L, L.dgc_decompress_status(P(ws), ctypes.byref(st), stream()))
    w = words(ws)
    assert w[1] == st.value, tag                      # the mirror reads the word the call reads
    assert st.value == status, (tag, st.value)
    assert w[3] == ovf, (tag, w[3], ovf)


class Packed:
    """A row's gathered buffer, its designed previous one and what the output holds after each."""

    def __init__(self, L, r, cap=None, ascending=None):
        self.r, self.cap = r, r.cap if cap is None else cap
        self.vd, self.idt = int(r.fp16), int(r.int32)
        self.stride, vo, io_ = K.layout(self.cap, self.vd, self.idt)
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        assert L.dgc_payload_layout(self.cap, self.vd, self.idt, ctypes.byref(a), ctypes.byref(b)) == self.stride
        assert (a.value, b.value) == (vo, io_)
        asc = (r.form == "ascending") if ascending is None else ascending
        self.pay = dev(K.pack(K.build(r.name), self.cap, self.vd, self.idt, ascending=asc))
        self.want = K.want(r.name)
        self.ovf = len(r.route[4]) if r.route[0] == "waves" else 0
        self.wsz = L.dgc_decompress_packed_workspace(r.n, r.W, self.cap)
        assert self.wsz == K.carve(r.n, r.W, self.cap)["bytes"]

    def args(self, out, ws, scale=True):
        r = self.r
        return (r.W, self.stride, self.cap, self.vd, self.idt, P(out), r.n) + ((r.scale,) if scale else ()) + \
               (P(ws), ws.numel(), stream())


@pytest.mark.parametrize("name,lead", [(r.name, lead) for r in K.PACKED for lead in r.leads])
def test_packed_row_through_four_forms(L, name, lead):
    r = K.ROW_BY_NAME[name]
    p = Packed(L, r)
    prev_runs = K.prev_of(name)
    prev = dev(K.pack(prev_runs, r.cap, p.vd, p.idt))
    held = dev(K.oracle_of(prev_runs, r.n, r.scale))       # what a persistent output holds before the step
    ws = workspace(p.wsz)
    a = K.arena(r.n, lead, DEV)
    check(L, L.dgc_decompress_packed(P(p.pay), *p.args(a.out, ws)))
    verify(L, ws, a, p.want, r.status, p.ovf, "dense")
    a.buf.fill_(float("nan"))
    check(L, L.dgc_fill_zero(P(a.out), r.n, stream()))
    check(L, L.dgc_scatter_packed(P(p.pay), *p.args(a.out, ws)))
    verify(L, ws, a, p.want, r.status, p.ovf, "fill + scatter")
    a.out.copy_(held)
    check(L, L.dgc_decompress_packed_over(P(p.pay), P(prev), *p.args(a.out, ws)))
    verify(L, ws, a, p.want, r.status, p.ovf, "over")
    a.out.copy_(held)
    check(L, L.dgc_clear_packed(P(prev), *p.args(a.out, ws, scale=False)))
    check(L, L.dgc_scatter_packed_cleared(P(p.pay), *p.args(a.out, ws)))
    verify(L, ws, a, p.want, r.status, p.ovf, "clear + scatter")


def _table_call(L, r_n, runs, scale, offsets, a, ws):
    v = dev(np.concatenate([v for v, _ in runs]).astype(np.float32))
    i = dev(np.concatenate([i for _, i in runs]).astype(np.int64))
    total = int(i.numel())
    if offsets:
        offs = np.cumsum([0] + [len(x) for _, x in runs])
        arr, nruns = (ctypes.c_int64 * len(offs))(*[int(o) for o in offs]), len(runs)
    else:
        arr, nruns = None, 0
    return L.dgc_decompress(P(v), 0, P(i), 0, total, arr, nruns, P(a.out), r_n, scale, P(ws), ws.numel(), stream())


@pytest.mark.parametrize("name", [r.name for r in K.TABLE])
def test_run_table_row(L, name):
    r = K.ROW_BY_NAME[name]
    runs = K.build(name)
    wsz = L.dgc_decompress_workspace(r.n, r.W)
    assert wsz == K.carve(r.n, r.W)["bytes"]
    ws = workspace(wsz)
    for lead in (0, 3):
        a = K.arena(r.n, lead, DEV)
        check(L, _table_call(L, r.n, runs, r.scale, True, a, ws))
        verify(L, ws, a, K.want(name), 0, len(r.route[4]) if r.route[0] == "waves" else 0, lead)
        assert words(ws)[0] == r.W


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


@pytest.mark.parametrize("name", list(K.DETECT))
def test_run_detection_row(L, name):
    n, builder, desc = K.DETECT[name]
    runs = K._norm(builder(), 9)
    want = K.oracle_of(runs, n, 0.5)
    wsz = L.dgc_decompress_workspace(n, 64)
    assert wsz == K.carve(n, 64)["bytes"]
    ws = workspace(wsz)
    a = K.arena(n, 1, DEV)
    rc = _table_call(L, n, runs, 0.5, False, a, ws)
    torch.cuda.synchronize()
    if desc is None:
        assert rc == ERR_UNSORTED and words(ws)[0] == 0 and words(ws)[2] == 64 and a.guards_intact()
        from dgc.compression import DGCCompressor          # the engine's stable-order fallback
        comp = quiet(DGCCompressor, 0.01)
        comp.world_size = 2
        quiet(comp.initialize, [("w", (n, [n]))])
        v = dev(np.concatenate([v for v, _ in runs]))
        i = dev(np.concatenate([i for _, i in runs]))
        out = comp.decompress([v, i], ("w", n, [n], torch.float32, torch.int64, a.out))
        torch.cuda.synchronize()
        assert K.same_bits(out.cpu().numpy(), want) and a.guards_intact()
        return
    check(L, rc)
    route = K.route(n, len(runs), 0, runs, "table")
    verify(L, ws, a, want, 0, len(route[4]) if route[0] == "waves" else 0, name)
    assert words(ws)[0] == desc + 1 and words(ws)[2] == desc


@pytest.mark.parametrize("name", [r.name for r in K.SPLIT])
def test_split_row_phases(L, name):
    r = K.ROW_BY_NAME[name]
    runs = [(np.array(v), np.array(i)) for v, i in K.build(name)]
    sp = Split(L, r.n, r.W, r.parts, r.cap, 0, 0)
    sp.ws.fill_(0xA5)
    g, heads = sp.gather(runs)
    for (v, i), h in zip(runs, heads):                      # the bounds the row was designed around
        h = h.cpu().numpy()
        for p in range(r.parts):
            later = i[(p + 1) * sp.pc:]
            assert h[p, 0] == max(0, min((p + 1) * sp.pc, len(i)) - p * sp.pc)
            assert h[p, 1] == (later.min() if later.size else K.INT64_MAX)
    for q, b in enumerate(r.claims.get("bounds", ())):
        assert tuple(int(x) for x in heads[q].cpu().numpy()[:, 1]) == tuple(b)
    want = K.want(name)
    for lead in (0, 3):
        a = K.arena(r.n, lead, DEV)
        check(L, L.dgc_fill_zero(P(a.out), r.n, stream()))
        sp.scatter(g, a.out, False, want)                   # after every phase each value written is final
        torch.cuda.synchronize()
        assert sp.status() == 0 and words(sp.ws)[1] == 0
        assert K.same_bits(a.out.cpu().numpy(), want) and a.guards_intact()
    # the same step over the previous output: dgc_clear_split, then the phases
    check(L, L.dgc_clear_split(P(g), r.W, r.parts, r.cap, 0, 0, P(a.out), r.n, P(sp.ws), sp.ws.numel(), stream()))
    sp.scatter(g, a.out, True, want)
    torch.cuda.synchronize()
    assert sp.status() == 0 and K.same_bits(a.out.cpu().numpy(), want) and a.guards_intact()


# ------------------------------------------------------------------ sequences: one workspace, one output
def _sequence(L, steps, check_flags=False):
    """steps: (row name, capacity or None, how the output is zeroed: dense / over / clear). One
    workspace (sized for the largest member, never re-initialised) and one output; `over` and
    `clear` re-zero the previous member's entries, re-packed at this member's capacity."""
    rows = [K.ROW_BY_NAME[s[0]] for s in steps]
    n = rows[0].n
    assert all(r.n == n for r in rows)
    ps = [Packed(L, r, cap=s[1]) for r, s in zip(rows, steps)]
    ws = workspace(max(p.wsz for p in ps))
    a = K.arena(n, 3, DEV)
    last = None
    for k, (r, p, (_, _, how)) in enumerate(zip(rows, ps, steps)):
        if how == "dense":
            check(L, L.dgc_decompress_packed(P(p.pay), *p.args(a.out, ws)))
        else:
            assert last.W == r.W and (last.fp16, last.int32) == (r.fp16, r.int32)
            prev = dev(K.pack(K.build(last.name), p.cap, p.vd, p.idt))
            if how == "over":
                check(L, L.dgc_decompress_packed_over(P(p.pay), P(prev), *p.args(a.out, ws)))
            else:
                check(L, L.dgc_clear_packed(P(prev), *p.args(a.out, ws, scale=False)))
                check(L, L.dgc_scatter_packed_cleared(P(p.pay), *p.args(a.out, ws)))
        route = K.route(n, r.W, p.cap, K.build(r.name), r.form)
        verify(L, ws, a, p.want, route.status, len(route[4]), (k, r.name))
        if check_flags:
            assert flags(ws, n, r.W, p.cap) == list(route[5]), (k, r.name)
        last = r


def test_sequence_waves_overflow_waves(L):
    _sequence(L, [("bnd_count_256", None, "dense"), ("occ_one_run_m1", None, "over"), ("bnd_count_255", None, "clear"),
                  ("occ_T_m1", None, "over"), ("bnd_gap_8_9", None, "over")])


def test_sequence_topk_order_then_ascending(L):
    """After a regrouped step the status and every unsorted flag are 0 again."""
    _sequence(L, [("regroup_inside_one_chunk", None, "dense"), ("occ_T_m4", None, "over"),
                  ("regroup_crowded", None, "clear"), ("occ_one_run_m4", None, "clear")], check_flags=True)


def test_sequence_granule_on_off_on(L):
    _sequence(L, [("gran_shared", None, "dense"), ("thr_pc23.98_gran_off", None, "over"), ("gran_edges", None, "over"),
                  ("gran_positions", 1199, "over"), ("gran_edges_lone", 1200, "clear")])


def test_sequence_64_runs_then_2(L):
    """The 2-run step finds 62 stale bounds rows, stale regrouped runs and stale flags."""
    _sequence(L, [("regroup_w64", None, "dense"), ("bnd_gap_8_9", None, "dense"), ("tile_64_runs", None, "dense"),
                  ("regroup_inside_one_chunk", None, "dense"), ("occ_T_m4", None, "over")], check_flags=True)


# ------------------------------------------------------------------ the engine's receive side
ENGINE_ROWS = ["tile_totals", "dup_two_indices", "fp16_i32", "single_asc_granules", "regroup_w64"]


def _exchange(L, r):
    from dgc.exchange import SingleExchange
    p = Packed(L, r)
    vt, it = (torch.float16 if r.fp16 else torch.float32), (torch.int32 if r.int32 else torch.int64)
    ex = SingleExchange(r.cap, r.n, r.W, p.stride, vt, it, DEV)
    assert ex.ws.numel() == p.wsz
    return p, ex


@pytest.mark.parametrize("name", ENGINE_ROWS)
def test_single_exchange_decompress(L, name):
    """SingleExchange.decompress with and without `prev`, on hand-made gathered buffers and no handles."""
    r = K.ROW_BY_NAME[name]
    p, ex = _exchange(L, r)
    prev_runs = K.prev_of(name)
    prev = dev(K.pack(prev_runs, r.cap, p.vd, p.idt))
    a = K.arena(r.n, 1, DEV)
    ex.decompress(prev, [], a.out, r.scale, None)
    pr = K.route(r.n, r.W, r.cap, prev_runs)
    verify(L, ex.ws, a, K.oracle_of(prev_runs, r.n, r.scale), pr.status, len(pr[4]) if r.W > 1 else 0, "prev")
    ex.decompress(p.pay, [], a.out, r.scale, prev)
    verify(L, ex.ws, a, p.want, r.status, p.ovf, "over prev")
    ex.decompress(p.pay, [], a.out, r.scale, None)
    verify(L, ex.ws, a, p.want, r.status, p.ovf, "dense")


@pytest.mark.parametrize("name", ENGINE_ROWS)
def test_single_exchange_clear_then_scatter(L, name):
    from dgc import _lib
    r = K.ROW_BY_NAME[name]
    p, ex = _exchange(L, r)
    prev_runs = K.prev_of(name)
    prev = dev(K.pack(prev_runs, r.cap, p.vd, p.idt))
    a = K.arena(r.n, 3, DEV)
    ex.fill(a.out, _lib.stream_of(DEV))
    ex.scatter(prev, [], a.out, r.scale, False)
    torch.cuda.synchronize()
    assert K.same_bits(a.out.cpu().numpy(), K.oracle_of(prev_runs, r.n, r.scale))
    ex.clear(prev, a.out, _lib.stream_of(DEV))
    ex.scatter(p.pay, [], a.out, r.scale, True)
    verify(L, ex.ws, a, p.want, r.status, p.ovf, "clear + scatter")
