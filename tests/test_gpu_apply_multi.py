"""dgc_apply_packed_multi: DGCSGD's step of T tensors, side by side in one flat index space,
from the gathered packed payload — no dense gradient read.

Single process, C ABI, hand-made rank payloads as tests/test_gpu_apply.py makes them (its
helpers are imported). Per tensor, parameters and momentum buffers must be, bit for bit
(uint32 views), the reference's op sequence (dgc/optim/sgd.py:42-68) on torch CPU tensors over
the oracle's decompress of the flat space sliced to the tensor — which must itself equal
oracle.dgcsgd_step32 — and what dgc_decompress_packed + dgc_sgd_step leave on the same views;
the accumulator must be all-zero bits after every call."""
import ctypes

import numpy as np
import pytest
import torch

import oracle.dgc_oracle as O
from test_gpu_apply import DEV, HYPERS, L, P, _rank_payload, bits, check, stream  # noqa: F401 (L: the fixture)

pytestmark = pytest.mark.gpu
SEG, CAP = 1024, 600

# the tensors' numels; every tensor at a 1024-aligned flat offset (dgc.batch.DGCBatch's layout)
LAYOUTS = {
    # 1 / 1023 / 1024 / 1025 around a segment, 4096 / 4099 around a dense-pass block, 9000: three
    # blocks, the last partial. `unaligned`: a view one element into its storage (4-B aligned);
    # `empty`: the tensor no rank sends an entry of
    "mixed": dict(numels=[1, 1023, 1024, 1025, 4096, 4099, 9000], unaligned=5, empty=2),
    # 70 rows: the lookups go past any 48- or 64-entry table
    "rows70": dict(numels=[1 + (37 * t) % 600 for t in range(70)], unaligned=33, empty=40),
}
# (lr, weight_decay, momentum, dampening, nesterov) per group, steps; the single-group cases are
# tests/test_gpu_apply.py's HYPERS at its LR
LR = 0.1
CASES = {name: ([(LR,) + h[:4]], h[4]) for name, h in HYPERS.items()}
# two groups in one call (tensor t in group t % 2): steps = 2 exercises `first` (1, then 0)
CASES["two_groups"] = ([(0.1, 0.0, 0.0, 0.0, 0), (0.05, 1e-4, 0.9, 0.1, 0)], 2)


def offsets_of(numels):
    offs, end = [], 0
    for n in numels:
        offs.append(end)
        end += -(-n // SEG) * SEG
    return offs, end


def make_runs(rng, numels, offs, flat, empty, W, fp16):
    """W rank runs (values, ascending flat indices) with, by construction: the first and last
    element of the first and of the last tensor (every rank: cross-rank duplicates at W > 1),
    a shared pool (more duplicates), a cancelling pair in ranks 0 and 1, no entry in tensor
    `empty`, one entry in a padding gap (rank 0) and one index >= flat (the last rank).
    Returns the runs and the named indices."""
    valid = np.concatenate([o + np.arange(n) for t, (o, n) in enumerate(zip(offs, numels)) if t != empty])
    T = len(numels)
    edges = np.unique([offs[0], offs[0] + numels[0] - 1, offs[T - 1], offs[T - 1] + numels[T - 1] - 1])
    gap = offs[1] - 1 if numels[0] % SEG else None
    assert gap is not None and gap >= offs[0] + numels[0]
    pool = np.setdiff1d(valid, edges)
    shared = rng.choice(pool, CAP // 3, replace=False)
    cancel = shared[:8] if W > 1 else shared[:0]
    runs = []
    for r in range(W):
        own = rng.choice(pool, CAP // 3, replace=False)
        idx = np.union1d(shared[rng.random(shared.size) < 0.6], own)
        idx = np.setdiff1d(idx, cancel)
        if r < 2:
            idx = np.union1d(idx, cancel)
        idx = np.union1d(idx, edges)
        if r == 0:
            idx = np.union1d(idx, [gap])
        if r == W - 1:
            idx = np.append(idx, flat + 5)   # ascending still: the largest
        idx = idx.astype(np.int64)
        v = rng.standard_normal(idx.size).astype(np.float32)
        if fp16:
            v = v.astype(np.float16).astype(np.float32)
        runs.append((v, idx))
    if W > 1:   # rank 1 sends -v where rank 0 sends v: the sums are +0.0
        (v0, i0), (v1, i1) = runs[0], runs[1]
        v1[np.searchsorted(i1, cancel)] = -v0[np.searchsorted(i0, cancel)]
    assert all(i.size <= CAP for _, i in runs)
    return runs, dict(edges=edges, gap=gap, bad=flat + 5, cancel=cancel)


def assert_case_is_what_it_says(runs, named, numels, offs, flat, empty, W):
    """No case silently degenerates: the generated payload holds what the test names."""
    every = np.concatenate([i for _, i in runs])
    for e in named["edges"]:
        assert e in every, ("boundary entry", e)
    assert {offs[0], offs[0] + numels[0] - 1, offs[-1], offs[-1] + numels[-1] - 1} <= set(named["edges"].tolist())
    assert named["gap"] in runs[0][1] and not any(o <= named["gap"] < o + n for o, n in zip(offs, numels))
    assert named["bad"] in runs[-1][1] and named["bad"] >= flat
    lo, hi = offs[empty], offs[empty] + numels[empty]
    assert not ((every >= lo) & (every < hi)).any(), "the empty tensor has an entry"
    if W > 1:
        seen = np.concatenate([np.unique(i) for _, i in runs])
        assert (np.unique(seen, return_counts=True)[1] >= 2).any(), "no cross-rank duplicate"
        assert named["cancel"].size >= 8
        assert all(c in runs[0][1] and c in runs[1][1] for c in named["cancel"])


def ref_step(p, buf, g, lr, wd, mom, damp, nesterov):
    """The reference's DGCSGD.step on CPU tensors (dgc/optim/sgd.py:50-68); returns the buffer."""
    if wd == 0:
        p.add_(g, alpha=-lr)
        return None
    d = wd * p
    if mom != 0:
        if buf is None:
            buf = d.clone()
        else:
            buf.mul_(mom).add_(d, alpha=1 - damp)
        d = d.add(buf, alpha=mom) if nesterov else buf
    p.add_(d.add(g), alpha=-lr)
    return buf


def device_tensor(n, unaligned):
    """An allocation of its own; `unaligned`: a view one element in (4-B aligned only)."""
    t = torch.zeros(n + 4, device=DEV)
    v = t[1:n + 1] if unaligned else t[:n]
    assert v.data_ptr() % 16 == (4 if unaligned else 0)
    return v


def plant_zeros(p_ref, local_touched):
    """+0.0 / -0.0 at two gathered and two never-gathered positions of a tensor, where it has
    them; returns how many of each kind were planted (touched +0, touched -0, free +0, free -0)."""
    n = p_ref.numel()
    free = np.setdiff1d(np.arange(n), local_touched)
    done = [0, 0, 0, 0]
    for k, (where, z) in enumerate(((local_touched[:1], 0.0), (local_touched[1:2], -0.0), (free[-1:], 0.0),
                                    (free[-2:-1], -0.0))):
        if where.size:
            p_ref[int(where[0])] = z
            done[k] = 1
    return done


def run_case(L, layout, W, fp16, int32, case, seed=0):
    from dgc import _lib
    numels, unaligned, empty = (LAYOUTS[layout][k] for k in ("numels", "unaligned", "empty"))
    groups, steps = CASES[case]
    T, G = len(numels), len(groups)
    offs, flat = offsets_of(numels)
    assert flat < 100_000
    gidx = [t % G for t in range(T)]
    use_buf = [wd != 0 and mom != 0 for _, wd, mom, _, _ in groups]
    rng = np.random.default_rng(1000 * W + 10 * T + seed + (1 if fp16 else 0))
    vd, idt = int(fp16), int(int32)
    stride = L.dgc_payload_layout(CAP, vd, idt, None, None)
    stride_tail = stride + 512   # the batched step's dense tail rides behind the entries
    lay = (W, stride_tail, CAP, vd, idt)
    ws = torch.empty(L.dgc_decompress_packed_workspace(flat, W, CAP), dtype=torch.uint8, device=DEV)
    stash = torch.empty(L.dgc_apply_packed_multi_workspace(W, CAP), dtype=torch.uint8, device=DEV)
    acc, out = torch.zeros(flat, device=DEV), torch.empty(flat, device=DEV)
    p_ref = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in numels]
    buf_ref = [None] * T
    p_new = [device_tensor(n, t == unaligned) for t, n in enumerate(numels)]
    p_old = [device_tensor(n, t == unaligned) for t, n in enumerate(numels)]
    buf_new = [device_tensor(n, t == unaligned) if use_buf[gidx[t]] else None for t, n in enumerate(numels)]
    buf_old = [device_tensor(n, t == unaligned) if use_buf[gidx[t]] else None for t, n in enumerate(numels)]
    table = _lib.ApplyTable(DEV)
    hs = (_lib.ApplyHyper * G)(*[_lib.ApplyHyper(lr, mom, damp, wd, nesterov) for lr, wd, mom, damp, nesterov in groups])
    planted = np.zeros(4, int)
    for step in range(steps):
        runs, named = make_runs(rng, numels, offs, flat, empty, W, fp16)
        assert_case_is_what_it_says(runs, named, numels, offs, flat, empty, W)
        every = np.concatenate([i for _, i in runs])
        for t, (o, n) in enumerate(zip(offs, numels)):
            local = np.unique(every[(every >= o) & (every < o + n)]) - o
            planted += plant_zeros(p_ref[t], local)
            p_new[t].copy_(p_ref[t])
            p_old[t].copy_(p_ref[t])
        # the expectation: the oracle's decompress of the entries inside the flat space, sliced
        good = [(v[i < flat], i[i < flat]) for v, i in runs]
        g_flat = O.decompress([v for v, _ in good], [i for _, i in good], flat, W)
        assert (bits(g_flat)[named["cancel"]] == 0).all(), "the cancelling pairs do not sum to +0.0"
        assert bits(g_flat)[named["gap"]] != 0
        for t, (o, n) in enumerate(zip(offs, numels)):
            lr, wd, mom, damp, nesterov = groups[gidx[t]]
            g = torch.from_numpy(g_flat[o:o + n].copy())
            p_in, buf_in = p_ref[t].numpy().copy(), None if buf_ref[t] is None else buf_ref[t].numpy().copy()
            buf_ref[t] = ref_step(p_ref[t], buf_ref[t], g, lr, wd, mom, damp, nesterov)
            p_o, buf_o = O.dgcsgd_step32(p_in, g.numpy(), buf_in, lr, mom, damp, wd, nesterov)
            assert np.array_equal(bits(p_o), bits(p_ref[t])), (case, step, t, "oracle / torch-CPU sequence")
            if use_buf[gidx[t]]:
                assert np.array_equal(bits(buf_o), bits(buf_ref[t])), (case, step, t, "oracle / torch-CPU buffer")
            if t == empty:   # no entry: exactly the dense pass's g = +0.0 result (the old bits, without weight decay)
                assert not bits(g).any()
                if wd == 0:
                    assert np.array_equal(bits(p_ref[t]), bits(p_in))
        # garbage past the counts: NaN values and indices >= flat + 7 (a count says where the entries end)
        gathered = torch.cat([torch.cat([_rank_payload(L, v, i, CAP, vd, idt, flat + 7),
                                         torch.full((stride_tail - stride,), 0xA5, dtype=torch.uint8, device=DEV)])
                              for v, i in runs])
        first = step == 0
        table.update([(p_new[t].data_ptr(), buf_new[t].data_ptr() if buf_new[t] is not None else 0, offs[t], numels[t],
                       int(first and use_buf[gidx[t]]), gidx[t], groups[gidx[t]][1] != 0) for t in range(T)])
        assert table.uploads == (step + 1 if any(use_buf) else 1)   # uploaded again only when `first` turned 0
        check(L, L.dgc_scatter_packed(P(gathered), *lay, P(acc), flat, 1.0 / W, P(ws), ws.numel(), stream()))
        st = ctypes.c_int32(-1)
        check(L, L.dgc_decompress_status(P(ws), ctypes.byref(st), stream()))
        assert st.value & 1, st.value   # the scatter reported the index >= flat
        check(L, L.dgc_apply_packed_multi(P(gathered), *lay, P(acc), flat, P(table.dev), T, table.dense_blocks, hs, G,
                                          P(stash), stash.numel(), stream()))
        torch.cuda.synchronize()
        assert int(acc.view(torch.int32).count_nonzero()) == 0, "acc is not all-zero bits after the apply"
        # the existing path on the same views: the dense decompress, then K7 per group
        check(L, L.dgc_decompress_packed(P(gathered), *lay, P(out), flat, 1.0 / W, P(ws), ws.numel(), stream()))
        for gi, (lr, wd, mom, damp, nesterov) in enumerate(groups):
            ts = [t for t in range(T) if gidx[t] == gi]
            arr = ctypes.c_void_p * len(ts)
            check(L, L.dgc_sgd_step(arr(*[p_old[t].data_ptr() for t in ts]),
                                    arr(*[out.data_ptr() + 4 * offs[t] for t in ts]),
                                    arr(*[buf_old[t].data_ptr() if buf_old[t] is not None else 0 for t in ts]),
                                    (ctypes.c_int64 * len(ts))(*[numels[t] for t in ts]),
                                    (ctypes.c_int32 * len(ts))(*[int(first)] * len(ts)), len(ts), lr, mom, damp, wd,
                                    nesterov, stream()))
        torch.cuda.synchronize()
        for t in range(T):
            assert np.array_equal(bits(p_old[t]), bits(p_ref[t])), (case, step, t, "existing path / reference")
            assert np.array_equal(bits(p_new[t]), bits(p_ref[t])), (case, step, t, numels[t], "param")
            if use_buf[gidx[t]]:
                assert np.array_equal(bits(buf_old[t]), bits(buf_ref[t])), (case, step, t, "existing path buffer")
                assert np.array_equal(bits(buf_new[t]), bits(buf_ref[t])), (case, step, t, "momentum buffer")
    assert planted.all(), planted   # +0.0 and -0.0 parameters, gathered and not


WIRES = [
    # W, fp16 values, int32 indices
    (1, False, False),
    (2, False, False),
    (4, True, True),
    (8, False, False),
    (8, True, True),
]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("W,fp16,int32", WIRES)
def test_apply_multi_matches_reference(L, W, fp16, int32, case):
    run_case(L, "mixed", W, fp16, int32, case)


@pytest.mark.parametrize("W,fp16,int32,case", [(2, False, False, "wd0"), (2, False, False, "wd_nesterov"),
                                               (1, False, False, "two_groups"), (8, True, True, "two_groups")])
def test_apply_multi_seventy_rows(L, W, fp16, int32, case):
    """A 70-row table of small tensors: the row lookup (entries) and the block lookup (dense
    pass) beyond any 48- or 64-entry boundary."""
    run_case(L, "rows70", W, fp16, int32, case, seed=3)
