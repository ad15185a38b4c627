"""Every arm of the host's dtype / index / flag dispatch (csrc/dispatch.hpp) launches the kernel it
names. Identical kernels do not prove the host picks the right one — a dispatcher that sent
DGC_I32 to the int64 arm would read garbage indices, one that swapped bf16 and fp16 would round
differently — so each entry point below is called once per member of its dispatch domain, at the
smallest shape that tells the members apart, and compared bit for bit with the torch-CPU op
sequence the neighbouring tests use (oracle/torch_cpu.py; index_put_(accumulate=True) + mul_ on a
tensor of the dtype for the 16-bit scatters).

Shape: n = 5001 (two 4096-element chunks, not a multiple of 4), W = 2 ranks of capacity 8, two
indices shared by both ranks, one -0.0 value, one value that rounds differently in bf16 and fp16
(1 + 2^-10), momentum 0.9 (Nesterov and plain differ), a clip coefficient 0.5 and a clamp bound
0.25 that bite (the three clip kinds differ). Every index is in range.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import test_gpu_split16 as split16   # run_case: K6-16's own check against both of its references
from oracle import torch_cpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, F16, BF16 = 0, 1, 2
I64, I32 = 0, 1
NONE, SCALE, CLAMP = 0, 1, 2
TORCH = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
ITORCH = {I64: torch.int64, I32: torch.int32}
N, W, CAP, MOM = 5001, 2, 8, 0.9
COEF, BOUND = 0.5, 0.25
IDX = [[3, 7, 100, 2500, 4095, 4096, 4999, 5000], [0, 7, 101, 2501, 4097, 4100, 4998, 5000]]
VAL = [[-0.0, 1.0009765625, 3.14159, -2.71828, 0.3333, 1e-3, -7.0, 0.1],
       [0.2, 1.0009765625, -1.5, 0.7071, 5.5, -0.0, 1.0009765625, 0.3]]
HALVES = [BF16, F16]
KINDS = [NONE, SCALE, CLAMP]


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    return _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(L, rc):
    assert rc == 0, L.dgc_last_error().decode()


def same(got, want):
    """Bit for bit (so -0.0 != +0.0 and every NaN pattern counts)."""
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape
    v = torch.int32 if got.dtype == torch.float32 else torch.int16
    bad = (got.view(v) != want.view(v)).nonzero().view(-1)
    assert bad.numel() == 0, "first differing element %d: %r != %r" % (bad[0], got[bad[0]].item(), want[bad[0]].item())


@pytest.fixture(scope="module")
def field():
    """Dense inputs shared by the cases (never modified): a gradient, a momentum and a velocity."""
    g = torch.Generator().manual_seed(5001)
    x = [torch.randn(N, generator=g) for _ in range(3)]
    x[0][:4] = torch.tensor([-0.0, 1.0009765625, 0.6, -0.6])
    return x


def gathered(vd, idt):
    """The W runs: wire values and indices as CPU tensors, rank-order concatenated."""
    vals = torch.tensor(VAL, dtype=torch.float32).to(TORCH[vd])
    idx = torch.tensor(IDX, dtype=ITORCH[idt])
    return vals.view(-1), idx.view(-1)


def scatter_oracle(vals, idx, dt, scale):
    """grad.zero_().index_put_([idx], values.type(dtype), accumulate=True); grad.mul_(scale), on the CPU."""
    out = torch.zeros(N, dtype=dt)
    out.index_put_([idx.long()], vals.to(dt), accumulate=True)
    return out.mul_(scale)


def packed(L, vals, idx, vd, idt):
    """The W packed payloads [count | order | values | indices] side by side; returns (device bytes, stride)."""
    voff, ioff = ctypes.c_int64(), ctypes.c_int64()
    stride = L.dgc_payload_layout(CAP, vd, idt, ctypes.byref(voff), ctypes.byref(ioff))
    buf = torch.zeros(W, stride, dtype=torch.uint8)
    for r in range(W):
        buf[r, :8] = torch.tensor([CAP], dtype=torch.int64).view(torch.uint8)
        v = vals[r * CAP:(r + 1) * CAP].contiguous().view(torch.uint8)
        i = idx[r * CAP:(r + 1) * CAP].contiguous().view(torch.uint8)
        buf[r, voff.value:voff.value + v.numel()] = v
        buf[r, ioff.value:ioff.value + i.numel()] = i
    return buf.to(DEV), stride


# ---------------------------------------------------------------- the 16-bit receive side (half.hip)
@pytest.mark.parametrize("form", ["runs", "sorted"])
@pytest.mark.parametrize("dt, vd, idt", list(itertools.product(HALVES, [F32, F16, BF16], [I64, I32])))
def test_decompress16(L, form, dt, vd, idt):
    """k_scatter16 / k_segsum16 <DT, VD, I> and k_scale16<DT>."""
    vals, idx = gathered(vd, idt)
    want = scatter_oracle(vals, idx, TORCH[dt], 0.5)
    if form == "sorted":   # one stably index-sorted run: duplicates keep their rank order
        order = torch.sort(idx.long(), stable=True)[1]
        vals, idx, offs, nruns = vals[order].contiguous(), idx[order].contiguous(), [0, W * CAP], -1
    else:
        offs, nruns = [0, CAP, 2 * CAP], W
    out = torch.full((N,), 3.0, dtype=TORCH[dt], device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    dv, di = vals.to(DEV), idx.to(DEV)
    ok(L, L.dgc_decompress16(P(dv), vd, P(di), idt, (ctypes.c_int64 * len(offs))(*offs), nruns, P(out), dt, N, 0.5, P(bad),
                             stream()))
    same(out, want)
    assert bad.item() == 0


@pytest.mark.parametrize("dt, vd, idt", list(itertools.product(HALVES, [F32, F16, BF16], [I64, I32])))
def test_decompress_packed16(L, dt, vd, idt):
    """k_scatter_packed16<DT, VD, I>."""
    vals, idx = gathered(vd, idt)
    buf, stride = packed(L, vals, idx, vd, idt)
    out = torch.full((N,), 3.0, dtype=TORCH[dt], device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok(L, L.dgc_decompress_packed16(P(buf), W, stride, CAP, vd, idt, P(out), dt, N, 0.5, P(bad), stream()))
    same(out, scatter_oracle(vals, idx, TORCH[dt], 0.5))
    assert bad.item() == 0


@pytest.mark.parametrize("entry", ["dgc_mask_indices16", "dgc_mask_indices", "dgc_mask_packed16"])
@pytest.mark.parametrize("idt", [I64, I32])
def test_mask(L, field, entry, idt):
    """k_mask16<I>, k_mask<I>, k_mask_packed16<I>: DGCSGDMemory.update's index_fill_."""
    dt = torch.float32 if entry == "dgc_mask_indices" else torch.bfloat16
    idx = torch.tensor(IDX[0], dtype=ITORCH[idt])
    m, v = field[1].to(dt, copy=True), field[2].to(dt, copy=True)
    dm, dv = m.to(DEV), v.to(DEV)
    if entry == "dgc_mask_packed16":
        buf, _ = packed(L, gathered(BF16, idt)[0], torch.tensor(IDX, dtype=ITORCH[idt]).view(-1), BF16, idt)
        ok(L, L.dgc_mask_packed16(P(buf), CAP, BF16, idt, P(dm), P(dv), N, stream()))
    else:
        bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        di = idx.to(DEV)
        ok(L, getattr(L, entry)(P(dm), P(dv), N, P(di), idt, CAP, P(bad), stream()))
        assert bad.item() == 0
    torch_cpu.update(m, v, idx.long())
    same(dm, m)
    same(dv, v)


@pytest.mark.parametrize("dt", HALVES)
def test_widen16(L, field, dt):
    x = field[0].to(TORCH[dt])
    y = torch.empty(N, dtype=torch.float32, device=DEV)
    dx = x.to(DEV)
    ok(L, L.dgc_widen16(P(dx), P(y), N, dt, stream()))
    same(y, x.float())


def clipped(g, kind, coef=COEF):
    """dgc/clip_grad.py's in-place clip of a gradient by a coefficient / a bound of its dtype."""
    g = g.clone()
    if kind == SCALE and coef < 1:
        g.mul_(coef)
    if kind == CLAMP:
        g.clamp_(min=-BOUND, max=BOUND)
    return g


def clip_abi(kind, coefs=(COEF,)):
    """(clip table on the device or None, clip value): SCALE reads the table, CLAMP the fixed bound."""
    return (torch.tensor(coefs, dtype=torch.float32, device=DEV) if kind == SCALE else None), BOUND


@pytest.mark.parametrize("dt, nest, acc, kind", list(itertools.product(HALVES, [0, 1], [0, 1], KINDS)))
def test_compensate16_clip(L, field, dt, nest, acc, kind):
    """k_compensate16<DT, NEST, ACC, CLIP>."""
    g, m, v = (x.to(TORCH[dt]) for x in field)
    dg, dm, dv = g.to(DEV), m.to(DEV), v.to(DEV)
    out = torch.zeros(N, dtype=TORCH[dt], device=DEV)
    img = torch.zeros(N, dtype=torch.float32, device=DEV)
    tab, value = clip_abi(kind)
    ok(L, L.dgc_compensate16_clip(P(dg), P(dm), P(dv), P(out), P(img), N, MOM, nest, acc, dt, kind, P(tab), value, stream()))
    res = torch_cpu.compensate(clipped(g, kind), m, v, MOM, bool(nest), bool(acc))
    same(dm, m)
    same(dv, v)
    if acc:
        same(img, v.float())
    else:
        same(out, res)


MT_N, MT_OFF, MT_FLAT, MT_COEFS = [3000, 2001], [0, 3072], 5120, (COEF, 2.0)   # the second tensor's coefficient >= 1


@pytest.mark.parametrize("dt, nest, kind", list(itertools.product(HALVES, [0, 1], KINDS)))
def test_compensate16_multi_clip(L, field, dt, nest, kind):
    """k_compensate16_mt<DT, NEST, CLIP>: two tensors of the flat buffers, one coefficient each; the padding stays +0."""
    flat = [torch.zeros(MT_FLAT, dtype=TORCH[dt]) for _ in range(3)]
    for t, (n, off) in enumerate(zip(MT_N, MT_OFF)):
        for f, x in zip(flat, field):
            f[off:off + n] = x[t * 3000:t * 3000 + n].to(TORCH[dt])
    g, m, v = flat
    dg, dm, dv = g.to(DEV), m.to(DEV), v.to(DEV)
    img = torch.zeros(MT_FLAT, dtype=torch.float32, device=DEV)
    tab, value = clip_abi(kind, MT_COEFS)
    ok(L, L.dgc_compensate16_multi_clip(P(dg), P(dm), P(dv), P(img), (ctypes.c_int64 * 2)(*MT_N), (ctypes.c_int64 * 2)(*MT_OFF),
                                        2, MT_FLAT, MOM, nest, dt, kind, P(tab), value, stream()))
    for t, (n, off) in enumerate(zip(MT_N, MT_OFF)):
        s = slice(off, off + n)
        torch_cpu.compensate(clipped(g[s], kind, MT_COEFS[t]), m[s], v[s], MOM, bool(nest), True)
    same(dm, m)
    same(dv, v)
    same(img, v.float())


# ---------------------------------------------------------------- fp32 K1 and the dense tensors (compensate.hip)
@pytest.mark.parametrize("nest, acc, kind", list(itertools.product([0, 1], [0, 1], KINDS)))
def test_compensate_clip(L, field, nest, acc, kind):
    """k_compensate4 / k_compensate1 <NEST, ACC, no sample, CLIP> (n = 5001: 1250 float4 and one scalar)."""
    g, m, v = (x.clone() for x in field)
    dg, dm, dv = g.to(DEV), m.to(DEV), v.to(DEV)
    out = torch.zeros(N, device=DEV)
    tab, value = clip_abi(kind)
    ok(L, L.dgc_compensate_clip(P(dg), P(dm), P(dv), None if acc else P(out), N, MOM, nest, acc, None, 0, 1, 0, kind, P(tab),
                                value, stream()))
    res = torch_cpu.compensate(clipped(g, kind), m, v, MOM, bool(nest), bool(acc))
    same(dm, m)
    same(dv, v)
    if not acc:
        same(out, res)


@pytest.mark.parametrize("nest, round_to, kind", list(itertools.product([0, 1], [F32, F16], KINDS)))
def test_compensate_multi_clip(L, field, nest, round_to, kind):
    """k_compensate_mt<NEST, ROUND16, CLIP>: the dense branch of two tensors from their own gradients."""
    srcs = [field[0][:MT_N[0]].clone().to(DEV), field[0][3000:3000 + MT_N[1]].clone().to(DEV)]
    m = torch.zeros(MT_FLAT)
    for t, (n, off) in enumerate(zip(MT_N, MT_OFF)):
        m[off:off + n] = field[1][t * 3000:t * 3000 + n]
    dm, out = m.to(DEV), torch.zeros(MT_FLAT, device=DEV)
    tab, value = clip_abi(kind, MT_COEFS)
    ok(L, L.dgc_compensate_multi_clip((ctypes.c_void_p * 2)(*[s.data_ptr() for s in srcs]), (ctypes.c_int64 * 2)(*MT_N),
                                      (ctypes.c_int64 * 2)(*MT_OFF), 2, round_to, P(dm), P(out), MOM, nest, kind, P(tab),
                                      value, stream()))
    want = torch.zeros(MT_FLAT)
    for t, (n, off) in enumerate(zip(MT_N, MT_OFF)):
        g = srcs[t].cpu()
        if round_to == F16:
            g = g.half().float()
        want[off:off + n] = torch_cpu.compensate(clipped(g, kind, MT_COEFS[t]), m[off:off + n], None, MOM, bool(nest), False)
    same(dm, m)
    same(out, want)


@pytest.mark.parametrize("nest", [0, 1])
@pytest.mark.parametrize("src, round_to", [(F32, F32), (F16, F32), (F32, F16)])
def test_compensate_wire(L, field, nest, src, round_to):
    """k_compensate_wire<NEST, mode>: fp32, fp16 widened, fp32 rounded through fp16."""
    x, m = field[0].to(TORCH[src]), field[1].clone()
    dx, dm, out = x.to(DEV), m.to(DEV), torch.zeros(N, device=DEV)
    ok(L, L.dgc_compensate_wire(P(dx), src, round_to, P(dm), P(out), N, MOM, nest, stream()))
    g = x.float() if round_to == F32 else x.half().float()
    want = torch_cpu.compensate(g, m, None, MOM, bool(nest), False)
    same(dm, m)
    same(out, want)


def rank_rows(field, dt):
    return torch.stack([field[0], field[2]]).to(TORCH[dt]).contiguous()


def rank_average(rows):
    acc = rows[0].clone()
    acc.add_(rows[1])
    return acc.div_(W)


@pytest.mark.parametrize("dt", [F32, F16, BF16])
def test_rank_sum(L, field, dt):
    """k_rank_sum<DT>: the rank-order sum and the Average's div_ in the wire dtype."""
    rows = rank_rows(field, dt)
    d, dst = rows.to(DEV), torch.zeros(N, dtype=TORCH[dt], device=DEV)
    ok(L, L.dgc_rank_sum(P(d), dt, W, N * rows.element_size(), N, 1, P(dst), stream()))
    same(dst, rank_average(rows))


@pytest.mark.parametrize("nest, dt", list(itertools.product([0, 1], [F32, F16])))
def test_compensate_ranks(L, field, nest, dt):
    """k_compensate_ranks<NEST, DT>."""
    rows, m = rank_rows(field, dt), field[1].clone()
    d, dm, out = rows.to(DEV), m.to(DEV), torch.zeros(N, device=DEV)
    ok(L, L.dgc_compensate_ranks(P(d), dt, W, N * rows.element_size(), P(dm), P(out), N, MOM, nest, stream()))
    want = torch_cpu.compensate(rank_average(rows).float(), m, None, MOM, bool(nest), False)
    same(dm, m)
    same(out, want)


# ---------------------------------------------------------------- the clip on its own (clip.hip)
@pytest.mark.parametrize("kind", [SCALE, CLAMP])
def test_clip_apply(L, field, kind):
    """k_clip_apply<SCALE | CLAMP> on two tensors, one coefficient each."""
    xs = [field[0][:MT_N[0]].clone(), field[0][3000:3000 + MT_N[1]].clone()]
    ds = [x.to(DEV) for x in xs]
    tab, value = clip_abi(kind, MT_COEFS)
    ok(L, L.dgc_clip_apply((ctypes.c_void_p * 2)(*[d.data_ptr() for d in ds]), (ctypes.c_int64 * 2)(*MT_N), 2, kind, P(tab),
                           value, stream()))
    for t in range(2):
        same(ds[t], clipped(xs[t], kind, MT_COEFS[t]))


# ---------------------------------------------------------------- the fp32 receive side (decompress.hip)
@pytest.mark.parametrize("vd, idt", list(itertools.product([F32, F16], [I64, I32])))
def test_decompress_packed(L, vd, idt):
    """run_scatter<VD, ID>: K6's several-runs scatter (bounds, waves, overflow) by wire dtypes."""
    vals, idx = gathered(vd, idt)
    buf, stride = packed(L, vals, idx, vd, idt)
    out = torch.full((N,), 3.0, device=DEV)
    wsz = L.dgc_decompress_packed_workspace(N, W, CAP)
    ws = torch.zeros(wsz, dtype=torch.uint8, device=DEV)
    ok(L, L.dgc_decompress_packed(P(buf), W, stride, CAP, vd, idt, P(out), N, 0.5, P(ws), wsz, stream()))
    same(out, scatter_oracle(vals, idx, torch.float32, 0.5))
    status = ctypes.c_int32(-1)
    ok(L, L.dgc_decompress_status(P(ws), ctypes.byref(status), stream()))
    assert status.value == 0


@pytest.mark.parametrize("dt, vd, idt", list(itertools.product(HALVES, [F32, F16, BF16], [I64, I32])))
def test_scatter_split16(L, dt, vd, idt):
    """run_scatter<VD, ID, OD> (K6-16) behind dgc_payload_split's k_payload_split<2 | 4, 4 | 8>: two phases of
    capacity 4, checked by tests/test_gpu_split16.py's run_case against dgc_decompress_packed16 and torch."""
    runs = [(np.array(v, np.float32), np.array(i, np.int64)) for v, i in zip(VAL, IDX)]
    split16.run_case(L, runs, N, W, 2, CAP, vd, idt, dt)


@pytest.mark.parametrize("vd, idt", list(itertools.product([F32, F16], [I64, I32])))
def test_decompress_finds_its_runs(L, vd, idt):
    """dgc_decompress without run offsets: k_find_descents<ID> finds the one descent between the two ranks' runs."""
    vals, idx = gathered(vd, idt)
    out = torch.full((N,), 3.0, device=DEV)
    wsz = L.dgc_decompress_workspace(N, 0)
    ws = torch.zeros(wsz, dtype=torch.uint8, device=DEV)
    dv, di = vals.to(DEV), idx.to(DEV)
    ok(L, L.dgc_decompress(P(dv), vd, P(di), idt, W * CAP, None, 0, P(out), N, 0.5, P(ws), wsz, stream()))
    same(out, scatter_oracle(vals, idx, torch.float32, 0.5))


PREV_IDX = [[2, 6, 99, 2499, 4094, 4098, 4990, 4997], [1, 6, 102, 2502, 4099, 4101, 4996, 4997]]


@pytest.mark.parametrize("entry", ["dgc_decompress_packed_over", "dgc_clear_packed"])
@pytest.mark.parametrize("idt", [I64, I32])
def test_sparse_rezero(L, entry, idt):
    """k_clear_packed<ID>: the output holds a previous payload's result; its entries are re-zeroed, not the bucket."""
    vals, idx = gathered(F32, idt)
    prev_idx = torch.tensor(PREV_IDX, dtype=ITORCH[idt]).view(-1)
    assert not set(prev_idx.tolist()) & set(idx.tolist())   # every previous entry must go back to +0.0
    buf, stride = packed(L, vals, idx, F32, idt)
    prev, _ = packed(L, vals.flip(0).contiguous(), prev_idx, F32, idt)
    out = torch.full((N,), 3.0, device=DEV)
    wsz = L.dgc_decompress_packed_workspace(N, W, CAP)
    ws = torch.zeros(wsz, dtype=torch.uint8, device=DEV)
    ok(L, L.dgc_decompress_packed(P(prev), W, stride, CAP, F32, idt, P(out), N, 0.5, P(ws), wsz, stream()))
    same(out, scatter_oracle(vals.flip(0), prev_idx, torch.float32, 0.5))
    if entry == "dgc_decompress_packed_over":
        ok(L, L.dgc_decompress_packed_over(P(buf), P(prev), W, stride, CAP, F32, idt, P(out), N, 0.5, P(ws), wsz, stream()))
    else:
        ok(L, L.dgc_clear_packed(P(prev), W, stride, CAP, F32, idt, P(out), N, P(ws), wsz, stream()))
        same(out, torch.zeros(N))
        ok(L, L.dgc_scatter_packed_cleared(P(buf), W, stride, CAP, F32, idt, P(out), N, 0.5, P(ws), wsz, stream()))
    same(out, scatter_oracle(vals, idx, torch.float32, 0.5))
