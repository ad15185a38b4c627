"""DGCBucket(grad_dtype=bf16 | fp16) on fp32 state: K1 with the 16-bit gradient widened in its
load (dgc_compress_begin_g16). The reference computes such a step through torch's type
promotion (dgc/memory.py:50-63: every op in fp32 on the exactly widened gradient), so the
expectation is the fp32 bucket on ``g.float()``: twin buckets with the same seed, A mixed and
fed ``g``, B fp32 and fed ``g.float()``, compared as integers after every step. One case is
also held against the numpy oracle on the widened gradient, so the twin is not the only
witness."""
import functools
import socket

import numpy as np
import pytest
import torch

import oracle.dgc_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATIO = 0.01
STEPS = 4
# sub-group tensors, the 4-element group and the n & 3 tail (with samples in it), the
# 1024-element segment, the 4096-element workgroup and the 1024-segment group (2^20)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4093, 4096, 4097, 4099, 5 * 4096 + 1021, 70001, 1048576 + 3]
DTYPES = {"bf16": (torch.bfloat16, 1.0), "fp16": (torch.float16, 0.01)}
WRITE_THROUGH_MAX = 48 << 20   # kWriteThroughMax (csrc/dgc_common.hpp): the other launch shape starts past it


def ibits(t):
    """A tensor's bits on the host, as integers."""
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()]).cpu().numpy()


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dgc import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def gradient16(seed, N, dname):
    """A 16-bit gradient on the host; shared, never written."""
    dt, scale = DTYPES[dname]
    return torch.from_numpy(synth.gradient(seed, N, "normal", scale)).to(dt)


def twins(N, dt, **kw):
    """(A, B): the mixed bucket and the fp32 bucket it must equal, same seed."""
    from dgc.bucket import DGCBucket
    kw = dict(dict(compress_ratio=RATIO, momentum=0.9, device=DEV, world_size=1, seed=11), **kw)
    return DGCBucket(N, grad_dtype=dt, **kw), DGCBucket(N, **kw)


def info_of(b):
    return {k: repr(v) for k, v in b.last_info().items()}   # (repr: a NaN threshold equals itself)


def entries(b):
    """The payload as (header, values, indices) of its count, as integers."""
    p = b.payload
    n = int(p[:8].view(torch.int64).item())
    vb = torch.empty(0, dtype=b.vdtype).element_size()
    ib = torch.empty(0, dtype=b.idtype).element_size()
    return ibits(p[:16]), ibits(p[b.voff: b.voff + n * vb].view(b.vdtype)), ibits(p[b.ioff: b.ioff + n * ib].view(b.idtype))


def assert_same_step(a, b, out_a, out_b, key):
    """Payload header and entries, the state before and after the flush, the info record and
    the output of the twins' last step."""
    assert a.start == b.start, key
    for x, y, what in zip(entries(a), entries(b), ("header", "values", "indices")):
        assert np.array_equal(x, y), (key, what)
    assert a._mmt.dtype == a._vec.dtype == torch.float32 and a._mmt.numel() == b._mmt.numel(), key
    assert np.array_equal(ibits(a._mmt), ibits(b._mmt)), (key, "_mmt")
    assert np.array_equal(ibits(a._vec), ibits(b._vec)), (key, "_vec")
    assert a._pending == b._pending, key
    assert info_of(a) == info_of(b), key
    if out_a is not None:
        assert np.array_equal(ibits(out_a), ibits(out_b)), (key, "out")
    assert np.array_equal(ibits(a.mmt), ibits(b.mmt)), (key, "mmt")   # flushed
    assert np.array_equal(ibits(a.vec), ibits(b.vec)), (key, "vec")


# ---------------------------------------------------------------- 1. edge sizes
@pytest.mark.parametrize("nesterov", [True, False], ids=["nest", "plain"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("N", SIZES)
def test_mixed_edges_against_the_fp32_twin(L, N, dname, nesterov):
    """Four steps per case. The gradient is the first N elements of a longer 16-bit tensor whose
    rest is NaN, and the outputs are NaN-filled before each step: an element past N that is
    used, or an output element that is not written, shows up. (70001, bf16) is also the numpy
    oracle's step on the widened gradient."""
    dt, _ = DTYPES[dname]
    a, b = twins(N, dt, nesterov=nesterov)
    assert a.grad_dtype == dt and b.grad_dtype is None and a.dtype == torch.float32
    full = torch.full((N + 1024 + 8,), float("nan"), dtype=dt, device=DEV)
    out_a, out_b = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    direct = (N, dname) == (70001, "bf16")
    if direct:
        attrs = O.attributes(N, RATIO)
        assert attrs == (N, a.k, a.num_samples, a.top_k_samples, a.stride)
        m_o, v_o = np.zeros(N, np.float32), np.zeros(N, np.float32)
    for s in range(STEPS):
        g = gradient16(500 + s, N, dname)
        full[:N].copy_(g)
        out_a.fill_(float("nan"))
        out_b.fill_(float("nan"))
        a.step(full[:N], out_a)
        b.step(full[:N].float(), out_b)
        key = (N, dname, nesterov, s)
        if direct:   # before assert_same_step flushes: the oracle's state has the masking applied
            ov, oi, _ = O.compress_step(g.float().numpy(), m_o, v_o, attrs, a.start, nesterov=nesterov)
            _, vals, idx = entries(a)
            assert np.array_equal(idx, oi), key
            assert np.array_equal(vals, ov.view(np.int32)), key
        assert_same_step(a, b, out_a, out_b, key)
        if direct:
            assert np.array_equal(ibits(a.mmt), m_o.view(np.int32)), key
            assert np.array_equal(ibits(a.vec), v_o.view(np.int32)), key
            assert np.array_equal(ibits(out_a), O.decompress([ov], [oi], N, 1).view(np.int32)), key


# ---------------------------------------------------------------- 2. special values
def specials(dt):
    """+-0, the dtype's smallest and largest subnormals, its largest finite value, +-inf, NaN."""
    fi = torch.finfo(dt)
    tiny, sub_max = fi.smallest_normal * fi.eps, fi.smallest_normal * (1 - fi.eps)
    v = torch.tensor([0.0, -0.0, tiny, -tiny, sub_max, -sub_max, fi.max, -fi.max, float("inf"), -float("inf"),
                      float("nan")], dtype=torch.float64).to(dt)
    assert float(v[2]) > 0 and float(v[4]) < fi.smallest_normal and float(v[6]) == fi.max   # they survived the cast
    return v


@pytest.mark.parametrize("dname", list(DTYPES))
def test_mixed_special_values(L, dname):
    """The gradient carries the specials in its vector body, on a segment edge and in its scalar
    tail; fp16's subnormals become fp32 normals. State bits equal the twin's after each of two steps."""
    dt, _ = DTYPES[dname]
    N = 3 * 4096 + 1027
    sp = specials(dt)
    a, b = twins(N, dt, nesterov=True)
    for s in range(2):
        g = gradient16(700 + s, N, dname).clone()
        for at in (8, 1024 - 5, 4096 + 64 * 4 - 3, N - sp.numel()):
            g[at: at + sp.numel()] = sp if s == 0 else sp.flip(0)
        g = g.to(DEV)
        out_a, out_b = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
        a.step(g, out_a)
        b.step(g.float(), out_b)
        assert np.array_equal(ibits(a._mmt), ibits(b._mmt)), (dname, s)
        assert np.array_equal(ibits(a._vec), ibits(b._vec)), (dname, s)
        assert np.array_equal(ibits(a.mmt), ibits(b.mmt)), (dname, s)
        assert np.array_equal(ibits(a.vec), ibits(b.vec)), (dname, s)
        for x, y in zip(entries(a), entries(b)):
            assert np.array_equal(x, y), (dname, s)


# ---------------------------------------------------------------- 3. the lists served a step
def test_mixed_lists_serve_a_step(L):
    """K1's candidate lists are used: on B, the reference side, some step selects with no full
    pass at a finite list threshold; A's record of that step is the same. (Without this a K1
    that wrote wrong lists would hide behind the full-pass fallback.) N % 4 == 0: such a step
    defers its masking into the next step's K1, and the state is compared with it pending."""
    N, dname = 1048576, "bf16"
    a, b = twins(N, torch.bfloat16, nesterov=True)
    out_a, out_b = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    served, deferred = [], 0
    for s in range(6):
        g = gradient16(500 + s, N, dname).to(DEV)
        a.step(g, out_a)
        b.step(g.float(), out_b)
        assert a._pending == b._pending, s
        deferred += b._pending
        assert torch.equal(a._mmt.view(torch.int32), b._mmt.view(torch.int32)), s   # (no flush)
        assert torch.equal(a._vec.view(torch.int32), b._vec.view(torch.int32)), s
        ia, ib = a.last_info(), b.last_info()
        print(s, {k: ib[k] for k in ("branch", "full_passes", "list_threshold", "threshold", "overflow_segments")})
        if ib["full_passes"] == 0 and np.isfinite(ib["list_threshold"]):
            served.append(s)
            assert {k: repr(v) for k, v in ia.items()} == {k: repr(v) for k, v in ib.items()}, s
            for x, y in zip(entries(a), entries(b)):
                assert np.array_equal(x, y), s
    assert served, "no step of the fp32 twin was served from K1's lists"
    assert deferred >= 2, "fewer than two steps of the fp32 twin left a masking to the next K1"
    assert torch.equal(a.vec.view(torch.int32), b.vec.view(torch.int32))   # flushed


# ---------------------------------------------------------------- 4. past the write-through size
def test_mixed_past_the_write_through_size(L):
    """The other launch shape (non-temporal stores, the LDS-bounded occupancy): payload and
    state against the twin, two steps."""
    N = WRITE_THROUGH_MAX + 4099
    a, b = twins(N, torch.bfloat16, compress_ratio=0.001, nesterov=True)
    gen = torch.Generator(device=DEV).manual_seed(9)
    for s in range(2):
        g = torch.randn(N, generator=gen, device=DEV).to(torch.bfloat16)
        a.compensate(g)
        a.select()
        g32 = g.float()
        del g
        b.compensate(g32)
        b.select()
        del g32
        assert torch.equal(a.payload[:16], b.payload[:16]), s
        n = int(a.payload[:8].view(torch.int64).item())
        assert 0 < n <= a.k, s
        assert torch.equal(a.payload[a.voff: a.voff + 4 * n], b.payload[b.voff: b.voff + 4 * n]), s
        assert torch.equal(a.payload[a.ioff: a.ioff + 8 * n], b.payload[b.ioff: b.ioff + 8 * n]), s
        assert torch.equal(a._mmt.view(torch.int32), b._mmt.view(torch.int32)), s
        assert torch.equal(a._vec.view(torch.int32), b._vec.view(torch.int32)), s
    assert torch.equal(a.mmt.view(torch.int32), b.mmt.view(torch.int32))
    assert torch.equal(a.vec.view(torch.int32), b.vec.view(torch.int32))
    assert info_of(a) == info_of(b)


# ---------------------------------------------------------------- 5. the engine
ENGINE_N = 200_003


@pytest.mark.parametrize("wire", [dict(), dict(fp16_values=True, int32_indices=True)], ids=["fp32-int64", "fp16-int32"])
@pytest.mark.parametrize("dname", list(DTYPES))
def test_mixed_step_against_the_twin(L, dname, wire):
    dt, _ = DTYPES[dname]
    a, b = twins(ENGINE_N, dt, nesterov=True, **wire)
    assert a.vdtype == (torch.float16 if wire else torch.float32)
    out_a, out_b = torch.empty(ENGINE_N, device=DEV), torch.empty(ENGINE_N, device=DEV)
    for s in range(5):
        g = gradient16(900 + s, ENGINE_N, dname).to(DEV)
        out_a.fill_(float("nan"))
        out_b.fill_(float("nan"))
        a.step(g, out_a)
        b.step(g.float(), out_b)
        assert_same_step(a, b, out_a, out_b, (dname, s))


def test_mixed_step_apply_against_the_twin(L):
    """step_apply(g16, DGCSGD) with weight decay and momentum: the fp32 parameter and the
    optimizer's momentum buffer against the twin's."""
    from dgc.optim import DGCSGD
    a, b = twins(ENGINE_N, torch.bfloat16, nesterov=True)
    p0 = torch.from_numpy(synth.gradient(7, ENGINE_N)).to(DEV)
    pa, pb = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    oa, ob = DGCSGD([pa], **kw), DGCSGD([pb], **kw)
    for s in range(5):
        g = gradient16(900 + s, ENGINE_N, "bf16").to(DEV)
        a.step_apply(g, oa)
        b.step_apply(g.float(), ob)
        assert np.array_equal(ibits(pa), ibits(pb)), s
        assert np.array_equal(ibits(oa.state[pa]["momentum_buffer"]), ibits(ob.state[pb]["momentum_buffer"])), s
        assert_same_step(a, b, None, None, s)
    assert not np.array_equal(ibits(pa), ibits(p0))   # the steps did move the parameter


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture
def rccl_one_rank(monkeypatch):
    """A one-rank RCCL group with the one-rank shortcut off: the exchange is a real collective."""
    import torch.distributed as dist
    from dgc import comm
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            device_id=DEV)
    monkeypatch.setattr(comm, "ONE_RANK_SHORTCUT", False)
    try:
        yield comm
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_mixed_over_rccl(L, rccl_one_rank):
    a, b = twins(ENGINE_N, torch.bfloat16, nesterov=True)
    assert a.exchanging and b.exchanging
    out_a, out_b = torch.empty(ENGINE_N, device=DEV), torch.empty(ENGINE_N, device=DEV)
    for s in range(5):
        g = gradient16(900 + s, ENGINE_N, "bf16").to(DEV)
        a.step(g, out_a)
        b.step(g.float(), out_b)
        torch.cuda.synchronize()
        assert np.array_equal(ibits(out_a), ibits(out_b)), s
    assert_same_step(a, b, out_a, out_b, "rccl")


# ---------------------------------------------------------------- 6. guards
def test_mixed_construction_refusals(L, monkeypatch):
    from dgc import clip_grad
    from dgc.bucket import DGCBucket
    from dgc.compression import DGCCompressor
    N = 5000
    kw = dict(compress_ratio=RATIO, device=DEV, world_size=1)
    for bad in (torch.float64, torch.int32, torch.complex64):
        with pytest.raises(NotImplementedError, match="grad_dtype"):
            DGCBucket(N, grad_dtype=bad, **kw)
    for dt, gdt in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16), (torch.bfloat16, torch.float32)):
        with pytest.raises(ValueError, match="grad_dtype"):
            DGCBucket(N, dtype=dt, grad_dtype=gdt, **kw)
    for clip in (clip_grad.clip_grad_norm_, clip_grad.clip_grad_value_):
        with pytest.raises(NotImplementedError, match="clip"):
            DGCBucket(N, grad_dtype=torch.bfloat16, clip=clip, **kw)
    # a sampled stride below 4 (the compressor's own strides are 1, unsampled, or >= 9)
    monkeypatch.setattr(DGCCompressor, "_attributes", classmethod(lambda cls, n, r, sr: (50, n // 2, 25, 2)))
    with pytest.raises(NotImplementedError, match="stride"):
        DGCBucket(N, grad_dtype=torch.float16, **kw)
    monkeypatch.undo()
    # grad_dtype that is the state's dtype is today's bucket
    assert DGCBucket(N, grad_dtype=torch.float32, **kw).grad_dtype is None
    assert DGCBucket(N, dtype=torch.bfloat16, grad_dtype=torch.bfloat16, **kw).grad_dtype is None


def test_mixed_compensate_refusals(L):
    from dgc.bucket import DGCBucket
    N = 5000
    b = DGCBucket(N, compress_ratio=RATIO, device=DEV, world_size=1, grad_dtype=torch.bfloat16)
    bad = [torch.zeros(N, dtype=torch.float32, device=DEV),                     # the state's dtype, not the gradient's
           torch.zeros(N, dtype=torch.float16, device=DEV),
           torch.zeros(N + 8, dtype=torch.bfloat16, device=DEV)[1:N + 1],      # 2-B aligned
           torch.zeros(N + 8, dtype=torch.bfloat16, device=DEV)[4:N + 4],      # 8-B aligned: the engine asks for 16
           torch.zeros(N + 1, dtype=torch.bfloat16, device=DEV),
           torch.zeros(N - 1, dtype=torch.bfloat16, device=DEV),
           torch.zeros(2 * N, dtype=torch.bfloat16, device=DEV)[::2],
           torch.zeros(N, dtype=torch.bfloat16),                               # on the host
           None]
    for g in bad:
        with pytest.raises(ValueError, match="bfloat16"):
            b.compensate(g)
    assert not b._mmt.any() and not b._vec.any()   # nothing ran
    # and it still steps: a refusal drew no sample start
    twin = DGCBucket(N, compress_ratio=RATIO, device=DEV, world_size=1)
    g = gradient16(500, N, "bf16").to(DEV)
    out_a, out_b = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    b.step(g, out_a)
    twin.step(g.float(), out_b)
    assert_same_step(b, twin, out_a, out_b, "after refusals")


class Spy:
    """The library with its dgc_compress_begin* calls recorded."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dgc_compress_begin"):
            return fn

        def recorded(*args):
            self.calls.append((name, len(args)))
            return fn(*args)
        return recorded


def test_default_bucket_still_makes_the_old_call(L):
    from dgc.bucket import DGCBucket
    N = 5000
    g = gradient16(500, N, "bf16").to(DEV)
    out = torch.empty(N, device=DEV)
    for kw in (dict(), dict(grad_dtype=None), dict(grad_dtype=torch.float32)):
        b = DGCBucket(N, compress_ratio=RATIO, device=DEV, world_size=1, **kw)
        b._L = spy = Spy(b._L)
        b.step(g.float(), out)
        assert spy.calls == [("dgc_compress_begin_clip", 15)], (kw, spy.calls)
    b = DGCBucket(N, compress_ratio=RATIO, device=DEV, world_size=1, grad_dtype=torch.bfloat16)
    b._L = spy = Spy(b._L)
    b.step(g, out)
    assert spy.calls == [("dgc_compress_begin_g16", 13)], spy.calls
