"""The split exchange of bf16 / fp16 parameters through the engines: DGCBucket(dtype=...,
exchange_parts=p), DGCBatch(dtype=..., exchange_parts=p) and DistributedOptimizer(batch=True)
under DGC_EXCHANGE_PARTS take ``HalfSplitExchange`` (dgc_fill_zero16 + the dgc_scatter_split16
phases) and give, bit for bit, what the one-allgather ``HalfExchange`` gives — which the
existing suite pins to the reference's 16-bit fixtures. ``"auto"`` alone still does not split,
and what 16-bit engines refused they still refuse.
"""
import contextlib
import io
import random

import pytest
import torch
import torch.distributed as dist

import gpu_split16_helpers as G16
from test_gpu_multirank import run
from test_gpu_rccl import rccl_one_rank  # noqa: F401  (the one-rank RCCL group fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int16)


def counted_allgathers(comm, monkeypatch):
    calls = [0]
    fn = dist.all_gather_into_tensor

    def wrapper(*a, **kw):
        calls[0] += 1
        return fn(*a, **kw)
    monkeypatch.setattr(comm.dist, "all_gather_into_tensor", wrapper)
    return calls


def heavy(shape, s, gen, scale=1.0):
    g = torch.randn(shape, generator=gen, device=DEV) * scale
    return g * torch.rand(shape, generator=gen, device=DEV).pow(8) * 50 if s % 2 else g


# ---------------------------------------------------------------- one-rank RCCL
@pytest.mark.timeout(300)
def test_bucket16_split_over_rccl(rccl_one_rank, monkeypatch):  # noqa: F811
    """DGCBucket(bf16, exchange_parts=2) through RCCL: two part collectives a step, the
    compute stream waiting on each in turn; outputs and state equal exchange_parts=1's."""
    from dgc.bucket import DGCBucket
    from dgc.exchange import HalfExchange, HalfSplitExchange
    calls = counted_allgathers(rccl_one_rank, monkeypatch)
    N, steps, dt = 3_000_017, 5, torch.bfloat16

    def run_engine(parts, kind):
        b = DGCBucket(N, compress_ratio=0.001, momentum=0.9, nesterov=True, device=DEV, world_size=1, seed=42,
                      dtype=dt, exchange_parts=parts)
        assert b.exchanging and b.parts == parts and isinstance(b.rx.xchg, kind)
        assert (b.xchg is b.rx.xchg) == (parts > 1) and b.dec_ws is None and b.fill == "inline" and b.extra_off is None
        out = torch.full((N,), float("nan"), dtype=dt, device=DEV)
        gen = torch.Generator(device=DEV).manual_seed(3)
        res, before = [], calls[0]
        for s in range(steps):
            b.step(heavy((N,), s, gen).to(dt), out)
            torch.cuda.synchronize()
            res.append((out.clone(), b.mmt.clone(), b.vec.clone()))
        b.status.check(sync=True)
        assert calls[0] - before == parts * steps
        return res

    got = run_engine(2, HalfSplitExchange)
    want = run_engine(1, HalfExchange)
    for s, (w, g) in enumerate(zip(want, got)):
        assert int(w[0].count_nonzero()) > 0
        for name, a, b in zip(("out", "mmt", "vec"), w, g):
            assert torch.equal(bits(a), bits(b)), (s, name)


@pytest.mark.timeout(300)
def test_batch16_split_over_rccl(rccl_one_rank, monkeypatch):  # noqa: F811
    """DGCBatch(fp16, exchange_parts=2) likewise, on test_batch_over_rccl's four shapes."""
    from dgc.batch import DGCBatch
    from dgc.exchange import HalfExchange, HalfSplitExchange
    calls = counted_allgathers(rccl_one_rank, monkeypatch)
    steps, dt = 5, torch.float16

    def run_engine(parts, kind):
        b = DGCBatch(G16.SHAPES, compress_ratio=0.001, momentum=0.9, nesterov=False, device=DEV, world_size=1, seed=7,
                     dtype=dt, exchange_parts=parts)
        assert b.exchanging and b.parts == parts and isinstance(b.rx.xchg, kind)
        assert b.dec_ws is None and b.fill == "inline" and b.extra_off is None
        gen = torch.Generator(device=DEV).manual_seed(3)
        res, before = [], calls[0]
        for s in range(steps):
            for n in b.names:
                b.grad(n).copy_(heavy(b.shapes[n], s, gen, 1e-3).to(dt))
            b.compress()
            b.exchange()
            out = b.decompress()
            torch.cuda.synchronize()
            res.append((out.clone(), b.mmt_flat.clone(), b.vec_flat.clone()))
        b.status.check(sync=True)
        assert calls[0] - before == parts * steps
        return res

    got = run_engine(2, HalfSplitExchange)
    want = run_engine(1, HalfExchange)
    for s, (w, g) in enumerate(zip(want, got)):
        assert int(w[0].count_nonzero()) > 0
        for name, a, b in zip(("out", "mmt", "vec"), w, g):
            assert torch.equal(bits(a), bits(b)), (s, name)


def _optimizer_steps(steps=3):
    """DistributedOptimizer(batch=True) around DGCSGD on a bf16 TinyNet; the weights after
    every step and the batch engine's part count."""
    from dgc.compression import DGCCompressor
    from dgc.horovod import DistributedOptimizer
    from dgc.memory import DGCSGDMemory
    from dgc.optim import DGCSGD
    from models import TinyNet
    torch.manual_seed(0)
    random.seed(5)
    model = TinyNet().to(DEV).to(torch.bfloat16)
    named = list(model.named_parameters())
    with contextlib.redirect_stdout(io.StringIO()):
        comp = DGCCompressor(0.01, memory=DGCSGDMemory(momentum=0.9))
        comp.memory.initialize(named)
        comp.initialize([(n, p) for n, p in named if p.dim() > 1])
    opt = DistributedOptimizer(DGCSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True),
                               named_parameters=named, compression=comp, batch=True)
    gen = torch.Generator(device=DEV).manual_seed(17)
    weights = []
    for s in range(steps):
        for _, p in named:
            p.grad = heavy(p.shape, s, gen, 1e-2).to(torch.bfloat16)
        for _, hook in reversed(opt._hook_fns):
            hook()
        opt.step()
        torch.cuda.synchronize()
        weights.append({n: p.detach().clone() for n, p in named})
        opt.zero_grad()
    return weights, opt._batched._plan["batch"].parts


@pytest.mark.timeout(300)
def test_batched_optimizer16_under_exchange_parts(rccl_one_rank, monkeypatch):  # noqa: F811
    """DGC_EXCHANGE_PARTS=2 reaches the 16-bit batch the optimizer builds with "auto"."""
    monkeypatch.setenv("HOROVOD_ELASTIC", "1")
    monkeypatch.setenv("DGC_EXCHANGE_PARTS", "2")
    got, parts = _optimizer_steps()
    assert parts == 2
    monkeypatch.delenv("DGC_EXCHANGE_PARTS")
    want, parts = _optimizer_steps()
    assert parts == 1
    start = None
    for s, (w, g) in enumerate(zip(want, got)):
        for n in w:
            assert torch.equal(bits(w[n]), bits(g[n])), (s, n)
        assert start is None or any(not torch.equal(bits(w[n]), bits(start[n])) for n in w), s   # the weights move
        start = w


# ---------------------------------------------------------------- W = 2 and 4 over gloo
@pytest.mark.timeout(200)
@pytest.mark.parametrize("world,parts", [(2, 2), (4, 4)])
def test_bucket16_split_multirank(world, parts):
    for rank, problems in run(G16.bucket16_pair_worker, world, parts).items():
        assert problems == [], (rank, problems)


@pytest.mark.timeout(200)
@pytest.mark.parametrize("world,parts", [(2, 2), (4, 4)])
def test_batch16_split_multirank(world, parts):
    for rank, problems in run(G16.batch16_pair_worker, world, parts).items():
        assert problems == [], (rank, problems)


# ---------------------------------------------------------------- what does not change
def test_refusals_unchanged_on_a_split_16bit_engine(monkeypatch):
    from dgc.batch import DGCBatch
    from dgc.bucket import DGCBucket
    monkeypatch.delenv("DGC_EXCHANGE_PARTS", raising=False)
    N, bf = 50_000, torch.bfloat16
    for fill in ("sparse", "allgather"):
        with pytest.raises(NotImplementedError, match=fill):
            DGCBucket(N, device=DEV, world_size=2, dtype=bf, fill=fill, exchange_parts=2)
    b = DGCBucket(N, device=DEV, world_size=2, dtype=bf, exchange_parts=2)
    assert b.parts == 2
    with pytest.raises(NotImplementedError, match="dense=False on torch.bfloat16"):
        b.decompress(torch.empty(N, dtype=bf, device=DEV), dense=False)
    with pytest.raises(NotImplementedError, match="fill='sparse' on torch.bfloat16"):
        b.rx.zero(torch.empty(N, dtype=bf, device=DEV), None, sparse=True)
    with pytest.raises(NotImplementedError, match="DGCBucket.apply: fp32 parameters only"):
        b.apply(torch.zeros(N, device=DEV), lr=0.1)
    with pytest.raises(RuntimeError, match="before exchange"):   # as any split exchange: nothing was sent
        b.decompress(torch.empty(N, dtype=bf, device=DEV))
    with pytest.raises(ValueError, match="exchange parts"):
        DGCBucket(N, device=DEV, world_size=2, dtype=bf, exchange_parts=9)
    t = DGCBatch(G16.SHAPES, device=DEV, world_size=2, dtype=torch.float16, exchange_parts=2)
    assert t.parts == 2
    with pytest.raises(NotImplementedError, match="DGCBatch.apply: fp32 parameters only"):
        t.apply(None, None)


def test_auto_alone_does_not_split_16bit(monkeypatch):
    """W = 8 and 2^18 entries per rank: fp32's "auto" splits in 4; a 16-bit bucket keeps one
    allgather until someone asks (an integer, or DGC_EXCHANGE_PARTS)."""
    from dgc.bucket import DGCBucket
    from dgc.exchange import HalfExchange, HalfSplitExchange, split_parts
    monkeypatch.delenv("DGC_EXCHANGE_PARTS", raising=False)
    N = 1 << 20
    b = DGCBucket(N, compress_ratio=0.25, device=DEV, world_size=8, dtype=torch.bfloat16, exchange_parts="auto")
    assert b.k >= 1 << 18 and split_parts(8, b.k, "auto") == 4
    assert b.parts == 1 and isinstance(b.rx.xchg, HalfExchange) and b.xchg is None
    assert DGCBucket(N, compress_ratio=0.25, device=DEV, world_size=8, dtype=torch.bfloat16).parts == 1
    monkeypatch.setenv("DGC_EXCHANGE_PARTS", "4")   # (no process group: nothing to agree with)
    b = DGCBucket(N, compress_ratio=0.25, device=DEV, world_size=8, dtype=torch.bfloat16)
    assert b.parts == 4 and isinstance(b.rx.xchg, HalfSplitExchange)
