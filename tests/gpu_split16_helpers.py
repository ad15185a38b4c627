"""Workers of the 16-bit split exchange's multi-rank tests (tests/test_gpu_split16_engine.py):
W processes on cuda:0 over gloo. Each rank runs TWO engines on bf16 parameters over the same
per-rank gradients — one with a single allgather (``HalfExchange``, pinned to the reference's
16-bit fixtures by the existing suite), one with the exchange split in ``parts`` collectives
(``HalfSplitExchange``: dgc_fill_zero16 + the dgc_scatter_split16 phases) — and reports every
step at which their outputs or 16-bit state differ in a bit.
"""
import torch

from gpu_dist_helpers import _init   # (also puts the repository and the package on sys.path)

STEPS = 4
SHAPES = [("a", (1000, 300)), ("b", (257, 3, 3, 64)), ("c", (70001,)), ("d", (2000, 500))]


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _gradient(shape, s, gen, dev, scale=1.0):
    """Seeded per rank; odd steps heavy-tailed, so the adaptation loop and the resample run."""
    g = torch.randn(shape, generator=gen, device=dev) * scale
    if s % 2:
        g = g * torch.rand(shape, generator=gen, device=dev).pow(8) * 50
    return g.to(torch.bfloat16)


def bucket16_pair_worker(rank, world, port, parts, queue):
    """DGCBucket(dtype=bf16) with exchange_parts = 1 and = parts."""
    import torch.distributed as dist
    _init(rank, world, port)
    problems = []
    try:
        from dgc.bucket import DGCBucket
        from dgc.exchange import HalfExchange, HalfSplitExchange
        dev = torch.device("cuda:0")
        N = 1_000_003
        make = lambda p: DGCBucket(N, compress_ratio=0.001, momentum=0.9, nesterov=True, device=dev,   # noqa: E731
                                   world_size=world, seed=42, dtype=torch.bfloat16, exchange_parts=p)
        one, split = make(1), make(parts)
        if (one.parts, split.parts) != (1, parts):
            problems.append(("parts", one.parts, split.parts))
        if not (isinstance(one.rx.xchg, HalfExchange) and isinstance(split.rx.xchg, HalfSplitExchange)):
            problems.append(("exchange", type(one.rx.xchg).__name__, type(split.rx.xchg).__name__))
        outs = [torch.full((N,), float("nan"), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        gen = torch.Generator(device=dev).manual_seed(1000 + rank)
        for s in range(STEPS):
            g = _gradient((N,), s, gen, dev)
            for b, out in zip((one, split), outs):
                b.step(g.clone(), out)
            torch.cuda.synchronize()
            if not _same(outs[0], outs[1]):
                problems.append(("out", s, int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())))
            if not (_same(one.mmt, split.mmt) and _same(one.vec, split.vec)):
                problems.append(("state", s))
            if int(outs[0].count_nonzero()) == 0:
                problems.append(("empty", s))
        for b in (one, split):
            b.status.check(sync=True)
        queue.put((rank, problems))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback
        queue.put((rank, [("error", repr(e), traceback.format_exc())]))
    finally:
        dist.destroy_process_group()


def batch16_pair_worker(rank, world, port, parts, queue):
    """DGCBatch(dtype=bf16) with exchange_parts = 1 and = parts."""
    import torch.distributed as dist
    _init(rank, world, port)
    problems = []
    try:
        from dgc.batch import DGCBatch
        from dgc.exchange import HalfSplitExchange
        dev = torch.device("cuda:0")
        make = lambda p: DGCBatch(SHAPES, compress_ratio=0.001, momentum=0.9, nesterov=False, device=dev,   # noqa: E731
                                  world_size=world, seed=7, dtype=torch.bfloat16, exchange_parts=p)
        one, split = make(1), make(parts)
        if (one.parts, split.parts) != (1, parts) or not isinstance(split.rx.xchg, HalfSplitExchange):
            problems.append(("parts", one.parts, split.parts, type(split.rx.xchg).__name__))
        gen = torch.Generator(device=dev).manual_seed(2000 + rank)
        for s in range(STEPS):
            grads = {n: _gradient(one.shapes[n], s, gen, dev, 1e-3) for n in one.names}
            for b in (one, split):
                for n in b.names:
                    b.grad(n).copy_(grads[n])
                b.compress()
                b.exchange()
                b.decompress()
            torch.cuda.synchronize()
            if not _same(one.out_flat, split.out_flat):
                problems.append(("out", s))
            if not (_same(one.mmt_flat, split.mmt_flat) and _same(one.vec_flat, split.vec_flat)):
                problems.append(("state", s))
            if int(one.out_flat.count_nonzero()) == 0:
                problems.append(("empty", s))
        for b in (one, split):
            b.status.check(sync=True)
        queue.put((rank, problems))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback
        queue.put((rank, [("error", repr(e), traceback.format_exc())]))
    finally:
        dist.destroy_process_group()
