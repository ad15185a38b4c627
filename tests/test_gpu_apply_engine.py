"""DGCBucket.step_apply / DGCBucket.apply / DGCSGD.step_sparse: the flat bucket's step ended by
the optimizer's update from the gathered entries. After every step the parameter, the
optimizer's momentum buffer and the bucket's momentum and velocity are bit-equal to
``bucket.step(g, out); p.grad = out; opt.step()`` on an identical twin."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, RATIO, STEPS = 200_003, 0.01, 5


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def gradient(seed, n=N):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen).to(DEV)


def twin(world, **opt_kw):
    """(bucket, parameter, optimizer), identical every time it is called."""
    from dgc.bucket import DGCBucket
    from dgc.optim import DGCSGD
    b = DGCBucket(N, compress_ratio=RATIO, world_size=world, seed=42, device=DEV)
    p = torch.nn.Parameter(gradient(7))
    return b, p, DGCSGD([p], lr=0.1, **opt_kw)


def assert_same(a, b, step):
    (ba, pa, oa), (bb, pb, ob) = a, b
    assert np.array_equal(bits(pa), bits(pb)), (step, "param")
    sa, sb = oa.state[pa].get("momentum_buffer"), ob.state[pb].get("momentum_buffer")
    assert (sa is None) == (sb is None), step
    if sa is not None:
        assert np.array_equal(bits(sa), bits(sb)), (step, "momentum_buffer")
    assert np.array_equal(bits(ba.mmt), bits(bb.mmt)), (step, "mmt")
    assert np.array_equal(bits(ba.vec), bits(bb.vec)), (step, "vec")


@pytest.mark.parametrize("opt_kw", [
    dict(momentum=0.9, weight_decay=1e-4, nesterov=True),
    dict(momentum=0.9, weight_decay=0, nesterov=True),
], ids=["wd", "wd0"])
def test_step_apply_equals_step_then_optimizer(opt_kw):
    a, b = twin(1, **opt_kw), twin(1, **opt_kw)
    out = torch.empty(N, device=DEV)
    before = bits(a[1]).copy()
    for s in range(STEPS):
        g = gradient(100 + s)
        a[0].step(g, out)
        a[1].grad = out
        a[2].step()
        ev = {"apply": (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))}
        b[0].step_apply(g, b[2], events=ev)
        assert b[1].grad is None   # never read, never made
        torch.cuda.synchronize()
        assert ev["apply"][0].elapsed_time(ev["apply"][1]) >= 0
        assert_same(a, b, s)
        assert int(b[0]._acc.view(torch.int32).count_nonzero()) == 0
    assert not np.array_equal(before, bits(b[1]))   # the steps did move the parameter
    assert ("momentum_buffer" in b[2].state[b[1]]) == (opt_kw["weight_decay"] != 0)
    b[0].last_info()   # raises what the status words hold


def test_apply_at_four_ranks_with_an_injected_gather():
    """W = 4 in one process: ranks 1 and 2 are peers' payloads of other gradients, rank 3
    repeats rank 0's (every index of it a duplicate); the gathered buffer is injected in
    place of the allgather."""
    from dgc.bucket import DGCBucket
    kw = dict(momentum=0.9, weight_decay=1e-4, nesterov=True)
    a, b = twin(4, **kw), twin(4, **kw)
    peers = [DGCBucket(N, compress_ratio=RATIO, world_size=4, seed=42, device=DEV) for _ in range(2)]
    out = torch.empty(N, device=DEV)
    for s in range(STEPS):
        for r, peer in enumerate(peers):
            peer.compensate(gradient(1000 * (r + 1) + s))
            peer.select()
        g = gradient(100 + s)
        for bucket in (a[0], b[0]):
            bucket.compensate(g)
            bucket.select()
            gathered = torch.cat([bucket.payload, peers[0].payload, peers[1].payload, bucket.payload])
            bucket._gathers = [gathered] * len(bucket._gathers)
        a[0].decompress(out)
        a[1].grad = out
        a[2].step()
        b[2].step_sparse(b[0])
        torch.cuda.synchronize()
        assert_same(a, b, s)
        assert int(b[0]._acc.view(torch.int32).count_nonzero()) == 0
    b[0].last_info()


def test_step_sparse_names_its_parameter():
    from dgc.optim import DGCSGD
    b, p, _ = twin(1)
    q = torch.nn.Parameter(torch.zeros(3, device=DEV))
    opt = DGCSGD([p, q], lr=0.1)
    with pytest.raises(ValueError, match="name the parameter"):
        opt.step_sparse(b)
    with pytest.raises(ValueError, match="not one of"):
        opt.step_sparse(b, torch.nn.Parameter(torch.zeros(N, device=DEV)))


def test_apply_refusals():
    from dgc.bucket import DGCBucket
    from dgc.optim import DGCSGD
    p = torch.zeros(N, device=DEV)
    half = DGCBucket(N, compress_ratio=RATIO, world_size=1, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp32"):
        half.apply(p, 0.1)
    b = DGCBucket(N, compress_ratio=RATIO, world_size=1, device=DEV)
    for bad in (torch.zeros(N, device=DEV, dtype=torch.float16), torch.zeros(N + 1, device=DEV), torch.zeros(N),
                torch.zeros(2 * N, device=DEV)[::2]):
        with pytest.raises(ValueError, match="param must be"):
            b.apply(bad, 0.1)
    with pytest.raises(ValueError, match="momentum_buffer must be"):
        b.apply(p, 0.1, momentum=0.9, weight_decay=1e-4)                       # needed, missing
    with pytest.raises(ValueError, match="momentum_buffer must be"):
        b.apply(p, 0.1, momentum=0.9, weight_decay=1e-4, momentum_buffer=torch.zeros(N))
    split = DGCBucket(N, compress_ratio=RATIO, world_size=2, device=DEV, exchange_parts=2)
    assert split.parts == 2
    with pytest.raises(ValueError, match="exchange_parts=1"):
        split.apply(p, 0.1)
    # through the optimizer: a refusal leaves no uninitialised momentum buffer behind
    q = torch.nn.Parameter(torch.zeros(N, device=DEV))
    opt = DGCSGD([q], lr=0.1, momentum=0.9, weight_decay=1e-4)
    with pytest.raises(ValueError, match="exchange_parts=1"):
        opt.step_sparse(split)
    assert "momentum_buffer" not in opt.state[q]
    assert not p.any()   # nothing ran
