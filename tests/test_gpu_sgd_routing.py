"""DGCSGD.step's routing: which parameters of a group go into the fused launches
(dgc_sgd_step for fp32, dgc_sgd_step16 per 16-bit dtype), which take the reference's own
op sequence, and that every one of them — and every momentum buffer — ends bit-identical
to its expectation: oracle.dgcsgd_step32 / dgcsgd_step16 for the fused ones, the
torch-CPU sequence on a CPU copy for the others. The launches are counted through a spy
on the two entry points."""
import copy

import numpy as np
import pytest
import torch

import oracle.dgc_oracle as O
from test_sgd32_port import H, H_IDS, assert_same_bits, torch_cpu_step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ORACLE_DTYPE = {torch.bfloat16: "bfloat16", torch.float16: "float16"}


class Spy:
    """Records (entry point, count, first flags, lr, momentum, dampening, wd, nesterov) of
    every fused launch."""

    def __init__(self, monkeypatch):
        from dgc import _lib
        self.calls = []
        L = _lib.lib()
        for name in ("dgc_sgd_step", "dgc_sgd_step16"):
            real = getattr(L, name)

            def spy(*a, _real=real, _name=name):
                self.calls.append((_name, a[5], [a[4][i] for i in range(a[5])]) + tuple(a[6:11]))
                return _real(*a)
            monkeypatch.setattr(L, name, spy)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def image(t):
    """A tensor's values as a flat fp32 numpy array (exact for bf16 / fp16)."""
    return t.detach().float().cpu().contiguous().numpy().reshape(-1)


class Fused:
    """A parameter the fused launch serves, and its oracle state."""

    def __init__(self, p):
        self.p, self.w, self.buf = p, image(p), None

    def expect(self, g, hyper):
        lr, mom, damp, wd, nest = hyper
        if self.p.dtype == torch.float32:
            self.w, self.buf = O.dgcsgd_step32(self.w, image(g), self.buf, lr, mom, damp, wd, nest)
        else:
            self.w, self.buf = O.dgcsgd_step16(self.w, image(g), self.buf, lr, mom, damp, wd, nest,
                                               ORACLE_DTYPE[self.p.dtype])

    def check(self, opt, what):
        assert_same_bits(image(self.p), self.w, (what, "p"))
        buf = opt.state[self.p].get("momentum_buffer") if self.p in opt.state else None
        assert (buf is None) == (self.buf is None), (what, "momentum buffer present")
        if buf is not None:
            assert buf.dtype == self.p.dtype and buf.shape == self.p.shape
            assert_same_bits(image(buf), self.buf, (what, "buf"))


class Fallback:
    """A parameter that takes the reference's op sequence: the expectation is that sequence
    with torch on a CPU copy (same dtypes, same memory format)."""

    def __init__(self, p, buf=None):
        self.p, self.w, self.buf = p, p.detach().cpu().clone(), buf

    def expect(self, g, hyper):
        lr, mom, damp, wd, nest = hyper
        self.buf = torch_cpu_step(self.w, self.buf, g.detach().cpu(), lr, mom, damp, wd, nest)

    def check(self, opt, what):
        assert_same_bits(image(self.p), image(self.w), (what, "p"))
        buf = opt.state[self.p].get("momentum_buffer") if self.p in opt.state else None
        assert (buf is None) == (self.buf is None), (what, "momentum buffer present")
        if buf is not None:
            assert buf.dtype == self.buf.dtype
            got, want = buf.detach().cpu(), self.buf
            if buf.dtype == torch.float64:   # compared as 64-bit patterns, NaN for NaN
                got, want = got.numpy().reshape(-1), want.numpy().reshape(-1)
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan)
                assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), (what, "buf")
            else:
                assert_same_bits(image(got), image(want), (what, "buf"))


def randn(gen, shape, scale, dtype=torch.float32):
    return (torch.randn(shape, generator=gen) * scale).to(dtype)


def set_grads(gen, params, skip=(), grad_dtype={}):
    for p in params:
        if any(p is q for q in skip):
            continue
        g = randn(gen, tuple(p.shape), 0.01, grad_dtype.get(id(p), p.dtype)).to(DEV)
        if p.dim() == 4 and not p.data.is_contiguous():
            g = g.contiguous(memory_format=torch.channels_last)
        p.grad = g


FP32_SHAPES = [(37,), (16,), (5, 7), (1000,), (4096,), (4097,), (8, 3, 3, 3), (333, 7), (1,), (8200,)]


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("hyper", H, ids=H_IDS)
def test_one_group_of_everything(hyper, monkeypatch, one_thread):
    """50 fusable fp32 parameters (one a +4 B view, one with zero elements), 3 bf16 and 3
    fp16, a channels_last convolution weight, a parameter without gradient and an fp32
    parameter with an fp16 gradient, in ONE group: one fp32 launch of 50 and one launch of
    3 per 16-bit dtype and step; the rest takes the reference's sequence."""
    from dgc.optim import DGCSGD
    lr, mom, damp, wd, nest = hyper
    gen = torch.Generator().manual_seed(77)
    fp32 = [torch.nn.Parameter(randn(gen, FP32_SHAPES[i % len(FP32_SHAPES)], 0.5).to(DEV)) for i in range(48)]
    base = torch.zeros(8200 + 4, device=DEV)
    view = torch.nn.Parameter(base[1:8201])
    view.data.copy_(randn(gen, (8200,), 0.5))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    empty = torch.nn.Parameter(torch.empty(0, device=DEV))
    fp32 = fp32[:20] + [view] + fp32[20:40] + [empty] + fp32[40:]
    assert len(fp32) == 50
    half = [torch.nn.Parameter(randn(gen, s, 0.5, dt).to(DEV))
            for dt in (torch.bfloat16, torch.float16) for s in ((37,), (1024, 3), (64,))]
    conv = torch.nn.Parameter(randn(gen, (8, 4, 3, 3), 0.5).to(DEV).contiguous(memory_format=torch.channels_last))
    assert not conv.data.is_contiguous()
    no_grad = torch.nn.Parameter(randn(gen, (33,), 0.5).to(DEV))
    half_grad = torch.nn.Parameter(randn(gen, (129,), 0.5).to(DEV))
    if hasattr(half_grad, "grad_dtype"):
        half_grad.grad_dtype = None   # newer torch: a gradient of another dtype needs this opt-in
    params = fp32[:25] + [conv] + half[:3] + [no_grad] + fp32[25:] + half[3:] + [half_grad]
    untouched = no_grad.detach().clone()
    opt = DGCSGD(params, lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nest)
    spy = Spy(monkeypatch)
    fused = [Fused(p) for p in fp32 + half]
    others = [Fallback(conv), Fallback(half_grad)]
    for s in range(3):
        set_grads(gen, params, skip=[no_grad], grad_dtype={id(half_grad): torch.float16})
        assert conv.grad.is_contiguous(memory_format=torch.channels_last) and not conv.grad.is_contiguous()
        assert half_grad.grad.dtype == torch.float16
        for t in fused + others:
            t.expect(t.p.grad, hyper)
        opt.step()
        torch.cuda.synchronize()
        calls = spy.take()
        assert sorted((c[0], c[1]) for c in calls) == [("dgc_sgd_step", 50), ("dgc_sgd_step16", 3),
                                                       ("dgc_sgd_step16", 3)], calls
        use_buf = wd != 0 and mom != 0
        for c in calls:
            assert c[2] == [int(use_buf and s == 0)] * c[1], (s, c)
        for k, t in enumerate(fused + others):
            t.check(opt, (hyper, s, k, tuple(t.p.shape), t.p.dtype))
    # the zero-element parameter: stepped without an error, still empty, state as the reference's
    assert empty.numel() == 0
    assert ("momentum_buffer" in opt.state[empty]) == (wd != 0 and mom != 0)
    # no gradient: untouched, no state created
    assert torch.equal(no_grad.detach(), untouched)
    assert no_grad not in opt.state or not opt.state[no_grad]


def test_two_groups_carry_their_own_hypers(monkeypatch, one_thread):
    """Two groups, one of them without weight decay: each group's launch gets its own
    values, and no momentum buffer appears in the wd = 0 group."""
    from dgc.optim import DGCSGD
    ha, hb = H[1], H[3]
    assert hb[3] == 0
    gen = torch.Generator().manual_seed(78)
    ga = [torch.nn.Parameter(randn(gen, s, 0.5).to(DEV)) for s in ((37,), (4097,), (8, 3, 3, 3))]
    gb = [torch.nn.Parameter(randn(gen, s, 0.5).to(DEV)) for s in ((1000,), (5, 7))]
    keys = ("lr", "momentum", "dampening", "weight_decay", "nesterov")
    opt = DGCSGD([dict(params=ga, **dict(zip(keys, ha))), dict(params=gb, **dict(zip(keys, hb)))], lr=1.0)
    spy = Spy(monkeypatch)
    fa, fb = [Fused(p) for p in ga], [Fused(p) for p in gb]
    for s in range(3):
        set_grads(gen, ga + gb)
        for t in fa:
            t.expect(t.p.grad, ha)
        for t in fb:
            t.expect(t.p.grad, hb)
        opt.step()
        torch.cuda.synchronize()
        calls = spy.take()
        assert [(c[0], c[1]) for c in calls] == [("dgc_sgd_step", 3), ("dgc_sgd_step", 2)], calls
        assert calls[0][3:] == tuple(float(x) for x in ha[:4]) + (int(ha[4]),)
        assert calls[1][3:] == tuple(float(x) for x in hb[:4]) + (int(hb[4]),)
        for k, t in enumerate(fa + fb):
            t.check(opt, (s, k))
    for p in gb:
        assert "momentum_buffer" not in opt.state.get(p, {})
    for p in ga:
        assert "momentum_buffer" in opt.state[p]


@pytest.mark.parametrize("cast", [False, True], ids=["same_dtype", "fp64_buffer"])
def test_state_round_trip(cast, monkeypatch, one_thread):
    """state_dict() after 2 steps -> a fresh DGCSGD over cloned parameters -> step 3 equals
    the uninterrupted run; the loaded buffers go in with first = 0. With one loaded buffer
    cast to fp64 that parameter takes the reference's sequence on those dtypes."""
    from dgc.optim import DGCSGD
    hyper = H[1]
    lr, mom, damp, wd, nest = hyper
    gen = torch.Generator().manual_seed(79)
    params = [torch.nn.Parameter(randn(gen, s, 0.5).to(DEV)) for s in ((37,), (4097,), (8, 3, 3, 3), (8200,))]
    kw = dict(lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nest)
    opt = DGCSGD(params, **kw)
    spy = Spy(monkeypatch)
    track = [Fused(p) for p in params]
    for s in range(2):
        set_grads(gen, params)
        for t in track:
            t.expect(t.p.grad, hyper)
        opt.step()
    torch.cuda.synchronize()
    assert [c[2] for c in spy.take()] == [[1] * 4, [0] * 4]
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = DGCSGD(clones, **kw)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    set_grads(gen, params)
    for p, q in zip(params, clones):
        q.grad = p.grad.clone()
    new = [Fused(q) for q in clones]
    for t, u in zip(track, new):
        u.w, u.buf = t.w.copy(), t.buf.copy()
    if cast:   # parameter 1's buffer in fp64: not fusable any more
        buf64 = opt2.state[clones[1]]["momentum_buffer"].double()
        opt2.state[clones[1]]["momentum_buffer"] = buf64
        new[1] = Fallback(clones[1], buf64.cpu().clone())
    for t in track + new:
        t.expect(t.p.grad, hyper)
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    calls = spy.take()
    assert [(c[0], c[1], c[2]) for c in calls] == [("dgc_sgd_step", 4, [0] * 4),
                                                   ("dgc_sgd_step", 3 if cast else 4, [0] * (3 if cast else 4))]
    for k, (t, u) in enumerate(zip(track, new)):
        t.check(opt, ("uninterrupted", k))
        u.check(opt2, ("reloaded", k))
        if not (cast and k == 1):
            assert torch.equal(t.p.detach(), u.p.detach())
