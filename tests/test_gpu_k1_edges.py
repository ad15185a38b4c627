"""K1's load path at its edges (csrc/select_k1.hpp: the state words and the twelve
streaming loads issued ahead of every use, the partial last float4 of a pointer-table
gradient patched in by the one wave that owns it, the spill count without a block
barrier), bit for bit against the numpy oracle — small sizes around the segment
(1024 elements) and workgroup (4096) boundaries, where a predicate, an offset or a tail
can be off by one."""
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle import dgc_oracle as O
from oracle import synth
from test_clip_host import clip_np

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEG, CAP = 1024, 64   # csrc/select_types.hpp: kSeg, kCap


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(t):
    return t.detach().view(-1).cpu().numpy()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def payload_of(b):
    n = int(b.payload[:8].view(torch.int64).item())
    gi = b.payload[b.ioff: b.ioff + 8 * n].view(torch.int64).cpu().numpy()
    gv = b.payload[b.voff: b.voff + 4 * n].view(torch.float32).cpu().numpy()
    return gv, gi


# ----------------------------------------------------------------------------- flat bucket
# gradient seeds (oracle/synth.py) at which the oracle takes a first-k branch in steps 1 and
# 2 for both nesterov values — a resample leaves no masking to the next K1 — found with
# the oracle alone (at these k the 3 top samples make the sampled threshold noisy)
SEEDS = {4093: 512, 4096: 512, 4097: 512, 5 * 4096 + 1021: 518, 1_048_576 + 3: 500}


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("N", list(SEEDS))
def test_bucket_edge_sizes_match_oracle(N, nesterov):
    """DGCBucket, three steps: steps 2 and 3 run the previous step's deferred masking inside
    K1, on the offsets it loaded ahead of its streaming loads. The state is read after the
    last step only (reading it would flush the masking out of K1)."""
    from dgc.bucket import DGCBucket
    ratio = 0.01
    b = DGCBucket(N, compress_ratio=ratio, momentum=0.9, nesterov=nesterov, device=DEV, seed=11)
    attrs = O.attributes(N, ratio)
    m_o, v_o = np.zeros(N, np.float32), np.zeros(N, np.float32)
    rng = random.Random(11)
    out = torch.full((N,), float("nan"), device=DEV)
    branches = []
    for s in range(3):
        g = synth.gradient(SEEDS[N] + s, N, "normal", 1.0)
        start = rng.randint(0, attrs[4] - 1) if attrs[0] != attrs[2] else 0
        b.step(to_dev(g), out)
        torch.cuda.synchronize()
        info = b.last_info()
        ov, oi, oinfo = O.compress_step(g, m_o, v_o, attrs, start, nesterov=nesterov)
        gv, gi = payload_of(b)
        assert info["branch"] == oinfo["branch"], (s, info)
        assert bits(np.float32(info["threshold0"])) == bits(oinfo["thresholds"][0]), (s, info)
        assert np.array_equal(gi, oi), (s, info)
        assert np.array_equal(bits(gv), bits(ov)), s
        assert np.array_equal(bits(host(out)), bits(O.decompress([ov], [oi], N, 1))), s
        branches.append(oinfo["branch"])
    assert np.array_equal(bits(host(b.vec)), bits(v_o))
    assert np.array_equal(bits(host(b.mmt)), bits(m_o))
    assert "resample" not in branches[:2], branches   # steps 2 and 3 masked inside K1


# ----------------------------------------------------------------------------- pointer table
NUMELS = [5, 1023, 1025, 4097, 70001]


def _clip_spec(mode, param):
    import functools
    from dgc import clip_grad as K
    if mode is None:
        return None
    fn = (functools.partial(K.clip_grad_norm_, max_norm=param) if mode == "norm2"
          else functools.partial(K.clip_grad_value_, clip_value=param))
    return K.spec_of(fn)


@pytest.mark.parametrize("mode,param", [(None, 0.0), ("norm2", 0.05), ("value", 0.002)],
                         ids=["unclipped", "clip_grad_norm_", "clamp"])
def test_batch_pointer_table_tails_match_flat_and_oracle(mode, param):
    """DGCBatch over five tensors whose gradients are exact-length, 16-B-aligned slices of
    one NaN-filled buffer — NaN right behind every last element, so a tail read that leaks
    past a gradient's end shows in mmt / vec — against the same batch fed through its flat
    gradient buffer and against the oracle per tensor, three steps."""
    from dgc.batch import DGCBatch
    shapes = [(f"t{i}", (n,)) for i, n in enumerate(NUMELS)]
    T = len(shapes)
    kw = dict(compress_ratio=0.01, momentum=0.9, nesterov=True, device=DEV, seed=5, resample_order="topk")
    a = DGCBatch(shapes, clip=_clip_spec(mode, param), **kw)
    f = DGCBatch(shapes, clip=_clip_spec(mode, param), **kw)
    offs, end = [], 0
    for n in NUMELS:
        offs.append(end)
        end = (end + n + 1 + 3) // 4 * 4   # the next slice 16-B aligned, at least one NaN in between
    buf = torch.full((end + 4,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    ptrs = (ctypes.c_void_p * T)(*[buf.data_ptr() + 4 * o for o in offs])
    attrs = [O.attributes(n, 0.01) for n in NUMELS]
    assert [tuple(x[1:]) for x in attrs] == [tuple(x) for x in a.attrs]
    state = [(np.zeros(n, np.float32), np.zeros(n, np.float32)) for n in NUMELS]
    clipped = 0
    for s in range(3):
        starts = a.draw_starts()
        grads = [synth.gradient(700 + 10 * s + t, n, "normal", 1e-3 * (1 + t)) for t, n in enumerate(NUMELS)]
        for t, (name, _) in enumerate(shapes):
            buf[offs[t]: offs[t] + NUMELS[t]].copy_(to_dev(grads[t]))
            f.grad(name).copy_(to_dev(grads[t]))
        assert bool(torch.isnan(buf[offs[-1] + NUMELS[-1]])) and bool(torch.isnan(buf[offs[0] + NUMELS[0]]))
        a.compensate(starts, grad_ptrs=ptrs)
        a.select()
        f.compress(starts)
        a.exchange()
        f.exchange()
        out_a, out_f = a.decompress(), f.decompress()
        torch.cuda.synchronize()
        sent_a, sent_f, infos = a.transmitted(), f.transmitted(), a.infos()
        assert torch.equal(out_a.view(torch.int32), out_f.view(torch.int32)), s
        coefs = None
        if mode == "norm2":
            assert torch.equal(a.clip_coefs.view(torch.int32), f.clip_coefs.view(torch.int32)), s
            coefs = a.clip_coefs.cpu().numpy()
        for t, (name, _) in enumerate(shapes):
            n, key = NUMELS[t], (mode, s, name)
            c = np.float32(param) if mode == "value" else (coefs[t] if mode == "norm2" else None)
            gc = grads[t] if mode is None else clip_np(grads[t], mode, c)
            clipped += mode is not None and not np.array_equal(bits(gc), bits(grads[t]))
            m_o, v_o = state[t]
            ov, oi, oinfo = O.compress_step(gc, m_o, v_o, attrs[t], starts[t], nesterov=True)
            gv, gi = sent_a[name]
            assert torch.equal(gi, sent_f[name][1]) and torch.equal(gv.view(torch.int32), sent_f[name][0].view(torch.int32)), key
            assert np.array_equal(gi.cpu().numpy(), oi), key
            assert np.array_equal(bits(gv.cpu().numpy()), bits(ov)), key
            assert infos[t]["branch"] == oinfo["branch"], key
            assert bits(np.float32(infos[t]["threshold0"])) == bits(oinfo["thresholds"][0]), key
            o = a.offsets[t]
            assert np.array_equal(bits(host(out_a)[o: o + n]), bits(O.decompress([ov], [oi], n, 1))), key
    # the state after the last step only: the whole flat buffers (padding included) against
    # the flat-fed batch, every tensor against the oracle
    assert torch.equal(a.mmt_flat.view(torch.int32), f.mmt_flat.view(torch.int32))
    assert torch.equal(a.vec_flat.view(torch.int32), f.vec_flat.view(torch.int32))
    for t, (name, _) in enumerate(shapes):
        assert np.array_equal(bits(host(a.momentum_of(name))), bits(state[t][0])), name
        assert np.array_equal(bits(host(a.velocity_of(name))), bits(state[t][1])), name
    assert mode is None or clipped >= 3 * (T - 1)   # the clip really changed the gradients


# ----------------------------------------------------------------------------- spill count
HOT = [3, 130, 131, 400, 517, 700, 901, 1023]   # the "hot" kind's segments, gradient x 2


def _spill_gradient(kind, seed, N):
    if kind == "layered":
        return synth.gradient(seed, N, "layered", 1.0)
    g = synth.gradient(seed, N, "normal", 1.0)
    for h in HOT:
        g[h * SEG: (h + 1) * SEG] *= np.float32(2.0)
    return g


@pytest.mark.parametrize("kind,ratio,seed,steps", [("layered", 0.05, 300, 3), ("hot", 0.01, 800, 5)])
def test_bucket_spill_count_matches_recount(kind, ratio, seed, steps):
    """K1's own spill count — one atomic per spilled wave — against a recount in numpy at the
    list threshold the step reports. It is what overflow_segments reports on a step its lists
    served, and what drops the lists (a full pass) when more than 1/32 of the segments spilled.

    "layered" at ratio 0.05 (the existing bucket test's case): whole 64-segment layers are
    hot, so every spilling step is past that limit and only the drop can be checked. "hot":
    eight segments of a normal gradient doubled, ratio 0.01 — in the oracle's replay their
    lists (and few others') hold more than kCap entries from the third step on while the
    threshold stays above the list threshold, so the lists serve and the count itself is
    compared; the test fails if that comparison never ran."""
    from dgc.bucket import DGCBucket
    N = 1_048_576
    b = DGCBucket(N, compress_ratio=ratio, momentum=0.9, nesterov=True, device=DEV, seed=7, fill="inline")
    attrs = O.attributes(N, ratio)
    m_o, v_o = np.zeros(N, np.float32), np.zeros(N, np.float32)
    rng = random.Random(7)
    out = torch.full((N,), float("nan"), device=DEV)
    spilled_steps = compared = dropped = 0
    for s in range(steps):
        g = _spill_gradient(kind, seed + s, N)
        start = rng.randint(0, attrs[4] - 1) if attrs[0] != attrs[2] else 0
        b.step(to_dev(g), out)
        torch.cuda.synchronize()
        info = b.last_info()
        v_new = O.compensate(g, m_o.copy(), v_o.copy(), 0.9, True)   # what K1 listed from
        ov, oi, oinfo = O.compress_step(g, m_o, v_o, attrs, start, nesterov=True)
        gv, gi = payload_of(b)
        assert info["branch"] == oinfo["branch"], (s, info)
        assert np.array_equal(gi, oi), (s, info)
        assert np.array_equal(bits(gv), bits(ov)), s
        tl = np.float32(info["list_threshold"])
        if np.isfinite(tl):
            per_seg = (np.abs(v_new) >= tl).reshape(-1, SEG).sum(axis=1)
            want = int((per_seg > CAP).sum())
            print(kind, "step", s, "list_threshold", tl, "spilled segments", want, "overflow_segments",
                  info["overflow_segments"], "full_passes", info["full_passes"])
            spilled_steps += want > 0
            if info["full_passes"] == 0:
                assert info["overflow_segments"] == want, (s, info, want)
                compared += want > 0
            if want * 32 > N // SEG:
                assert info["full_passes"] >= 1, (s, info, want)   # too many spilled lists: dropped
                dropped += 1
    assert spilled_steps >= 1
    if kind == "hot":
        assert compared >= 1, "no step compared a non-zero spill count"
    else:
        assert dropped >= 1
    assert np.array_equal(bits(host(b.vec)), bits(v_o)) and np.array_equal(bits(host(b.mmt)), bits(m_o))
