"""DGCBucket on bf16 / fp16 parameters: K1-16 (dgc_compress_begin16: 16-bit state, the
velocity's fp32 image, the strided sample and the candidate lists in one kernel), the pure
selection on the image (dgc_compress_finish), the 16-bit masking from the payload and the
packed 16-bit decompress. Bit for bit against the reference's own 16-bit fixtures
(tests/golden/half.*) and against the torch-CPU port on 16-bit tensors (oracle.torch_cpu,
pinned to the same fixtures by test_half_port.py)."""
import functools
import random

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import torch_cpu as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATIO = 0.01
STEPS = 4
# around the vector width (4), the segment (1024), the workgroup (4096) and the
# 1024-segment group (2^20)
SIZES = [4093, 4096, 4097, 4099, 5 * 4096 + 1021, 70001, 1048576 + 3]
DTYPES = {"bf16": (torch.bfloat16, 1.0), "fp16": (torch.float16, 0.01)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 8: np.uint64}[a.dtype.itemsize])


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dgc import _lib
    return _lib.lib()


def payload_of(b):
    """(values, indices) of the bucket's own payload, exact length."""
    p = b.payload
    n = int(p[:8].view(torch.int64).item())
    vb = torch.empty(0, dtype=b.vdtype).element_size()
    ib = torch.empty(0, dtype=b.idtype).element_size()
    return p[b.voff: b.voff + n * vb].view(b.vdtype), p[b.ioff: b.ioff + n * ib].view(b.idtype)


# ---------------------------------------------------------------- 1. the reference's fixtures
def test_bucket16_against_reference_goldens(L, golden_half):
    """Every case and step of tests/golden/half.*, one DGCBucket per rank, the allgather
    emulated by concatenating the ranks' payloads: indices in the fixture's order
    (resample_order="topk"), values, wire dtype, the 16-bit state's digests, the dense
    output and its digest."""
    from dgc.bucket import DGCBucket
    meta, arrays = golden_half
    assert len(meta) == 11
    for name, case in meta.items():
        dt = getattr(torch, case["dtype"])
        N, W = case["N"], case["W"]
        bs = [DGCBucket(N, compress_ratio=case["ratio"], momentum=0.9, nesterov=case["nesterov"],
                        momentum_masking=case["masking"], resample=case["resample"], fp16_values=case["fp16"],
                        int32_indices=case["int32"], device=DEV, world_size=W, seed=42, dtype=dt) for _ in range(W)]
        assert (N, bs[0].k, bs[0].num_samples, bs[0].top_k_samples, bs[0].stride) == tuple(case["attrs"]), name
        out = torch.empty(N, dtype=dt, device=DEV)
        for s, step in enumerate(case["per_step"]):
            for q, rk in enumerate(step["ranks"]):
                g = torch.from_numpy(synth.gradient(rk["seed"], N, case["kind"], case["scale"]).copy()).to(dt)
                bs[q].compensate(g.to(DEV))
                bs[q].select()
                key = f"{name}/s{s}/r{q}"
                vals, idx = payload_of(bs[q])
                assert vals.dtype == getattr(torch, rk["values_dtype"].split(".")[1]), key
                assert np.array_equal(idx.cpu().numpy(), arrays[key + "/indices"]), key
                assert np.array_equal(bits(vals.float().cpu().numpy()), bits(arrays[key + "/values"])), key
                assert bs[q].mmt.dtype == dt and bs[q].mmt.numel() == N, key
                assert synth.digest(bs[q].mmt.float().cpu().numpy()) == rk["mmt_sha"], key
                assert synth.digest(bs[q].vec.float().cpu().numpy()) == rk["vec_sha"], key
            b0 = bs[0]
            if W > 1:   # the allgather: rank order
                gathered = torch.cat([b.payload for b in bs])
                b0._gathers = [gathered] * len(b0._gathers)
            out.fill_(float("nan"))
            b0.decompress(out)
            got = out.float().cpu().numpy()
            want = np.zeros(N, np.float32)
            want[arrays[f"{name}/s{s}/dec_nz_idx"]] = arrays[f"{name}/s{s}/dec_nz_val"]
            assert np.array_equal(bits(got), bits(want)), (name, s)
            assert synth.digest(got) == step["dense_sha"], (name, s)
        bs[0].last_info()   # raises what the status words hold


# ---------------------------------------------------------------- 2. edges against the torch-CPU port
@functools.lru_cache(maxsize=8)
def gradient32(seed, N, kind, scale):
    return synth.gradient(seed, N, kind, scale)


def oracle_branch(vec, attrs, start, upper=1.3, lower=0.8, max_iters=10):
    """The path oracle.torch_cpu.sparsify takes on ``vec`` — the same comparisons on the
    same 16-bit tensors — as (threshold0, [steps]): "lower" / "raise" for every threshold
    move, then "resample", "trunc" (more than k kept, cut to k), "ok" or "exhausted"."""
    numel, k, S, ks, stride = attrs
    imp = vec.view(-1).abs()
    samples = imp if numel == S else imp[start::stride]
    thr = torch.topk(samples, ks, 0, largest=True, sorted=False)[0].min()
    thr0 = thr.clone()
    n = int(torch.ge(imp, thr).sum())
    trace = []
    if numel > S:
        for _ in range(max_iters):
            if n > k:
                if n > k * upper:
                    trace.append("resample")
                    return thr0, trace
                trace.append("trunc")
                return thr0, trace
            elif n < lower * k:
                thr = thr * lower
                trace.append("lower")
            else:
                trace.append("ok")
                return thr0, trace
            n = int(torch.ge(imp, thr).sum())
        trace.append("exhausted")
        return thr0, trace
    trace.append("trunc" if n > k else "ok")
    return thr0, trace


_traces = {}   # (N, kind, dtype name, nesterov) -> the oracle's branch trace of every step


def oracle_steps(N, kind, dname, nesterov):
    """The torch-CPU port on 16-bit tensors, step by step (seed 11's sample starts): yields
    what the bucket must reproduce; its branch traces are kept in ``_traces``."""
    dt, scale = DTYPES[dname]
    attrs = TC.attributes(N, RATIO)
    rng = random.Random(11)
    m_ref, v_ref = torch.zeros(N, dtype=dt), torch.zeros(N, dtype=dt)
    traces = []
    for s in range(STEPS):
        g = torch.from_numpy(gradient32(500 + s, N, kind, scale)).to(dt)
        start = rng.randint(0, attrs[4] - 1) if N != attrs[2] else 0
        TC.compensate(g, m_ref, v_ref, 0.9, nesterov)
        thr0, trace = oracle_branch(v_ref, attrs, start)
        traces.append(tuple(trace))
        want_v, want_i = TC.sparsify(v_ref, *attrs, start)
        want_v, want_i = want_v.clone(), want_i.clone()
        image = v_ref.float().clone()   # before the masking: what the selection read
        TC.update(m_ref, v_ref, want_i)
        want_out = TC.decompress(want_v, want_i, torch.empty(N, dtype=dt), 1)
        yield dict(g=g, start=start, thr0=thr0, trace=trace, values=want_v, indices=want_i, image=image, mmt=m_ref,
                   vec=v_ref, out=want_out)
    _traces[(N, kind, dname, nesterov)] = traces


@pytest.mark.parametrize("nesterov", [True, False], ids=["nest", "plain"])
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("N", SIZES)
def test_bucket16_edges_against_torch_cpu(L, N, kind, dname, nesterov):
    """Four steps per case. The gradient is the first N elements of a longer tensor whose
    rest is NaN, and the output is NaN-filled before each step: an element past N that is
    used, or an output element that is not written, shows up. Bit for bit per step:
    threshold0, indices in order, values, the 16-bit momentum and velocity, the image
    (the emitted values at the emitted indices — the selection is pure — and vec elsewhere)
    and the dense output."""
    from dgc.bucket import DGCBucket
    dt, scale = DTYPES[dname]
    b = DGCBucket(N, compress_ratio=RATIO, momentum=0.9, nesterov=nesterov, device=DEV, world_size=1, seed=11,
                  dtype=dt)
    attrs = TC.attributes(N, RATIO)
    assert attrs == (N, b.k, b.num_samples, b.top_k_samples, b.stride)
    full = torch.full((N + 1024 + 5,), float("nan"), dtype=dt, device=DEV)
    out = torch.empty(N, dtype=dt, device=DEV)
    for s, o in enumerate(oracle_steps(N, kind, dname, nesterov)):
        g, start, thr0, trace = o["g"], o["start"], o["thr0"], o["trace"]
        want_v, want_i, image, m_ref, v_ref, want_out = (o[k] for k in ("values", "indices", "image", "mmt", "vec",
                                                                        "out"))
        # the bucket
        full[:N].copy_(g.to(DEV))
        out.fill_(float("nan"))
        b.step(full[:N], out)
        key = (N, kind, dname, nesterov, s, trace)
        info = b.last_info()
        assert np.float32(info["threshold0"]).view(np.uint32) == np.float32(thr0.float().item()).view(np.uint32), key
        assert b.start == start, key
        vals, idx = payload_of(b)
        assert vals.dtype == dt and idx.dtype == torch.int64, key
        assert np.array_equal(idx.cpu().numpy(), want_i.numpy()), key
        assert np.array_equal(bits16(vals), bits16(want_v)), key
        assert np.array_equal(bits16(b.mmt), bits16(m_ref)), key
        assert np.array_equal(bits16(b.vec), bits16(v_ref)), key
        img = b._vec32[:N].cpu()
        assert np.array_equal(bits(img.numpy()), bits(image.numpy())), key
        assert np.array_equal(bits(img[want_i].numpy()), bits(want_v.float().numpy())), key
        rest = torch.ones(N, dtype=torch.bool)
        rest[want_i] = False
        assert np.array_equal(bits(img[rest].numpy()), bits(b.vec.float().cpu()[rest].numpy())), key
        assert not b._vec32[N:].any() and not b._mmt[N:].any() and not b._vec[N:].any(), key   # padding stays +0
        assert np.array_equal(bits16(out), bits16(want_out)), key


def test_bucket16_edge_cases_cover_the_branches():
    """A condition on the cases above, not a measurement: over them the oracle's own path
    contains trunc, ok, resample and a lowering followed by resample, for each dtype.
    (The traces are the ones the edge tests left; a case that has not run is run here.)"""
    for dname in DTYPES:
        seen = set()
        for N in SIZES:
            for kind in ("normal", "ties"):
                for nesterov in (True, False):
                    case = (N, kind, dname, nesterov)
                    if case not in _traces:
                        for _ in oracle_steps(*case):
                            pass
                    assert len(_traces[case]) == STEPS
                    seen.update(_traces[case])
        for need in (("trunc",), ("ok",), ("resample",)):
            assert need in seen, (dname, need, sorted(seen))
        assert any(t[0] == "lower" and t[-1] == "resample" for t in seen), (dname, sorted(seen))


# ---------------------------------------------------------------- 3. the lists served a step
@pytest.mark.parametrize("dname", list(DTYPES))
def test_bucket16_lists_serve_a_step(L, dname):
    """K1-16's candidate lists are used: some step selects with no full pass over the image
    at a finite list threshold. (Without this a K1-16 that wrote wrong lists would hide
    behind the full-pass fallback; the indices of such steps are checked above.)"""
    from dgc.bucket import DGCBucket
    dt, scale = DTYPES[dname]
    N = 1048576 + 3
    b = DGCBucket(N, compress_ratio=RATIO, momentum=0.9, nesterov=True, device=DEV, world_size=1, seed=11, dtype=dt)
    out = torch.empty(N, dtype=dt, device=DEV)
    infos = []
    for s in range(STEPS):
        g = torch.from_numpy(gradient32(500 + s, N, "normal", scale)).to(dt).to(DEV)
        b.step(g, out)
        infos.append(b.last_info())
        print(dname, s, {k: infos[-1][k] for k in ("branch", "full_passes", "list_threshold", "threshold",
                                                   "overflow_segments")})
    assert any(i["full_passes"] == 0 and np.isfinite(i["list_threshold"]) for i in infos), infos


# ---------------------------------------------------------------- 4. guards
def test_bucket16_guards(L):
    from dgc.bucket import DGCBucket
    N = 5000
    b = DGCBucket(N, compress_ratio=RATIO, device=DEV, world_size=1, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bfloat16"):
        b.compensate(torch.zeros(N, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        b.compensate(torch.zeros(N + 8, dtype=torch.bfloat16, device=DEV)[1:N + 1])   # not 16-B aligned
    with pytest.raises(ValueError):
        b.compensate(torch.zeros(N + 1, dtype=torch.bfloat16, device=DEV))
    for fill in ("sparse", "allgather"):
        with pytest.raises(NotImplementedError, match=fill):
            DGCBucket(N, device=DEV, world_size=1, dtype=torch.float16, fill=fill)
    g = torch.from_numpy(gradient32(500, N, "normal", 1.0)).to(torch.bfloat16).to(DEV)
    b.step(g, torch.empty(N, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(ValueError, match="bfloat16"):
        b.decompress(torch.empty(N, dtype=torch.float32, device=DEV))
    with pytest.raises(NotImplementedError, match="dense=False"):
        b.decompress(torch.empty(N, dtype=torch.bfloat16, device=DEV), dense=False)
    with pytest.raises(NotImplementedError, match="float64"):
        DGCBucket(N, device=DEV, world_size=1, dtype=torch.float64)
    b.flush()   # a no-op: nothing is ever deferred
    assert b.mmt.numel() == N and b.vec.dtype == torch.bfloat16
