"""Native local gradient clipping on bf16 / fp16 state: K0-16 (dgc_grad_stats16,
dgc_clip_coefs16) and the clip in K1-16's load — the per-tensor path
(dgc_compensate16_clip), DGCBatch (dgc_compensate16_multi_clip) and DGCBucket
(dgc_compress_begin16_clip; dgc_compress_begin_clip for fp32). Bit for bit against the
reference's own fixtures (tests/golden/clip16.*, clip.*) and against the written-out port
(tests/clip16_port.py + oracle/torch_cpu.py), which test_clip16_port.py pins to the same
fixtures."""
import contextlib
import ctypes
import functools
import io
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import clip16_port as P
from conftest import GOLDEN
from oracle import synth
from oracle import torch_cpu as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DSCALE = {"bf16": 1.0, "fp16": 0.01}
NORM2, ABSMAX = 1, 2
MODES = ("norm2", "norminf", "value")
KIND = {"norm2": NORM2, "norminf": ABSMAX}


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden_clip16():
    with open(os.path.join(GOLDEN, "clip16.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "clip16.npz"))


@pytest.fixture(scope="module")
def golden_clip():
    with open(os.path.join(GOLDEN, "clip.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "clip.npz"))


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 8: np.uint64}[a.dtype.itemsize])


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def fbits(t):
    """fp32 bit patterns of a float tensor, every NaN as one pattern (P.canon)."""
    return [P.canon(int(b)) for b in bits(t.detach().float().cpu().numpy().reshape(-1))]


def clip_fn(mode, param):
    from dgc import clip_grad as K
    if mode == "norm2":
        return functools.partial(K.clip_grad_norm_, max_norm=param)
    if mode == "norminf":
        return functools.partial(K.clip_grad_norm_, max_norm=param, norm_type=math.inf)
    return functools.partial(K.clip_grad_value_, clip_value=param)


@functools.lru_cache(maxsize=16)
def gradient32(seed, N, kind, scale):
    return synth.gradient(seed, N, kind, scale)


def case_gradient(meta, case, s):
    st = case["per_step"][s]
    g = torch.from_numpy(gradient32(st["seed"], case["N"], "normal", st["scale"]).copy())
    if "dtype" in case:
        g = g.to(DT[case["dtype"]])
    if case.get("poison") and s == 0:
        g[meta["poison"]["nan"]], g[meta["poison"]["inf"]] = float("nan"), float("inf")
    return g


# ------------------------------------------------------------------ 1. statistics
def stats16(tensors, kind):
    from dgc import _lib
    L = _lib.lib()
    T = len(tensors)
    ptrs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in tensors])
    nums = (ctypes.c_int64 * T)(*[t.numel() for t in tensors])
    wsz = L.dgc_grad_stats_workspace(nums, T)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    out = torch.full((T,), -7.0, device=DEV)
    _lib.check(L.dgc_grad_stats16(ptrs, nums, T, kind, _lib.VD[tensors[0].dtype], _lib.ptr(out), _lib.ptr(ws), wsz,
                                  _lib.stream_of(DEV)), "dgc_grad_stats16")
    return out.cpu()


def stats32(tensors, kind):
    from dgc import _lib
    L = _lib.lib()
    T = len(tensors)
    ptrs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in tensors])
    nums = (ctypes.c_int64 * T)(*[t.numel() for t in tensors])
    wsz = L.dgc_grad_stats_workspace(nums, T)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    out = torch.full((T,), -7.0, device=DEV)
    _lib.check(L.dgc_grad_stats(ptrs, nums, T, kind, 0, _lib.ptr(out), _lib.ptr(ws), wsz, _lib.stream_of(DEV)),
               "dgc_grad_stats")
    return out.cpu()


STAT_SIZES = [1, 3, 4, 1023, 1024, 4095, 4096, 4097, 70001, 2 ** 20 + 3]


def at_offset(x, off):
    """x's elements at element offset `off` of a fresh 16-B aligned buffer whose other elements
    are NaN: a read outside the tensor shows in the statistic."""
    buf = torch.full((x.numel() + 16,), float("nan"), dtype=x.dtype, device=DEV)
    buf[off: off + x.numel()].copy_(x)
    v = buf[off: off + x.numel()]
    assert v.data_ptr() % 8 == 2 * off
    return v


@pytest.mark.parametrize("dname", list(DT))
def test_stats16_equal_the_rounded_fp32_statistic(dname):
    """dgc_grad_stats16(x) is the dtype rounding of dgc_grad_stats(x.float()) for both kinds,
    every size, at an 8-B aligned pointer and at one that is only 2-B aligned, alone and in a
    table of 70 tensors (two launch pairs)."""
    dt = DT[dname]
    xs = [torch.from_numpy(gradient32(700 + i, n, "normal", (0.5 + i) * DSCALE[dname]).copy()).to(dt).to(DEV)
          for i, n in enumerate(STAT_SIZES)]
    wide = [x.float() for x in xs]
    for kind in (NORM2, ABSMAX):
        want = P.rdt(stats32(wide, kind), dt)
        for off in (0, 1):
            placed = [at_offset(x, off) for x in xs]
            alone = torch.cat([stats16([x], kind) for x in placed])
            assert fbits(alone) == fbits(want), (dname, kind, off)
            # 70 tensors: the ten sizes seven times over, at alternating alignments
            table = [placed[i % len(xs)] if (i // len(xs)) % 2 == 0 else xs[i % len(xs)] for i in range(70)]
            got = stats16(table, kind)
            assert fbits(got) == fbits(want.repeat(7)), (dname, kind, off)
        # and it is what the port computes (float64 sum, rounded to fp32, then to the dtype)
        port = torch.stack([P.total_norm(x.cpu(), "norm2" if kind == NORM2 else "norminf") for x in xs])
        assert fbits(want) == fbits(port), (dname, kind)


@pytest.mark.parametrize("dname", list(DT))
def test_stats16_nan_and_overflow(dname):
    dt = DT[dname]
    x = torch.from_numpy(gradient32(799, 5000, "normal", 1.0).copy()).to(dt)
    x[17] = float("nan")
    x[4100] = float("inf")
    for kind in (NORM2, ABSMAX):
        assert math.isnan(float(stats16([x.to(DEV)], kind)[0]))
    x[17] = 0
    for kind in (NORM2, ABSMAX):
        assert float(stats16([x.to(DEV)], kind)[0]) == math.inf
    if dname == "fp16":   # finite elements, a norm above 65504: inf in fp16, as the reference's norm is
        big = torch.full((4097,), 2000.0, dtype=dt, device=DEV)
        assert float(stats16([big], NORM2)[0]) == math.inf
        assert float(stats16([big], ABSMAX)[0]) == 2000.0


def coefs16(stats, max_norm, dt):
    from dgc import _lib
    s = stats.to(DEV).float().contiguous()
    out = torch.empty_like(s)
    _lib.check(_lib.lib().dgc_clip_coefs16(_lib.ptr(s), s.numel(), max_norm, _lib.VD[dt], _lib.ptr(out),
                                           _lib.stream_of(DEV)), "dgc_clip_coefs16")
    return out.cpu()


def test_stats16_and_coefs16_equal_the_fixtures(golden_clip16):
    """The reference's total_norm from its input, and its coefficient from its norm."""
    meta, _ = golden_clip16
    n = 0
    for name, case in meta["cases"].items():
        if case["mode"] == "value":
            continue
        dt = DT[case["dtype"]]
        for s, st in enumerate(case["per_step"]):
            g = case_gradient(meta, case, s).to(DEV)
            total = stats16([g], KIND[case["mode"]])
            assert fbits(total) == [P.canon(st["total_norm_bits"])], (name, s)
            ref_norm = torch.from_numpy(np.array([st["total_norm_bits"]], np.uint32).view(np.float32).copy())
            assert fbits(coefs16(ref_norm, case["param"], dt)) == [P.canon(st["coef_bits"])], (name, s)
            n += 1
    assert n >= 40


@pytest.mark.parametrize("dname", list(DT))
def test_coefs16_edge_norms_equal_the_port(dname):
    dt = DT[dname]
    norms = torch.tensor([0.0, math.inf, math.nan, 1.0, 3.0, 1e-6, 65504.0 if dname == "fp16" else 1e30, 0.3333])
    norms = P.rdt(norms, dt)
    for max_norm in (1.0, 2.5, 0.01, 15.811):
        got = coefs16(norms, max_norm, dt)
        want = torch.stack([P.coefficient(x, max_norm, dt) for x in norms])
        assert fbits(got) == fbits(want), (dname, max_norm)


# ------------------------------------------------------------------ 3. per-tensor path
def make_pair(case, dt):
    from dgc.compression import DGCCompressor
    from dgc.memory import DGCSGDMemory
    mem = DGCSGDMemory(momentum=0.9, nesterov=case["nesterov"], gradient_clipping=clip_fn(case["mode"], case["param"]))
    comp = quiet(DGCCompressor, case.get("ratio", 0.01), memory=mem)
    p = torch.zeros(case["N"], dtype=dt, device=DEV)
    quiet(mem.initialize, [("w", p)])
    quiet(comp.initialize, [("w", p)])
    return mem, comp


def test_per_tensor_path_equals_the_fixtures(golden_clip16):
    """DGCSGDMemory(gradient_clipping=partial(...)) + DGCCompressor on a 16-bit parameter:
    every tensor case and step — the coefficient, the indices in order, the values, the
    state's digests (the state in full for N = 1000) — and the gradient left as it was."""
    meta, arr = golden_clip16
    for name, case in meta["cases"].items():
        if case["kind"] != "tensor":
            continue
        dt = DT[case["dtype"]]
        mem, comp = make_pair(case, dt)
        assert mem.clip_spec().fusable(dt)
        random.seed(42)
        for s, st in enumerate(case["per_step"]):
            key = f"{name}/s{s}"
            g = case_gradient(meta, case, s).to(DEV)
            keep = g.clone()
            (vals, idx), _ = comp.compress(g, "w")
            assert np.array_equal(bits16(g), bits16(keep)), key
            if case["mode"] == "value":
                assert mem.last_clip_coef is None
            else:
                assert fbits(mem.last_clip_coef) == [P.canon(st["coef_bits"])], key
            assert vals.dtype == dt
            assert np.array_equal(idx.view(-1).cpu().numpy(), arr[key + "/indices"]), key
            assert np.array_equal(bits(vals.view(-1).float().cpu().numpy()), bits(arr[key + "/values"])), key
            m, v = P.image(mem.momentums["w"]), P.image(mem.velocities["w"])
            assert synth.digest(m) == st["mmt_sha"] and synth.digest(v) == st["vec_sha"], key
            if key + "/mmt" in arr:
                assert np.array_equal(bits(m), bits(arr[key + "/mmt"])), key
                assert np.array_equal(bits(v), bits(arr[key + "/vec"])), key


def test_dense_compensate_equals_the_fixtures(golden_clip16):
    from dgc.memory import DGCSGDMemory
    meta, arr = golden_clip16
    for name, case in meta["cases"].items():
        if case["kind"] != "dense":
            continue
        dt = DT[case["dtype"]]
        mem = DGCSGDMemory(momentum=0.9, nesterov=case["nesterov"],
                           gradient_clipping=clip_fn(case["mode"], case["param"]))
        quiet(mem.initialize, [("b", torch.zeros(case["N"], dtype=dt, device=DEV))])
        for s, st in enumerate(case["per_step"]):
            key = f"{name}/s{s}"
            g = case_gradient(meta, case, s).to(DEV)
            keep = g.clone()
            out = mem.compensate(g, "b", accumulate=False)
            assert np.array_equal(bits16(g), bits16(keep)), key
            if case["mode"] != "value":
                assert fbits(mem.last_clip_coef) == [P.canon(st["coef_bits"])], key
            assert out.dtype == dt
            assert np.array_equal(bits(P.image(out)), bits(arr[key + "/out"])), key
            assert np.array_equal(bits(P.image(mem.momentums["b"])), bits(arr[key + "/mmt"])), key


# ------------------------------------------------------------------ 4. DGCBatch(dtype, clip)
BATCH_PARAM = {"norm2": 30.0, "norminf": 2.5, "value": 1.5}


def batch_against_singles(shapes, dname, mode, from_ptrs, steps=3):
    from dgc import clip_grad as K
    from dgc.batch import DGCBatch
    from dgc.compression import DGCCompressor
    from dgc.memory import DGCSGDMemory
    dt, ds = DT[dname], DSCALE[dname]
    fn = clip_fn(mode, BATCH_PARAM[mode] * ds)
    b = DGCBatch(shapes, compress_ratio=0.01, momentum=0.9, nesterov=True, device=DEV, seed=42, dtype=dt,
                 resample_order="topk", clip=K.spec_of(fn), world_size=1)
    T = len(shapes)
    mem = DGCSGDMemory(momentum=0.9, nesterov=True, gradient_clipping=fn)
    comp = quiet(DGCCompressor, 0.01, memory=mem)
    params = [(n, torch.zeros(shp, dtype=dt, device=DEV)) for n, shp in shapes]
    quiet(mem.initialize, params)
    quiet(comp.initialize, params)
    for s in range(steps):
        starts = b.draw_starts()
        scale = (1.0, 0.1, 2.0)[s % 3] * ds
        grads = [torch.from_numpy(gradient32(1300 + 10 * s + (t % 7), b.numels[t], "normal", scale * (1 + t % 3))
                                  .copy()).to(dt).to(DEV) for t in range(T)]
        if from_ptrs:
            b.grad_flat.fill_(float("nan"))   # must be overwritten by the gather where it is read
            for t in range(T):                 # (the padding between tensors holds +0 gradients)
                end = b.offsets[t] + b.numels[t]
                b.grad_flat[end: -(-end // 1024) * 1024].zero_()
            b.compensate(starts, (ctypes.c_void_p * T)(*[g.data_ptr() for g in grads]))
        else:
            for t, (n, _) in enumerate(shapes):
                b.grad(n).copy_(grads[t].view(b.shapes[n]))
            b.compensate(starts)
        b.select()
        out = b.decompress()
        torch.cuda.synchronize()
        sent = b.transmitted()
        for t, (n, shp) in enumerate(shapes):
            key = (dname, mode, from_ptrs, s, n)
            comp._sample_start = lambda name, st=starts[t]: st
            (vals, idx), ctx = comp.compress(grads[t].view(shp), n)
            gv, gi = sent[n]
            order = torch.argsort(idx.view(-1))
            gorder = torch.argsort(gi)
            assert torch.equal(gi[gorder], idx.view(-1)[order]), key
            assert np.array_equal(bits16(gv[gorder]), bits16(vals.view(-1)[order])), key
            assert np.array_equal(bits16(b.momentum_of(n)), bits16(mem.momentums[n])), key
            assert np.array_equal(bits16(b.velocity_of(n)), bits16(mem.velocities[n])), key
            if mode != "value":
                assert fbits(b.clip_coefs[t: t + 1]) == fbits(mem.last_clip_coef), key
            dense = comp.decompress((vals, idx), ctx)
            assert np.array_equal(bits16(b.out(n)), bits16(dense)), key
    assert not b._vec32.isnan().any() and out.numel() == b.flat_numel


@pytest.mark.parametrize("from_ptrs", [False, True], ids=["flat", "ptrs"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dname", list(DT))
def test_batch16_with_clip_equals_per_tensor(dname, mode, from_ptrs):
    shapes = [("a", (1000,)), ("b", (4097,)), ("c", (70001,)), ("d", (5 * 4096 + 1021,))]
    batch_against_singles(shapes, dname, mode, from_ptrs)


@pytest.mark.parametrize("from_ptrs", [False, True], ids=["flat", "ptrs"])
@pytest.mark.parametrize("dname", list(DT))
def test_batch16_with_clip_70_small_tensors(dname, from_ptrs):
    """More tensors than one launch's table holds (64); three steps, every mode once."""
    shapes = [(f"t{i}", (600 + 37 * i,)) for i in range(70)]
    batch_against_singles(shapes, dname, "norm2" if from_ptrs else "norminf", from_ptrs)


@pytest.mark.parametrize("nesterov", [True, False], ids=["nest", "plain"])
@pytest.mark.parametrize("dname", list(DT))
def test_compensate16_multi_clip_none_is_compensate16(dname, nesterov):
    """dgc_compensate16_multi_clip with DGC_CLIP_NONE over 70 tensors of a flat buffer equals
    dgc_compensate16 over the whole buffer on the tensors' elements, and leaves the padding
    between the tensors (here NaN gradients over +0 state) untouched."""
    from dgc import _lib
    L, st, dt = _lib.lib(), _lib.stream_of(DEV), DT[dname]
    numels = [1 + 611 * i for i in range(70)]
    offs, end = [], 0
    for n in numels:
        offs.append(end)
        end += -(-n // 1024) * 1024
    own = torch.zeros(end, dtype=torch.bool)
    for n, o in zip(numels, offs):
        own[o: o + n] = True
    own = own.to(DEV)
    g = torch.from_numpy(gradient32(1500, end, "normal", DSCALE[dname]).copy()).to(dt).to(DEV)
    state = [torch.from_numpy(gradient32(1501 + i, end, "normal", DSCALE[dname]).copy()).to(dt).to(DEV) for i in (0, 1)]
    m1, v1 = (x.clone() for x in state)
    i1 = torch.zeros(end, device=DEV)
    _lib.check(L.dgc_compensate16(_lib.ptr(g), _lib.ptr(m1), _lib.ptr(v1), None, _lib.ptr(i1), end, 0.9, int(nesterov),
                                  1, _lib.VD[dt], st), "dgc_compensate16")
    g2 = torch.where(own, g, torch.full_like(g, float("nan")))
    m2, v2 = (torch.where(own, x, torch.zeros_like(x)) for x in state)
    i2 = torch.zeros(end, device=DEV)
    ns, os_ = (ctypes.c_int64 * 70)(*numels), (ctypes.c_int64 * 70)(*offs)
    _lib.check(L.dgc_compensate16_multi_clip(_lib.ptr(g2), _lib.ptr(m2), _lib.ptr(v2), _lib.ptr(i2), ns, os_, 70, end,
                                             0.9, int(nesterov), _lib.VD[dt], 0, None, 0.0, st),
               "dgc_compensate16_multi_clip")
    for a, b in ((m1, m2), (v1, v2)):
        assert torch.equal(a.view(torch.int16)[own], b.view(torch.int16)[own])
        assert not b.view(torch.int16)[~own].any()
    assert torch.equal(i1.view(torch.int32)[own], i2.view(torch.int32)[own]) and not i2[~own].any()


# ------------------------------------------------------------------ 5. DGCBucket(clip=)
def payload_of(b):
    p = b.payload
    n = int(p[:8].view(torch.int64).item())
    vb = torch.empty(0, dtype=b.vdtype).element_size()
    ib = torch.empty(0, dtype=b.idtype).element_size()
    return p[b.voff: b.voff + n * vb].view(b.vdtype), p[b.ioff: b.ioff + n * ib].view(b.idtype)


def norm2_coef_candidates(g, param):
    """The fp32 norm-2 coefficients K0 may give: the reference's arithmetic on the float64 norm
    rounded to fp32 and on its two fp32 neighbours (K0's fixed-order fp64 sum is within 1 ulp)."""
    F = np.float32
    n64 = F(math.sqrt(float(np.sum(g.astype(np.float64) ** 2))))
    return [int(bits(F(F(1) / F(x + F(1e-6))) * F(param))[0])
            for x in (np.nextafter(n64, F(0)), n64, np.nextafter(n64, F(np.inf)))]


@pytest.mark.parametrize("which", ["fp32", "16bit"])
def test_bucket_clip_equals_the_fixtures(which, golden_clip, golden_clip16):
    """Every tensor case and step of clip.* (fp32) / clip16.* through DGCBucket(clip=...).
    16-bit, and fp32's norm-inf and clamp: the coefficient's bits, the indices in order, the
    values and the state's digests are the fixture's. fp32 norm-2 has no fixed answer in the
    reference (torch's fp32 accumulation; K0 sums in fp64 in a fixed order), so there every step
    holds the coefficient to the reference's arithmetic on the float64 norm or one of its two
    fp32 neighbours, and is the fixture's bit for bit as long as the coefficients have agreed.
    Every fp32 step of every mode is also bit for bit the per-tensor path's (DGCSGDMemory +
    DGCCompressor with the same clip and sample start): coefficient, payload and state."""
    from dgc.bucket import DGCBucket
    meta, arr = golden_clip if which == "fp32" else golden_clip16
    ran = on_fixture = 0
    for name, case in meta["cases"].items():
        if case["kind"] != "tensor":
            continue
        fp32 = which == "fp32"
        dt = torch.float32 if fp32 else DT[case["dtype"]]
        b = DGCBucket(case["N"], compress_ratio=case["ratio"], momentum=0.9, nesterov=case["nesterov"], device=DEV,
                      world_size=1, seed=42, dtype=dt, clip=clip_fn(case["mode"], case["param"]))
        assert [case["N"], b.k, b.num_samples, b.top_k_samples, b.stride] == case["attrs"], name
        mem, comp = make_pair(case, dt) if fp32 else (None, None)
        fixture = True   # the state is still on the fixture's path
        for s, st in enumerate(case["per_step"]):
            key = f"{name}/s{s}"
            g = case_gradient(meta, case, s)
            host = g.numpy().copy() if fp32 else None
            g = g.to(DEV)
            keep = g.clone()
            b.compensate(g)
            if st["start"] is not None:
                assert b.start == st["start"], key
            if case["mode"] == "value":
                assert b.clip_coef is None
            elif fp32 and case["mode"] == "norm2":
                got = fbits(b.clip_coef)[0]
                if case["poison"] and s == 0:
                    assert got == 0x7FC00000, key
                else:
                    assert got in norm2_coef_candidates(host, case["param"]), (key, got)
                fixture = fixture and got == P.canon(st["coef_bits"])
            else:
                assert fbits(b.clip_coef) == [P.canon(st["coef_bits"])], key
            b.select()
            vals, idx = payload_of(b)
            assert torch.equal(g.view(torch.uint8), keep.view(torch.uint8)), key
            if fp32:   # the per-tensor path on the same input with the bucket's sample start
                comp._sample_start = lambda _name, start=b.start: start
                (pv, pi), _ = comp.compress(g.clone(), "w")
                if case["mode"] != "value":
                    assert fbits(mem.last_clip_coef) == fbits(b.clip_coef), key
                assert torch.equal(idx, pi.view(-1)), key
                assert torch.equal(vals.view(torch.int32), pv.view(-1).view(torch.int32)), key
                assert torch.equal(b.mmt.view(torch.int32), mem.momentums["w"].view(torch.int32)), key
                assert torch.equal(b.vec.view(torch.int32), mem.velocities["w"].view(torch.int32)), key
            ran += 1
            if not fixture:
                continue
            assert np.array_equal(idx.cpu().numpy(), arr[key + "/indices"]), key
            assert np.array_equal(bits(vals.float().cpu().numpy()), bits(arr[key + "/values"])), key
            # (clip16.* stores every NaN of the state as one pattern; clip.* the fp32 bits as they are)
            img = (lambda t: t.cpu().numpy()) if fp32 else P.image
            assert synth.digest(img(b.mmt)) == st["mmt_sha"], key
            assert synth.digest(img(b.vec)) == st["vec_sha"], key
            on_fixture += 1
        b.last_info()
    print(which, "steps:", ran, "of them on the fixture's path:", on_fixture)
    # every step of every case ran; off the fixture's path only fp32 norm-2 steps can be
    assert ran == (68 if which == "16bit" else 33), ran
    assert on_fixture >= (68 if which == "16bit" else 22), on_fixture


BUCKET_SIZES = [4093, 4096, 4097, 4099, 5 * 4096 + 1021, 70001, 1048576 + 3]   # test_gpu_bucket16.SIZES


@pytest.mark.parametrize("dname", list(DT))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", BUCKET_SIZES)
def test_bucket16_clip_edges_against_the_port(N, mode, dname):
    """Two steps per case against clip16_port + oracle.torch_cpu. The gradient is the first N
    elements of a longer tensor whose rest is NaN, the output is NaN-filled: an element past N
    that is used, or an output element that is not written, shows up. Per step: the
    coefficient, indices in order, values, 16-bit state, image, padding +0, dense output."""
    from dgc.bucket import DGCBucket
    dt, ds = DT[dname], DSCALE[dname]
    param = {"norm2": round(math.sqrt(N) / 2, 3), "norminf": 2.5, "value": 1.5}[mode] * ds
    b = DGCBucket(N, compress_ratio=0.01, momentum=0.9, nesterov=True, device=DEV, world_size=1, seed=11, dtype=dt,
                  clip=clip_fn(mode, param))
    attrs = TC.attributes(N, 0.01)
    rng = random.Random(11)
    m_ref, v_ref = torch.zeros(N, dtype=dt), torch.zeros(N, dtype=dt)
    full = torch.full((N + 1024 + 5,), float("nan"), dtype=dt, device=DEV)
    out = torch.empty(N, dtype=dt, device=DEV)
    served = []
    for s in range(2):
        g = torch.from_numpy(gradient32(500 + s, N, "normal", (1.0, 0.1)[s] * ds)).to(dt)
        start = rng.randint(0, attrs[4] - 1) if N != attrs[2] else 0
        gc, total, coef = P.clip(g, mode, param)
        TC.compensate(gc, m_ref, v_ref, 0.9, True)
        want_v, want_i = TC.sparsify(v_ref, *attrs, start)
        want_v, want_i = want_v.clone(), want_i.clone()
        image = v_ref.float().clone()
        TC.update(m_ref, v_ref, want_i)
        want_out = TC.decompress(want_v, want_i, torch.empty(N, dtype=dt), 1)
        full[:N].copy_(g.to(DEV))
        out.fill_(float("nan"))
        b.step(full[:N], out)
        key = (N, mode, dname, s)
        info = b.last_info()
        served.append(info["full_passes"] == 0 and np.isfinite(info["list_threshold"]))
        assert b.start == start, key
        if mode != "value":
            assert fbits(b.clip_coef) == [P.f32_bits(coef)], key
        assert np.array_equal(bits16(full[:N]), bits16(g)), key
        vals, idx = payload_of(b)
        assert np.array_equal(idx.cpu().numpy(), want_i.numpy()), key
        assert np.array_equal(bits16(vals), bits16(want_v)), key
        assert np.array_equal(bits16(b.mmt), bits16(m_ref)), key
        assert np.array_equal(bits16(b.vec), bits16(v_ref)), key
        assert np.array_equal(bits(b._vec32[:N].cpu().numpy()), bits(image.numpy())), key
        assert not b._vec32[N:].any() and not b._mmt[N:].any() and not b._vec[N:].any(), key
        assert np.array_equal(bits16(out), bits16(want_out)), key
    print(N, mode, dname, "served from the lists:", served)


@pytest.mark.parametrize("dname", list(DT))
def test_bucket16_clip_step_served_from_the_lists(dname):
    """The clipped K1-16's candidate lists are used: some step selects with no full pass."""
    from dgc.bucket import DGCBucket
    dt, ds = DT[dname], DSCALE[dname]
    N = 1048576 + 3
    b = DGCBucket(N, compress_ratio=0.01, momentum=0.9, nesterov=True, device=DEV, world_size=1, seed=11, dtype=dt,
                  clip=clip_fn("norm2", 300.0 * ds))
    out = torch.empty(N, dtype=dt, device=DEV)
    infos = []
    for s in range(4):
        b.step(torch.from_numpy(gradient32(500 + s, N, "normal", ds)).to(dt).to(DEV), out)
        infos.append(b.last_info())
    assert float(b.clip_coef[0]) < 1
    assert any(i["full_passes"] == 0 and np.isfinite(i["list_threshold"]) for i in infos), infos


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_bucket_clip_none_is_the_bucket_without_the_argument(dt):
    from dgc.bucket import DGCBucket
    N = 70001
    kw = dict(compress_ratio=0.01, momentum=0.9, nesterov=True, device=DEV, world_size=1, seed=3, dtype=dt)
    a, b = DGCBucket(N, **kw), DGCBucket(N, clip=None, **kw)
    oa, ob = torch.empty(N, dtype=dt, device=DEV), torch.empty(N, dtype=dt, device=DEV)
    for s in range(3):
        g = torch.from_numpy(gradient32(600 + s, N, "normal", 0.01)).to(dt).to(DEV)
        a.step(g, oa)
        b.step(g, ob)
        assert b.clip_coef is None
        assert torch.equal(a.payload, b.payload) and torch.equal(oa.view(torch.uint8), ob.view(torch.uint8)), s
        assert torch.equal(a.mmt.view(torch.uint8), b.mmt.view(torch.uint8)), s
        assert torch.equal(a.vec.view(torch.uint8), b.vec.view(torch.uint8)), s


# ------------------------------------------------------------------ 6. guards
def test_guards():
    from dgc import clip_grad as K
    from dgc.batch import DGCBatch
    from dgc.bucket import DGCBucket
    bad = [functools.partial(K.clip_grad_value_by_global_norm_, name="w"),
           functools.partial(K.clip_grad_norm_2_by_global_, max_norm=1.0, name="w"),
           functools.partial(K.clip_grad_norm_, max_norm=1.0, norm_type=3), lambda g: g]
    for dt in (torch.float32, torch.bfloat16):
        for fn in bad:
            with pytest.raises(NotImplementedError, match="clip"):
                DGCBucket(5000, device=DEV, world_size=1, dtype=dt, clip=fn)
            spec = K.spec_of(fn)
            if spec is not None:
                with pytest.raises(NotImplementedError, match="clip"):
                    DGCBatch([("a", (5000,))], device=DEV, world_size=1, dtype=dt, clip=spec)
        with pytest.raises(NotImplementedError, match="clip"):
            DGCBatch([("a", (5000,))], device=DEV, world_size=1, dtype=dt, clip=lambda g: g)
    spec = K.ClipSpec("norm2", 1.0)
    assert spec.fusable(torch.float32) and spec.fusable(torch.bfloat16) and spec.fusable(torch.float16)
    assert K.ClipSpec("global_norm2", 1.0).fusable(torch.float32)
    assert not K.ClipSpec("global_norm2", 1.0).fusable(torch.bfloat16)
    assert not K.ClipSpec("normp", 1.0, norm_type=3.0).fusable(torch.float16)
    assert DGCBucket(5000, device=DEV, world_size=1, dtype=torch.float16, clip=spec).clip == spec


def test_batched_optimizer_still_refuses_clipping_on_16bit_parameters(monkeypatch):
    monkeypatch.setenv("HOROVOD_ELASTIC", "1")
    from dgc.compression import DGCCompressor
    from dgc.horovod import DistributedOptimizer
    from dgc.memory import DGCSGDMemory
    model = torch.nn.Linear(64, 32).to(DEV).to(torch.bfloat16)
    mem = DGCSGDMemory(momentum=0.9, gradient_clipping=clip_fn("norm2", 1.0))
    comp = quiet(DGCCompressor, 0.01, memory=mem)
    quiet(mem.initialize, model.named_parameters())
    quiet(comp.initialize, [(n, p) for n, p in model.named_parameters() if p.dim() > 1])
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(NotImplementedError, match="clipping"):
        DistributedOptimizer(opt, named_parameters=model.named_parameters(), compression=comp, batch=True)
