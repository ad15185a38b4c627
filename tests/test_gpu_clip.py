"""Local gradient clipping on the MI355X (dgc/clip_grad.py, the K0 entry points of
include/dgc_hip.h and the clipped K1s), against tests/golden/clip.* recorded from the
reference and the numpy oracle.

The 2-norm is the one quantity the reference gives no fixed answer for (torch's CPU sum
order is its own; the fixture's norm sits 4 ulp from the float64 value at N = 70 001), so:
the device norm is held to fl32(sqrt(sum of squares in float64)) within 1 ulp — the
fixed-order fp64 sum is within n * 2^-53 of it, only a rounding boundary can move the
result to a neighbour — and everything downstream is checked bit for bit GIVEN the
coefficient: with the recorded coefficient injected (the link to the reference), and with
the device's own coefficient against the oracle on the gradient clipped with it
(tests/test_clip_host.py shows that method reproduces the fixtures). Norm-inf and the
clamp have no such freedom and match the fixtures end to end.
"""
import contextlib
import ctypes
import functools
import io
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import GOLDEN, load_json
from oracle import dgc_oracle as O
from oracle import synth
from test_clip_host import bits, case_input, clip_np, coef_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
SUMSQ, NORM2, ABSMAX = 0, 1, 2
P = functools.partial


@pytest.fixture(scope="module")
def golden_clip():
    return load_json("clip.json"), np.load(os.path.join(GOLDEN, "clip.npz"))


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def clip_fn(mode, param):
    from dgc import clip_grad as K
    if mode == "norm2":
        return P(K.clip_grad_norm_, max_norm=param)
    if mode == "norminf":
        return P(K.clip_grad_norm_, max_norm=param, norm_type=math.inf)
    if mode == "normp":
        return P(K.clip_grad_norm_, max_norm=param, norm_type=3)
    return P(K.clip_grad_value_, clip_value=param)


def ulps(a, b):
    return abs(int(bits(F32(a))[0]) - int(bits(F32(b))[0]))


# ------------------------------------------------------------------ statistics
def stats_of(tensors, kind, round_to=torch.float32):
    from dgc import _lib
    L = _lib.lib()
    T = len(tensors)
    ptrs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in tensors])
    nums = (ctypes.c_int64 * T)(*[t.numel() for t in tensors])
    wsz = L.dgc_grad_stats_workspace(nums, T)
    ws = torch.empty(wsz, dtype=torch.uint8, device=DEV)
    out = torch.full((T,), -7.0, device=DEV)
    _lib.check(L.dgc_grad_stats(ptrs, nums, T, kind, _lib.VD[round_to], _lib.ptr(out), _lib.ptr(ws), wsz,
                                _lib.stream_of(DEV)), "dgc_grad_stats")
    return out.cpu().numpy()


STAT_SIZES = [0, 1, 3, 255, 1024, 4097, 70001, 1000003]


@pytest.fixture(scope="module")
def stat_inputs():
    """(host arrays, device tensors): the sizes of the issue, then a copy of the 70 001
    tensor at a pointer that is only 4-B aligned, then one holding a NaN and an inf."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    host =[synth.gradient(300 + i, n, "normal", 0.5 + i) for i, n in enumerate(STAT_SIZES)]
    host.append(host[6].copy())
    poisoned = synth.gradient(399, 5000)
    poisoned[[17, 4100]] = [np.nan, np.inf]
    host.append(poisoned)
    dev = [torch.from_numpy(h).to(DEV) for h in host]
    buf = torch.zeros(70001 + 1, device=DEV)
    buf[1:].copy_(dev[6])
    dev[8] = buf[1:]
    assert dev[8].data_ptr() % 16 == 4
    return host, dev


def test_stats_against_float64(stat_inputs):
    host, dev = stat_inputs
    norm, sumsq, amax = (stats_of(dev, k) for k in (NORM2, SUMSQ, ABSMAX))
    for i, h in enumerate(host):
        if np.isnan(h).any():
            assert np.isnan(norm[i]) and np.isnan(sumsq[i]) and np.isnan(amax[i])   # abs().max() propagates NaN
            continue
        s64 = float(np.sum(h.astype(np.float64) ** 2))
        assert ulps(norm[i], F32(math.sqrt(s64))) <= 1, (h.size, norm[i], math.sqrt(s64))
        assert ulps(sumsq[i], F32(s64)) <= 1, (h.size, sumsq[i], s64)
        assert bits(amax[i])[0] == bits(np.abs(h).max() if h.size else F32(0))[0], h.size
    assert norm[0] == 0 and sumsq[0] == 0 and amax[0] == 0                           # numel 0
    # the statistic of the values K1 sees behind an fp16 wire
    r16 = stats_of(dev[:8], NORM2, torch.float16)
    for i, h in enumerate(host[:8]):
        s64 = float(np.sum(h.astype(np.float16).astype(np.float64) ** 2))
        assert ulps(r16[i], F32(math.sqrt(s64))) <= 1, h.size


def test_stats_are_deterministic_and_composition_independent(stat_inputs):
    host, dev = stat_inputs
    for kind in (NORM2, SUMSQ, ABSMAX):
        a, b = stats_of(dev, kind), stats_of(dev, kind)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # alone, in another position, and at another alignment: the same bits
        for i in (3, 5, 6, 7, 9):
            assert stats_of([dev[i]], kind).view(np.uint32)[0] == a.view(np.uint32)[i], (kind, i)
        rev = stats_of(dev[::-1], kind)[::-1]
        assert np.array_equal(rev.view(np.uint32), a.view(np.uint32))
        assert a.view(np.uint32)[6] == a.view(np.uint32)[8]          # 16-B aligned vs 4-B aligned copy


def test_stats_table_of_70_tensors(stat_inputs):
    """More than the 64 tensors of one launch: tiny tensors of 1..70 elements around a
    large one, each equal to its statistic alone."""
    host, dev = stat_inputs
    tiny = [synth.gradient(500 + n, n) for n in range(1, 71)]
    tensors = [torch.from_numpy(t).to(DEV) for t in tiny]
    tensors.insert(65, dev[7])
    tiny.insert(65, host[7])
    norm, amax = stats_of(tensors, NORM2), stats_of(tensors, ABSMAX)
    for i, h in enumerate(tiny):
        assert ulps(norm[i], F32(math.sqrt(float(np.sum(h.astype(np.float64) ** 2))))) <= 1, i
        assert amax[i] == np.abs(h).max(), i
    assert stats_of([dev[7]], NORM2).view(np.uint32)[0] == norm.view(np.uint32)[65]


def test_clip_coefs_are_the_reference_arithmetic():
    from dgc import _lib
    L = _lib.lib()
    stats = np.array([0.0, 1e-7, 0.3, 1.0, 2.5, 263.35217, 3.4e38, np.inf, np.nan], F32)
    dev = torch.from_numpy(stats).to(DEV)
    out = torch.empty_like(dev)
    max_norm = 0.7
    with np.errstate(all="ignore"):
        want = {0: (F32(1) / (stats + F32(1e-6))).astype(F32) * F32(max_norm),
                1: np.sqrt(stats),
                2: (F32(1) / (np.sqrt(stats) + F32(1e-6))).astype(F32) * F32(max_norm)}
    for mode in (0, 1, 2):
        _lib.check(L.dgc_clip_coefs(_lib.ptr(dev), stats.size, mode, max_norm, _lib.ptr(out), _lib.stream_of(DEV)),
                   "dgc_clip_coefs")
        got = out.cpu().numpy()
        same = (np.isnan(got) & np.isnan(want[mode])) | (bits(got) == bits(want[mode]))
        assert same.all(), (mode, got, want[mode])


# ------------------------------------------------------------------ per tensor
def make_pair(case, clipping, fp16=False):
    from dgc.compression import DGCCompressor
    from dgc.memory import DGCSGDMemory
    mem = DGCSGDMemory(momentum=0.9, nesterov=case["nesterov"], gradient_clipping=clipping)
    comp = quiet(DGCCompressor, case.get("ratio", 0.01), memory=mem, fp16_values=fp16)
    p = torch.zeros(case["N"], device=DEV)
    quiet(mem.initialize, [("w", p)])
    quiet(comp.initialize, [("w", p)])
    return mem, comp


def tensor_cases(meta, modes=("norm2", "norminf", "value")):
    return [(n, c) for n, c in meta["cases"].items() if c["kind"] == "tensor" and c["mode"] in modes]


def step_input(meta, case, s):
    step = case["per_step"][s]
    g = case_input(case, step, False)
    if case["poison"] and s == 0:
        g[meta["poison"]["nan"]], g[meta["poison"]["inf"]] = np.nan, np.inf
    return g


def assert_golden_step(arr, key, step, vals, idx, mem):
    assert np.array_equal(idx.view(-1).cpu().numpy(), arr[key + "/indices"]), key
    assert np.array_equal(bits(vals.view(-1).cpu().numpy()), bits(arr[key + "/values"])), key
    assert synth.digest(mem.momentums["w"].cpu().numpy()) == step["mmt_sha"], key
    assert synth.digest(mem.velocities["w"].cpu().numpy()) == step["vec_sha"], key


def test_clipped_k1_with_the_golden_coefficient(golden_clip, monkeypatch):
    """The reference's coefficient written into the clip table, then the clipped
    dgc_compress_begin + dgc_compress_finish: state, indices and values are the
    reference's bit for bit, for every per-tensor case (norm-2 included)."""
    meta, arr = golden_clip
    from dgc import clip_grad as K
    for name, case in tensor_cases(meta):
        mem, comp = make_pair(case, clip_fn(case["mode"], case["param"]))
        spec = mem.clip_spec()
        random.seed(42)
        for s, step in enumerate(case["per_step"]):
            table = torch.from_numpy(np.array([step["coef_bits"]], np.uint32).view(F32)).to(DEV)
            monkeypatch.setattr(mem, "fused_clip", lambda g, t=table: (spec.kind, t, 0.0))
            g = torch.from_numpy(step_input(meta, case, s)).to(DEV)
            keep = g.clone()
            (vals, idx), _ = comp.compress(g, "w")
            assert_golden_step(arr, f"{name}/s{s}", step, vals, idx, mem)
            assert torch.equal(bits_t(g), bits_t(keep))           # the fused clip leaves the input alone


def bits_t(t):
    return t.contiguous().view(torch.int32)


def test_compressor_with_native_clipping(golden_clip):
    """DGCSGDMemory + DGCCompressor with a functools.partial of the module's functions.
    Norm-inf and the clamp reproduce the fixtures with nothing injected (coefficient
    included); norm-2 reproduces the oracle on the gradient clipped with the coefficient
    the device computed, which is within the norm's 1 ulp of the float64 one."""
    meta, arr = golden_clip
    for name, case in tensor_cases(meta):
        mem, comp = make_pair(case, clip_fn(case["mode"], case["param"]))
        random.seed(42)
        N = case["N"]
        m_o, v_o = np.zeros(N, F32), np.zeros(N, F32)
        for s, step in enumerate(case["per_step"]):
            g = step_input(meta, case, s)
            (vals, idx), _ = comp.compress(torch.from_numpy(g).to(DEV), "w")
            key = f"{name}/s{s}"
            if case["mode"] == "value":
                assert mem.last_clip_coef is None
                assert_golden_step(arr, key, step, vals, idx, mem)
                continue
            c = mem.last_clip_coef.cpu().numpy()[0]
            if case["mode"] == "norminf":
                assert bits(c)[0] == step["coef_bits"] or (np.isnan(c) and np.isnan(coef_of(step))), key
                assert_golden_step(arr, key, step, vals, idx, mem)
                continue
            if case["poison"] and s == 0:
                assert np.isnan(c)
            else:
                n64 = F32(math.sqrt(float(np.sum(g.astype(np.float64) ** 2))))
                near = [F32(F32(1) / F32(x + F32(1e-6))) * F32(case["param"])
                        for x in (np.nextafter(n64, F32(0)), n64, np.nextafter(n64, F32(np.inf)))]
                assert any(bits(c)[0] == bits(x)[0] for x in near), (key, c, near)
            ov, oi, _ = O.compress_step(clip_np(g, "norm2", c), m_o, v_o, tuple(case["attrs"]), step["start"] or 0,
                                        nesterov=case["nesterov"])
            assert np.array_equal(idx.view(-1).cpu().numpy(), oi), key
            assert np.array_equal(bits(vals.view(-1).cpu().numpy()), bits(ov)), key
            assert np.array_equal(bits(mem.momentums["w"].cpu().numpy()), bits(m_o)), key
            assert np.array_equal(bits(mem.velocities["w"].cpu().numpy()), bits(v_o)), key


@pytest.mark.parametrize("mode,param", [("norm2", 30.0), ("norminf", 2.5), ("value", 1.5), ("normp", 8.0)])
def test_fused_equals_opaque_callable(mode, param):
    """The same function behind a lambda (an opaque callable: called as the reference
    calls it, in place, before K1) gives the bits of the recognised spec (clipped in K1's
    registers), for compress and for the dense compensate(accumulate=False)."""
    fn = clip_fn(mode, param)
    case = dict(N=70001, nesterov=True, ratio=0.001)
    runs = []
    for clipping in (fn, lambda g: fn(g)):
        mem, comp = make_pair(case, clipping)
        assert (mem.clip_spec() is not None) == (clipping is fn)
        quiet(mem.initialize, [("w", torch.zeros(case["N"], device=DEV)), ("b", torch.zeros(1027, device=DEV))])
        random.seed(5)
        out = []
        for s, scale in enumerate((1.0, 0.05, 3.0)):
            g = torch.from_numpy(synth.gradient(700 + s, case["N"], "normal", scale)).to(DEV)
            (vals, idx), _ = comp.compress(g, "w")
            d = torch.from_numpy(synth.gradient(710 + s, 1027, "normal", scale)).to(DEV)
            dense = mem.compensate(d, "b", accumulate=False)
            out.append([vals.clone(), idx.clone(), dense.clone(), mem.momentums["w"].clone(),
                        mem.velocities["w"].clone(), mem.momentums["b"].clone()])
        runs.append(out)
    for s, (a, b) in enumerate(zip(*runs)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x.view(-1).view(torch.int32 if x.dtype == torch.float32 else x.dtype),
                               y.view(-1).view(torch.int32 if y.dtype == torch.float32 else y.dtype)), (mode, s, i)


def test_dense_compensate_matches_the_goldens(golden_clip):
    meta, arr = golden_clip
    from dgc.memory import DGCSGDMemory
    for name, case in meta["cases"].items():
        if case["kind"] != "dense":
            continue
        mem = DGCSGDMemory(momentum=0.9, nesterov=case["nesterov"], gradient_clipping=clip_fn(case["mode"], case["param"]))
        quiet(mem.initialize, [("b", torch.zeros(case["N"], device=DEV))])
        m_o = np.zeros(case["N"], F32)
        for s, step in enumerate(case["per_step"]):
            g = case_input(case, step, False)
            out = mem.compensate(torch.from_numpy(g).to(DEV), "b", accumulate=False).cpu().numpy()
            if case["mode"] == "norm2":   # given the device coefficient
                want = O.compensate(clip_np(g, "norm2", mem.last_clip_coef.cpu().numpy()[0]), m_o, None, 0.9,
                                    case["nesterov"], accumulate=False)
                assert np.array_equal(bits(out), bits(want)), (name, s)
            else:
                assert np.array_equal(bits(out), bits(arr[f"{name}/s{s}/out"])), (name, s)
                assert np.array_equal(bits(mem.momentums["b"].cpu().numpy()), bits(arr[f"{name}/s{s}/mmt"])), (name, s)


def test_module_functions_clip_in_place():
    from dgc import clip_grad as K
    h = synth.gradient(800, 4097)
    n64 = F32(math.sqrt(float(np.sum(h.astype(np.float64) ** 2))))
    g = torch.from_numpy(h).to(DEV)
    assert K.clip_grad_norm_(g, 1e6) is g and np.array_equal(bits(g.cpu().numpy()), bits(h))      # coef >= 1
    assert K.clip_grad_norm_(g, 3.0) is g
    got = g.cpu().numpy()
    near = [F32(F32(1) / F32(x + F32(1e-6))) * F32(3.0) for x in (np.nextafter(n64, F32(0)), n64, np.nextafter(n64, F32(1e9)))]
    assert any(np.array_equal(bits(got), bits((h * c).astype(F32))) for c in near)
    g = torch.from_numpy(h).to(DEV)
    assert K.clip_grad_norm_(g, 0.5, norm_type=math.inf) is g
    c = F32(F32(1) / F32(np.abs(h).max() + F32(1e-6))) * F32(0.5)
    assert np.array_equal(bits(g.cpu().numpy()), bits((h * c).astype(F32)))
    hp = h.copy()
    hp[[3, 9, 11]] = [np.nan, np.inf, -np.inf]
    g = torch.from_numpy(hp).to(DEV)
    assert K.clip_grad_value_(g, 0.25) is g
    want = torch.from_numpy(hp).clamp_(min=-0.25, max=0.25).numpy()
    got = g.cpu().numpy()
    assert np.isnan(got[3]) and np.array_equal(bits(np.delete(got, 3)), bits(np.delete(want, 3)))
    # the global variants in a world of one rank: the Average is the identity
    g = torch.from_numpy(h).to(DEV)
    assert K.clip_grad_norm_2_by_global_(g, 3.0) is g
    s32 = F32(float(np.sum(h.astype(np.float64) ** 2)))
    near = [F32(F32(1) / F32(np.sqrt(x) + F32(1e-6))) * F32(3.0)
            for x in (np.nextafter(s32, F32(0)), s32, np.nextafter(s32, F32(1e30)))]
    assert any(np.array_equal(bits(g.cpu().numpy()), bits((h * c).astype(F32))) for c in near)
    g = torch.from_numpy(h * 100).to(DEV)[::2]                    # a non-contiguous view, clamped through a copy
    keep = g.clone()
    assert K.clip_grad_value_by_global_norm_(g) is g
    bound = math.sqrt(float(np.sum((h[::2] * 100).astype(np.float64) ** 2)))
    assert torch.equal(g, keep.clamp(-bound, bound))              # nothing reaches the global norm
    # a p-norm from torch, the coefficient and the scaling from the library
    g = torch.from_numpy(h).to(DEV)
    total = g.norm(3.0).cpu().numpy()
    assert K.clip_grad_norm_(g, 2.0, norm_type=3) is g
    c = F32(F32(1) / F32(total + F32(1e-6))) * F32(2.0)
    assert c < 1 and np.array_equal(bits(g.cpu().numpy()), bits((h * c).astype(F32)))
    # 16-bit tensors: the reference's formula in ATen ops
    g16 = torch.from_numpy(h).to(DEV).to(torch.bfloat16)
    w16 = g16.clone()
    coef = 3.0 / (w16.norm(2.0) + 1e-6)
    assert K.clip_grad_norm_(g16, 3.0) is g16 and torch.equal(g16, w16 * coef)


# ------------------------------------------------------------------ multi-tensor dense K1
@pytest.mark.parametrize("round_to", [torch.float32, torch.float16], ids=["fp32", "fp16-wire"])
@pytest.mark.parametrize("mode", ["norm2", "norminf", "value"])
def test_compensate_multi_clip(mode, round_to):
    """A 70-tensor dense set (past the 64 tensors of a launch), one with numel % 4 != 0
    and more than a block, one at a 4-B aligned pointer: stats -> coefs -> the clipped
    multi-tensor K1 equals the oracle on each clipped (and fp16-rounded) gradient."""
    from dgc import _lib
    from dgc import clip_grad as K
    spec = K.spec_of(clip_fn(mode, {"norm2": 2.0, "norminf": 1.0, "value": 0.7}[mode]))
    sizes = [n % 9 + 1 for n in range(68)] + [4099, 1027]
    host = [synth.gradient(600 + i, n, "normal", 1.0 + (i % 3)) for i, n in enumerate(sizes)]
    dev = [torch.from_numpy(h).to(DEV) for h in host]
    buf = torch.zeros(1028, device=DEV)
    buf[1:].copy_(dev[-1])
    dev[-1] = buf[1:]
    T = len(sizes)
    offs, end = [], 0
    for n in sizes:
        offs.append(end)
        end += -(-n // 4) * 4
    ptrs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in dev])
    nums = (ctypes.c_int64 * T)(*sizes)
    coffs = (ctypes.c_int64 * T)(*offs)
    mmt = torch.from_numpy(synth.gradient(699, end)).to(DEV)
    mmt0 = mmt.cpu().numpy()
    out = torch.zeros(end, device=DEV)
    coefs = spec.table_coefs(ptrs, nums, T, DEV, round_to)
    _lib.check(_lib.lib().dgc_compensate_multi_clip(ptrs, nums, coffs, T, _lib.VD[round_to], _lib.ptr(mmt),
                                                    _lib.ptr(out), 0.9, 1, spec.kind, _lib.ptr(coefs), spec.param,
                                                    _lib.stream_of(DEV)), "dgc_compensate_multi_clip")
    got_out, got_mmt = out.cpu().numpy(), mmt.cpu().numpy()
    cs = coefs.cpu().numpy() if coefs is not None else np.full(T, spec.param, F32)
    for t, (h, o, n) in enumerate(zip(host, offs, sizes)):
        seen = h.astype(np.float16).astype(F32) if round_to == torch.float16 else h
        if mode == "norm2":
            n64 = F32(math.sqrt(float(np.sum(seen.astype(np.float64) ** 2))))
            near = [F32(F32(1) / F32(x + F32(1e-6))) * F32(2.0)
                    for x in (np.nextafter(n64, F32(0)), n64, np.nextafter(n64, F32(np.inf)))]
            assert any(bits(cs[t])[0] == bits(x)[0] for x in near), (t, cs[t], near)
        elif mode == "norminf":
            assert bits(cs[t])[0] == bits(F32(F32(1) / F32(np.abs(seen).max() + F32(1e-6))) * F32(1.0))[0], t
        m = mmt0[o: o + n].copy()
        want = O.compensate(clip_np(seen, mode, cs[t]), m, None, 0.9, True, accumulate=False)
        assert np.array_equal(bits(got_out[o: o + n]), bits(want)), (mode, t)
        assert np.array_equal(bits(got_mmt[o: o + n]), bits(m)), (mode, t)
    pad = np.ones(end, bool)
    for o, n in zip(offs, sizes):
        pad[o: o + n] = False
    assert not got_out[pad].any() and np.array_equal(bits(got_mmt[pad]), bits(mmt0[pad]))   # nothing written past a tensor


# ------------------------------------------------------------------ batched
@pytest.mark.parametrize("mode,param", [("norm2", 0.05), ("norminf", 0.004), ("value", 0.002)])
def test_batch_with_clip_equals_per_tensor_compressors(mode, param):
    """DGCBatch(clip=...) over four tensors, 4 steps, against one DGCCompressor per
    tensor driven with the same sample starts: payload, state and coefficients bit for
    bit, the selection records' branch and recount count too. Step 1 is heavy-tailed and
    step 2 0.3x the others, to move the sampled thresholds both ways between steps."""
    from dgc import clip_grad as K
    from dgc.batch import DGCBatch
    from dgc.compression import DGCCompressor
    from dgc.memory import DGCSGDMemory
    shapes = [("a", (1728,)), ("b", (4096,)), ("c", (70001,)), ("d", (512, 512))]
    fn = clip_fn(mode, param)
    b = DGCBatch(shapes, compress_ratio=0.01, momentum=0.9, nesterov=True, device=DEV, seed=42,
                 resample_order="topk", clip=K.spec_of(fn))
    singles = {}
    for n, shp in shapes:
        mem = DGCSGDMemory(momentum=0.9, nesterov=True, gradient_clipping=fn)
        comp = quiet(DGCCompressor, 0.01, memory=mem)
        p = torch.zeros(shp, device=DEV)
        quiet(mem.initialize, [(n, p)])
        quiet(comp.initialize, [(n, p)])
        singles[n] = (mem, comp)
    seen = set()
    for s in range(4):
        starts = b.draw_starts()
        grads = {}
        for t, (n, shp) in enumerate(shapes):
            scale = 1e-3 * (1 + t) * (0.3 if s == 2 else 1.0)
            kind = "layered" if s == 1 else "normal"
            grads[n] = torch.from_numpy(synth.gradient(900 + 10 * s + t, b.numels[t], kind, scale)).to(DEV)
            b.grad(n).copy_(grads[n].view(shp))
        b.compress(starts)
        torch.cuda.synchronize()
        sent, infos = b.transmitted(), b.infos()
        for t, (n, shp) in enumerate(shapes):
            mem, comp = singles[n]
            state = random.getstate()
            comp._sample_start = lambda name, st=starts[t]: st      # the batch's draw for this tensor
            (vals, idx), _ = comp.compress(grads[n].view(shp), n)
            random.setstate(state)
            key = (mode, s, n)
            single = comp.last_info()
            assert (single["branch"], single["recounts"]) == (infos[t]["branch"], infos[t]["recounts"]), key
            seen.add((single["branch"], single["recounts"], bool(single["threshold"] < single["threshold0"])))
            gv, gi = sent[n]
            assert torch.equal(gi, idx.view(-1)), key
            assert torch.equal(bits_t(gv), bits_t(vals.view(-1))), key
            assert torch.equal(bits_t(b.momentum_of(n)), bits_t(mem.momentums[n])), key
            assert torch.equal(bits_t(b.velocity_of(n)), bits_t(mem.velocities[n])), key
            if mode != "value":
                assert torch.equal(bits_t(b.clip_coefs[t: t + 1]), bits_t(mem.last_clip_coef)), key
    print("branches (branch, recounts, threshold lowered):", sorted(seen))
    # these seeded gradients give every mode a step whose sampled threshold is lowered
    # (count < 0.8 k: `threshold *= 0.8`, one recount) before it resamples
    assert any(lowered for _, _, lowered in seen) and {"direct", "trunc", "resample"} <= {b for b, _, _ in seen}


def _tinynet_steps(batch, clipping, fp16, monkeypatch, steps=3):
    """``steps`` of DistributedOptimizer on TinyNet with seeded gradients, every hook
    fired by hand (W = 1 registers them with HOROVOD_ELASTIC); returns the weights."""
    from dgc.compression import DGCCompressor
    from dgc.horovod import DistributedOptimizer
    from dgc.memory import DGCSGDMemory
    from dgc.optim import DGCSGD
    from models import TinyNet
    monkeypatch.setenv("HOROVOD_ELASTIC", "1")
    torch.manual_seed(7)
    model = TinyNet().to(DEV)
    named = list(model.named_parameters())
    mem = DGCSGDMemory(momentum=0.9, gradient_clipping=clipping)
    comp = quiet(DGCCompressor, 0.01, memory=mem, fp16_values=fp16, int32_indices=fp16, warmup_epochs=-1)
    quiet(mem.initialize, named)
    quiet(comp.initialize, [(n, p) for n, p in named if p.dim() > 1])
    opt = DistributedOptimizer(DGCSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True),
                               named_parameters=named, compression=comp, batch=batch)
    random.seed(7)
    gen = torch.Generator(device=DEV).manual_seed(13)
    out = []
    for s in range(steps):
        for i, (n, p) in enumerate(named):
            p.grad = torch.randn(p.shape, generator=gen, device=DEV) * (0.01 * (1 + i) * (0.2 if s == 1 else 1.0))
        for p, hook in reversed(opt._hook_fns):
            hook()
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        out.append({n: p.detach().clone() for n, p in named})
    return opt, out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fp16", [False, True], ids=["wire-fp32-int64", "wire-fp16-int32"])
@pytest.mark.parametrize("mode,param", [("norm2", 0.3), ("norminf", 0.02), ("value", 0.004)])
def test_auto_takes_the_batched_step_and_equals_per_tensor(mode, param, fp16, monkeypatch):
    """batch="auto" with a recognised local spec takes the batched step (it fell back to
    the per-tensor hooks for any gradient_clipping before), and through a one-rank RCCL
    group — the exchange, the rank-order Average into the flat buffer and the clipped
    multi-tensor K1 of the W > 1 dense leg — its weights equal batch=False's bit for bit
    over 3 steps; so do the shortcut's (the W = 1 dense leg). A global variant and a
    lambda keep the per-tensor path."""
    import socket
    import torch.distributed as dist
    from dgc import clip_grad as K
    from dgc import comm
    fn = clip_fn(mode, param)
    want_opt, want = _tinynet_steps(False, fn, fp16, monkeypatch)
    assert want_opt._batched is None
    got_opt, got = _tinynet_steps("auto", fn, fp16, monkeypatch)
    assert got_opt._batched is not None and got_opt._batched.clip == K.spec_of(fn)
    for opaque in (lambda g: fn(g), K.clip_grad_value_by_global_norm_):
        assert _tinynet_steps("auto", opaque, fp16, monkeypatch, steps=0)[0]._batched is None
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=DEV)
    monkeypatch.setattr(comm, "ONE_RANK_SHORTCUT", False)
    try:
        rccl_opt, rccl = _tinynet_steps("auto", fn, fp16, monkeypatch)
        assert rccl_opt._batched is not None and "dense_avg" in rccl_opt._batched._plan
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    for s in range(3):
        for n in want[s]:
            assert torch.equal(bits_t(want[s][n]), bits_t(got[s][n])), (mode, s, n, "shortcut")
            assert torch.equal(bits_t(want[s][n]), bits_t(rccl[s][n])), (mode, s, n, "one-rank group")
    assert not torch.equal(want[2]["fc1.weight"], _tinynet_steps(False, None, fp16, monkeypatch)[1][2]["fc1.weight"])


# ------------------------------------------------------------------ W = 2
def _spawn(fn, world, *args):
    import dist_helpers as H
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = H.free_port()
    procs = [ctx.Process(target=fn, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=150)
        if p.exitcode is None:
            p.kill()
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    out = {}
    while not q.empty():
        rank, res = q.get()
        out[rank] = res
    assert sorted(out) == list(range(world))
    return out


@pytest.mark.timeout(200)
@pytest.mark.parametrize("batch", [False, "default"], ids=["per-tensor", "default"])
@pytest.mark.parametrize("label", ["opt_norminf_fp32", "opt_value_fp16"])
def test_optimizer_w2_reproduces_the_clipped_reference_weights(label, batch):
    """The reference's DistributedOptimizer with a clipping memory at W = 2 (two processes
    on cuda:0 over gloo), replayed from its recorded gradients: the reference's weights
    after every step, per tensor and with the default batched step."""
    import gpu_clip_helpers as C
    for rank, problems in _spawn(C.clip_optimizer_worker, 2, label, batch).items():
        assert problems == [], (rank, problems)


@pytest.mark.timeout(200)
@pytest.mark.parametrize("label", ["global_norm2", "global_value"])
def test_global_variant_w2(label):
    import gpu_clip_helpers as C
    for rank, problems in _spawn(C.clip_global_worker, 2, label).items():
        assert problems == [], (rank, problems)
