"""Local gradient clipping (dgc/clip_grad.py), everything that needs no GPU: the module's
interface, ``spec_of``, which configurations the batched optimizer step takes, the new
library entry points' argument checks, and — against tests/golden/clip.* recorded from
the reference — the method the GPU tests rely on: "apply the recorded coefficient to
the gradient, then the oracle's compress step" is the reference's clipped step bit for
bit."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_json
from oracle import dgc_oracle as O
from oracle import synth

F32 = np.float32


@pytest.fixture(scope="module")
def golden_clip():
    return load_json("clip.json"), np.load(os.path.join(GOLDEN, "clip.npz"))


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def coef_of(step):
    return np.array([step["coef_bits"]], np.uint32).view(F32)[0]


def clip_np(g, mode, c):
    """The clip kinds of include/dgc_hip.h on a numpy gradient, given the coefficient."""
    if mode in ("value", "global_value"):
        return g if np.isnan(c) else np.where(np.isnan(g), g, np.minimum(np.maximum(g, -c), c)).astype(F32)
    return (g * c).astype(F32) if c < 1 else g   # a NaN coefficient compares false


def case_input(case, step, poison):
    g = synth.gradient(step["seed"], case["N"], "normal", step["scale"])
    assert synth.digest(g) == step["input_sha"], "oracle/synth.py drifted from the fixture"
    return g


# ------------------------------------------------------------------ interface
def test_module_has_the_reference_names():
    import inspect
    from dgc import clip_grad
    want = {"clip_grad_norm_": ["grad", "max_norm", "norm_type"], "clip_grad_value_": ["grad", "clip_value"],
            "clip_grad_value_by_global_norm_": ["grad", "name"], "clip_grad_norm_2_by_global_": ["grad", "max_norm", "name"]}
    for name, params in want.items():
        fn = getattr(clip_grad, name)
        assert name in clip_grad.__all__
        assert list(inspect.signature(fn).parameters) == params
    sig = inspect.signature(clip_grad.clip_grad_norm_)
    assert sig.parameters["norm_type"].default == 2
    assert inspect.signature(clip_grad.clip_grad_norm_2_by_global_).parameters["name"].default is None


def test_spec_of_recognises_functions_and_partials():
    from dgc import clip_grad as K
    P = functools.partial
    s = K.spec_of(P(K.clip_grad_norm_, max_norm=3))
    assert (s.mode, s.param, s.kind, s.batchable, s.is_global) == ("norm2", 3.0, K.CLIP_SCALE, True, False)
    s = K.spec_of(P(K.clip_grad_norm_, max_norm=0.5, norm_type=math.inf))
    assert (s.mode, s.param, s.batchable) == ("norminf", 0.5, True)
    s = K.spec_of(P(K.clip_grad_norm_, max_norm=0.5, norm_type="inf"))
    assert s.mode == "norminf"
    s = K.spec_of(P(K.clip_grad_norm_, max_norm=1, norm_type=3))
    assert (s.mode, s.norm_type, s.batchable) == ("normp", 3.0, False)
    s = K.spec_of(P(K.clip_grad_value_, clip_value=0.25))
    assert (s.mode, s.param, s.kind, s.batchable) == ("value", 0.25, K.CLIP_CLAMP, True)
    s = K.spec_of(K.clip_grad_value_by_global_norm_)          # complete without arguments
    assert (s.mode, s.kind, s.is_global, s.batchable) == ("global_value", K.CLIP_CLAMP, True, False)
    s = K.spec_of(P(K.clip_grad_norm_2_by_global_, max_norm=2.0, name="g"))
    assert (s.mode, s.param, s.name, s.is_global, s.batchable) == ("global_norm2", 2.0, "g", True, False)
    # a partial of a partial is one partial; equal specs compare equal
    assert K.spec_of(P(P(K.clip_grad_norm_, norm_type=2), max_norm=3)) == K.spec_of(P(K.clip_grad_norm_, max_norm=3))
    # not a complete call with the gradient alone, or not ours
    assert K.spec_of(K.clip_grad_norm_) is None                # max_norm missing
    assert K.spec_of(P(K.clip_grad_norm_, 3.0)) is None        # a positional argument binds `grad`
    assert K.spec_of(P(K.clip_grad_value_, clip_value=1, bogus=2)) is None
    assert K.spec_of(lambda g: K.clip_grad_norm_(g, 3)) is None
    assert K.spec_of(P(lambda g, m: g, m=1)) is None
    assert K.spec_of(None) is None and K.spec_of([]) is None


def test_batched_supported_with_clipping():
    from dgc import clip_grad as K
    from dgc.compression import DGCCompressor
    from dgc.horovod import batched
    from dgc.memory import DGCSGDMemory
    import contextlib
    import io

    def supported(fn, **kw):
        with contextlib.redirect_stdout(io.StringIO()):
            comp = DGCCompressor(0.01, memory=DGCSGDMemory(gradient_clipping=fn), **kw)
        return batched.supported(comp)

    P = functools.partial
    assert supported(None)
    assert supported(P(K.clip_grad_norm_, max_norm=1.0))
    assert supported(P(K.clip_grad_norm_, max_norm=1.0, norm_type=math.inf))
    assert supported(P(K.clip_grad_value_, clip_value=0.1))
    assert not supported(P(K.clip_grad_norm_, max_norm=1.0, norm_type=3))
    assert not supported(K.clip_grad_value_by_global_norm_)
    assert not supported(P(K.clip_grad_norm_2_by_global_, max_norm=1.0))
    assert not supported(lambda g: g)
    assert not supported(P(K.clip_grad_norm_, max_norm=1.0), strided_sample=False)


def test_functions_refuse_cpu_tensors():
    """No CPU fallback: the module functions raise on a host tensor, like the rest."""
    import torch
    from dgc import clip_grad as K
    with pytest.raises(RuntimeError, match="MI355X"):
        K.clip_grad_norm_(torch.ones(8), 1.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.clip_grad_value_(torch.ones(8), 1.0)


# ------------------------------------------------------------------ library arguments
@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


INVALID, DTYPE, WORKSPACE = 1, 2, 5


def test_new_entry_points_fail_without_gpu(L):
    from dgc import _lib
    P = ctypes.c_void_p
    fake = P(4096)                      # never dereferenced: every call below fails first
    ptrs = (P * 2)(4096, 8192)
    nums = (ctypes.c_int64 * 2)(5000, 3)
    offs = (ctypes.c_int64 * 2)(0, 5000)
    # workspace query: 8 B per 4096-element partial, at least one 256-B unit
    assert L.dgc_grad_stats_workspace(nums, 2) == 256
    big = (ctypes.c_int64 * 1)(10 ** 9)
    assert L.dgc_grad_stats_workspace(big, 1) >= 8 * (10 ** 9 // 4096)
    assert L.dgc_grad_stats_workspace(None, 1) == 0
    assert L.dgc_grad_stats_workspace((ctypes.c_int64 * 1)(-1), 1) == 0
    # dgc_grad_stats
    assert L.dgc_grad_stats(None, nums, 2, 0, 0, fake, fake, 256, None) == INVALID
    assert L.dgc_grad_stats(ptrs, nums, 2, 0, 0, None, fake, 256, None) == INVALID
    assert L.dgc_grad_stats(ptrs, nums, 2, 7, 0, fake, fake, 256, None) == INVALID and b"kind" in L.dgc_last_error()
    assert L.dgc_grad_stats(ptrs, nums, 2, 0, 2, fake, fake, 256, None) == DTYPE          # round_to bf16
    assert L.dgc_grad_stats(ptrs, nums, 2, 0, 0, fake, fake, 128, None) == WORKSPACE      # short
    assert L.dgc_grad_stats(ptrs, nums, 2, 0, 0, fake, None, 256, None) == WORKSPACE
    assert L.dgc_grad_stats(ptrs, nums, 2, 0, 0, fake, P(4096 + 64), 256, None) == WORKSPACE   # misaligned
    odd = (P * 2)(4096, 8193)
    assert L.dgc_grad_stats(odd, nums, 2, 0, 0, fake, fake, 256, None) == INVALID and b"4-B" in L.dgc_last_error()
    assert L.dgc_grad_stats(ptrs, nums, 0, 0, 0, None, None, 0, None) == 0                 # nothing to do
    # dgc_clip_coefs
    assert L.dgc_clip_coefs(None, 2, 0, 1.0, fake, None) == INVALID
    assert L.dgc_clip_coefs(fake, 2, 0, 1.0, None, None) == INVALID
    assert L.dgc_clip_coefs(fake, 2, 3, 1.0, fake, None) == INVALID and b"mode" in L.dgc_last_error()
    # dgc_clip_apply
    assert L.dgc_clip_apply(None, nums, 2, 1, fake, 0.0, None) == INVALID
    assert L.dgc_clip_apply(ptrs, nums, 2, 0, fake, 0.0, None) == INVALID                  # DGC_CLIP_NONE
    assert L.dgc_clip_apply(ptrs, nums, 2, 3, fake, 0.0, None) == INVALID
    assert L.dgc_clip_apply(ptrs, nums, 2, 1, None, 0.0, None) == INVALID and b"table" in L.dgc_last_error()
    # the clipped K1s: a bad clip kind, SCALE without its table
    assert L.dgc_compensate_clip(fake, fake, fake, None, 16, 0.9, 0, 1, None, 0, 1, 0, 5, fake, 0.0, None) == INVALID
    assert L.dgc_compensate_clip(fake, fake, fake, None, 16, 0.9, 0, 1, None, 0, 1, 0, 1, None, 0.0, None) == INVALID
    assert L.dgc_compensate_clip(None, fake, fake, None, 16, 0.9, 0, 1, None, 0, 1, 0, 2, None, 1.0, None) == INVALID
    assert L.dgc_compensate_multi_clip(ptrs, nums, offs, 2, 0, fake, fake, 0.9, 0, 4, fake, 0.0, None) == INVALID
    assert L.dgc_compensate_multi_clip(ptrs, nums, offs, 2, 0, fake, fake, 0.9, 0, 1, None, 0.0, None) == INVALID
    assert L.dgc_compensate_multi_clip(ptrs, nums, offs, 2, 2, fake, fake, 0.9, 0, 2, None, 1.0, None) == DTYPE
    p = _lib.SelectParams()
    p.numel, p.num_selects, p.num_samples, p.max_iters = 10000, 10, 10000, 10
    assert L.dgc_compress_begin_clip(fake, fake, fake, 0.9, 0, 0, 1, ctypes.byref(p), None, 9, fake, 0.0, fake, 0,
                                     None) == INVALID
    assert L.dgc_compress_begin_clip(fake, fake, fake, 0.9, 0, 0, 1, ctypes.byref(p), None, 1, None, 0.0, fake, 0,
                                     None) == INVALID
    assert L.dgc_compress_begin_clip(fake, fake, fake, 0.9, 0, 0, 1, ctypes.byref(p), None, 1, fake, 0.0, None, 0,
                                     None) == WORKSPACE
    T = 1
    arr = lambda xs: (ctypes.c_int64 * T)(*xs)   # noqa: E731
    keep = [arr([5000]), arr([0]), arr([5]), arr([5000]), arr([5]), arr([1])]
    d = _lib.BatchDesc()
    d.count = T
    d.numel, d.offset, d.num_selects, d.num_samples, d.top_k_samples, d.sample_stride = keep
    d.flat_numel, d.upper_bound, d.lower_bound, d.max_iters, d.resample = 5120, 1.3, 0.8, 10, 1
    starts = arr([0])
    for fn, g in ((L.dgc_batch_compress_begin_clip, fake), (L.dgc_batch_compress_begin_ptrs_clip, (P * 1)(4096))):
        assert fn(ctypes.byref(d), g, fake, fake, starts, 6, fake, 0.0, fake, 0, None) == INVALID
        assert fn(ctypes.byref(d), g, fake, fake, starts, 1, None, 0.0, fake, 0, None) == INVALID
        assert fn(ctypes.byref(d), g, fake, fake, starts, 2, None, 1.0, None, 0, None) == WORKSPACE


# ------------------------------------------------------------------ the fixture and the method
def test_fixture_norm2_coefficient_crosses_one(golden_clip):
    """Every norm-2 case clips on at least one step and leaves the gradient alone on at
    least one (the `if clip_coef < 1` branch both ways)."""
    meta, _ = golden_clip
    seen = 0
    for name, case in meta["cases"].items():
        if case["kind"] == "tensor" and case["mode"] == "norm2" and not case["poison"]:
            coefs = [coef_of(s) for s in case["per_step"]]
            assert any(c < 1 for c in coefs) and any(c >= 1 for c in coefs), (name, coefs)
            seen += 1
    assert seen == 3
    g2 = meta["cases"]["global_norm2"]["per_step"]
    assert coef_of(g2[0]["ranks"][0]) < 1 <= coef_of(g2[1]["ranks"][0])


def test_fixture_norms_and_coefficient_arithmetic(golden_clip):
    """The recorded 2-norm is torch's fp32 CPU accumulation, whose order is torch's own:
    it sits a few ulp from fl32(sqrt(sum of squares in float64)) (4 ulp at N = 70 001),
    which is why the device norm is held to the float64 value and not to this one; here
    it only has to agree to 1e-5. The recorded max |g| is exact, and the recorded
    coefficient is reciprocal().mul(max_norm) of the recorded norm, bit for bit."""
    meta, _ = golden_clip
    for name, case in meta["cases"].items():
        if case["kind"] not in ("tensor", "dense") or case["mode"] == "value" or case.get("poison"):
            continue
        for step in case["per_step"]:
            g = case_input(case, step, False)
            total = np.array([step["total_norm_bits"]], np.uint32).view(F32)[0]
            if case["mode"] == "norm2":
                want = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
                assert abs(float(total) - want) <= 1e-5 * want, (name, total, want)
            else:
                assert total == np.abs(g).max()
            coef = F32(F32(1) / F32(total + F32(1e-6))) * F32(case["param"])
            assert bits(coef)[0] == step["coef_bits"], name


def test_oracle_on_the_clipped_gradient_reproduces_the_goldens(golden_clip):
    """clip(g, recorded coefficient) -> oracle compress_step == the reference's clipped
    compress, state and payload, bit for bit, for every per-tensor case."""
    meta, arr = golden_clip
    poison = meta["poison"]
    checked = 0
    for name, case in meta["cases"].items():
        if case["kind"] != "tensor":
            continue
        N = case["N"]
        attrs = tuple(case["attrs"])
        mmt, vec = np.zeros(N, F32), np.zeros(N, F32)
        for s, step in enumerate(case["per_step"]):
            g = case_input(case, step, case["poison"])
            if case["poison"] and s == 0:
                g[poison["nan"]], g[poison["inf"]] = np.nan, np.inf
            gc = clip_np(g, case["mode"], coef_of(step))
            vals, idx, _ = O.compress_step(gc, mmt, vec, attrs, step["start"] or 0, nesterov=case["nesterov"])
            key = f"{name}/s{s}"
            assert np.array_equal(idx, arr[key + "/indices"]), key
            assert np.array_equal(bits(vals), bits(arr[key + "/values"])), key
            assert synth.digest(mmt) == step["mmt_sha"] and synth.digest(vec) == step["vec_sha"], key
            if key + "/mmt" in arr:
                assert np.array_equal(bits(mmt), bits(arr[key + "/mmt"]))
                assert np.array_equal(bits(vec), bits(arr[key + "/vec"]))
            checked += 1
    assert checked == 3 * 3 * 3 + 3 * 2


def test_oracle_dense_and_global_cases(golden_clip):
    meta, arr = golden_clip
    for name, case in meta["cases"].items():
        if case["kind"] == "dense":
            mmt = np.zeros(case["N"], F32)
            for s, step in enumerate(case["per_step"]):
                g = clip_np(case_input(case, step, False), case["mode"], coef_of(step))
                out = O.compensate(g, mmt, None, 0.9, case["nesterov"], accumulate=False)
                assert np.array_equal(bits(out), bits(arr[f"{name}/s{s}/out"])), (name, s)
                assert np.array_equal(bits(mmt), bits(arr[f"{name}/s{s}/mmt"])), (name, s)
        elif case["kind"] == "global":
            W, N = case["W"], case["N"]
            state = [(np.zeros(N, F32), np.zeros(N, F32)) for _ in range(W)]
            for s, step in enumerate(case["per_step"]):
                grads = [synth.gradient(r["seed"], N, "normal", r["scale"]) for r in step["ranks"]]
                # the statistic the reference averages: fl32 sums of squares, rank-order Average
                sums = [F32(np.sum(g.astype(np.float64) ** 2)) for g in grads]
                for q, r in enumerate(step["ranks"]):
                    c = coef_of(r)
                    total = np.sqrt(F32(F32(sums[0] + sums[1]) / F32(W)))
                    near = total if case["mode"] == "global_value" else F32(case["param"]) / total
                    assert abs(float(c) - float(near)) <= 4e-6 * abs(float(near)), (name, s, q)   # the sums' order
                    gc = clip_np(grads[q], case["mode"], c)
                    vals, idx, _ = O.compress_step(gc, state[q][0], state[q][1], tuple(case["attrs"]), step["start"],
                                                   nesterov=True)
                    assert np.array_equal(idx, arr[f"{name}/s{s}/r{q}/indices"])
                    assert np.array_equal(bits(vals), bits(arr[f"{name}/s{s}/r{q}/values"]))
                    assert synth.digest(state[q][1]) == r["vec_sha"]
