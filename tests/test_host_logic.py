"""Host-side logic of the drop-in classes (no GPU): attribute tuples, warmup
schedule, adaptation bounds, and the loud failure of the product path on CPU."""
import math

import pytest
import torch

from dgc.compression import DGCCompressor
from dgc.memory import DGCSGDMemory, Memory


def quiet(fn, *a, **kw):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def test_attributes_match_reference(golden_attributes):
    rows = golden_attributes["rows"]
    by_cfg = {}
    for r in rows:
        by_cfg.setdefault((r["sample_ratio"], r["ratio"]), []).append(r)
    for (sr, ratio), group in by_cfg.items():
        comp = quiet(DGCCompressor, 0.001, sample_ratio=sr)
        comp.compress_ratio = ratio
        quiet(comp.initialize, [(f"t{r['numel']}", (r["numel"], [r["numel"]])) for r in group])
        for r in group:
            numel, shape, k, S, ks, stride = comp.attributes[f"t{r['numel']}"]
            assert [numel, k, S, ks, stride] == r["attrs"], (sr, ratio, r)
            assert shape == [r["numel"]]


def test_warmup_matches_reference(golden_attributes):
    for label, sched in golden_attributes["schedules"].items():
        comp = quiet(DGCCompressor, sched["base_ratio"], **sched["kwargs"])
        quiet(comp.initialize, [("w", (1000000, [1000, 1000]))])
        for epoch, (ratio, attrs) in enumerate(sched["per_epoch"]):
            quiet(comp.warmup_compress_ratio, epoch)
            assert comp.compress_ratio == ratio, (label, epoch)
            assert list(comp.attributes["w"][2:]) == attrs, (label, epoch)


def test_select_params_bounds():
    comp = quiet(DGCCompressor, 0.001)
    quiet(comp.initialize, [("w", (1000000, [1000000])), ("v", (3000, [3000]))])
    p = comp._select_params("w", True, True)
    assert (p.num_selects, p.upper_count, p.lower_count) == (1000, 1300, 800)
    assert p.upper == pytest.approx(1.3) and p.max_iters == 10 and p.resample == 1
    q = comp._select_params("v", False, False)
    k = 3
    assert q.upper_count == math.floor(k * 1.3) and q.lower_count == math.ceil(0.8 * k)


def test_int32_default_off_and_dtypes():
    comp = quiet(DGCCompressor, 0.01, fp16_values=True, int32_indices=True)
    quiet(comp.initialize, [("w", (5000, [5000]))])
    p = comp._select_params("w", True, True)
    assert (p.vdtype, p.idtype) == (1, 1)


def test_select_params_builder():
    """_lib.select_params is the one place a dgc_select_params is filled: with a compressor's
    settings it equals the compressor's own record field for field; _lib.clip_args turns
    fused_clip's triple (or None) into a *_clip entry point's three arguments."""
    from dgc import _lib
    comp = quiet(DGCCompressor, 0.001, fp16_values=True, int32_indices=True)
    quiet(comp.initialize, [("w", (5000, [5000]))])
    numel, _, k, S, _, _ = comp.attributes["w"]
    assert numel == 5000
    for masking, update, dt in ((True, True, torch.float32), (False, False, torch.bfloat16)):
        p = comp._select_params("w", masking, update, dt)
        q = _lib.select_params(numel, k, S, comp.compress_upper_bound, comp.compress_lower_bound,
                               comp.max_adaptation_iters, comp.resample, masking, update, torch.float16, torch.int32,
                               thr_dtype=dt)
        for field, _ in _lib.SelectParams._fields_:
            assert getattr(p, field) == getattr(q, field), field
        assert (p.vdtype, p.idtype, p.thr_dtype) == (1, 1, _lib.VD[dt])
        assert (p.masking, p.update_memory, p.resample_order, p.status_sink) == (int(masking), int(update), 0, None)
        assert (p.upper_count, p.lower_count) == (math.floor(k * 1.3), math.ceil(0.8 * k))
    assert comp._select_params("w", True, True) is comp._select_params("w", True, True)   # cached
    s = _lib.select_params(10, 2, 10, 1.3, 0.8, 10, True, True, 2, torch.float32, torch.int64,
                           resample_order="index", status_sink=4096)
    assert (s.update_memory, s.resample_order, s.status_sink, s.thr_dtype) == (2, 1, 4096, 0)

    assert _lib.NO_CLIP == (0, None, 0.0)
    assert _lib.clip_args(None) == _lib.NO_CLIP
    coef = torch.ones(1)
    kind, ptr, value = _lib.clip_args((1, coef, 0.25))
    assert (kind, ptr.value, value) == (1, coef.data_ptr(), 0.25)
    assert _lib.clip_args((2, None, 3.0)) == (2, None, 3.0)


def test_product_path_refuses_cpu_tensors():
    mem = DGCSGDMemory(momentum=0.9)
    comp = quiet(DGCCompressor, 0.01, memory=mem)
    w = torch.zeros(5000)
    quiet(mem.initialize, [("w", w)])
    quiet(comp.initialize, [("w", w)])
    with pytest.raises(RuntimeError, match="MI355X"):
        comp.compress(torch.randn(5000), "w")
    with pytest.raises(RuntimeError, match="MI355X"):
        mem.compensate(torch.randn(5000), "w")


def test_dense_branch_passthrough_and_memory_api():
    comp = quiet(DGCCompressor, 0.01, fp16_values=True)
    t = torch.randn(10)
    out, ctx = comp.compress(t, "bias")         # not in attributes -> dense path
    assert out.dtype == torch.float16 and ctx == ("bias", None, None, torch.float32, None, None)
    assert Memory.compensate(t) is t and Memory.state_dict() is None
    mem = DGCSGDMemory()
    quiet(mem.initialize, [("a", torch.zeros(3))])
    sd = mem.state_dict()
    mem2 = DGCSGDMemory()
    quiet(mem2.initialize, [("a", torch.ones(3))])
    mem2.load_state_dict(sd)
    assert mem2.momentums["a"] is sd["momentums"]["a"]


def test_distributed_optimizer_default_picks_batched_only_when_equivalent():
    """DistributedOptimizer's default batch="auto" (dgc.horovod.batched.auto) takes the
    batched step only where it computes what the per-tensor hooks would: not for host
    parameters, an overriding subclass, an op other than Average, mixed dtypes or a
    non-DGC compressor (the gloo CPU tests' oracle doubles keep their per-tensor calls)."""
    from dgc.comm import Average, Sum
    from dgc.horovod import batched

    class Sub(DGCCompressor):
        def compress(self, tensor, name):
            return super().compress(tensor, name)

    mem = DGCSGDMemory(momentum=0.9)
    comp = quiet(DGCCompressor, 0.01, memory=mem)
    cpu = [("w", torch.nn.Parameter(torch.zeros(4, 4)))]
    assert not batched.auto(comp, cpu, Average)                    # host parameters
    assert not batched.auto(quiet(Sub, 0.01, memory=mem), cpu, Average)
    assert not batched.auto(comp, cpu, Sum)
    assert not batched.auto(quiet(DGCCompressor, 0.01), cpu, Average)   # Memory, not DGCSGDMemory
    assert not batched.auto(quiet(DGCCompressor, 0.01, memory=mem, strided_sample=False), cpu, Average)


def test_reuse_guard_on_cpu_tensors():
    """The receive side's "output still holds last step's result" guard (fill="sparse",
    dgc/exchange.py) on plain tensors: torch's version counter sees in-place writes; it
    does not see writes through ``.data`` — the documented blind spot, pinned here so it
    is not changed silently."""
    from dgc.exchange import ReuseMemory
    mem, gathered = ReuseMemory(), torch.zeros(4, dtype=torch.uint8)
    out, other = torch.zeros(8), torch.zeros(8)
    assert not mem.reusable(out)
    mem.remember(out, gathered)
    assert mem.reusable(out)
    assert not mem.reusable(other)
    out.data.add_(1)
    assert mem.reusable(out)
    out.add_(1)
    assert not mem.reusable(out)
    mem.remember(out, gathered)
    assert mem.reusable(out)
    mem.forget()
    assert not mem.reusable(out) and not mem.reusable(other)
