"""CPU: the written-out formulas of tests/clip16_port.py (the reference's local clipping on a
bf16 / fp16 tensor, one rounding per ATen op) followed by the torch-CPU port of the
reference's compensate / sparsify / update (oracle/torch_cpu.py) reproduce the reference's
own fixtures (tests/golden/clip16.*, made by make_goldens_clip16.py) bit for bit: the
total_norm, the coefficient, the transmitted indices in order, the values and the 16-bit
state. This pins the model the GPU tests (test_gpu_clip16.py) compare against."""
import json
import os

import numpy as np
import pytest
import torch

import clip16_port as P
from conftest import GOLDEN
from oracle import synth
from oracle import torch_cpu as TC

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def golden_clip16():
    with open(os.path.join(GOLDEN, "clip16.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "clip16.npz"))


def gradient(case, st, s, poison_at):
    g = synth.gradient(st["seed"], case["N"], "normal", st["scale"])
    assert synth.digest(g) == st["input_sha"]
    g = torch.from_numpy(g.copy()).to(DT[case["dtype"]])
    if case.get("poison") and s == 0:
        g[poison_at["nan"]], g[poison_at["inf"]] = float("nan"), float("inf")
    return g


def check_clip(key, st, mode, total, coef):
    if mode == "value":   # the fixture holds the clamp's parameter as given, not its rounding to the dtype
        assert st["total_norm_bits"] is None
        return
    assert P.f32_bits(total) == P.canon(st["total_norm_bits"]), (key, float(total))
    assert P.f32_bits(coef) == P.canon(st["coef_bits"]), (key, float(coef))


def test_fixture_covers_the_cases(golden_clip16):
    meta, _ = golden_clip16
    cases = meta["cases"]
    tensor = [c for c in cases.values() if c["kind"] == "tensor"]
    assert len(tensor) == 2 * 3 * 4 + 1 and sum(c["kind"] == "dense" for c in cases.values()) == 6
    for dname in DT:
        for mode in ("norm2", "norminf"):
            coefs = [p["coef"] for c in tensor if c["dtype"] == dname and c["mode"] == mode and not c["poison"]
                     for p in c["per_step"]]
            assert min(coefs) < 1 < max(coefs), (dname, mode)
    over = cases["fp16_norm2_n4097_overflow"]["per_step"][0]
    assert over["total_norm_bits"] == 0x7F800000 and over["coef_bits"] == 0   # inf, then a zero coefficient


def test_port_matches_tensor_fixtures(golden_clip16):
    meta, arrays = golden_clip16
    for name, case in meta["cases"].items():
        if case["kind"] != "tensor":
            continue
        dt = DT[case["dtype"]]
        N = case["N"]
        numel, k, S, ks, stride = case["attrs"]
        m, v = torch.zeros(N, dtype=dt), torch.zeros(N, dtype=dt)
        for s, st in enumerate(case["per_step"]):
            key = f"{name}/s{s}"
            g = gradient(case, st, s, meta["poison"])
            gc, total, coef = P.clip(g, case["mode"], case["param"])
            check_clip(key, st, case["mode"], total, coef)
            TC.compensate(gc, m, v, 0.9, case["nesterov"])
            vals, idx = TC.sparsify(v, numel, k, S, ks, stride, st["start"] or 0)
            vals, idx = vals.clone(), idx.clone()
            TC.update(m, v, idx)
            assert np.array_equal(idx.numpy(), arrays[key + "/indices"]), key
            assert np.array_equal(bits(vals.float().numpy()), bits(arrays[key + "/values"])), key
            assert synth.digest(P.image(m)) == st["mmt_sha"], key
            assert synth.digest(P.image(v)) == st["vec_sha"], key
            if key + "/mmt" in arrays:
                assert np.array_equal(bits(P.image(m)), bits(arrays[key + "/mmt"])), key
                assert np.array_equal(bits(P.image(v)), bits(arrays[key + "/vec"])), key


def test_port_matches_dense_fixtures(golden_clip16):
    meta, arrays = golden_clip16
    for name, case in meta["cases"].items():
        if case["kind"] != "dense":
            continue
        dt = DT[case["dtype"]]
        m = torch.zeros(case["N"], dtype=dt)
        for s, st in enumerate(case["per_step"]):
            key = f"{name}/s{s}"
            g = gradient(case, st, s, meta["poison"])
            gc, total, coef = P.clip(g, case["mode"], case["param"])
            check_clip(key, st, case["mode"], total, coef)
            out = TC.compensate(gc, m, None, 0.9, case["nesterov"], accumulate=False)
            assert np.array_equal(bits(P.image(out)), bits(arrays[key + "/out"])), key
            assert np.array_equal(bits(P.image(m)), bits(arrays[key + "/mmt"])), key


@pytest.mark.parametrize("dname", list(DT))
def test_port_edge_coefficients(dname):
    """A zero norm gives rdt(max_norm / rdt(1e-6)), an inf norm 0, a NaN norm NaN (and the
    comparison `coef < 1` is then false: the tensor is left alone)."""
    dt = DT[dname]
    x = torch.zeros(8, dtype=dt)
    out, total, coef = P.clip(x, "norm2", 1.0)
    assert float(total) == 0 and float(coef) > 1 and torch.equal(out, x)
    assert float(P.coefficient(torch.tensor(float("inf")), 1.0, dt)) == 0
    x[3] = float("nan")
    out, total, coef = P.clip(x, "norminf", 1.0)
    assert np.isnan(float(total)) and np.isnan(float(coef))
    assert np.array_equal(out.view(torch.int16).numpy(), x.view(torch.int16).numpy())
