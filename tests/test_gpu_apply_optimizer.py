"""DistributedOptimizer(batch="apply"): DGCSGD's step on the compressed tensors applied from
the gathered entries (DGCBatch.apply -> dgc_apply_packed_multi), no dense gradient written
for the optimizer to read back.

* W = 2 over gloo (two processes on one MI355X): the recorded reference runs replayed with
  batch="apply" — the goldens' weights after every step, and every step an apply step.
* W = 1 (HOROVOD_ELASTIC=1): bit-equal weights and optimizer state to batch=True at every
  step of a script that alternates apply steps with the steps that must decompress.
* The refusals."""
import pytest
import torch

import gpu_apply_helpers as A
from test_gpu_multirank import run

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.timeout(200)
@pytest.mark.parametrize("label", ["tinynet", "resnet20"])
def test_apply_w2_reproduces_reference_weights(label):
    """"resnet20" covers the warmup's re-layouts (a new table each) and the fp16/int32 wire."""
    out = run(A.apply_replay_worker, 2, label)
    for rank, problems in out.items():
        assert problems == [], (rank, problems)


@pytest.fixture(scope="module")
def dense_trails():
    """The batch=True runs: computed once, shared, left unchanged."""
    return {}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("setting", A.SETTINGS)
def test_apply_w1_equals_batched(monkeypatch, dense_trails, setting):
    """TinyNet, 6 steps (A.SCRIPT): apply steps alternate with an explicit synchronize() +
    skip_synchronize() step and a closure step, both zero_grad forms, an lr change and an
    optimizer.load_state_dict mid-run; weights and momentum buffers equal batch=True's at
    every step, the counters tell the two kinds of step apart, and only a step that
    decompressed leaves the compressed parameters a .grad."""
    monkeypatch.setenv("HOROVOD_ELASTIC", "1")
    if setting not in dense_trails:
        dense_trails[setting] = A.tiny_run(True, setting, DEV)
    want, _ = dense_trails[setting]
    got, compressed = A.tiny_run("apply", setting, DEV)
    assert len(compressed) == 2
    applied = dense = 0
    for s, (g, w) in enumerate(zip(got, want)):
        for n in w["weights"]:
            assert torch.equal(g["weights"][n], w["weights"][n]), (setting, s, n, "weights")
            assert (g["state"][n] is None) == (w["state"][n] is None), (setting, s, n, "momentum buffer exists")
            if w["state"][n] is not None:
                assert torch.equal(g["state"][n], w["state"][n]), (setting, s, n, "momentum buffer")
        applied += A.APPLIED[s]
        dense += not A.APPLIED[s]
        assert g["counts"] == (applied, dense), (setting, s, g["counts"])
        # an apply step leaves the compressed parameters without a .grad; a step that decompressed, with
        assert g["with_grad"] == ([] if A.APPLIED[s] else compressed), (setting, s, g["with_grad"])
        assert w["with_grad"] == compressed, (setting, s)
        assert g["acc_nonzero"] == 0, (setting, s, "accumulator not all-zero bits")
    assert applied == 4 and dense == 2


def test_apply_refuses_another_optimizer(monkeypatch):
    monkeypatch.setenv("HOROVOD_ELASTIC", "1")
    with pytest.raises(ValueError, match="DGCSGD"):
        A.tiny_setup("apply", "wd0", DEV, optimizer=lambda params: torch.optim.SGD(params, lr=0.1))


def test_apply_refuses_bf16_parameters(monkeypatch):
    monkeypatch.setenv("HOROVOD_ELASTIC", "1")
    with pytest.raises(NotImplementedError, match="fp32"):
        A.tiny_setup("apply", "wd0", DEV, dtype=torch.bfloat16)


def test_batch_apply_refuses_split_and_16_bit():
    from dgc import _lib
    from dgc.batch import DGCBatch
    shapes = [("a", (300, 100)), ("b", (5000,))]
    table, hypers = _lib.ApplyTable(DEV), [(0.1, 0.0, 0.0, 0.0, False)]
    split = DGCBatch(shapes, compress_ratio=0.01, world_size=2, device=DEV, exchange_parts=2)
    assert split.rx.parts == 2
    with pytest.raises(ValueError, match="exchange_parts=1"):
        split.apply(table, hypers)
    half = DGCBatch(shapes, compress_ratio=0.01, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp32"):
        half.apply(table, hypers)
