"""Split exchange (dgc_payload_split / dgc_scatter_split / dgc_clear_split): the
allgather of dgc/compression.py:200-212 in `parts` collectives, the decompress
(dgc/compression.py:179-194) of each part scattered as it lands.

Single process: W ranks' packed payloads are split on the device, assembled
part-major as the `parts` allgathers would leave them, and scattered phase by phase.
The dense result must be the oracle's sequential index_put_ sums bit for bit, and
after every phase each value already written must be final (a phase never writes an
index whose entries have not all landed).
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle.dgc_oracle as O
from gpu_split_helpers import DEV, P, Split, _rank_payload, bits, check, stream   # noqa: F401 (test_gpu_corrupt.py reads them here)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    return _lib.lib()


def _runs(rng, N, W, cap, overlap, shuffled, full=False, prefix=None):
    shared = np.sort(rng.choice(N, cap, replace=False))
    runs = []
    for r in range(W):
        c = cap if full else int(rng.integers(cap // 2, cap + 1))
        own = rng.choice(prefix or N, c, replace=False)
        pick = rng.random(c) < overlap
        idx = np.unique(np.where(pick, shared[:c], own))[:c]
        v = rng.standard_normal(idx.size).astype(np.float32)
        if shuffled == 2 or (shuffled == 1 and r == W - 1):
            o = rng.permutation(idx.size)
            v, idx = v[o], idx[o]
        runs.append((v, idx.astype(np.int64)))
    return runs


@pytest.mark.parametrize("N,W,parts,cap,overlap,fp16,int32,shuffled", [
    (1_000_003, 2, 2, 1000, 0.5, False, False, 0),
    (1_000_003, 8, 4, 1000, 0.3, True, False, 0),
    (1_000_003, 8, 8, 1001, 0.3, False, True, 0),   # 8 parts of a ragged capacity
    (1_000_000, 4, 2, 10000, 0.2, False, False, 0),   # crowded super-chunks: the overflow path per phase
    (300_000, 8, 3, 30000, 0.3, False, True, 0),
    (1_000_003, 4, 2, 1000, 0.3, False, False, 1),  # the last rank in topk order: its bound is a true minimum
    (300_000, 8, 4, 30000, 0.3, True, True, 2),     # every rank shuffled: everything lands in the last phase
    (50_000, 2, 2, 7, 0.0, False, False, 0),        # fewer entries than parts * chunks
])
def test_split_scatter_matches_oracle(L, N, W, parts, cap, overlap, fp16, int32, shuffled):
    rng = np.random.default_rng(N + 31 * W + parts)
    runs = _runs(rng, N, W, cap, overlap, shuffled)
    vd, idt = int(fp16), int(int32)
    sp = Split(L, N, W, parts, cap, vd, idt)
    g, heads = sp.gather(runs)
    # headers: counts and bounds (the smallest index in the later parts)
    for (v, i), h in zip(runs, heads):
        h = h.cpu().numpy()
        for p in range(parts):
            lo, hi = p * sp.pc, min((p + 1) * sp.pc, len(i))
            assert h[p, 0] == max(0, hi - lo)
            later = i[(p + 1) * sp.pc:]
            assert h[p, 1] == (later.min() if later.size else np.iinfo(np.int64).max)
    wv = [v.astype(np.float16).astype(np.float32) if fp16 else v for v, _ in runs]
    want = O.decompress(wv, [i for _, i in runs], N, W)
    out = torch.full((N,), float("nan"), device=DEV)
    check(L, L.dgc_fill_zero(P(out), N, stream()))
    sp.scatter(g, out, False, want)
    torch.cuda.synchronize()
    assert sp.status() == (2 if shuffled else 0)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


@pytest.mark.parametrize("N,W,parts,cap,fp16,int32,shuffled", [
    (1_000_003, 2, 2, 2000, False, False, 0),
    (500_000, 8, 4, 3000, True, True, 1),
])
def test_split_clear_over_previous_output(L, N, W, parts, cap, fp16, int32, shuffled):
    """dgc_clear_split re-zeroes the previous step's split gathered entries; the
    phases then write the new step's: three steps, each the oracle's result."""
    rng = np.random.default_rng(N + parts)
    vd, idt = int(fp16), int(int32)
    sp = Split(L, N, W, parts, cap, vd, idt)
    out = torch.full((N,), float("nan"), device=DEV)
    prev = None
    for step in range(3):
        runs = _runs(rng, N, W, cap, 0.3, shuffled, prefix=N // 3 if step == 1 else None)
        g, _ = sp.gather(runs)
        wv = [v.astype(np.float16).astype(np.float32) if fp16 else v for v, _ in runs]
        want = O.decompress(wv, [i for _, i in runs], N, W)
        if prev is None:
            check(L, L.dgc_fill_zero(P(out), N, stream()))
        else:
            check(L, L.dgc_clear_split(P(prev), W, parts, cap, vd, idt, P(out), N, P(sp.ws), sp.ws.numel(), stream()))
        sp.scatter(g, out, prev is not None)
        torch.cuda.synchronize()
        assert sp.status() == (2 if shuffled else 0), step
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), step
        prev = g


def test_split_refusals(L):
    assert L.dgc_payload_split_bytes(100, 0, 0, 0) == 0
    assert L.dgc_payload_split_bytes(100, 9, 0, 0) == 0
    assert L.dgc_decompress_split_workspace(1000, 16, 8, 100) == 0   # 128 runs > 64
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1000, device=DEV)
    assert L.dgc_scatter_split(P(buf), 2, 2, 2, 100, 0, 0, P(out), 1000, 0.5, 0, P(buf), buf.numel(), stream()) != 0
    assert L.dgc_scatter_split(P(buf), 2, 1, 0, 100, 0, 0, P(out), 1000, 0.5, 0, P(buf), buf.numel(), stream()) != 0
