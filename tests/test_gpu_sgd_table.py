"""K7 / K7-16 through the C ABI (dgc_sgd_step, dgc_sgd_step16) with hand-built tensor
tables: length edges of the per-block vector / scalar paths, mixed alignments inside one
launch, tables on the 48-tensor chunk boundary with zero-length entries, first flags that
differ between tensors and steps, and the argument refusals.

Every tensor of a case is a view into one arena per role (p, g, buf) with canaries
between neighbours. After every launch: the canaries and the whole g arena are unchanged
(and the buf arena when no momentum buffer is in use), and p and buf equal, as bit
patterns, oracle.dgcsgd_step32 (pinned to the reference by tests/golden/sgd32.*) or
oracle.dgcsgd_step16 (tests/golden/sgd16.*); where the expectation is NaN, a NaN is
required. A buffer whose first flag is set holds NaN before the launch: it is not read."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle.dgc_oracle as O
from conftest import PKG
from test_sgd32_port import H, H_IDS, assert_same_bits, plant_specials

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ("f32", "bf16", "f16")
ORACLE_DTYPE = {"bf16": "bfloat16", "f16": "float16"}
VD = {"f16": 1, "bf16": 2}                     # dgc_vdtype
CANARY = {4: 0x7FC0DEAD, 2: 0x7FDE}            # a NaN in fp32, and in bf16 and fp16
GUARD = 8                                      # canary elements between neighbouring views
DGC_OK, DGC_ERR_INVALID, DGC_ERR_DTYPE = 0, 1, 2


def _constants():
    """kSgdPerBlock, kSgd16PerBlock and kSgdMaxTensors as the sources define them."""
    env = {}
    for name in ("dgc_common.hpp", "sgd.hip"):
        src = open(os.path.join(PKG, "csrc", name)).read()
        for m in re.finditer(r"constexpr int (k\w+) = ([\w\s*+]+);", src):
            try:
                env[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(env)))
            except (NameError, SyntaxError):   # a constant of another header: not needed here
                pass
    return env["kSgdPerBlock"], env["kSgd16PerBlock"], env["kSgdMaxTensors"]


B32, B16, CHUNK = _constants()


def test_block_sizes_read_from_the_sources():
    assert (B32, B16, CHUNK) == (256 * 16, 256 * 4, 48)


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    return _lib.lib()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_bits(x, kind):
    """fp32 image (a value of the dtype) -> the dtype's bit patterns."""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "f32":
        return x.view(np.uint32).copy()
    if kind == "f16":
        return x.astype(np.float16).view(np.uint16)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def to_image(b, kind):
    if kind == "f32":
        return b.view(np.float32)
    if kind == "f16":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def rounded(x, kind):
    x = np.ascontiguousarray(x, np.float32)
    return x if kind == "f32" else O.round16(x, ORACLE_DTYPE[kind])


class Arena:
    """One device allocation holding every tensor of a role: GUARD or more canaries, then
    view i at ``mis[i]`` elements past a 16-B boundary, and so on."""

    def __init__(self, ns, mis, kind):
        self.size = 4 if kind == "f32" else 2
        per16 = 16 // self.size
        self.starts, pos = [], 0
        for n, m in zip(ns, mis):
            pos = -(-(pos + GUARD) // per16) * per16 + m
            self.starts.append(pos)
            pos += n
        self.ns = list(ns)
        utype = np.uint32 if self.size == 4 else np.uint16
        self.host = np.full(pos + GUARD, CANARY[self.size], utype)
        self.inside = np.zeros(self.host.size, bool)
        for s, n in zip(self.starts, ns):
            self.inside[s:s + n] = True
        self.dev = torch.empty(self.host.size, dtype=torch.int32 if self.size == 4 else torch.int16, device=DEV)
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, i):
        return self.dev.data_ptr() + self.starts[i] * self.size

    def view(self, i):
        return self.host[self.starts[i]:self.starts[i] + self.ns[i]]

    def upload(self):
        self.dev.copy_(torch.from_numpy(self.host.view(np.int32 if self.size == 4 else np.int16)))

    def download(self):
        """The device's content; the canaries must be what they were."""
        got = self.dev.cpu().numpy().view(self.host.dtype)
        assert (got[~self.inside] == CANARY[self.size]).all(), "a canary was overwritten"
        return got


class Table:
    """The tensors of one case, their oracle state (fp32 images) and the launches."""

    def __init__(self, L, kind, ns, hyper, seed, mis=None, steps=3, null_empty=False):
        self.L, self.kind, self.ns, self.hyper, self.null_empty = L, kind, list(ns), hyper, null_empty
        k = len(ns)
        mis = mis or {}
        self.arena = {r: Arena(ns, mis.get(r, [0] * k), kind) for r in "pgb"}
        rng = np.random.default_rng(seed)
        self.p = [(rng.standard_normal(n) * 0.5).astype(np.float32) for n in ns]
        self.b = [(rng.standard_normal(n) * 1e-3).astype(np.float32) for n in ns]
        self.g = [[(rng.standard_normal(n) * 0.01).astype(np.float32) for n in ns] for _ in range(steps)]
        if ns[0] > 0:
            plant_specials(self.p[0], [g[0] for g in self.g])
        self.p = [rounded(x, kind) for x in self.p]
        self.b = [rounded(x, kind) for x in self.b]
        self.g = [[rounded(x, kind) for x in g] for g in self.g]
        for i in range(k):
            self.arena["p"].view(i)[:] = to_bits(self.p[i], kind)
            self.arena["b"].view(i)[:] = to_bits(self.b[i], kind)
        self.arena["p"].upload()
        lr, mom, damp, wd, nest = hyper
        self.use_buf = wd != 0 and mom != 0

    def ptrs(self, role, idx):
        """The pointer table of a role; null_empty: a zero-length entry carries NULL."""
        a = self.arena[role]
        return (ctypes.c_void_p * len(idx))(*[None if self.null_empty and self.ns[i] == 0 else a.ptr(i) for i in idx])

    def call(self, idx, first, bufs=True):
        """The entry point over the tensors ``idx`` of the arenas; returns its status."""
        n = len(idx)
        P, G = self.ptrs("p", idx), self.ptrs("g", idx)
        Bf = self.ptrs("b", idx) if bufs else None
        N = (ctypes.c_int64 * n)(*[self.ns[i] for i in idx])
        F = (ctypes.c_int32 * n)(*first)
        lr, mom, damp, wd, nest = self.hyper
        args = (P, G, Bf, N, F, n, lr, mom, damp, wd, int(nest))
        if self.kind == "f32":
            rc = self.L.dgc_sgd_step(*args, stream())
        else:
            rc = self.L.dgc_sgd_step16(*args, VD[self.kind], stream())
        torch.cuda.synchronize()
        return rc

    def step(self, s, first, idx=None, bufs=True, what=()):
        """Step ``s`` over the tensors ``idx`` (all by default) with their ``first`` flags,
        compared with the oracle; tensors outside ``idx`` must stay as they are."""
        kind, k = self.kind, len(self.ns)
        idx = list(range(k)) if idx is None else list(idx)
        first = [int(bool(f)) for f in first]
        assert len(first) == len(idx)
        A = self.arena
        for i in range(k):
            A["g"].view(i)[:] = to_bits(self.g[s][i], kind)
        if self.use_buf:
            nan = to_bits(np.full(1, np.nan, np.float32), kind)[0]
            for i, f in zip(idx, first):
                if f:
                    A["b"].view(i)[:] = nan   # created on this step: never read
        A["g"].upload()
        A["b"].upload()
        rc = self.call(idx, first, bufs)
        assert rc == DGC_OK, self.L.dgc_last_error().decode()
        got_p, got_g, got_b = A["p"].download(), A["g"].download(), A["b"].download()
        assert np.array_equal(got_g, A["g"].host), (what, s, "the gradient arena changed")
        if not self.use_buf:
            assert np.array_equal(got_b, A["b"].host), (what, s, "the buffer arena changed without momentum")
        lr, mom, damp, wd, nest = self.hyper
        for i, f in zip(idx, first):
            buf = None if (f or not self.use_buf) else self.b[i]
            if kind == "f32":
                self.p[i], nb = O.dgcsgd_step32(self.p[i], self.g[s][i], buf, lr, mom, damp, wd, nest)
            else:
                self.p[i], nb = O.dgcsgd_step16(self.p[i], self.g[s][i], buf, lr, mom, damp, wd, nest,
                                                ORACLE_DTYPE[kind])
            if self.use_buf:
                self.b[i] = nb
        for i in range(k):   # the tensors outside idx included: their expectation did not move
            lo, hi = A["p"].starts[i], A["p"].starts[i] + self.ns[i]
            assert_same_bits(to_image(got_p[lo:hi], kind), self.p[i], (what, kind, s, i, self.ns[i], "p"))
            if self.use_buf:
                lo, hi = A["b"].starts[i], A["b"].starts[i] + self.ns[i]
                assert_same_bits(to_image(got_b[lo:hi], kind), self.b[i], (what, kind, s, i, self.ns[i], "buf"))
        A["p"].host[:] = got_p
        A["b"].host[:] = got_b


def length_edges(kind):
    if kind == "f32":
        return [1, 3, 4, 5, B32 - 1, B32, B32 + 1, 2 * B32, 3 * B32 + 1]
    return [1, 31, 32, 33, B16 - 1, B16, B16 + 1, 2 * B16 + 31, 2 * B16 + 32]


@pytest.mark.parametrize("hyper", H, ids=H_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_tensor_length_edges(L, kind, hyper):
    """One tensor per launch: the last full block, the partial block after it, and the
    16-bit kernels' n - n % 32 body / tail boundary inside a block, on a block boundary
    and in the last block."""
    for n in length_edges(kind):
        t = Table(L, kind, [n], hyper, seed=n)
        t.step(0, [1], what=n)
        t.step(1, [0], what=n)
        t.step(2, [0], what=n)


@pytest.mark.parametrize("hyper", H, ids=H_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_alignment_mix_in_one_launch(L, kind, hyper):
    """8 tensors of 2 B + 5 elements whose p, g and buf views start at every combination of
    {16-B aligned, one element later}: vector and scalar blocks side by side in one grid;
    each single misaligned pointer forces the scalar path on its own."""
    B = B32 if kind == "f32" else B16
    size = 4 if kind == "f32" else 2
    combos = [(c & 1, c >> 1 & 1, c >> 2 & 1) for c in range(8)]
    mis = {"p": [c[0] for c in combos], "g": [c[1] for c in combos], "b": [c[2] for c in combos]}
    t = Table(L, kind, [2 * B + 5] * 8, hyper, seed=11, mis=mis)
    for i, c in enumerate(combos):
        got = tuple(t.arena[r].ptr(i) % 16 for r in "pgb")
        assert got == tuple(size * m for m in c), (i, got)
    t.step(0, [1] * 8)
    t.step(1, [0] * 8)
    t.step(2, [0] * 8)


def chunk_lengths(count, B):
    cycle = [0, 1, 5, B, B + 1, 37, 2 * B]
    ns = [cycle[i % 7] for i in range(count)]
    for i in (CHUNK - 1, CHUNK):          # last of the first chunk, first of the second
        if i < count:
            ns[i] = 0
    if count > 2 * CHUNK:                 # the whole middle chunk: no block, nothing launched for it
        for i in range(CHUNK, 2 * CHUNK):
            ns[i] = 0
        assert ns[2 * CHUNK] > 0
    return ns


@pytest.mark.parametrize("hyper", H, ids=H_IDS)
@pytest.mark.parametrize("count", [47, 48, 49, 60, 97])
@pytest.mark.parametrize("kind", KINDS)
def test_chunk_boundary_and_zero_length_entries(L, kind, count, hyper):
    """Tables around the 48-tensor chunk: zero-length entries (non-null pointers) first in
    the table, last in a chunk, first of the next, two in a row, and a whole chunk of
    them; first flags that differ inside a chunk (parity) and between chunks. Indices 48
    (and, at 97, 48..95) are empty and chunk 2 has the flags of chunk 0 under (i // 48) % 2,
    so count = 60 (non-empty tensors at 49..59) and the pattern i >= 48 are what tell
    first[i] from a chunk-local first[j] at 60 and at 97."""
    ns = chunk_lengths(count, B32 if kind == "f32" else B16)
    assert ns[0] == 0 and sum(ns) < 1_500_000
    if count > CHUNK:
        assert ns[CHUNK - 1] == 0 and ns[CHUNK] == 0
    for name, pattern in (("parity", lambda i: i % 2), ("chunk", lambda i: (i // CHUNK) % 2),
                          ("later", lambda i: int(i >= CHUNK))):
        t = Table(L, kind, ns, hyper, seed=count)
        t.step(0, [pattern(i) for i in range(count)], what=name)
        t.step(1, [0] * count, what=name)
        t.step(2, [0] * count, what=name)


@pytest.mark.parametrize("hyper", H, ids=H_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_first_across_steps(L, kind, hyper):
    """Step 0: every buffer created; step 1: one more tensor joins with first = 1 beside
    first = 0 ones; step 2: none created."""
    B = B32 if kind == "f32" else B16
    ns = [B + 3, 37, 2 * B, 5, B + 1]
    t = Table(L, kind, ns, hyper, seed=5)
    t.step(0, [1, 1, 1, 1], idx=[0, 1, 2, 3])
    t.step(1, [0, 0, 0, 0, 1])
    t.step(2, [0, 0, 0, 0, 0])


# ---------------------------------------------------------------- argument refusals
WD_MOM = (0.1, 0.9, 0.0, 1e-4, False)


def _raw(L, kind, P, G, Bf, N, F, count, hyper=WD_MOM, dtype=None):
    lr, mom, damp, wd, nest = hyper
    args = (P, G, Bf, N, F, count, lr, mom, damp, wd, int(nest))
    if kind == "f32":
        rc = L.dgc_sgd_step(*args, stream())
    else:
        rc = L.dgc_sgd_step16(*args, VD[kind] if dtype is None else dtype, stream())
    torch.cuda.synchronize()
    return rc


def _tables(t, count):
    P, G, Bf = (t.ptrs(r, range(count)) for r in "pgb")
    N = (ctypes.c_int64 * count)(*t.ns[:count])
    F = (ctypes.c_int32 * count)()
    return P, G, Bf, N, F


@pytest.mark.parametrize("kind", KINDS)
def test_argument_refusals_launch_nothing(L, kind):
    count = CHUNK + 2
    t = Table(L, kind, [5] * count, WD_MOM, seed=3)
    for r in "gb":
        t.arena[r].upload()
    before = {r: t.arena[r].download().copy() for r in "pgb"}
    P, G, Bf, N, F = _tables(t, count)
    assert _raw(L, kind, P, G, Bf, N, F, -1) == DGC_ERR_INVALID
    assert _raw(L, kind, None, G, Bf, N, F, count) == DGC_ERR_INVALID
    assert _raw(L, kind, P, None, Bf, N, F, count) == DGC_ERR_INVALID
    assert _raw(L, kind, P, G, Bf, None, F, count) == DGC_ERR_INVALID
    assert _raw(L, kind, P, G, None, N, F, count) == DGC_ERR_INVALID          # momentum with no buffers
    N2 = (ctypes.c_int64 * count)(*t.ns)
    N2[1] = -1
    assert _raw(L, kind, P, G, Bf, N2, F, count) == DGC_ERR_INVALID
    B2 = t.ptrs("b", range(count))
    B2[CHUNK + 1] = None                                                      # in the second chunk
    assert _raw(L, kind, P, G, B2, N, F, count) == DGC_ERR_INVALID
    P2 = t.ptrs("p", range(count))
    P2[CHUNK] = None                                                          # a null pointer with n > 0
    assert _raw(L, kind, P2, G, Bf, N, F, count) == DGC_ERR_INVALID
    if kind != "f32":
        assert _raw(L, kind, P, G, Bf, N, F, count, dtype=0) == DGC_ERR_DTYPE   # DGC_F32
        assert _raw(L, kind, P, G, Bf, N, F, count, dtype=7) == DGC_ERR_DTYPE
    assert L.dgc_last_error()
    for r in "pgb":   # a refusal in the second chunk included: nothing ran
        assert np.array_equal(t.arena[r].download(), before[r]), r
    assert _raw(L, kind, P, G, Bf, N, F, 0) == DGC_OK
    assert _raw(L, kind, None, None, None, None, None, 0) == DGC_OK
    for r in "pgb":
        assert np.array_equal(t.arena[r].download(), before[r]), r


@pytest.mark.parametrize("kind", KINDS)
def test_null_pointers_of_zero_length_entries_are_accepted(L, kind):
    """A zero-element CUDA tensor's data_ptr() is 0: an entry with numels[i] == 0 may carry
    null p / g / buf pointers (in either chunk); its neighbours are updated as usual."""
    count = CHUNK + 3
    ns = [7] * count
    for i in (0, 3, CHUNK - 1, CHUNK, count - 1):
        ns[i] = 0
    t = Table(L, kind, ns, WD_MOM, seed=9, null_empty=True)
    assert t.ptrs("p", [0])[0] is None and t.ptrs("b", [CHUNK])[0] is None and t.ptrs("g", [1])[0]
    t.step(0, [1] * count)
    t.step(1, [0] * count)


@pytest.mark.parametrize("kind", KINDS)
def test_momentum_without_weight_decay_needs_no_buffers(L, kind):
    """momentum != 0 with weight_decay == 0 keeps no buffer: bufs = NULL is accepted and p
    is updated."""
    t = Table(L, kind, [37, 2 * (B32 if kind == "f32" else B16) + 1], (0.1, 0.9, 0.0, 0.0, False), seed=4)
    before = [x.copy() for x in t.p]
    t.step(0, [0, 0], bufs=False)
    assert not np.array_equal(before[1], t.p[1])
