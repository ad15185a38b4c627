"""dgc_apply_packed: DGCSGD's step from the gathered packed payload, no dense gradient read.

Single process, C ABI: W hand-made rank payloads (as tests/test_gpu_split.py builds them) are
scattered into a +0.0 accumulator with dgc_scatter_packed, then applied. ``param`` and the
momentum buffer must be, bit for bit (compared as uint32), the reference's op sequence
(dgc/optim/sgd.py:42-68) run with torch on the CPU over the oracle's decompress — which must
itself equal oracle.dgcsgd_step32, the expectation K7 is pinned to — and what
the existing path (dgc_decompress_packed + dgc_sgd_step) leaves; the accumulator must be
+0.0 everywhere after every call."""
import ctypes

import numpy as np
import pytest
import torch

import oracle.dgc_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LR = 0.1

# (weight_decay, momentum, dampening, nesterov, steps)
HYPERS = {
    "wd0": (0.0, 0.0, 0.0, 0, 1),
    "wd": (1e-4, 0.0, 0.0, 0, 1),
    "wd_mom_damp": (1e-4, 0.9, 0.1, 0, 2),
    "wd_nesterov": (1e-4, 0.9, 0.0, 1, 2),
}


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    return _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(L, rc):
    assert rc == 0, L.dgc_last_error().decode()


def bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


def _rank_payload(L, v, i, cap, vd, idt, garbage_from=None):
    """One rank's packed payload. garbage_from: the slots past the count are filled with
    indices >= garbage_from and NaN values (a count says where the entries end)."""
    vo, io = ctypes.c_int64(0), ctypes.c_int64(0)
    stride = L.dgc_payload_layout(cap, vd, idt, ctypes.byref(vo), ctypes.byref(io))
    p = np.zeros(stride, np.uint8)
    count = len(i)
    if garbage_from is not None:
        v = np.concatenate([v, np.full(cap - count, np.nan, np.float32)])
        i = np.concatenate([i, garbage_from + np.arange(cap - count, dtype=np.int64)])
    v = v.astype(np.float16 if vd else np.float32)
    i = i.astype(np.int32 if idt else np.int64)
    p[:8] = np.frombuffer(np.int64(count).tobytes(), np.uint8)
    p[vo.value: vo.value + v.nbytes] = np.frombuffer(v.tobytes(), np.uint8)
    p[io.value: io.value + i.nbytes] = np.frombuffer(i.tobytes(), np.uint8)
    return torch.from_numpy(p).to(DEV)


def _runs(rng, N, W, cap, overlap, shuffled):
    shared = np.sort(rng.choice(N, cap, replace=False))
    runs = []
    for r in range(W):
        c = int(rng.integers(cap // 2, cap + 1))
        own = rng.choice(N, c, replace=False)
        pick = rng.random(c) < overlap
        idx = np.unique(np.where(pick, shared[:c], own))[:c]
        v = rng.standard_normal(idx.size).astype(np.float32)
        if shuffled and r == W - 1:   # the last rank in topk (arbitrary) order
            o = rng.permutation(idx.size)
            v, idx = v[o], idx[o]
        runs.append((v, idx.astype(np.int64)))
    return runs


def _same_runs(rng, N, W, cap):
    """Every rank sends the same indices; rank 2 sends nothing."""
    idx = np.sort(rng.choice(N, cap * 5 // 8, replace=False)).astype(np.int64)
    return [(rng.standard_normal(idx.size).astype(np.float32), idx) if r != 2 else
            (np.zeros(0, np.float32), np.zeros(0, np.int64)) for r in range(W)]


def _cancelling_runs(rng, N, cap):
    """W = 2: at 16 shared indices rank 1 sends -v where rank 0 sends v."""
    runs = _runs(rng, N, 2, cap, 0.5, False)
    (v0, i0), (v1, i1) = runs
    common = np.intersect1d(i0, i1)[:16]
    v1 = v1.copy()
    v1[np.searchsorted(i1, common)] = -v0[np.searchsorted(i0, common)]
    return [(v0, i0), (v1, i1)], common


def _bad_index_runs(rng, N, cap):
    """W = 2: rank 1 ends with one index >= N."""
    runs = _runs(rng, N, 2, cap - 1, 0.5, False)
    v1, i1 = runs[1]
    runs[1] = (np.append(v1, np.float32(3.0)), np.append(i1, np.int64(N + 5)))
    return runs


def _wire(runs, fp16):
    return [v.astype(np.float16).astype(np.float32) if fp16 else v for v, _ in runs]


def ref_step(p, buf, g, wd, mom, damp, nesterov):
    """The reference's DGCSGD.step on CPU tensors (dgc/optim/sgd.py:50-68); returns the
    momentum buffer."""
    if wd == 0:
        p.add_(g, alpha=-LR)
        return None
    d = wd * p
    if mom != 0:
        if buf is None:
            buf = d.clone()
        else:
            buf.mul_(mom).add_(d, alpha=1 - damp)
        d = d.add(buf, alpha=mom) if nesterov else buf
    p.add_(d.add(g), alpha=-LR)
    return buf


class Apply:
    """The buffers of one (N, W, capacity, wire format): workspaces, the accumulator, and the
    calls under test / of the existing path."""

    def __init__(self, L, N, W, cap, vd, idt):
        self.L, self.N, self.W, self.cap, self.vd, self.idt = L, N, W, cap, vd, idt
        self.stride = L.dgc_payload_layout(cap, vd, idt, None, None)
        self.ws = torch.empty(L.dgc_decompress_packed_workspace(N, W, cap), dtype=torch.uint8, device=DEV)
        nstash = L.dgc_apply_packed_workspace(W, cap)
        assert nstash >= 4 * W * cap
        self.stash = torch.empty(nstash, dtype=torch.uint8, device=DEV)
        self.acc = torch.zeros(N, device=DEV)
        self.out = torch.empty(N, device=DEV)

    def layout(self):
        return self.W, self.stride, self.cap, self.vd, self.idt

    def gather(self, runs, garbage=False):
        return torch.cat([_rank_payload(self.L, v, i, self.cap, self.vd, self.idt, self.N + 7 if garbage else None)
                          for v, i in runs])

    def apply(self, g, p, buf, first, wd, mom, damp, nesterov):
        L = self.L
        check(L, L.dgc_scatter_packed(P(g), *self.layout(), P(self.acc), self.N, 1.0 / self.W, P(self.ws),
                                      self.ws.numel(), stream()))
        status = self.status()
        check(L, L.dgc_apply_packed(P(g), *self.layout(), P(self.acc), P(p), P(buf), int(first), self.N, LR, mom, damp,
                                    wd, nesterov, P(self.stash), self.stash.numel(), stream()))
        torch.cuda.synchronize()
        assert int(self.acc.view(torch.int32).count_nonzero()) == 0, "acc is not +0.0 after the apply"
        return status

    def existing(self, g, p, buf, first, wd, mom, damp, nesterov):
        """The path this replaces: the dense decompress, then K7 reading it."""
        L = self.L
        check(L, L.dgc_decompress_packed(P(g), *self.layout(), P(self.out), self.N, 1.0 / self.W, P(self.ws),
                                         self.ws.numel(), stream()))
        one = ctypes.c_void_p * 1
        bufs = one(buf.data_ptr() if buf is not None else 0)
        check(L, L.dgc_sgd_step(one(p.data_ptr()), one(self.out.data_ptr()), bufs, (ctypes.c_int64 * 1)(self.N),
                                (ctypes.c_int32 * 1)(int(first)), 1, LR, mom, damp, wd, nesterov, stream()))
        torch.cuda.synchronize()

    def status(self):
        st = ctypes.c_int32(-1)
        check(self.L, self.L.dgc_decompress_status(P(self.ws), ctypes.byref(st), stream()))
        return st.value


def _plant_zeros(p_ref, touched, N):
    """+0.0 and -0.0 in the parameter at gathered and at never-gathered positions; returns
    the positions (touched +0, touched -0, untouched +0, untouched -0)."""
    touched = np.unique(touched[(touched >= 0) & (touched < N)])
    free = np.setdiff1d(np.arange(N - 64, N), touched)   # includes the tail after the last float4
    assert touched.size >= 4 and free.size >= 4
    pos = (touched[[0, -1]], touched[[1, -2]], free[[0, -1]], free[[1, -2]])
    for q, z in zip(pos, (0.0, -0.0, 0.0, -0.0)):
        p_ref[torch.from_numpy(q)] = z
    b = bits(p_ref)
    assert (b[pos[0]] == 0).all() and (b[pos[1]] == 0x80000000).all()
    assert (b[pos[2]] == 0).all() and (b[pos[3]] == 0x80000000).all()
    return pos


def _device_view(N, offset):
    """A parameter-sized view, at a 1-element (4-B) offset of a larger tensor when asked:
    not 16-B aligned, K7's scalar path."""
    t = torch.zeros(N + 4, device=DEV)
    return t[1:N + 1] if offset else t[:N]


def run_case(L, N, W, cap, fp16, int32, hyper, make_runs, offset=False, garbage=False, shuffled=False,
             bad_index=False, seed=0):
    wd, mom, damp, nesterov, steps = HYPERS[hyper]
    rng = np.random.default_rng(N + 31 * W + cap + seed)
    ap = Apply(L, N, W, cap, int(fp16), int(int32))
    p_ref = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    buf_ref = None
    use_buf = wd != 0 and mom != 0
    p_new, p_old = _device_view(N, offset), _device_view(N, offset)
    buf_new = _device_view(N, offset) if use_buf else None
    buf_old = _device_view(N, offset) if use_buf else None
    if offset:
        assert p_new.data_ptr() % 16 == 4
    for step in range(steps):
        runs = make_runs(rng)
        assert all(len(i) <= cap for _, i in runs)
        idx_all = np.concatenate([i for _, i in runs])
        if W > 1:   # an index in at least two runs: the duplicates' path runs
            seen = np.concatenate([np.unique(i) for _, i in runs])
            assert (np.unique(seen, return_counts=True)[1] >= 2).any()
        _plant_zeros(p_ref, idx_all, N)
        for t in (p_new, p_old):
            t.copy_(p_ref)
        # the expectation: the entries inside [0, N) (all of them, but for the bad-index case)
        good = [(wv[(i >= 0) & (i < N)], i[(i >= 0) & (i < N)]) for wv, (_, i) in zip(_wire(runs, fp16), runs)]
        assert bad_index or sum(len(i) for _, i in good) == idx_all.size
        g_ref = torch.from_numpy(O.decompress([v for v, _ in good], [i for _, i in good], N, W))
        p_in, buf_in = p_ref.numpy().copy(), None if buf_ref is None else buf_ref.numpy().copy()
        buf_ref = ref_step(p_ref, buf_ref, g_ref, wd, mom, damp, nesterov)
        # the second expectation: the fp32 oracle (pinned to the reference by tests/golden/sgd32.*)
        p_o, buf_o = O.dgcsgd_step32(p_in, g_ref.numpy(), buf_in, LR, mom, damp, wd, nesterov)
        assert np.array_equal(bits(p_o), bits(p_ref)), (hyper, step, "oracle / torch-CPU sequence")
        if use_buf:
            assert np.array_equal(bits(buf_o), bits(buf_ref)), (hyper, step, "oracle / torch-CPU sequence buffer")
        g = ap.gather(runs, garbage)
        first = use_buf and step == 0
        status = ap.apply(g, p_new, buf_new, first, wd, mom, damp, nesterov)
        if bad_index:
            assert status & 1, status   # the scatter reported the index; the apply skipped it
        else:
            assert status == (2 if shuffled else 0), status
        ap.existing(g, p_old, buf_old, first, wd, mom, damp, nesterov)
        assert np.array_equal(bits(p_old), bits(p_ref)), (hyper, step, "existing path / reference")
        assert np.array_equal(bits(p_new), bits(p_ref)), (hyper, step, "param")
        if use_buf:
            assert np.array_equal(bits(buf_old), bits(buf_ref)), (hyper, step, "existing path / reference buffer")
            assert np.array_equal(bits(buf_new), bits(buf_ref)), (hyper, step, "momentum buffer")
    return g_ref


SHAPES = [
    # N, W, cap, overlap, fp16, int32, shuffled, offset
    (50_003, 1, 500, 0.0, False, False, False, False),     # one run; N no multiple of 4 or 4096
    (50_003, 1, 500, 0.0, False, False, False, True),      # param and buf unaligned: K7's scalar path
    (1_000_003, 2, 1000, 0.5, False, False, False, False),  # duplicates across ranks
    (1_000_003, 8, 1000, 0.3, True, True, False, False),   # fp16 wire values, int32 indices
    (300_000, 8, 30000, 0.3, False, False, False, False),  # crowded chunks
    (1_000_003, 4, 1000, 0.3, False, False, True, False),  # the last rank in topk order
]


@pytest.mark.parametrize("hyper", list(HYPERS))
@pytest.mark.parametrize("N,W,cap,overlap,fp16,int32,shuffled,offset", SHAPES)
def test_apply_matches_reference(L, N, W, cap, overlap, fp16, int32, shuffled, offset, hyper):
    run_case(L, N, W, cap, fp16, int32, hyper, lambda rng: _runs(rng, N, W, cap, overlap, shuffled), offset=offset,
             shuffled=shuffled)


@pytest.mark.parametrize("hyper", list(HYPERS))
def test_apply_same_indices_empty_rank_and_garbage_slots(L, hyper):
    """Every rank sends the same indices, rank 2 nothing; the slots past every count hold
    indices >= N and NaN values, which the count alone must keep out."""
    N, W, cap = 20_000, 4, 64
    run_case(L, N, W, cap, False, False, hyper, lambda rng: _same_runs(rng, N, W, cap), garbage=True)


@pytest.mark.parametrize("hyper", list(HYPERS))
def test_apply_skips_sums_of_zero(L, hyper):
    """v in rank 0 and -v in rank 1 at >= 10 indices: their sums are +0.0, the slots the
    apply skips — the reference's result there is the g = +0 one all the same."""
    N, cap = 1_000_003, 1000
    found = []

    def make(rng):
        runs, common = _cancelling_runs(rng, N, cap)
        found.append(common)
        return runs

    g_ref = run_case(L, N, 2, cap, False, False, hyper, make, seed=1)
    assert len(found[-1]) >= 10
    assert (bits(g_ref)[found[-1]] == 0).all()


@pytest.mark.parametrize("hyper", ["wd0", "wd_nesterov"])
def test_apply_skips_an_index_out_of_range(L, hyper):
    """One index >= N in rank 1: dgc_decompress_status reports bit 0 and every element equals
    the expectation computed without that entry (the kernels check the bounds before any
    access: nothing is read or written outside the tensors)."""
    N, cap = 1_000_003, 1000
    run_case(L, N, 2, cap, False, False, hyper, lambda rng: _bad_index_runs(rng, N, cap), bad_index=True, seed=2)
