"""Split exchange: the packed allgather of a step (dgc/compression.py:200-212) in
``parts`` collectives, with the decompress (dgc/compression.py:179-194) of each part
scattered while the later parts are still in flight.

The W-dependent part of a flat step is the scatter of the W*k gathered entries: at
W = 8 and k = 1M it is ~0.3 ms, exposed after a single allgather. Split, the rank's
packed payload is re-laid out as ``parts`` part buffers (``dgc_payload_split``: the
entries in payload order, each part's header carrying the smallest index of the parts
after it), each part goes out in its own RCCL allgather on torch's NCCL stream, and
the compute stream waits for them one at a time: after part p it scatters every index
below the smallest such bound over the ranks (all of that index's entries have landed),
so only the last part's share is exposed. The dense result is the single-collective
decompress's bit for bit (same rank-order sums; tests/test_gpu_split.py).

Used by DGCBucket / DGCBatch at W > 1, through the ``Receiver`` both engines share: the
back half of a step — packed payload -> allgather (``SingleExchange`` or ``SplitExchange``;
for 16-bit parameters ``HalfExchange``, one allgather, or ``HalfSplitExchange``) ->
zero_() or sparse re-zero -> scatter; ``parts="auto"`` splits a
step of >= 2^21 gathered entries (2 parts at W <= 4, 4 at W = 8) and leaves smaller ones
to one allgather: each extra collective costs ~35 us of fixed hand-off
and hides at most its share of the scatter, which at 2M entries (flat-1B, W = 2: 0.07
ms) only breaks even and at VGG-16-BN's 1.1M (W = 8) loses.

16-bit parameters (bf16 / fp16) split only when asked — an integer ``exchange_parts`` or
``DGC_EXCHANGE_PARTS``; ``"auto"`` alone keeps their one allgather, its thresholds being
fp32 measurements. Their phases are K6-16 (``dgc_scatter_split16``): the same windows, each
index written once with its rank-order sum, every add and the 1/W scale rounded to the
dtype — ``dgc_decompress_packed16``'s result bit for bit (tests/test_gpu_split16.py) with
no pass over the output but the zero fill, so nothing dense is left after the last part.

``DGC_EXCHANGE_PARTS`` overrides ``"auto"``; every rank must issue the same collectives,
so an override is checked across the ranks when the layout is built (``agree``).
"""
import ctypes
import os

import torch

from . import _lib, comm

__all__ = ["HalfExchange", "HalfSplitExchange", "Receiver", "ReceiveSide", "ReuseMemory", "SingleExchange",
           "SplitExchange", "split_parts"]


def split_parts(world, capacity, parts="auto"):
    """The number of collectives for a step of ``capacity`` entries per rank."""
    env = os.environ.get("DGC_EXCHANGE_PARTS")
    if parts == "auto" and env:
        parts = int(env)
    multi = world > 1 or comm.one_rank_collectives()
    if parts == "auto":
        if not multi or world * capacity < (1 << 21):
            return 1
        return 2 if world <= 4 else 4
    parts = int(parts)
    if not multi or parts <= 1:
        parts = 1
    elif parts > 8 or world * parts > 64:
        raise ValueError(f"exchange parts must be 1..8 with world * parts <= 64 (world {world}, parts {parts})")
    if env and multi:
        agree(parts)
    return parts


def agree(parts):
    """Raises unless every rank chose ``parts`` (a per-rank DGC_EXCHANGE_PARTS that
    differs would issue different collectives and hang or corrupt the exchange). One
    MAX-allreduce of (parts, -parts) over the process group, at layout time only."""
    import torch.distributed as dist
    if not comm.is_initialized():
        return
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.tensor([parts, -parts], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    hi, lo = int(t[0]), -int(t[1])
    if hi != parts or lo != parts:
        raise RuntimeError(f"DGC_EXCHANGE_PARTS differs across ranks (parts between {lo} and {hi}); set the "
                           "same value on every rank")


class _Exchange:
    """What the exchanges share. All offer ``send(payload, gathered)`` -> handles,
    ``clear(prev_gathered, out, stream)``, ``scatter(gathered, handles, out, scale,
    cleared)`` (the entries onto an ``out`` that holds +0.0) and ``decompress`` (zero_()
    + scatter); ``streamed``: the handles are waited for one by one by the scatter."""

    def fill(self, out, stream):
        """zero_() of ``out`` (dgc/compression.py:191) as one dense fill on ``stream``."""
        _lib.check(self._L.dgc_fill_zero(out.data_ptr(), self.numel, stream), "dgc_fill_zero")

    def decompress(self, gathered, handles, out, scale, prev):
        """out = scale * (rank-order sum of the gathered entries), +0.0 elsewhere. The
        zero_() goes first, so it runs under the first part's collective: the dense fill,
        or (``prev``: the gathered buffer whose result ``out`` still holds) the re-zero."""
        st = _lib.stream_of(self.device)
        if prev is None:
            self.fill(out, st)
        else:
            self.clear(prev, out, st)
        self.scatter(gathered, handles, out, scale, prev is not None)


class SingleExchange(_Exchange):
    """One allgather of the whole payload and the packed decompress's workspace."""
    parts, streamed = 1, False

    def __init__(self, capacity, numel, world, rank_stride, vdtype, idtype, device):
        L = self._L = _lib.lib()
        self.numel, self.device = int(numel), device
        self.ws = torch.empty(L.dgc_decompress_packed_workspace(self.numel, world, capacity), dtype=torch.uint8,
                              device=device)
        self._layout = (world, rank_stride, capacity, _lib.VD[vdtype], _lib.ID[idtype])

    def send(self, payload, gathered):
        """Nothing is issued between this and the wait, so the allgather goes out on the
        current stream (``comm.COLLECTIVE_ISSUE``)."""
        return [comm.allgather_packed_async(payload, out=gathered, wait=True)]

    def _run(self, name, bufs, handles, out, scale=None, stream=None):
        for h in handles:
            h.wait()
        args = [b.data_ptr() for b in bufs] + [*self._layout, out.data_ptr(), self.numel]
        args += [] if scale is None else [scale]
        stream = _lib.stream_of(self.device) if stream is None else stream
        _lib.check(getattr(self._L, name)(*args, self.ws.data_ptr(), self.ws.numel(), stream), name)

    def scatter(self, gathered, handles, out, scale, cleared):
        self._run("dgc_scatter_packed_cleared" if cleared else "dgc_scatter_packed", [gathered], handles, out, scale)

    def clear(self, prev_gathered, out, stream):
        self._run("dgc_clear_packed", [prev_gathered], (), out, stream=stream)

    def decompress(self, gathered, handles, out, scale, prev):
        """The zero_() and the scatter in one call (the fill also resets the scatter's
        status words)."""
        if prev is None:
            self._run("dgc_decompress_packed", [gathered], handles, out, scale)
        else:
            self._run("dgc_decompress_packed_over", [gathered, prev], handles, out, scale)


def _dense_only16(what, dtype):
    """The refusal of a scatter without its fill (dense=False) on 16-bit parameters."""
    return NotImplementedError(f"{what}.decompress: dense=False on {dtype} parameters")


class HalfExchange(_Exchange):
    """One allgather of the whole payload and the 16-bit packed decompress (bf16 / fp16
    parameters): zero_(), the runs in rank order (each add rounded to the dtype) and the
    1/W scale in one call, always dense. It has no workspace; its error bits go straight
    to ``status``, whose name (the engine's) its refusals carry."""
    parts, streamed = 1, False
    send = SingleExchange.send

    def __init__(self, capacity, numel, world, rank_stride, vdtype, idtype, dtype, device, status):
        self._L, self.numel, self.device, self.dtype, self.status = _lib.lib(), int(numel), device, dtype, status
        self._layout = (world, rank_stride, capacity, _lib.VD[vdtype], _lib.ID[idtype])

    def decompress(self, gathered, handles, out, scale, prev):
        for h in handles:
            h.wait()
        _lib.check(self._L.dgc_decompress_packed16(
            gathered.data_ptr(), *self._layout, out.data_ptr(), _lib.VD[self.dtype], self.numel, scale,
            ctypes.c_void_p(self.status.decompress_words), _lib.stream_of(self.device)), "dgc_decompress_packed16")

    def scatter(self, gathered, handles, out, scale, cleared):
        raise _dense_only16(self.status.what, self.dtype)

    def clear(self, prev_gathered, out, stream):
        raise NotImplementedError(f"{self.status.what}: fill='sparse' on {self.dtype} parameters (the 16-bit "
                                  "decompress is the dense fill with the scatter)")


class _SplitLayout(_Exchange):
    """What the split exchanges share: the split payload of this rank, ``nbuf`` part-major
    gather buffers, the phase scatter's workspace (sized by ``workspace``, the name of
    its C entry point) and ``send``."""
    streamed = True
    workspace = "dgc_decompress_split_workspace"

    def __init__(self, capacity, numel, world, parts, vdtype, idtype, device, nbuf):
        L = self._L = _lib.lib()
        self.capacity, self.numel, self.world, self.parts = int(capacity), int(numel), int(world), int(parts)
        self.vd, self.id = _lib.VD[vdtype], _lib.ID[idtype]
        pc = ctypes.c_int64(0)
        self.part_bytes = L.dgc_payload_split_layout(self.capacity, self.parts, self.vd, self.id, ctypes.byref(pc))
        self.part_capacity = pc.value
        nb = L.dgc_payload_split_bytes(self.capacity, self.parts, self.vd, self.id)
        if self.part_bytes <= 0 or nb <= 0:
            raise ValueError(f"dgc_payload_split_layout: capacity {capacity}, parts {parts}")
        self.split = torch.zeros(nb, dtype=torch.uint8, device=device)   # its scratch must start zero
        self.gathers = [torch.zeros(self.parts * self.world * self.part_bytes, dtype=torch.uint8, device=device)
                        for _ in range(nbuf)]
        wsz = getattr(L, self.workspace)(self.numel, self.world, self.parts, self.capacity)
        if wsz == 0:
            raise ValueError(f"{self.workspace}: world {world}, parts {parts}")
        self.ws, self.device = torch.empty(wsz, dtype=torch.uint8, device=device), device

    def send(self, payload, gathered):
        """Splits this rank's payload and issues one allgather per part (in order on
        torch's collective stream, behind everything issued so far); returns the handles."""
        L, st = self._L, _lib.stream_of(self.device)
        _lib.check(L.dgc_payload_split(payload.data_ptr(), self.capacity, self.parts, self.vd, self.id,
                                       self.split.data_ptr(), st), "dgc_payload_split")
        pb, W = self.part_bytes, self.world
        return [comm.allgather_packed_async(self.split[p * pb:(p + 1) * pb],
                                            out=gathered[p * W * pb:(p + 1) * W * pb])
                for p in range(self.parts)]


class SplitExchange(_SplitLayout):
    """The split exchange of fp32 parameters: K6's phase scatter and the sparse re-zero."""

    def scatter(self, gathered, handles, out, scale, cleared):
        """The phases: each waits for its part (a stream wait under RCCL) and scatters
        what has landed. ``out`` holds +0.0 (cleared: re-zeroed by ``clear`` on this
        workspace)."""
        L, st = self._L, _lib.stream_of(self.device)
        for p, h in enumerate(handles):
            h.wait()
            _lib.check(L.dgc_scatter_split(gathered.data_ptr(), self.world, self.parts, p, self.capacity, self.vd,
                                           self.id, out.data_ptr(), self.numel, scale, int(bool(cleared) and p == 0),
                                           self.ws.data_ptr(), self.ws.numel(), st), "dgc_scatter_split")

    def clear(self, prev_gathered, out, stream):
        """The previous step's entries re-zeroed in ``out`` (which holds exactly that
        step's result), on ``stream``; also resets the phase scatter's status words."""
        _lib.check(self._L.dgc_clear_split(prev_gathered.data_ptr(), self.world, self.parts, self.capacity, self.vd,
                                           self.id, out.data_ptr(), self.numel, self.ws.data_ptr(), self.ws.numel(),
                                           stream), "dgc_clear_split")


class HalfSplitExchange(_SplitLayout):
    """The split exchange of bf16 / fp16 parameters: ``dgc_fill_zero16``, then K6-16's phase
    scatter (``dgc_scatter_split16``) — every index written once with its rank-order sum,
    each add and the 1/W scale rounded to the dtype, ``HalfExchange``'s result bit for bit
    with no pass over ``out`` but the fill. Always dense, as ``HalfExchange``: ``clear``
    refuses with its message (``Receiver.scatter`` refuses dense=False)."""
    workspace = "dgc_decompress_split16_workspace"
    clear = HalfExchange.clear

    def __init__(self, capacity, numel, world, parts, vdtype, idtype, dtype, device, status):
        super().__init__(capacity, numel, world, parts, vdtype, idtype, device, 1)
        self.dtype, self.status = dtype, status

    def fill(self, out, stream):
        """zero_() of the 16-bit ``out`` as one dense fill on ``stream``."""
        _lib.check(self._L.dgc_fill_zero16(out.data_ptr(), self.numel, stream), "dgc_fill_zero16")

    def scatter(self, gathered, handles, out, scale, cleared):
        """The phases onto an ``out`` that holds +0: each waits for its part, then
        scatters what has landed."""
        L, st = self._L, _lib.stream_of(self.device)
        for p, h in enumerate(handles):
            h.wait()
            _lib.check(L.dgc_scatter_split16(gathered.data_ptr(), self.world, self.parts, p, self.capacity, self.vd,
                                             self.id, out.data_ptr(), _lib.VD[self.dtype], self.numel, scale,
                                             self.ws.data_ptr(), self.ws.numel(), st), "dgc_scatter_split16")


class ReuseMemory:
    """Which output the last decompress wrote, and from which gathered buffer: what the
    sparse re-zero (``Receiver``) needs to know before it trusts an output's contents."""
    _last_out = _last_gathered = None   # (data_ptr, numel, _version) after the last decompress; its buffer

    def remember(self, out, gathered):
        self._last_out = (out.data_ptr(), out.numel(), out._version)
        self._last_gathered = gathered

    def forget(self):
        self._last_out = self._last_gathered = None

    def reusable(self, out):
        """out still holds exactly the last decompress's result: same storage, and no
        in-place write since by torch's version counter (ours are raw-pointer writes).
        **The blind spot**: writes through ``out.data`` (the reference's own idiom, e.g.
        ``grad.data.mul_``) and raw-pointer writes do not bump that counter, so after
        one this still answers True and a re-zero would leave stale values."""
        return self._last_gathered is not None and self._last_out == (out.data_ptr(), out.numel(), out._version)


class Receiver(ReuseMemory):
    """The receive side of a step, shared by DGCBucket and DGCBatch: this rank's packed
    payload ``[count | values | indices | extra]`` -> the exchange (one allgather, or
    ``parts`` of them; none at W = 1, where the gather buffers are the payload buffers)
    -> ``grad.zero_()`` (dgc/compression.py:191) -> the scatter of the gathered entries.

    ``dtype``: the parameters'. bf16 / fp16 take ``HalfExchange``: one part, always the
    dense 16-bit decompress, no fp32 decompress workspace (``dec_ws`` is None) — or, with
    an explicit ``exchange_parts`` / ``DGC_EXCHANGE_PARTS`` above 1, ``HalfSplitExchange``
    (``"auto"`` alone never splits them); dense too, ``fill`` stays ``"inline"``.

    ``fill``: how the zero_() is done. ``"inline"`` (``"auto"``, and always for 16-bit
    parameters) is a dense fill with the scatter. ``"sparse"`` (opt-in) treats ``out``
    as a persistent output: when it is the tensor the previous step decompressed into,
    not aliased to the gradient, unwritten since (``reusable``) and that step's gathered
    buffer is not the current one, it is +0.0 except at the previous step's W * capacity
    gathered indices, so only those slots are re-zeroed — the dense result is the same,
    bit for bit; any other ``out`` gets the dense fill. Payload and gather buffers then
    alternate between two (``begin``), so the previous step's indices survive the
    current step. Because of ``reusable``'s blind spot only a caller that owns ``out``
    and never writes it (the bench) should opt in. Any other value (DGCBucket's
    ``"allgather"``) is the caller's own orchestration of ``zero`` and ``scatter``.

    A bad index or gathered count in the decompress lands in ``status`` (raised at the
    next step); ``unsent`` is the error of a split decompress before its exchange."""

    def __init__(self, capacity, numel, world, vdtype, idtype, device, status, fill="auto", exchange_parts="auto",
                 payload_extra=0, dtype=torch.float32, unsent="decompress of a split exchange before send()"):
        self.capacity, self.numel, self.world = int(capacity), int(numel), int(world)
        self.scale, self.unsent = 1.0 / self.world, unsent
        half = dtype in _lib.HALF   # the parameters' dtype: 16-bit takes HalfExchange
        # the dense zero_() is always right; the re-zero is opt-in (fp32)
        self.fill = "inline" if fill == "auto" or half else fill
        self.rank_stride, self.voff, self.ioff = _lib.payload_layout(self.capacity, vdtype, idtype)
        # (W = 1 exchanges too when comm.one_rank_collectives(): the RCCL tests' one-rank group)
        self.exchanging = self.world > 1 or comm.one_rank_collectives()
        # 16-bit: "auto" alone never splits ("auto"'s thresholds are fp32 W > 1 measurements;
        # the 16-bit scatter has none yet); an explicit count or DGC_EXCHANGE_PARTS does
        asked = exchange_parts != "auto" or bool(os.environ.get("DGC_EXCHANGE_PARTS"))
        self.parts = split_parts(self.world, self.capacity, exchange_parts) if asked or not half else 1
        self.half, self.dtype, self.status = half, dtype, status
        # bytes appended to every rank's payload, after the packed entries (None when the
        # exchange is split, which carries the sparse entries only)
        self.extra_off = None
        if payload_extra > 0 and self.parts == 1:
            self.extra_off = self.rank_stride
            self.rank_stride = -(-(self.rank_stride + payload_extra) // 256) * 256
        nbuf = 2 if self.fill == "sparse" else 1
        self.payloads = [torch.zeros(self.rank_stride, dtype=torch.uint8, device=device) for _ in range(nbuf)]
        if self.parts > 1:
            self.xchg = (HalfSplitExchange(self.capacity, self.numel, self.world, self.parts, vdtype, idtype, dtype,
                                           device, status) if half else
                         SplitExchange(self.capacity, self.numel, self.world, self.parts, vdtype, idtype, device, nbuf))
            self.gathers = self.xchg.gathers
        else:
            self.gathers = ([torch.zeros(self.world * self.rank_stride, dtype=torch.uint8, device=device)
                             for _ in range(nbuf)] if self.exchanging else self.payloads)
            self.xchg = (HalfExchange(self.capacity, self.numel, self.world, self.rank_stride, vdtype, idtype, dtype,
                                      device, status) if half else
                         SingleExchange(self.capacity, self.numel, self.world, self.rank_stride, vdtype, idtype, device))
        # what other files read: the split exchange or None, the fp32 single one's workspace or None
        self.split = self.xchg if self.parts > 1 else None
        self.dec_ws = None if half or self.parts > 1 else self.xchg.ws
        if not half or self.parts > 1:   # (the one-allgather 16-bit decompress writes status's words itself)
            status.bind(self.xchg.ws)
        self._par, self._inflight = 0, []

    def begin(self):
        """A step starts: the other payload / gather buffer."""
        self._par += 1

    @property
    def payload(self):
        """This rank's packed payload of the current step."""
        return self.payloads[self._par % len(self.payloads)]

    @property
    def gathered(self):
        """The allgather buffer of the current step (the payload itself at W = 1)."""
        return self.gathers[self._par % len(self.gathers)]

    def send(self):
        """Issues the exchange of the current payload: one allgather, or one per part."""
        if self.exchanging:
            self._inflight = self.xchg.send(self.payload, self.gathered)

    def wait(self):
        """Waits for a single allgather; a split one is waited for part by part as
        ``scatter`` / ``decompress`` scatter it."""
        if not self.xchg.streamed:
            for h in self._take():
                h.wait()

    def _take(self):
        handles, self._inflight = self._inflight, []
        if self.xchg.streamed and not handles:
            raise RuntimeError(self.unsent)
        return handles

    def zero(self, out, stream, sparse=False):
        """zero_() of ``out`` on ``stream``: the dense fill, or (``sparse``; the caller
        checked ``reusable(out)`` before this step began) the re-zero of the previous
        step's entries."""
        if sparse:
            self.xchg.clear(self._last_gathered, out, stream)
        else:
            self.xchg.fill(out, stream)

    def scatter(self, out, cleared=False):
        """Only the entries, onto an ``out`` that ``zero`` filled (``cleared``: re-zeroed).
        16-bit parameters refuse (``HalfExchange.scatter``), split or not."""
        if self.half and self.parts > 1:
            raise _dense_only16(self.status.what, self.dtype)
        cur = self.gathered
        self.xchg.scatter(cur, self._take(), out, self.scale, cleared)
        self.remember(out, cur)

    def decompress(self, out, aliased=False):
        """out = the rank-order sum of the gathered entries / W, +0.0 elsewhere.
        ``aliased``: ``out`` shares storage with the gradient (the reference's in-place
        layout), rewritten by every backward: always the dense fill, nothing remembered."""
        cur, handles = self.gathered, self._take()
        sparse = (self.fill == "sparse" and not aliased and self.reusable(out) and self._last_gathered is not cur)
        self.xchg.decompress(cur, handles, out, self.scale, self._last_gathered if sparse else None)
        self.remember(out, cur)
        if aliased:
            self.forget()


def _rx(name):
    """An engine attribute that lives in its ``rx``: read and assigned through the engine."""
    return property(lambda self: getattr(self.rx, name), lambda self, value: setattr(self.rx, name, value))


class ReceiveSide:
    """The engines' view of their ``rx`` (a ``Receiver``), as bench.py, horovod/batched.py,
    tools/ and the tests read it — and assign it: bench.py switches a sparse bucket's
    ``fill`` to "inline" and back, a test injects ``_gathers``. ``xchg``: None unless split."""
    payload, gathered, rank_stride, voff, ioff = map(_rx, ("payload", "gathered", "rank_stride", "voff", "ioff"))
    extra_off, parts, exchanging, dec_ws, xchg = map(_rx, ("extra_off", "parts", "exchanging", "dec_ws", "split"))
    fill, _gathers = _rx("fill"), _rx("gathers")

    def exchange(self):
        """The packed allgather (RCCL over xGMI; gloo stages through the host), waited
        for on the spot. Split (``parts`` > 1): the parts' collectives are only issued;
        decompress waits for each as it scatters it."""
        self.rx.send()
        self.rx.wait()
