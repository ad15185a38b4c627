"""Flat-bucket DGC step with no host synchronisation (the padded fast path).

One gradient bucket per rank (fp32, or bf16 / fp16 with ``dtype``) goes through the
whole DGC step of the reference — compensate -> sample -> threshold -> select/adapt/resample -> update
(dgc/memory.py:50-77, dgc/compression.py:109-177) -> allgather
(dgc/compression.py:200-212) -> decompress (dgc/compression.py:179-194) — with
every decision kept on the device:

* the payload is fixed-capacity: ``[count | values(k) | indices(k)]`` per rank
  (``dgc_payload_layout``), so the RCCL allgather needs no size exchange and the
  decompress reads each rank's count on the device;
* the selection runs in ``DGC_SYNC_DEVICE`` mode (adaptation recounts and the
  resample chain are launched and early-exit on a device flag);
* the decompress is ``grad.zero_()`` (dgc/compression.py:191) followed by a sparse
  scatter of the gathered entries, both done by the receive side this engine shares with
  DGCBatch (``Receiver``, dgc/exchange.py; ``fill`` is explained there).
  ``"inline"`` (``"auto"``, the default) runs fill + scatter after the allgather.
  ``fill="allgather"`` issues the fill on a side stream right after the RCCL
  allgather is enqueued (ordered after the selection), so at W > 1 the 4 B/elem
  zero fill runs under the xGMI transfer instead of after it; the decompress then
  only scatters. ``"sparse"`` (opt-in, for a caller that owns ``out`` and never writes
  it: see ``Receiver``) re-zeroes only the previous step's W*k gathered slots of a
  persistent output, on a side stream at the start of the step so they run under K1.
* at W > 1 with a large step (``exchange_parts``, dgc/exchange.py) the allgather goes
  out in parts and each part is scattered as it lands, so only the last part's share
  of the W-dependent scatter is exposed after the exchange.

``dtype=torch.bfloat16`` / ``torch.float16``: momentum, velocity, gradient and output are
16-bit, every op of the reference rounded to the dtype as on the per-tensor path. K1-16
(``dgc_compress_begin16_clip``) streams the 16-bit state, writes the new velocity's exact fp32
image and takes the samples and the candidate lists from it; the selection then runs
pure on the image and the 16-bit state is masked from the payload
(``dgc_mask_packed16``), so nothing is ever deferred. The receive side is the 16-bit
packed decompress (``dgc_decompress_packed16``: dense fill, one exchange part).

``grad_dtype=torch.bfloat16`` / ``torch.float16`` with fp32 ``dtype``: fp32 momentum and
velocity under a 16-bit gradient, what the reference's compensate computes through torch's
type promotion (dgc/memory.py:50-63: every op in fp32 on the exactly widened gradient), so
bit for bit the fp32 step on ``grad.float()``. ``compensate`` takes the 16-bit gradient
(``dgc_compress_begin_g16``: K1 loads four 16-bit elements per lane and widens them in
registers, 18 B/elem, no widened copy); everything after it is the fp32 bucket's, ``out``
and ``apply``'s parameters fp32. No ``clip`` (a 16-bit gradient is clipped in its own dtype).

``clip=``: the reference's local gradient clipping (a ``dgc.clip_grad.ClipSpec``, or one of
``clip_grad_norm_`` (norm 2 / inf) / ``clip_grad_value_``, bare or as a ``functools.partial``)
fused into K1's load of the gradient: the bucket's statistic (``dgc_grad_stats`` /
``dgc_grad_stats16``), the coefficient (``dgc_clip_coefs`` / ``dgc_clip_coefs16``), then K1's
one call per precision, ``dgc_compress_begin_clip`` / ``dgc_compress_begin16_clip``, with
them (``_lib.NO_CLIP`` without a clip) — stream-ordered, nothing read back; ``clip_coef``
holds the device coefficient of the last step. The gradient stays as it was.

``step_apply(grad, optimizer)`` (fp32, one exchange part) ends the step with the optimizer's
update instead of a dense output: ``apply`` scatters the gathered entries into the bucket's
own accumulator and ``dgc_apply_packed`` steps the parameter from them
(``DGCSGD.step_sparse``), bit for bit ``step(grad, out)`` then ``DGCSGD.step()``.

The numerics are those of the drop-in ``DGCCompressor`` + ``DGCSGDMemory`` (same
kernels); the sample start is drawn from a ``random.Random`` seeded identically on
every rank, one draw per step, like the reference's global ``random`` call.
"""
import ctypes
import random

import torch
import torch.distributed as dist

from . import _lib
from . import clip_grad
from .compression import DGCCompressor
from .exchange import ReceiveSide, Receiver

__all__ = ["DGCBucket", "algorithmic_bytes"]

SEG = 1024   # the kernels' segment: a 16-bit bucket pads its state to whole segments


def algorithmic_bytes(numel, k, num_samples, world, vbytes=4, ibytes=8, sbytes=4, gbytes=None):
    """Bytes one rank must move per step:
    compensate 20N + select re-read 4N + dense decompress write 4N, the samples 4S,
    masking 8k, payload written k(vb+ib) + gathered W*k(vb+ib) read, scatter RMW 8Wk.
    sbytes: the state element size. 2 (a 16-bit bucket): compensate 3 x 2N read + 2 x 2N
    written + the 4N image, the image re-read 4N, the decompress write 2N, masking and
    scatter 2 B per entry and array. gbytes: the gradient's element size where it is not
    the state's (2 with sbytes 4, ``grad_dtype``: compensate 18N)."""
    image = 4 if sbytes < 4 else 0
    gbytes = sbytes if gbytes is None else gbytes
    return ((5 * sbytes + gbytes + image + 4) * numel + 4 * num_samples + 2 * sbytes * k
            + (1 + world) * k * (vbytes + ibytes) + 2 * sbytes * world * k)


class DGCBucket(ReceiveSide):
    def __init__(self, numel, compress_ratio=0.001, momentum=0.9, nesterov=True, momentum_masking=True,
                 sample_ratio=0.01, compress_upper_bound=1.3, compress_lower_bound=0.8,
                 max_adaptation_iters=10, resample=True, fp16_values=False, int32_indices=False,
                 device=None, world_size=None, seed=42, fill="auto", deferred_masking=True, exchange_parts="auto",
                 resample_order="topk", dtype=torch.float32, clip=None, grad_dtype=None):
        if fill not in ("auto", "inline", "allgather", "sparse"):
            raise ValueError(f"fill must be 'auto', 'inline', 'allgather' or 'sparse', not {fill!r}")
        if dtype not in (torch.float32,) + _lib.HALF:
            raise NotImplementedError(f"DGCBucket: fp32, bf16 or fp16 parameters (got {dtype})")
        if grad_dtype not in (None, torch.float32) + _lib.HALF:
            raise NotImplementedError(f"DGCBucket: fp32, bf16 or fp16 gradients (got grad_dtype={grad_dtype})")
        self.dtype = dtype
        self.half = dtype in _lib.HALF
        if grad_dtype not in (None, dtype):
            if self.half:
                raise ValueError(f"DGCBucket: {dtype} state takes {dtype} gradients (got grad_dtype={grad_dtype}); "
                                 "a 16-bit gradient onto fp32 state is dtype=torch.float32 with grad_dtype")
            if clip is not None:
                raise NotImplementedError(f"DGCBucket: clip with grad_dtype={grad_dtype} onto fp32 state (a 16-bit "
                                          "gradient is clipped in its own dtype before it is widened; not built)")
        # mixed: fp32 state, a bf16 / fp16 gradient widened in K1's load (dgc_compress_begin_g16)
        self.grad_dtype = grad_dtype if grad_dtype in _lib.HALF and not self.half else None
        if self.half and fill in ("allgather", "sparse"):
            raise NotImplementedError(f"DGCBucket: fill={fill!r} on {dtype} parameters (the 16-bit decompress is the "
                                      "dense fill with the scatter)")
        if clip is not None:
            spec = clip if isinstance(clip, clip_grad.ClipSpec) else clip_grad.spec_of(clip)
            if spec is None or not spec.batchable:
                raise NotImplementedError(f"DGCBucket: clip takes a local dgc.clip_grad function or spec (norm-2, "
                                          f"norm-inf or value; got {clip!r})")
            clip = spec
        self.clip = clip
        self.clip_coef = None   # device float[1] of the last step (None: no clip, or a fixed clamp)
        self.device = torch.device(device or "cuda")
        self.numel = N = int(numel)
        self.k, self.num_samples, self.top_k_samples, self.stride = DGCCompressor._attributes(
            N, *DGCCompressor._normalized(compress_ratio, sample_ratio))
        if self.grad_dtype is not None and N != self.num_samples and self.stride < 4:
            raise NotImplementedError(f"DGCBucket: grad_dtype={grad_dtype} onto fp32 state needs a sample stride >= 4 "
                                      f"(sample_ratio {sample_ratio} gives {self.stride}): the listing K1 has no "
                                      "unfused fallback")
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.world = world_size or (dist.get_world_size() if dist.is_initialized() else 1)
        self.momentum_masking = bool(momentum_masking)
        self.vdtype = torch.float16 if fp16_values else dtype
        self.idtype = torch.int32 if int32_indices else torch.int64
        self.rng = random.Random(seed)

        self.status = _lib.StatusSink("DGCBucket", self.device)   # DGC_K5_BROKEN, checked every step
        # update_memory 2: the first-k branches' DGCSGDMemory.update zeroing rides in the
        # next step's K1, which streams vec/mmt anyway (mmt/vec below flush it on read).
        # resample_order "index" (opt-in): an untied resample lists its set in index order
        # (DGCBatch's default); a flat bucket's resample (up to 64k candidates) mostly exceeds
        # the one-workgroup set path, so it keeps torch.topk's order by default
        p = _lib.select_params(N, self.k, self.num_samples, compress_upper_bound, compress_lower_bound,
                               max_adaptation_iters, resample, momentum_masking, 2 if deferred_masking else 1,
                               self.vdtype, self.idtype, resample_order=resample_order,
                               status_sink=self.status.address)
        if self.half:
            # the selection runs pure on the fp32 image (update_memory 0; with masking set and
            # no momentum dgc_compress_finish writes nothing), its threshold *= bound products
            # rounded to the dtype; momentum_masking decides what dgc_mask_packed16 masks
            p.update_memory, p.masking, p.thr_dtype = 0, 1, _lib.VD[dtype]
        self.params = p

        dev = self.device
        # 16-bit: state and image padded to whole 1024-element segments (+0, and K1-16 keeps
        # them so), so the kernel needs no scalar tail on them
        self.padded = -(-N // SEG) * SEG if self.half else N
        self._mmt = torch.zeros(self.padded, dtype=dtype, device=dev)
        self._vec = torch.zeros(self.padded, dtype=dtype, device=dev)
        self._vec32 = torch.zeros(self.padded, dtype=torch.float32, device=dev) if self.half else None
        self._pending = False
        L = _lib.lib()
        self.sampled = N != self.num_samples
        # zero-filled: per-tensor state (deferred masking, spill and window counts) lives in it
        self.ws = torch.zeros(L.dgc_compress_workspace(N, self.k, self.num_samples), dtype=torch.uint8,
                              device=dev)
        self.spec = torch.full((8,), float("inf"), dtype=torch.float32, device=dev)
        self.info = torch.zeros(_lib.INFO_BYTES, dtype=torch.uint8, device=dev)
        # the payload and gather buffers, the exchange and the decompress (dgc/exchange.py)
        self.rx = Receiver(self.k, N, self.world, self.vdtype, self.idtype, dev, self.status, fill, exchange_parts,
                           dtype=dtype, unsent="DGCBucket: decompress of a split exchange before exchange()")
        self._L = L
        if clip is not None:
            self._clip_numel = (ctypes.c_int64 * 1)(N)
        if self.fill in ("allgather", "sparse"):
            self.side = torch.cuda.Stream(device=dev)
            self._ev_go = torch.cuda.Event()
            self._ev_filled = torch.cuda.Event()

    # ---------------------------------------------------------------- state
    def flush(self):
        """Applies a deferred masking now (no-op when none is pending)."""
        if self._pending:
            _lib.check(self._L.dgc_compress_flush(self._vec.data_ptr(), self._mmt.data_ptr(), self.stride,
                                                  ctypes.byref(self.params), self.ws.data_ptr(), self.ws.numel(),
                                                  _lib.stream_of(self.device)), "dgc_compress_flush")
            self._pending = False

    @property
    def mmt(self):
        """Momentum (DGCSGDMemory.momentums), masking applied."""
        self.flush()
        return self._mmt[:self.numel] if self.half else self._mmt

    @property
    def vec(self):
        """Velocity (DGCSGDMemory.velocities), masking applied."""
        self.flush()
        return self._vec[:self.numel] if self.half else self._vec

    # ---------------------------------------------------------------- phases
    def compensate(self, grad):
        """K1: compensate + fused strided sample + speculative candidate lists. Raises
        first if a previous step's resample replay reported DGC_K5_BROKEN, or its
        decompress met an index or a gathered count out of range (``status``)."""
        self.status.check()
        L = self._L
        want = self.grad_dtype if self.grad_dtype is not None else self.dtype if self.half else None
        if want is not None:
            # exactly N elements of a 16-bit dtype: K1 (grad_dtype, which also names the state's
            # device) and K1-16 read the gradient to its last element. A refusal draws no sample start
            dev = self._mmt.device if self.grad_dtype is not None else None
            if not (torch.is_tensor(grad) and grad.is_cuda and dev in (None, grad.device) and grad.dtype == want
                    and grad.is_contiguous() and grad.numel() == self.numel and grad.data_ptr() % 16 == 0):
                raise ValueError(f"DGCBucket.compensate: grad must be a contiguous, 16-B aligned {want} CUDA tensor "
                                 f"of {self.numel} elements" + (f" on {dev}" if dev is not None else ""))
        self.rx.begin()
        self.start = self.rng.randint(0, self.stride - 1) if self.sampled else 0
        self.cnt = (self.numel - self.start + self.stride - 1) // self.stride if self.sampled else self.numel
        if self.grad_dtype is not None:   # (never with a clip)
            _lib.check(L.dgc_compress_begin_g16(grad.data_ptr(), _lib.VD[self.grad_dtype], self._mmt.data_ptr(),
                                                self._vec.data_ptr(), self.momentum, int(self.nesterov), self.start,
                                                self.stride, ctypes.byref(self.params), self.spec.data_ptr(),
                                                self.ws.data_ptr(), self.ws.numel(), _lib.stream_of(self.device)),
                       "dgc_compress_begin_g16")
            self._pending = False   # K1 applied it
            return
        clip = None
        if self.clip is not None:   # the bucket's statistic and coefficient, then the clip in K1's load
            self.clip_coef = self.clip.table_coefs((ctypes.c_void_p * 1)(grad.data_ptr()), self._clip_numel, 1,
                                                   self.device, dtype=self.dtype)
            clip = (self.clip.kind, self.clip_coef, self.clip.param)
        st = _lib.stream_of(self.device)
        if self.half:
            _lib.check(L.dgc_compress_begin16_clip(grad.data_ptr(), self._mmt.data_ptr(), self._vec.data_ptr(),
                                                   self._vec32.data_ptr(), self.momentum, int(self.nesterov),
                                                   self.start, self.stride, ctypes.byref(self.params),
                                                   self.spec.data_ptr(), *_lib.clip_args(clip), self.ws.data_ptr(),
                                                   self.ws.numel(), _lib.VD[self.dtype], st),
                       "dgc_compress_begin16_clip")
            return
        _lib.check(L.dgc_compress_begin_clip(grad.data_ptr(), self._mmt.data_ptr(), self._vec.data_ptr(),
                                             self.momentum, int(self.nesterov), self.start, self.stride,
                                             ctypes.byref(self.params), self.spec.data_ptr(), *_lib.clip_args(clip),
                                             self.ws.data_ptr(), self.ws.numel(), st), "dgc_compress_begin_clip")
        self._pending = False   # K1 applied it

    def select(self):
        """K3 threshold + K4 selection / adaptation / resample / emit + masking, into the payload."""
        L = self._L
        base = self.payload.data_ptr()
        self.params.order_out = base + 8   # header word 1: the W = 1 scatter's ascending-order flag
        if self.half:   # the pure selection on the image, then DGCSGDMemory.update on the 16-bit state
            st = _lib.stream_of(self.device)
            _lib.check(L.dgc_compress_finish(self._vec32.data_ptr(), None, self.start, self.stride, self.top_k_samples,
                                             ctypes.byref(self.params), self.spec.data_ptr(), _lib.SPEC_MARGIN,
                                             base + self.voff, base + self.ioff, base, self.info.data_ptr(),
                                             self.ws.data_ptr(), self.ws.numel(), _lib.SYNC_DEVICE, st),
                       "dgc_compress_finish")
            _lib.mask_packed16(self.payload, self.k, self.vdtype, self.idtype,
                               self._mmt if self.momentum_masking else None, self._vec, self.numel, self.device)
            return
        self._pending = self.params.update_memory == 2
        _lib.check(L.dgc_compress_finish(self._vec.data_ptr(), self._mmt.data_ptr(), self.start, self.stride,
                                         self.top_k_samples, ctypes.byref(self.params), self.spec.data_ptr(),
                                         _lib.SPEC_MARGIN, base + self.voff, base + self.ioff, base,
                                         self.info.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                         _lib.SYNC_DEVICE, _lib.stream_of(self.device)), "dgc_compress_finish")

    def decompress(self, out, dense=True, aliased=False):
        """dense: out = scale * (rank-order sum of the gathered entries), zeros elsewhere.
        dense=False: out already holds +0.0 (see ``Receiver.zero``); only the entries are
        written. fill="sparse": a dense decompress into the previous step's untouched
        output re-zeroes only the previous entries (see ``Receiver``). A 16-bit bucket:
        zero_(), the runs in rank order (each add rounded to the dtype), the 1/W scale,
        always dense (``HalfExchange``, or ``HalfSplitExchange`` when ``exchange_parts`` asked for
        a split: the same bits); its ``out`` is checked. ``aliased``: see ``step``."""
        if not dense:
            self.rx.scatter(out)
            return
        if self.half:
            _lib.require_out(out, self.dtype, self.numel, self.device, "DGCBucket.decompress")
        self.rx.decompress(out, aliased)

    def _zero_on_side(self, out, sparse):
        """zero_() of the output on the side stream. sparse: the re-zero of the previous
        step's entries, at the start of the step (ordered after everything already issued,
        e.g. an optimizer reading out), so it runs under K1 instead of before the scatter.
        Otherwise the dense fill, ordered after the event recorded at the end of the
        selection (so it never races a reader of the previous step)."""
        if sparse:
            self.side.wait_stream(torch.cuda.current_stream(self.device))
        else:
            self.side.wait_event(self._ev_go)
        self.rx.zero(out, self.side.cuda_stream, sparse)
        self._ev_filled.record(self.side)

    def step(self, grad, out, events=None):
        """compensate -> threshold -> select -> allgather -> decompress into ``out``;
        ``events`` maps a phase name to a (start, end) pair of torch.cuda.Event recorded
        around it on the current stream."""
        ev = events or {}
        self.status.check()   # before anything of this step is issued
        # an output that shares storage with the gradient (the reference's in-place
        # layout) is rewritten with each new gradient: always the dense fill there
        aliased = out.untyped_storage().data_ptr() == grad.untyped_storage().data_ptr()
        if aliased:
            self.rx.forget()
        cleared = self.fill == "sparse" and not aliased and self.rx.reusable(out)
        if cleared:
            self._zero_on_side(out, True)

        def decompress():
            if cleared or self.fill == "allgather":   # the entries onto the re-zeroed / filled output
                torch.cuda.current_stream(self.device).wait_event(self._ev_filled)
                self.rx.scatter(out, cleared)
            else:   # (16-bit: always)
                self.decompress(out, aliased=aliased)

        for name, fn in (("compensate", lambda: self.compensate(grad)), ("select", self.select),
                         ("allgather", self.exchange), ("decompress", decompress)):
            pair = ev.get(name)
            if pair:
                pair[0].record()
            fn()
            if pair:
                pair[1].record()
            if self.fill == "allgather":
                if name == "select":      # the fill may start once the selection is done ...
                    self._ev_go.record(torch.cuda.current_stream(self.device))
                elif name == "allgather":  # ... and is enqueued behind the RCCL launch
                    self._zero_on_side(out, False)

    # ---------------------------------------------------------------- sparse optimizer step
    _acc = _apply_ws = None   # apply's accumulator (+0.0 between steps) and stash, made on first use

    def _require_param(self, t, name):
        dev = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == torch.float32
                and t.is_contiguous() and t.numel() == self.numel):
            got = f"{t.dtype} [{t.numel()}] on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"DGCBucket.apply: {name} must be a contiguous fp32 CUDA tensor of {self.numel} elements "
                             f"on {dev} (got {got})")

    def apply(self, param, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, momentum_buffer=None,
              first=False):
        """In place of ``decompress(out)`` after ``exchange()``: DGCSGD's step on ``param``
        (dgc/optim/sgd.py:42-68) from the gathered entries, bit for bit ``decompress(p.grad)``
        then ``DGCSGD.step()``, with no dense gradient written for the optimizer to read back.
        The entries are scattered (K6, unchanged: rank-order sums, 1/W, status) into ``acc``,
        the bucket's own accumulator, +0.0 between steps; ``dgc_apply_packed`` then walks them,
        takes each sum out of ``acc`` and updates ``param`` — O(W * k) without weight decay, a
        dense pass over ``param`` (and ``momentum_buffer``) that loads no gradient with it.
        ``momentum_buffer`` / ``first``: DGCSGD's ``state[p]["momentum_buffer"]`` and whether
        this step creates it (needed when weight_decay and momentum are both nonzero).
        ``fill="sparse"``'s memory of the last ``out`` is left alone."""
        if self.half:
            raise NotImplementedError(f"DGCBucket.apply: fp32 parameters only (a {self.dtype} bucket takes decompress "
                                      "and DGCSGD.step)")
        if self.rx.parts > 1:
            raise ValueError(f"DGCBucket.apply: the exchange is split in {self.rx.parts} parts, whose part-major "
                             "gather layout apply does not walk; construct the bucket with exchange_parts=1")
        self._require_param(param, "param")
        use_buf = weight_decay != 0 and momentum != 0
        if use_buf:
            self._require_param(momentum_buffer, "momentum_buffer")
        if not lr >= 0:
            raise ValueError(f"DGCBucket.apply: lr must be >= 0 (got {lr})")
        L, rx = self._L, self.rx
        if self._acc is None:
            self._acc = torch.zeros(self.numel, dtype=torch.float32, device=param.device)
            self._apply_ws = torch.empty(L.dgc_apply_packed_workspace(self.world, self.k), dtype=torch.uint8,
                                         device=param.device)
        cur = rx.gathered
        # the exchange's scatter, not Receiver.scatter: acc is not a decompress output to remember
        rx.xchg.scatter(cur, rx._take(), self._acc, rx.scale, False)
        _lib.check(L.dgc_apply_packed(cur.data_ptr(), self.world, rx.rank_stride, self.k, _lib.VD[self.vdtype],
                                      _lib.ID[self.idtype], self._acc.data_ptr(), param.data_ptr(),
                                      momentum_buffer.data_ptr() if use_buf else None, int(bool(first)), self.numel,
                                      float(lr), float(momentum), float(dampening), float(weight_decay),
                                      int(bool(nesterov)), self._apply_ws.data_ptr(), self._apply_ws.numel(),
                                      _lib.stream_of(self.device)), "dgc_apply_packed")

    def step_apply(self, grad, optimizer, param=None, events=None):
        """compensate -> threshold -> select -> allgather -> ``optimizer.step_sparse(self,
        param)`` (a ``dgc.optim.DGCSGD``): ``step(grad, out)`` followed by the optimizer's
        ``step()`` on ``p.grad = out``, without ``out``. ``events`` as in ``step``; the last
        phase is ``"apply"``."""
        ev = events or {}
        self.status.check()   # before anything of this step is issued
        for name, fn in (("compensate", lambda: self.compensate(grad)), ("select", self.select),
                         ("allgather", self.exchange), ("apply", lambda: optimizer.step_sparse(self, param))):
            pair = ev.get(name)
            if pair:
                pair[0].record()
            fn()
            if pair:
                pair[1].record()

    def last_info(self):
        self.status.check(sync=True)
        return _lib.read_infos(self.info, ["DGCBucket"])[0]
