"""Every compressed tensor of a training step through ONE set of launches.

The reference compresses tensor by tensor, from one autograd hook per parameter,
with two Horovod allgathers per tensor (dgc/horovod/optimizer.py:116-155,
dgc/compression.py:155-212). ``DGCBatch`` keeps the per-tensor numerics exactly —
the same attributes (dgc/compression.py:56-89), one ``random.randint(0, stride - 1)``
per tensor and step in the tensors' order (dgc/compression.py:118), the same
compensate / threshold / adaptation / resample / masking per tensor — but lays the
tensors side by side in three flat fp32 buffers (gradients, momentums, velocities;
each tensor at a 1024-element-aligned offset) and runs

    dgc_batch_compress   K1 over all tensors, K3 for all thresholds, the selection
                         chain with per-tensor state, one packed payload (called as its
                         halves dgc_batch_compress_begin[_ptrs]_clip — the clip, or
                         ``_lib.NO_CLIP``, is K1's argument — and dgc_batch_compress_finish)
    one allgather        the packed payload, RCCL over xGMI (gloo stages via the host)
    decompress           zero fill + scatter over the flat output (``fill="auto"``/``"inline"``,
                         the default), or — opted in with ``fill="sparse"`` by a caller that
                         owns the output and never writes it — only the previous step's
                         gathered indices are re-zeroed, as in ``DGCBucket``: the receive side
                         both engines share (``Receiver``, dgc/exchange.py) explains it

with O(1) launches per phase and no host synchronisation. The payload carries flat
indices (tensor offset + index in the tensor), tensor after tensor.

``grad(name)`` / ``momentum(name)`` / ``velocity(name)`` / ``out(name)`` are views in
the flat buffers (the parameter-shaped tensors the reference keeps per name).
"""
import ctypes
import math
import random

import torch
import torch.distributed as dist

from . import _lib
from .compression import DGCCompressor
from .exchange import ReceiveSide, Receiver

__all__ = ["DGCBatch"]

SEG = 1024   # tensors start at multiples of this many elements (the kernels' segment)


class DGCBatch(ReceiveSide):
    def __init__(self, named_shapes, compress_ratio=0.001, momentum=0.9, nesterov=False, momentum_masking=True,
                 sample_ratio=0.01, compress_upper_bound=1.3, compress_lower_bound=0.8, max_adaptation_iters=10,
                 resample=True, fp16_values=False, int32_indices=False, device=None, world_size=None, seed=None,
                 deferred_masking=True, fill="auto", dtype=torch.float32, exchange_parts="auto",
                 resample_order="index", payload_extra=0, clip=None):
        if fill not in ("auto", "inline", "sparse"):
            raise ValueError(f"fill must be 'auto', 'inline' or 'sparse', not {fill!r}")
        if dtype not in (torch.float32,) + _lib.HALF:
            raise NotImplementedError(f"DGCBatch: fp32, bf16 or fp16 parameters (got {dtype})")
        self.dtype = dtype
        self.half = dtype in _lib.HALF
        # local gradient clipping fused into K1: a dgc.clip_grad.ClipSpec (norm-2, norm-inf
        # or value) — one statistic per tensor over K1's own pointer table, the
        # coefficients, then the clipped K1: three more launches per step up to 64 tensors.
        # 16-bit: the statistics over the flat buffer's tensors (dgc_grad_stats16), the
        # coefficients in the dtype, then the multi-tensor K1-16 (dgc_compensate16_multi_clip)
        if clip is not None and not getattr(clip, "batchable", False):
            raise NotImplementedError(f"DGCBatch: clip takes a local dgc.clip_grad spec (norm-2, norm-inf or value; "
                                      f"got {clip!r})")
        self.clip = clip
        self.clip_coefs = None   # device float[T] of the last step (None: a fixed clamp)
        self._fill = fill
        self.exchange_parts = exchange_parts
        _lib.resample_order_flag(resample_order)   # validates
        # "index": a resampled tensor whose k-th largest candidate is untied lists its
        # top-k set in index order (the decompress and the memory update depend on the
        # set only; dgc_select_params.resample_order); "topk": torch.topk's order always
        self.resample_order = resample_order
        # bytes appended to every rank's payload (after the packed entries): the batched
        # optimizer's dense wire values ride in the same allgather (``extra_off``; None
        # when the exchange is split, which carries the sparse entries only)
        self.payload_extra = int(payload_extra)
        self.device = torch.device(device or "cuda")
        self.names = [n for n, _ in named_shapes]
        self.shapes = {n: tuple(s) for n, s in named_shapes}
        self.numels = [math.prod(self.shapes[n]) for n in self.names]
        self.momentum, self.nesterov, self.momentum_masking = float(momentum), bool(nesterov), bool(momentum_masking)
        _, self.sample_ratio = DGCCompressor._normalized(compress_ratio, sample_ratio)
        self.upper, self.lower = float(compress_upper_bound), float(compress_lower_bound)
        self.max_iters, self.resample = int(max_adaptation_iters), bool(resample)
        self.vdtype = torch.float16 if fp16_values else dtype
        self.idtype = torch.int32 if int32_indices else torch.int64
        self.world = world_size or (dist.get_world_size() if dist.is_initialized() else 1)
        self.rng = random.Random(seed) if seed is not None else random   # the reference draws from `random`
        offs, end = [], 0
        for n in self.numels:
            offs.append(end)
            end += -(-n // SEG) * SEG
        self.offsets = offs
        self.flat_numel = max(end, SEG)
        dev = self.device
        self.grad_flat = torch.zeros(self.flat_numel, dtype=dtype, device=dev)
        self._mmt_flat = torch.zeros(self.flat_numel, dtype=dtype, device=dev)
        self._vec_flat = torch.zeros(self.flat_numel, dtype=dtype, device=dev)
        # 16-bit: K1-16 (dgc_compensate16_clip) rounds every op to the dtype and writes the new
        # velocity's exact fp32 image, which the selection reads (dgc_batch_select); the
        # 16-bit state is masked from the payload (dgc_mask_packed16)
        self._vec32 = torch.zeros(self.flat_numel, dtype=torch.float32, device=dev) if self.half else None
        self.deferred_masking = bool(deferred_masking) and not self.half
        self._pending = False
        self.out_flat = torch.zeros(self.flat_numel, dtype=dtype, device=dev)
        self._L = _lib.lib()
        self.info = torch.zeros(len(self.names) * _lib.INFO_BYTES, dtype=torch.uint8, device=dev)
        # DGC_K5_BROKEN and the decompress's bad index / gathered count (a peer's payload
        # corrupted in transit), written by the kernels into pinned words, checked every step
        self.status = _lib.StatusSink("DGCBatch", dev)
        self._acc = None   # apply()'s fp32 accumulator over the flat layout, made on first use
        self.set_ratio(compress_ratio)

    # ---------------------------------------------------------------- layout
    def set_ratio(self, compress_ratio):
        """(Re-)derive every tensor's attributes for a compress ratio and write the
        device tables — ``DGCCompressor.initialize`` (dgc/compression.py:56-89), also
        what ``warmup_compress_ratio`` re-runs on a ratio change (:91-107)."""
        ratio, _ = DGCCompressor._normalized(compress_ratio, self.sample_ratio)
        self.flush()   # a pending masking lives in the old workspace
        self.ratio = ratio
        T = len(self.names)
        self.attrs = [DGCCompressor._attributes(n, ratio, self.sample_ratio) for n in self.numels]
        arr = lambda xs: (ctypes.c_int64 * T)(*xs)   # noqa: E731
        self._arrays = [arr(self.numels), arr(self.offsets), arr([a[0] for a in self.attrs]),
                        arr([a[1] for a in self.attrs]), arr([a[2] for a in self.attrs]), arr([a[3] for a in self.attrs])]
        d = _lib.BatchDesc()
        d.count = T
        d.numel, d.offset, d.num_selects, d.num_samples, d.top_k_samples, d.sample_stride = self._arrays
        d.flat_numel = self.flat_numel
        d.upper_bound, d.lower_bound = self.upper, self.lower
        d.max_iters, d.resample, d.momentum_masking = self.max_iters, int(self.resample), int(self.momentum_masking)
        d.fp16_values, d.int32_indices = int(self.vdtype == torch.float16), int(self.idtype == torch.int32)
        d.nesterov, d.momentum, d.spec_margin = int(self.nesterov), self.momentum, _lib.SPEC_MARGIN
        d.deferred_masking = int(self.deferred_masking)
        d.dtype = _lib.VD[self.dtype]
        d.status_sink = self.status.address
        d.resample_order = _lib.resample_order_flag(self.resample_order)
        self.desc = d
        L = self._L
        wsz = L.dgc_batch_workspace(ctypes.byref(d))
        if wsz == 0:
            raise RuntimeError(f"dgc_batch_workspace: {L.dgc_last_error().decode()}")
        self.ws = torch.empty(wsz, dtype=torch.uint8, device=self.device)
        _lib.check(L.dgc_batch_init(ctypes.byref(d), self.ws.data_ptr(), wsz, _lib.stream_of(self.device)),
                   "dgc_batch_init")
        self.capacity = sum(a[0] for a in self.attrs)
        self._apply_ws = None   # apply()'s stash: a word per gathered slot of this capacity
        # a new layout: a new receive side (payload / gather buffers, exchange, decompress
        # workspace bound to ``status``), which remembers nothing of the previous step
        self.rx = Receiver(self.capacity, self.flat_numel, self.world, self.vdtype, self.idtype, self.device,
                           self.status, self._fill, self.exchange_parts, self.payload_extra, self.dtype,
                           unsent="DGCBatch: decompress of a split exchange before send() / exchange()")

    def flush(self):
        """Applies a deferred masking now (no-op when none is pending)."""
        if self._pending:
            _lib.check(self._L.dgc_batch_flush(ctypes.byref(self.desc), self._mmt_flat.data_ptr(),
                                               self._vec_flat.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                               _lib.stream_of(self.device)), "dgc_batch_flush")
            self._pending = False

    @property
    def mmt_flat(self):
        """Flat momentum buffer, masking applied."""
        self.flush()
        return self._mmt_flat

    @property
    def vec_flat(self):
        """Flat velocity buffer, masking applied."""
        self.flush()
        return self._vec_flat

    def _view(self, flat, name):
        i = self.names.index(name)
        return flat[self.offsets[i]: self.offsets[i] + self.numels[i]].view(self.shapes[name])

    def grad(self, name):
        return self._view(self.grad_flat, name)

    def momentum_of(self, name):
        return self._view(self.mmt_flat, name)

    def velocity_of(self, name):
        return self._view(self.vec_flat, name)

    def out(self, name):
        return self._view(self.out_flat, name)

    # ---------------------------------------------------------------- phases
    def draw_starts(self):
        """random.randint(0, stride - 1) per sampled tensor, in the tensors' order (dgc/compression.py:118)."""
        starts = []
        for n, (k, S, ks, stride) in zip(self.numels, self.attrs):
            starts.append(self.rng.randint(0, stride - 1) if n != S else 0)
        return starts

    def _arrays16(self):
        if not hasattr(self, "_g16"):
            T = len(self.names)
            self._g16 = ((ctypes.c_int64 * T)(*self.numels), (ctypes.c_int64 * T)(*self.offsets))
        return self._g16

    def compensate(self, starts=None, grad_ptrs=None):
        """K1 over every tensor: compensate + strided samples + candidate lists (and any
        masking the previous select left pending). The gradients come from ``grad_flat``,
        or — ``grad_ptrs``, a ctypes array of T device pointers, each to the tensor's
        numel contiguous fp32 elements, 16-B aligned — from wherever they are (the
        batched optimizer's p.grad tensors, read in place). Raises first if a previous
        step's resample replay reported DGC_K5_BROKEN, or its decompress met an index
        or a gathered count out of range (``status``)."""
        self.status.check()
        starts = self.draw_starts() if starts is None else starts
        self.starts = starts
        self.rx.begin()
        arr = (ctypes.c_int64 * len(starts))(*starts)
        self._starts_arr = arr
        L, st = self._L, _lib.stream_of(self.device)
        T = len(self.names)
        flat = (self.grad_flat.data_ptr(), self._mmt_flat.data_ptr(), self._vec_flat.data_ptr())
        if self.half:
            if grad_ptrs is not None:   # the 16-bit gradients into the flat buffer (2-B gather)
                _lib.check(L.dgc_gather16(grad_ptrs, *self._arrays16(), T, flat[0], st), "dgc_gather16")
            # two kernels, so two calls: the whole-buffer K1-16 (padding included) without a
            # clip, the multi-tensor K1-16 (one coefficient per tensor) with one
            if self.clip is None:
                _lib.check(L.dgc_compensate16_clip(*flat, None, self._vec32.data_ptr(), self.flat_numel,
                                                   self.momentum, int(self.nesterov), 1, _lib.VD[self.dtype],
                                                   *_lib.NO_CLIP, st), "dgc_compensate16_clip")
                return
            numels, offs = self._arrays16()
            flat_ptrs = (ctypes.c_void_p * T)(*[flat[0] + 2 * o for o in self.offsets])
            self.clip_coefs = self.clip.table_coefs(flat_ptrs, numels, T, self.device, dtype=self.dtype)
            _lib.check(L.dgc_compensate16_multi_clip(*flat, self._vec32.data_ptr(), numels, offs, T, self.flat_numel,
                                                     self.momentum, int(self.nesterov), _lib.VD[self.dtype],
                                                     self.clip.kind, _lib.ptr(self.clip_coefs), self.clip.param, st),
                       "dgc_compensate16_multi_clip")
            return
        clip = None
        if self.clip is not None:
            if grad_ptrs is None:   # the statistics read a pointer table: grad_flat's tensors
                grad_ptrs = (ctypes.c_void_p * T)(*[flat[0] + 4 * o for o in self.offsets])
            self.clip_coefs = self.clip.table_coefs(grad_ptrs, self._arrays[0], T, self.device)
            clip = (self.clip.kind, self.clip_coefs, self.clip.param)
        # an unclipped step from grad_flat keeps the flat form (no pointer table to read)
        if grad_ptrs is None:
            begin, src, what = L.dgc_batch_compress_begin_clip, flat[0], "dgc_batch_compress_begin_clip"
        else:
            begin, src, what = L.dgc_batch_compress_begin_ptrs_clip, grad_ptrs, "dgc_batch_compress_begin_ptrs_clip"
        _lib.check(begin(ctypes.byref(self.desc), src, flat[1], flat[2], arr, *_lib.clip_args(clip),
                         self.ws.data_ptr(), self.ws.numel(), st), what)
        self._pending = False

    def select(self):
        """K3 thresholds + selection / adaptation / resample / pack / masking of every tensor."""
        if self.half:
            L, st = self._L, _lib.stream_of(self.device)
            _lib.check(L.dgc_batch_select(ctypes.byref(self.desc), self._vec32.data_ptr(), None, self._starts_arr,
                                          self.payload.data_ptr(), self.info.data_ptr(), self.ws.data_ptr(),
                                          self.ws.numel(), _lib.SYNC_DEVICE, st), "dgc_batch_select")
            _lib.mask_packed16(self.payload, self.capacity, self.vdtype, self.idtype,
                               self._mmt_flat if self.momentum_masking else None, self._vec_flat, self.flat_numel,
                               self.device)
            return
        _lib.check(self._L.dgc_batch_compress_finish(ctypes.byref(self.desc), self._mmt_flat.data_ptr(),
                                                     self._vec_flat.data_ptr(), self.payload.data_ptr(),
                                                     self.info.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                     _lib.SYNC_DEVICE, _lib.stream_of(self.device)),
                   "dgc_batch_compress_finish")
        self._pending = self.deferred_masking

    def compress(self, starts=None):
        """Every tensor: compensate -> sample -> threshold -> select -> pack -> masking."""
        self.compensate(starts)
        self.select()

    def send(self):
        """Issues the exchange of this step's payload (W > 1): one allgather, or one per
        part (split); ``decompress`` waits for it. Nothing is issued in between, so a
        single allgather goes out on the current stream (``comm.COLLECTIVE_ISSUE``)."""
        self.rx.send()

    def decompress(self, out_flat=None):
        """out = the rank-order sum of the gathered entries / W, +0.0 elsewhere (every tensor).

        fill="sparse": when ``out`` still holds exactly the previous decompress's result
        and is not the gradient buffer (the batched optimizer decompresses into p.grad,
        rewritten by every backward), only the previous step's gathered indices are
        re-zeroed instead of the whole buffer (``Receiver``, dgc/exchange.py)."""
        out = self.out_flat if out_flat is None else out_flat
        _lib.require_out(out, self.dtype, self.flat_numel, self.device, "DGCBatch.decompress", "out_flat")
        # (16-bit: zero_(), the runs in rank order, each add rounded, the 1/W scale: HalfExchange)
        self.rx.decompress(out, out.untyped_storage().data_ptr() == self.grad_flat.untyped_storage().data_ptr())
        return out

    def apply(self, table, hypers):
        """In place of ``decompress()`` after ``send()``: DGCSGD's step (dgc/optim/sgd.py:42-68)
        on every tensor of the batch from the gathered entries, bit for bit ``decompress()``
        then ``DGCSGD.step()`` on the output's views, with no dense gradient written or read.
        ``table``: an ``_lib.ApplyTable`` whose rows are the batch's tensors in order (row t:
        parameter and momentum buffer of ``names[t]``, ``offsets[t]``, ``numels[t]``);
        ``hypers``: per parameter group of the table ``(lr, momentum, dampening, weight_decay,
        nesterov)``. The entries are scattered (K6, unchanged: rank-order sums, 1/W, status)
        into the batch's own accumulator, +0.0 between steps; ``dgc_apply_packed_multi`` then
        walks them. ``fill="sparse"``'s memory of the last output is left alone."""
        if self.half:
            raise NotImplementedError(f"DGCBatch.apply: fp32 parameters only (a {self.dtype} batch takes decompress "
                                      "and DGCSGD.step)")
        rx = self.rx
        if rx.parts > 1:
            raise ValueError(f"DGCBatch.apply: the exchange is split in {rx.parts} parts, whose part-major gather "
                             "layout apply does not walk; construct the batch with exchange_parts=1")
        if table.count != len(self.names) or not 1 <= len(hypers) <= _lib.APPLY_MAX_GROUPS:
            raise ValueError(f"DGCBatch.apply: a table of the batch's {len(self.names)} tensors and 1.."
                             f"{_lib.APPLY_MAX_GROUPS} parameter groups (got {table.count} rows, {len(hypers)} groups)")
        L = self._L
        if self._acc is None:
            self._acc = torch.zeros(self.flat_numel, dtype=torch.float32, device=self.device)
        if self._apply_ws is None:
            self._apply_ws = torch.empty(L.dgc_apply_packed_multi_workspace(self.world, self.capacity),
                                         dtype=torch.uint8, device=self.device)
        hs = (_lib.ApplyHyper * len(hypers))(*[_lib.ApplyHyper(float(lr), float(mom), float(damp), float(wd),
                                                               int(bool(nesterov)))
                                               for lr, mom, damp, wd, nesterov in hypers])
        cur = rx.gathered
        # the exchange's scatter, not Receiver.scatter: acc is not a decompress output to remember
        rx.xchg.scatter(cur, rx._take(), self._acc, rx.scale, False)
        _lib.check(L.dgc_apply_packed_multi(cur.data_ptr(), self.world, rx.rank_stride, self.capacity,
                                            _lib.VD[self.vdtype], _lib.ID[self.idtype], self._acc.data_ptr(),
                                            self.flat_numel, table.dev.data_ptr(), table.count, table.dense_blocks,
                                            hs, len(hypers), self._apply_ws.data_ptr(), self._apply_ws.numel(),
                                            _lib.stream_of(self.device)), "dgc_apply_packed_multi")

    def step(self, starts=None):
        self.compress(starts)
        self.exchange()
        return self.decompress()

    # ---------------------------------------------------------------- results
    def infos(self):
        self.status.check(sync=True)
        return _lib.read_infos(self.info, [f"DGCBatch tensor {n}" for n in self.names])

    def transmitted(self, rank_payload=None):
        """{name: (values, indices)} of one rank's payload (this rank's by default), with
        indices relative to the tensor — what the reference's compress returns."""
        p = self.payload if rank_payload is None else rank_payload
        total = int(p[:8].view(torch.int64).item())
        vals, idxs = _lib.payload_views(p, self.voff, self.ioff, self.vdtype, self.idtype, total)
        counts = [i["count"] for i in self.infos()]
        res, pos = {}, 0
        for name, off, c in zip(self.names, self.offsets, counts):
            res[name] = (vals[pos: pos + c], idxs[pos: pos + c].to(torch.int64) - off)
            pos += c
        return res
