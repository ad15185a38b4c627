"""Momentum-correction memory for DGC — drop-in for the reference ``dgc/memory.py``.

Same classes, constructor arguments, methods and state layout as the reference
(``Memory`` static API, dgc/memory.py:9-28; ``DGCSGDMemory``, dgc/memory.py:31-88).
The arithmetic runs in ``libdgc_hip.so`` on the MI355X:

* ``compensate``  -> ``dgc_compensate_clip`` (K1: one fused streaming pass, fp32 with the
  reference's two separate roundings, no FMA contraction; the clip is an argument,
  ``_lib.NO_CLIP`` without one);
* ``update``      -> ``dgc_mask_indices`` (the same masking that ``dgc_compress``
  fuses into its emit kernel when the compressor drives this memory);
* ``gradient_clipping`` -> when it is one of ``dgc.clip_grad``'s functions (or a
  ``functools.partial`` of one) and the gradient is fp32: ``dgc_grad_stats`` ->
  ``dgc_clip_coefs`` -> ``dgc_compensate_clip``, the clip applied in registers as K1
  loads the gradient (the input gradient stays as it was). A local clip (norm-2,
  norm-inf, value) of a bf16 / fp16 gradient is fused the same way, in the dtype's
  arithmetic: ``dgc_grad_stats16`` -> ``dgc_clip_coefs16`` -> ``dgc_compensate16_clip``.
  Any other callable is called as the reference calls it, before K1.

``momentums`` / ``velocities`` stay plain param-shaped tensors of the parameter's dtype
keyed by name, so ``state_dict`` / ``load_state_dict`` and checkpoints are unchanged.
bf16 / fp16 parameters run ``dgc_compensate16_clip`` / ``dgc_mask_indices16``: every op of
the reference rounds to the dtype, as ATen does on a 16-bit tensor.
"""
import ctypes

import torch

from . import _lib
from . import clip_grad
from . import comm

__all__ = ["Memory", "DGCSGDMemory"]


class Memory:
    """No-op memory (dgc/memory.py:9-28)."""

    @staticmethod
    def initialize(*args, **kwargs):
        pass

    @staticmethod
    def compensate(tensor, *args, **kwargs):
        return tensor

    @staticmethod
    def update(*args, **kwargs):
        pass

    @staticmethod
    def state_dict():
        return None

    @staticmethod
    def load_state_dict(state_dict):
        pass


class DGCSGDMemory(Memory):
    """Memory for momentum correction in DGC for momentum SGD (dgc/memory.py:31-88)."""

    def __init__(self, momentum=0.9, nesterov=False, gradient_clipping=None, momentum_masking=True):
        self.gradient_clipping = gradient_clipping
        self.momentum_masking = momentum_masking
        self.momentum = momentum
        self.nesterov = nesterov
        self.momentums = {}
        self.velocities = {}
        self._status = {}   # device -> StatusSink: update() with an index outside the state
        # callables run before the state is read or replaced: a batched step
        # (dgc/horovod/batched.py) applies a deferred momentum masking there
        self._before_read = []
        self._clip_spec = (None, None)   # (callable, its dgc.clip_grad.ClipSpec or None)
        self.last_clip_coef = None       # device float[1] of the last fused clip (None: a fixed clamp)

    def _sync(self):
        for fn in self._before_read:
            fn()
        self.check()

    def check(self, sync=False):
        """Raises if an ``update`` issued earlier got an index outside [-n, n) (the
        reference's index_fill_ raises there, dgc/memory.py:76-77): the kernel stores a
        flag in pinned host memory, read here for free at every call (``sync=True``
        waits for the stream first)."""
        for sink in self._status.values():
            sink.check(sync)

    def initialize(self, named_parameters):
        """zeros_like per parameter (dgc/memory.py:43-48)."""
        if comm.rank() == 0:
            print("=> initializing dgc sgd memory")
        self._sync()
        for name, param in named_parameters:
            self.momentums[name] = torch.zeros_like(param.data)
            self.velocities[name] = torch.zeros_like(param.data)

    # ------------------------------------------------------------------ K1
    def _clip(self, grad):
        return self.gradient_clipping(grad) if self.gradient_clipping is not None else grad

    def clip_spec(self):
        """The ``ClipSpec`` of ``gradient_clipping`` when it is a ``dgc.clip_grad`` function
        (None: no clipping, or an opaque callable)."""
        fn = self.gradient_clipping
        if fn is None:
            return None
        if self._clip_spec[0] is not fn:
            self._clip_spec = (fn, clip_grad.spec_of(fn))
        return self._clip_spec[1]

    def fused_clip(self, grad):
        """(clip kind, device coefficient or None, clamp value) for K1 (``_lib.clip_args``) when
        the clip of ``grad`` (contiguous) can be fused: a recognised spec on an fp32 device
        tensor, or a local one on a bf16 / fp16 device tensor (``ClipSpec.fusable``). The
        statistic and the coefficient are issued here, stream-ordered; None otherwise."""
        return self._issue_clip(grad) if self._fusable(grad) else None

    def _fusable(self, grad):
        spec = self.clip_spec()
        return spec is not None and torch.is_tensor(grad) and grad.is_cuda and spec.fusable(grad.dtype)

    def _issue_clip(self, grad):
        spec = self.clip_spec()
        _lib.require_cuda_float(grad, "DGCSGDMemory.gradient_clipping")
        coef = self.last_clip_coef = spec.coef(grad)
        return spec.kind, coef, spec.param

    def state_of(self, name, like, accumulate=True, what="DGCSGDMemory.compensate"):
        """(momentum, velocity or None) of ``name``, checked before their pointers reach a
        kernel: contiguous tensors of ``like``'s dtype, device and size. ``load_state_dict``
        rebinds them to whatever the checkpoint holds (a CPU map_location, fp32 state for a
        16-bit parameter); the reference's ATen ops would raise on the device mismatch and
        promote the dtype, the kernels would fault or misread — so this raises instead."""
        out = []
        for kind, store in (("momentum", self.momentums), ("velocity", self.velocities if accumulate else None)):
            if store is None:
                out.append(None)
                continue
            t = store[name]
            _lib.require_cuda_float(t, f"{what} ({kind} of {name})")
            if t.dtype != like.dtype or t.device != like.device or t.numel() != like.numel():
                raise TypeError(f"{what}: {kind} of {name} is {t.dtype} [{t.numel()}] on {t.device}, the gradient "
                                f"{like.dtype} [{like.numel()}] on {like.device}; load the state with the "
                                "parameter's dtype and device")
            out.append(t)
        return out[0], out[1]

    def compensate(self, grad, name, accumulate=True):
        """Momentum correction + local accumulation (dgc/memory.py:50-70).

        accumulate=True returns ``velocities[name]`` itself (updated in place);
        accumulate=False (dense tensors) returns a new tensor."""
        self._sync()
        fusable = self._fusable(grad)
        g = (grad if fusable else self._clip(grad)).contiguous()
        _lib.require_cuda_float(g, "DGCSGDMemory.compensate")
        return self._k1(g, name, accumulate, clip=self._issue_clip(g) if fusable else None)

    def _k1(self, g, name, accumulate, vec32=None, clip=None):
        """K1 / K1-16 on the contiguous device gradient ``g``, by its dtype; clip:
        ``fused_clip``'s result, applied as the gradient is loaded (None: unclipped); vec32
        (16-bit state only): optional fp32 image of the new velocity for the selection
        (the compressor's 16-bit branch)."""
        mmt, vec = self.state_of(name, g, accumulate)
        out = None if accumulate else torch.empty_like(mmt)
        L = _lib.lib()
        head = (_lib.ptr(g), _lib.ptr(mmt), _lib.ptr(vec), _lib.ptr(out))
        tail = (float(self.momentum), int(bool(self.nesterov)), int(accumulate))
        if g.dtype in _lib.HALF:
            _lib.check(L.dgc_compensate16_clip(*head, _lib.ptr(vec32) if accumulate else None, mmt.numel(), *tail,
                                               _lib.VD[g.dtype], *_lib.clip_args(clip), _lib.stream_of(g.device)),
                       "dgc_compensate16_clip")
        else:   # no samples: (samples, start, stride, count) = (NULL, 0, 1, 0)
            _lib.check(L.dgc_compensate_clip(*head, mmt.numel(), *tail, None, 0, 1, 0, *_lib.clip_args(clip),
                                             _lib.stream_of(g.device)), "dgc_compensate_clip")
        return vec if accumulate else out

    def update(self, name, ctx):
        """Zero the transmitted slots (dgc/memory.py:72-77)."""
        self._sync()
        indices = ctx[0]
        vec = self.velocities[name]
        dt = _lib.require_cuda_float(vec, "DGCSGDMemory.update")
        mmt, _ = self.state_of(name, vec, False, "DGCSGDMemory.update")
        idx = indices.reshape(-1)
        if idx.dtype not in _lib.ID:
            idx = idx.to(torch.int64)
        idx = idx.contiguous()
        sink = self._status.get(vec.device)
        if sink is None:
            sink = self._status[vec.device] = _lib.StatusSink("DGCSGDMemory.update", vec.device)
        L = _lib.lib()
        fn = L.dgc_mask_indices16 if dt in _lib.HALF else L.dgc_mask_indices
        _lib.check(fn(_lib.ptr(mmt) if self.momentum_masking else None, _lib.ptr(vec),
                      vec.numel(), _lib.ptr(idx), _lib.ID[idx.dtype], idx.numel(),
                      ctypes.c_void_p(sink.index_flag), _lib.stream_of(vec.device)), "dgc_mask_indices")

    def state_dict(self):
        self._sync()
        return dict(momentums=self.momentums, velocities=self.velocities)

    def load_state_dict(self, state_dict):
        self._sync()
        momentums = state_dict["momentums"]
        velocities = state_dict["velocities"]
        for name in self.momentums.keys():
            if name in momentums:
                self.momentums[name] = momentums[name]
                self.velocities[name] = velocities[name]
