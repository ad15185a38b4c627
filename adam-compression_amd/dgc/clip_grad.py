"""Local gradient clipping for DGC — drop-in for the reference ``dgc/clip_grad.py``.

The four functions of the reference (dgc/clip_grad.py:10-42), same names, argument names
and defaults, meant to be passed to ``DGCSGDMemory(gradient_clipping=...)`` (usually as a
``functools.partial``). On an fp32 tensor on the MI355X each is three stream-ordered
library calls, none of which reads anything back to the host:

    dgc_grad_stats   the tensor's statistic: fl32(sqrt(sum g^2)) (fp64 squares and sum in
                     a fixed order), max |g|, or fl32(sum g^2) for the global variants
    dgc_clip_coefs   the coefficient, in the reference's 0-dim fp32 tensor arithmetic
                     (``max_norm / (total_norm + 1e-6)`` is reciprocal().mul(max_norm))
    dgc_clip_apply   ``if clip_coef < 1: grad.mul_(clip_coef)`` / ``clamp_`` in place

The global variants put one ``comm.allreduce_async_(stat, Average)`` (the project's
rank-order Average, dgc/comm.py) between the first two, where the reference calls
``horovod.torch.allreduce_(average=True)``. ``clip_grad_norm_`` with a ``norm_type`` other
than 2 or inf takes the norm from torch on the device and the rest from the library.

One deviation: every function returns the tensor. The reference's ``clip_grad_value_`` and
``clip_grad_value_by_global_norm_`` return None, which makes ``DGCSGDMemory.compensate``
(dgc/memory.py:52-53) fail on them.

``spec_of`` recognises these functions (bare or as a ``functools.partial``) so that
``DGCSGDMemory``, ``DGCCompressor``, ``DGCBatch`` and the batched optimizer can fuse the
clip into K1's load of the gradient instead of calling them: the clipped value is then
formed in registers and the input gradient stays as it was.

Called directly on a bf16 / fp16 tensor, the module functions take the reference's formula
in ATen ops on the device (each op rounds to the dtype, as the reference's do), without a
host synchronisation. Fused (``ClipSpec.fusable``), a local clip of a 16-bit gradient is the
same three steps in the dtype's arithmetic: ``dgc_grad_stats16`` -> ``dgc_clip_coefs16`` ->
the clip in K1-16's load (``dgc_compensate16_clip``, ``dgc_compensate16_multi_clip``,
``dgc_compress_begin16_clip``).
"""
import ctypes
import functools
import inspect
from math import inf

import torch

from . import _lib
from . import comm

__all__ = ["clip_grad_norm_", "clip_grad_value_", "clip_grad_value_by_global_norm_", "clip_grad_norm_2_by_global_",
           "ClipSpec", "spec_of"]

STAT_SUMSQ, STAT_NORM2, STAT_ABSMAX = 0, 1, 2
COEF_NORM, COEF_GLOBAL_VALUE, COEF_GLOBAL_NORM2 = 0, 1, 2
CLIP_NONE, CLIP_SCALE, CLIP_CLAMP = 0, 1, 2


def _table1(g):
    """The one-entry (pointers, numels) table of the tensor ``g``."""
    return (ctypes.c_void_p * 1)(g.data_ptr()), (ctypes.c_int64 * 1)(g.numel())


class ClipSpec:
    """What a clipping callable does: ``mode`` ("norm2", "norminf", "normp", "value",
    "global_value", "global_norm2"), its parameter (``max_norm`` or ``clip_value``;
    ``norm_type`` for "normp") and the allreduce ``name`` of a global variant."""

    __slots__ = ("mode", "param", "norm_type", "name")
    _STAT = {"norm2": STAT_NORM2, "norminf": STAT_ABSMAX, "global_value": STAT_SUMSQ, "global_norm2": STAT_SUMSQ}
    _COEF = {"norm2": COEF_NORM, "norminf": COEF_NORM, "normp": COEF_NORM, "global_value": COEF_GLOBAL_VALUE,
             "global_norm2": COEF_GLOBAL_NORM2}

    def __init__(self, mode, param=0.0, norm_type=None, name=None):
        self.mode, self.param, self.norm_type, self.name = mode, float(param), norm_type, name

    def __repr__(self):
        return f"ClipSpec({self.mode!r}, {self.param!r}, norm_type={self.norm_type!r}, name={self.name!r})"

    def __eq__(self, other):
        return isinstance(other, ClipSpec) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __hash__(self):
        return hash((self.mode, self.param, self.norm_type, self.name))

    @property
    def kind(self):
        """The dgc_clip_kind K1 applies."""
        return CLIP_CLAMP if self.mode in ("value", "global_value") else CLIP_SCALE

    @property
    def is_global(self):
        return self.mode.startswith("global")

    @property
    def stat(self):
        """The dgc_stat_kind, or None when no library statistic is needed."""
        return self._STAT.get(self.mode)

    @property
    def batchable(self):
        """A local clip whose statistic the library computes for a whole pointer table:
        what ``DGCBatch`` and the batched optimizer take."""
        return self.mode in ("norm2", "norminf", "value")

    def fusable(self, dtype):
        """Whether the engines fuse this clip into K1's load of a gradient of ``dtype``: the
        local clips on fp32 / bf16 / fp16, the global variants (and a p-norm, whose norm
        torch takes) on fp32 only."""
        return dtype == torch.float32 or (self.batchable and dtype in _lib.HALF)

    # ------------------------------------------------------------------ device steps
    def table_coefs(self, ptrs, numels, count, device, round_to=torch.float32, dtype=torch.float32):
        """stats -> coefs over a ctypes table of ``count`` device pointers / numels:
        the device float[count] coefficient table (None for the fixed clamp). ``dtype``:
        the tensors' (bf16 / fp16: the statistic and the coefficient in that dtype's
        arithmetic, stored as fp32 images; a local clip only)."""
        if self.mode == "value":
            return None
        L, st = _lib.lib(), _lib.stream_of(device)
        stats = torch.empty(max(count, 1), dtype=torch.float32, device=device)
        wsz = L.dgc_grad_stats_workspace(numels, count)
        ws = torch.empty(wsz, dtype=torch.uint8, device=device)
        if dtype in _lib.HALF:
            if not self.batchable:
                raise NotImplementedError(f"dgc.clip_grad: {self!r} is not fused on {dtype} tensors")
            _lib.check(L.dgc_grad_stats16(ptrs, numels, count, self.stat, _lib.VD[dtype], _lib.ptr(stats),
                                          _lib.ptr(ws), wsz, st), "dgc_grad_stats16")
            _lib.check(L.dgc_clip_coefs16(_lib.ptr(stats), count, self.param, _lib.VD[dtype], _lib.ptr(stats), st),
                       "dgc_clip_coefs16")
            return stats
        _lib.check(L.dgc_grad_stats(ptrs, numels, count, self.stat, _lib.VD[round_to], _lib.ptr(stats), _lib.ptr(ws),
                                    wsz, st), "dgc_grad_stats")
        return self.coefs_of(stats, count)

    def coefs_of(self, stats, count):
        """stats (device float[count]) -> the coefficient table, in place; a global
        variant averages the statistics over the ranks first."""
        if self.is_global:
            comm.synchronize(comm.allreduce_async_(stats, name=self.name, op=comm.Average))
        _lib.check(_lib.lib().dgc_clip_coefs(_lib.ptr(stats), count, self._COEF[self.mode], self.param,
                                             _lib.ptr(stats), _lib.stream_of(stats.device)), "dgc_clip_coefs")
        return stats

    def coef(self, g):
        """The device float[1] coefficient of the contiguous fp32 tensor ``g`` (None for
        the fixed clamp); of a bf16 / fp16 tensor for a local clip."""
        if self.mode == "value":
            return None
        if self.mode == "normp" and g.dtype == torch.float32:
            stats = g.norm(self.norm_type).reshape(1)
            return self.coefs_of(stats, 1)
        return self.table_coefs(*_table1(g), 1, g.device, dtype=g.dtype)

    def apply_(self, grad):
        """The clip in place on ``grad.data``; returns ``grad``."""
        data = grad.data
        if not (torch.is_tensor(data) and data.is_cuda):
            raise RuntimeError(f"dgc.clip_grad: the DGC hot path runs on the MI355X only (got a "
                               f"{'CPU' if torch.is_tensor(data) else type(data).__name__} tensor)")
        if data.dtype in _lib.HALF:
            return self._apply16_(grad)
        g = data if data.is_contiguous() else data.contiguous()
        _lib.require_cuda_float(g, "dgc.clip_grad", dtypes=(torch.float32,))
        _lib.check(_lib.lib().dgc_clip_apply(*_table1(g), 1, self.kind, _lib.ptr(self.coef(g)), self.param,
                                             _lib.stream_of(g.device)), "dgc_clip_apply")
        if g is not data:
            data.copy_(g)
        return grad

    def _apply16_(self, grad):
        """The reference's formula in ATen ops on a bf16 / fp16 tensor (the multiply by a
        coefficient >= 1 replaced by a multiply by 1, so no host synchronisation)."""
        data = grad.data
        if self.mode == "value":
            data.clamp_(min=-self.param, max=self.param)
            return grad
        if self.is_global:
            s = torch.sum(data.square())
            s = comm.synchronize(comm.allreduce_async_(s, name=self.name, op=comm.Average))
            total = torch.sqrt(s)
            if self.mode == "global_value":
                data.clamp_(min=-total, max=total)
                return grad
        elif self.mode == "norminf":
            total = data.abs().max()
        else:
            total = data.norm(2.0 if self.mode == "norm2" else self.norm_type)
        coef = self.param / (total + 1e-6)
        data.mul_(torch.where(coef < 1, coef, torch.ones_like(coef)))
        return grad


def clip_grad_norm_(grad, max_norm, norm_type=2):
    """dgc/clip_grad.py:10-20."""
    return _norm_spec(max_norm, norm_type).apply_(grad)


def clip_grad_value_(grad, clip_value):
    """dgc/clip_grad.py:23-25 (returns the tensor; the reference returns None)."""
    return ClipSpec("value", float(clip_value)).apply_(grad)


def clip_grad_value_by_global_norm_(grad, name=None):
    """dgc/clip_grad.py:29-32 (returns the tensor; the reference returns None)."""
    return ClipSpec("global_value", 0.0, name=name).apply_(grad)


def clip_grad_norm_2_by_global_(grad, max_norm, name=None):
    """dgc/clip_grad.py:35-42."""
    return ClipSpec("global_norm2", float(max_norm), name=name).apply_(grad)


def _norm_spec(max_norm, norm_type=2):
    max_norm, norm_type = float(max_norm), float(norm_type)
    if norm_type == inf:
        return ClipSpec("norminf", max_norm)
    if norm_type == 2.0:
        return ClipSpec("norm2", max_norm)
    return ClipSpec("normp", max_norm, norm_type=norm_type)


_SPECS = {
    clip_grad_norm_: lambda grad, max_norm, norm_type=2: _norm_spec(max_norm, norm_type),
    clip_grad_value_: lambda grad, clip_value: ClipSpec("value", float(clip_value)),
    clip_grad_value_by_global_norm_: lambda grad, name=None: ClipSpec("global_value", 0.0, name=name),
    clip_grad_norm_2_by_global_: lambda grad, max_norm, name=None: ClipSpec("global_norm2", float(max_norm), name=name),
}


def spec_of(fn):
    """The ``ClipSpec`` of one of this module's functions, bare or wrapped in a
    ``functools.partial`` (positional or keyword arguments), when calling it with the
    gradient alone is a complete call; None for anything else (a lambda, another
    callable, a partial that binds the gradient or misses a required argument)."""
    args, kwargs = (), {}
    if isinstance(fn, functools.partial):
        fn, args, kwargs = fn.func, fn.args, fn.keywords
    try:
        make = _SPECS.get(fn)
    except TypeError:   # unhashable callable
        return None
    if make is None or args:
        # a positional argument of a partial would bind `grad`, the first parameter
        return None
    try:
        inspect.signature(make).bind(None, **kwargs)
        return make(None, **kwargs)
    except (TypeError, ValueError):
        return None
