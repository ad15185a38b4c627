"""Data-parallel optimizer wrapper — drop-in for the reference's patched Horovod
``DistributedOptimizer`` (dgc/horovod/optimizer.py:34-194, 370-417).

Per parameter, an autograd grad-accumulator hook calls
``compression.compress(p.grad, name)`` and then ``compression.communicate`` (found
by ``getattr``, falling back to a plain allreduce); ``step()`` / ``synchronize()``
wait on every handle, ``decompress`` the result and ``p.grad.set_`` it before the
wrapped optimizer steps (dgc/horovod/optimizer.py:105-187). Hooks are registered
only when the world has more than one rank (or ``HOROVOD_ELASTIC=1``), exactly as
the reference does (dgc/horovod/optimizer.py:79-80).

The transport is ``dgc.comm`` (torch.distributed; RCCL over xGMI on MI355X)
instead of Horovod/MPI. The Adasum delta-model variant
(dgc/horovod/optimizer.py:197-367) is not part of the DGC path and is refused.
"""
import os
import warnings
from contextlib import contextmanager

import torch

from dgc import comm
from dgc.comm import Adasum, Average
from dgc.horovod.compression import Compression

__all__ = ["DistributedOptimizer"]

_BATCHED = "batched"   # hook handle of a gradient left to the grouped exchange


class _DistributedOptimizer(torch.optim.Optimizer):
    def __init__(self, params, named_parameters, compression, backward_passes_per_step=1, op=Average,
                 batch="auto"):
        super(self.__class__, self).__init__(params)
        self._compression = compression
        self._communicate_ = getattr(compression, "communicate", None) or \
            (lambda t, name, op: comm.allreduce_async_(t, name=name, op=op))
        self._synchronize_ = getattr(compression, "synchronize", comm.synchronize)

        if named_parameters is not None:
            named_parameters = list(named_parameters)
        else:
            named_parameters = [(f"allreduce.noname.{i}", v)
                                for group in self.param_groups for i, v in enumerate(group["params"])]
        if any(not isinstance(p, tuple) for p in named_parameters):
            raise ValueError("named_parameters should be a sequence of tuples (name, parameter), "
                             "usually produced by model.named_parameters().")
        names = [k for k, _ in named_parameters]
        dups = {n for n in names if names.count(n) > 1}
        if dups:
            raise ValueError("Parameter names in named_parameters must be unique. Found duplicates: "
                             + ", ".join(sorted(dups)))
        all_ids = {id(v) for group in self.param_groups for v in group["params"]}
        unnamed = all_ids - {id(v) for _, v in named_parameters}
        if unnamed:
            raise ValueError("named_parameters was specified, but one or more model parameters were "
                             "not named. Python object ids: " + ", ".join(str(i) for i in unnamed))

        self._parameter_names = {v: k for k, v in sorted(named_parameters, key=lambda kv: kv[0])}
        self.backward_passes_per_step = backward_passes_per_step
        self._allreduce_delay = {v: backward_passes_per_step for _, v in named_parameters}
        self.op = op
        self._handles = {}
        self._grad_accs = []
        self._hook_fns = []   # (parameter, hook) in registration order (bench.py fires them directly)
        self._requires_update = set()
        self._synchronized = False
        self._should_synchronize = True
        self._batched = None
        self._order = []
        self._cells = {}        # batch mode: name -> [backward passes left]
        self._fired = [False]   # batch mode: a hook fired since the last synchronize()
        if batch == "auto":
            from dgc.horovod import batched
            batch = batched.auto(compression, named_parameters, op)
        self._apply_mode = batch == "apply"   # the compressed tensors stepped from the gathered entries
        if batch:
            from dgc.horovod import batched
            if not batched.supported(compression):
                raise ValueError("batch=True needs a DGCCompressor driving a DGCSGDMemory with strided sampling "
                                 "and no gradient clipping other than a local dgc.clip_grad function")
            if self._apply_mode:
                from dgc.optim import DGCSGD
                if not isinstance(self, DGCSGD):
                    raise ValueError(f"batch='apply' applies dgc.optim.DGCSGD's step from the gathered entries; "
                                     f"a {type(self).__name__} runs with batch=True")
            self._batched = batched.BatchedStep(compression, named_parameters,
                                                fill="sparse" if batch == "sparse" else "inline",
                                                apply=self if self._apply_mode else None)
        if comm.size() > 1 or os.environ.get("HOROVOD_ELASTIC") == "1":
            self._register_hooks()

    def load_state_dict(self, *args, **kwargs):
        self._handles = {}
        self._synchronized = False
        self._should_synchronize = True
        for p in self._allreduce_delay:
            self._allreduce_delay[p] = self.backward_passes_per_step
        self._reset_cells()
        super(self.__class__, self).load_state_dict(*args, **kwargs)

    def set_backward_passes_per_step(self, passes):
        self.backward_passes_per_step = passes
        for p in self._allreduce_delay:
            self._allreduce_delay[p] = passes
        self._reset_cells()

    def _reset_cells(self):
        bpps = self.backward_passes_per_step
        for c in self._cells.values():
            c[0] = bpps
        self._fired[0] = False

    def _register_hooks(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.requires_grad:
                    p.grad = p.data.new(p.size()).zero_()
                    self._requires_update.add(p)
                    grad_acc = p.expand_as(p).grad_fn.next_functions[0][0]
                    hook = self._make_hook(p) if self._batched is None else self._make_batched_hook(p)
                    grad_acc.register_hook(hook)
                    self._grad_accs.append(grad_acc)
                    self._hook_fns.append((p, hook))

    def _allreduce_grad_async(self, p):
        name = self._parameter_names.get(p)
        tensor_compressed, ctx = self._compression.compress(p.grad, name)
        handle = self._communicate_(tensor_compressed, name=name, op=self.op)
        return handle, ctx

    def _make_hook(self, p):
        def hook(*ignore):
            if p in self._handles and self._handles[p][0] is not None:
                if self._allreduce_delay[p] <= 0:
                    raise AssertionError("Gradients were computed more than backward_passes_per_step times "
                                         "before call to step(). Increase backward_passes_per_step to "
                                         "accumulate gradients locally.")
            assert not p.grad.requires_grad
            assert self._allreduce_delay[p] > 0
            handle, ctx = None, None
            self._allreduce_delay[p] -= 1
            if self._allreduce_delay[p] == 0:
                if self._batched is not None:   # exchanged with all the others in synchronize()
                    self._order.append(self._parameter_names.get(p))
                    handle = _BATCHED
                else:
                    handle, ctx = self._allreduce_grad_async(p)
            self._handles[p] = (handle, ctx)
        return hook

    def _make_batched_hook(self, p):
        """The hook of batch mode: the reference's bookkeeping (the backward_passes_per_step
        countdown and its errors, dgc/horovod/optimizer.py:105-129) on a per-parameter cell
        instead of tensor-keyed dicts, and the parameter's name appended to the hook order
        when its countdown ends — the exchange itself is synchronize()'s."""
        name = self._parameter_names.get(p)
        cell = self._cells[name] = [self.backward_passes_per_step]
        order, fired = self._order, self._fired

        def hook(*ignore):
            if cell[0] <= 0:
                raise AssertionError("Gradients were computed more than backward_passes_per_step times "
                                     "before call to step(). Increase backward_passes_per_step to "
                                     "accumulate gradients locally.")
            assert not p.grad.requires_grad
            cell[0] -= 1
            fired[0] = True
            if cell[0] == 0:   # exchanged with all the others in synchronize()
                order.append(name)
        return hook

    def synchronize(self):
        """Exchanges every gradient and leaves the result in ``p.grad`` (batch="apply" too:
        whoever calls this wants the gradients; only ``step()``'s own call applies)."""
        self._synchronize()

    def _synchronize(self, apply=False):
        if self._batched is not None:
            try:
                if self._requires_update:
                    # one grouped compress -> allgather -> decompress (+ one dense allreduce)
                    self._batched.step(self._order, apply=apply)
            finally:   # a step that raised (a corrupted payload reported) leaves the hooks re-armed
                self._reset_cells()
                self._order.clear()
                self._handles.clear()
            self._synchronized = True
            return
        for p in self._requires_update - set(self._handles.keys()):
            self._handles[p] = self._allreduce_grad_async(p)
        for p, (handle, ctx) in list(self._handles.items()):
            if handle is None:
                self._handles[p] = self._allreduce_grad_async(p)
        for p, (handle, ctx) in self._handles.items():
            output = self._synchronize_(handle)
            self._allreduce_delay[p] = self.backward_passes_per_step
            p.grad.set_(self._compression.decompress(output, ctx))
        self._handles.clear()
        self._synchronized = True

    @contextmanager
    def skip_synchronize(self):
        """Use after an explicit ``optimizer.synchronize()`` so ``step()`` does not sync again."""
        self._should_synchronize = False
        try:
            yield
        finally:
            self._should_synchronize = True

    def step(self, closure=None):
        if self._should_synchronize:
            if self._synchronized:
                warnings.warn("optimizer.step() called without optimizer.skip_synchronize() context after "
                              "optimizer.synchronize(). This can cause training slowdown. You may want to "
                              "consider using optimizer.skip_synchronize() context if you use "
                              "optimizer.synchronize() in your code.")
            # batch="apply": this call synchronizes and no closure wants the gradients
            self._synchronize(apply=self._apply_mode and closure is None)
        self._synchronized = False
        return super(self.__class__, self).step(closure)

    def zero_grad(self, *args, **kwargs):
        if self._handles or self._fired[0]:
            raise AssertionError("optimizer.zero_grad() was called after loss.backward() but before "
                                 "optimizer.step() or optimizer.synchronize(). This is prohibited as it "
                                 "can cause a race condition.")
        # torch >= 2: zero_grad(set_to_none=True) by default, as the wrapped optimizer does
        set_to_none = kwargs.get("set_to_none", args[0] if args else True)
        if self._batched is not None:
            # set_to_none=False: the gradients (the batched step's output views) zeroed in
            # place; True: released, as torch does it, without its per-call profiling scaffold
            if self._batched.zero_grads() if not set_to_none else self._batched.release_grads(self.param_groups):
                return None
        return super(self.__class__, self).zero_grad(*args, **kwargs)


def DistributedOptimizer(optimizer, named_parameters=None, compression=Compression.none,
                         backward_passes_per_step=1, op=Average, batch="auto"):
    """Wrap ``optimizer`` so gradients are compressed, exchanged across ranks and
    decompressed before it steps (dgc/horovod/optimizer.py:370-417).

    ``batch="auto"`` (the default) takes the batched step below whenever it computes
    exactly what the per-tensor hooks would (dgc.horovod.batched.auto: a DGCCompressor
    + DGCSGDMemory, neither overriding the methods the hooks call, Average, and the
    parameters on the MI355X in one dtype) — the weights are the same bit for bit, the
    step ~40x faster on ResNet-50 — and the reference's per-tensor hooks otherwise;
    ``batch=False`` forces the per-tensor hooks.

    ``batch=True`` (not in the reference; DGCCompressor + DGCSGDMemory only) exchanges
    every gradient of a step at once in ``synchronize()``: one K1 launch reading the
    gradients where autograd left them, one packed allgather and one decompress for all
    compressed tensors, one allreduce for the dense ones, no host synchronisation and no
    per-parameter launch (dgc/horovod/batched.py). The numerics, the sample-start draws
    and so the weights are those of the per-tensor path. ``batch="sparse"`` also
    replaces decompress's dense ``zero_()`` by a re-zero of the previous step's entries
    when the gradients were not written in between (see dgc/horovod/batched.py for what
    it cannot see).

    ``batch="apply"`` (a ``dgc.optim.DGCSGD`` around fp32 parameters, at most 8 parameter
    groups holding compressed tensors) is ``batch=True`` whose ``step()`` does not decompress
    the compressed tensors into ``p.grad``: their update is applied from the gathered
    entries (``dgc_apply_packed_multi``), the weights and the optimizer state are the same
    bit for bit, and those parameters have ``p.grad = None`` afterwards. A step given a
    closure, or under ``skip_synchronize()`` after an explicit ``synchronize()``, or whose
    exchange is split or has no compressed tensor, decompresses as ``batch=True`` does
    (``BatchedStep.apply_steps`` / ``dense_steps`` count both kinds)."""
    if op == Adasum and comm.size() > 1:
        raise NotImplementedError("Adasum is not part of the DGC path (dgc/horovod/optimizer.py:197-367)")
    if batch and op != Average:
        raise NotImplementedError("batch=True exchanges with Average (dgc/compression.py:23)")
    cls = type(optimizer.__class__.__name__, (optimizer.__class__,), dict(_DistributedOptimizer.__dict__))
    return cls(optimizer.param_groups, named_parameters, compression, backward_passes_per_step, op, batch)
