"""The refusals of the entry points whose argument checks go through csrc/payload.hpp and
csrc/dispatch.hpp — a table of bad calls per entry point, some with two faults at once to pin
which one wins — answer with the status and the dgc_last_error() text they had before those
headers existed. No GPU needed: each row is refused before the library touches HIP (no launch,
no allocation); the pointers are never dereferenced. (dgc_compress reaches the same checks as
dgc_compress_finish, but only behind its K1 launch, so it has no row.)

The expected (status, message) pairs in tests/golden/abi_refusals.json were recorded from a
library built from the commit before the headers (tests/golden/make_abi_refusals.py).
"""
import ctypes
import json
import os

import pytest

from conftest import GOLDEN

OK, INVALID, DTYPE, OVERFLOW, HIP, WORKSPACE = 0, 1, 2, 3, 4, 5
F32, F16, BF16 = 0, 1, 2
I64, I32 = 0, 1
NONE, SCALE, CLAMP = 0, 1, 2
NORM2 = 1                 # dgc_stat_kind
PTR = 4096                # non-null, 256-B aligned; never dereferenced on these paths
N, W, CAP, PARTS = 5001, 2, 8, 2
STRIDE = 256              # dgc_payload_layout(8, any value dtype, any index dtype)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _ptrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


def _params(thr_dtype=BF16, update_memory=0):
    """A dgc_select_params the one-tensor compress entry points accept (exact path: every element sampled)."""
    from dgc import _lib
    p = _lib.SelectParams()
    p.numel = p.num_samples = N
    p.num_selects, p.upper_count, p.lower_count = 50, 65, 40
    p.upper, p.lower, p.max_iters = 1.3, 0.8, 10
    p.vdtype, p.idtype, p.thr_dtype, p.update_memory = thr_dtype, I64, thr_dtype, update_memory
    return ctypes.pointer(p)


_BATCH_KEEP = []   # the tables a dgc_batch_desc points at


def _batch(dtype=F32):
    """A dgc_batch_desc every dgc_batch_* entry point lays out: two unsampled tensors of one flat buffer."""
    from dgc import _lib
    b = _lib.BatchDesc()
    tables = dict(numel=_i64(3000, 2001), offset=_i64(0, 3072), num_selects=_i64(30, 20), num_samples=_i64(3000, 2001),
                  top_k_samples=_i64(30, 20), sample_stride=_i64(1, 1))
    _BATCH_KEEP.append(tables)
    for k, v in tables.items():
        setattr(b, k, v)
    b.count, b.flat_numel, b.upper_bound, b.lower_bound, b.max_iters = 2, 5120, 1.3, 0.8, 10
    b.momentum_masking, b.nesterov, b.momentum, b.spec_margin, b.dtype = 1, 1, 0.9, 0.8, dtype
    return ctypes.pointer(b)


_HYPERS = (ctypes.c_float * 5)(0.1, 0.9, 0.0, 1e-4, 0.0)   # one dgc_apply_hyper with weight decay (20 bytes)

# name -> (argument names in ABI order, a call that passes every check; it is never made)
FUNCS = {
    "dgc_compensate16": ("grad mmt vec out vec32 n momentum nesterov accumulate dtype stream",
                         dict(grad=PTR, mmt=PTR, vec=PTR, n=N, momentum=0.9, accumulate=1, dtype=BF16)),
    "dgc_compensate16_clip": ("grad mmt vec out vec32 n momentum nesterov accumulate dtype clip_kind clip clip_value stream",
                              dict(grad=PTR, mmt=PTR, vec=PTR, n=N, momentum=0.9, accumulate=1, dtype=F16,
                                   clip_kind=SCALE, clip=PTR)),
    "dgc_compensate16_multi_clip": ("grad mmt vec vec32 numels offsets count flat_numel momentum nesterov dtype "
                                    "clip_kind clip clip_value stream",
                                    dict(grad=PTR, mmt=PTR, vec=PTR, numels=_i64(1000, 5), offsets=_i64(0, 1024), count=2,
                                         flat_numel=2048, momentum=0.9, dtype=BF16, clip_kind=CLAMP, clip_value=0.5)),
    "dgc_widen16": ("x y n dtype stream", dict(x=PTR, y=PTR, n=N, dtype=BF16)),
    "dgc_mask_indices16": ("mmt vec n indices idtype count bad_flag stream",
                           dict(mmt=PTR, vec=PTR, n=N, indices=PTR, idtype=I32, count=CAP, bad_flag=PTR)),
    "dgc_mask_indices": ("mmt vec n indices idtype count bad_flag stream",
                         dict(mmt=PTR, vec=PTR, n=N, indices=PTR, idtype=I32, count=CAP, bad_flag=PTR)),
    "dgc_decompress16": ("values vdtype indices idtype run_offsets nruns grad dtype n scale bad_flag stream",
                         dict(values=PTR, vdtype=BF16, indices=PTR, idtype=I64, run_offsets=_i64(0, CAP, 2 * CAP), nruns=2,
                              grad=PTR, dtype=BF16, n=N, scale=0.5, bad_flag=PTR)),
    "dgc_mask_packed16": ("payload capacity vdtype idtype mmt vec n stream",
                          dict(payload=PTR, capacity=CAP, vdtype=BF16, idtype=I64, mmt=PTR, vec=PTR, n=N)),
    "dgc_decompress_packed16": ("payload world rank_stride capacity vdtype idtype grad dtype n scale bad_flag stream",
                                dict(payload=PTR, world=W, rank_stride=STRIDE, capacity=CAP, vdtype=BF16, idtype=I64,
                                     grad=PTR, dtype=BF16, n=N, scale=0.5, bad_flag=PTR)),
    "dgc_decompress": ("values vdtype indices idtype total run_offsets nruns grad n scale ws ws_bytes stream",
                       dict(values=PTR, vdtype=F32, indices=PTR, idtype=I64, total=2 * CAP, run_offsets=_i64(0, CAP, 2 * CAP),
                            nruns=2, grad=PTR, n=N, scale=0.5, ws=PTR, ws_bytes=1 << 24)),
    "dgc_payload_split": ("payload capacity parts vdtype idtype split stream",
                          dict(payload=PTR, capacity=CAP, parts=PARTS, vdtype=F32, idtype=I64, split=PTR)),
    "dgc_scatter_split": ("gathered world parts part capacity vdtype idtype grad n scale cleared ws ws_bytes stream",
                          dict(gathered=PTR, world=W, parts=PARTS, capacity=CAP, vdtype=F32, idtype=I64, grad=PTR, n=N,
                               scale=0.5, ws=PTR, ws_bytes=1 << 24)),
    "dgc_clear_split": ("prev world parts capacity vdtype idtype grad n ws ws_bytes stream",
                        dict(prev=PTR, world=W, parts=PARTS, capacity=CAP, vdtype=F32, idtype=I64, grad=PTR, n=N, ws=PTR,
                             ws_bytes=1 << 24)),
    "dgc_scatter_split16": ("gathered world parts part capacity vdtype idtype grad dtype n scale ws ws_bytes stream",
                            dict(gathered=PTR, world=W, parts=PARTS, capacity=CAP, vdtype=BF16, idtype=I64, grad=PTR,
                                 dtype=BF16, n=N, scale=0.5, ws=PTR, ws_bytes=1 << 24)),
    "dgc_decompress_packed_over": ("payload prev world rank_stride capacity vdtype idtype grad n scale ws ws_bytes stream",
                                   dict(payload=PTR, prev=2 * PTR, world=W, rank_stride=STRIDE, capacity=CAP, vdtype=F32,
                                        idtype=I64, grad=PTR, n=N, scale=0.5, ws=PTR, ws_bytes=1 << 24)),
    "dgc_clear_packed": ("prev world rank_stride capacity vdtype idtype grad n ws ws_bytes stream",
                         dict(prev=PTR, world=W, rank_stride=STRIDE, capacity=CAP, vdtype=F32, idtype=I64, grad=PTR, n=N,
                              ws=PTR, ws_bytes=1 << 24)),
    "dgc_apply_packed": ("payload world rank_stride capacity vdtype idtype acc param buf first n lr momentum dampening "
                         "weight_decay nesterov ws ws_bytes stream",
                         dict(payload=PTR, world=W, rank_stride=STRIDE, capacity=CAP, vdtype=F32, idtype=I64, acc=PTR,
                              param=PTR, buf=PTR, n=N, lr=0.1, momentum=0.9, weight_decay=1e-4, ws=PTR, ws_bytes=1 << 20)),
    "dgc_apply_packed_multi": ("payload world rank_stride capacity vdtype idtype acc flat_numel table count dense_blocks "
                               "hypers groups ws ws_bytes stream",
                               dict(payload=PTR, world=W, rank_stride=STRIDE, capacity=CAP, vdtype=F32, idtype=I64, acc=PTR,
                                    flat_numel=N, table=PTR, count=1, dense_blocks=2, hypers=_HYPERS, groups=1, ws=PTR,
                                    ws_bytes=1 << 20)),
    "dgc_sgd_step16": ("params grads bufs numels first count lr momentum dampening weight_decay nesterov dtype stream",
                       dict(params=_ptrs(PTR), grads=_ptrs(PTR), numels=_i64(N), count=1, lr=0.1, dtype=BF16)),
    "dgc_compensate_clip": ("grad mmt vec out n momentum nesterov accumulate samples s_start s_stride s_count clip_kind "
                            "clip clip_value stream",
                            dict(grad=PTR, mmt=PTR, vec=PTR, n=N, momentum=0.9, accumulate=1, s_stride=1, clip_kind=SCALE,
                                 clip=PTR)),
    "dgc_compensate_multi_clip": ("srcs numels offsets count round_to mmt out momentum nesterov clip_kind clip clip_value "
                                  "stream",
                                  dict(srcs=_ptrs(PTR, PTR), numels=_i64(1000, 5), offsets=_i64(0, 1024), count=2, mmt=PTR,
                                       out=PTR, momentum=0.9, clip_kind=SCALE, clip=PTR)),
    "dgc_gather_cast": ("srcs numels offsets count dst dtype stream",
                        dict(srcs=_ptrs(PTR, PTR), numels=_i64(1000, 5), offsets=_i64(0, 1024), count=2, dst=PTR, dtype=F16)),
    "dgc_rank_sum": ("src dtype world rank_stride n average dst stream",
                     dict(src=PTR, dtype=BF16, world=W, rank_stride=2 * N, n=N, average=1, dst=PTR)),
    "dgc_compensate_ranks": ("src dtype world rank_stride mmt out n momentum nesterov stream",
                             dict(src=PTR, dtype=F16, world=W, rank_stride=2 * N, mmt=PTR, out=PTR, n=N, momentum=0.9)),
    "dgc_grad_stats16": ("srcs numels count kind dtype stats ws ws_bytes stream",
                         dict(srcs=_ptrs(PTR, PTR), numels=_i64(1000, 5), count=2, kind=NORM2, dtype=BF16, stats=PTR, ws=PTR,
                              ws_bytes=1 << 20)),
    "dgc_clip_coefs16": ("stats count max_norm dtype clip stream", dict(stats=PTR, count=2, max_norm=1.0, dtype=F16, clip=PTR)),
    "dgc_clip_apply": ("tensors numels count kind clip value stream",
                       dict(tensors=_ptrs(PTR, PTR), numels=_i64(1000, 5), count=2, kind=SCALE, clip=PTR)),
    "dgc_compress_begin16_clip": ("grad mmt vec vec32 momentum nesterov s_start s_stride select_params spec clip_kind clip "
                                  "clip_value ws ws_bytes dtype stream",
                                  dict(grad=PTR, mmt=PTR, vec=PTR, vec32=PTR, momentum=0.9, s_stride=1, select_params=None,
                                       clip_kind=SCALE, clip=PTR, ws=PTR, ws_bytes=1 << 24, dtype=BF16)),
    "dgc_compress_begin_clip": ("grad mmt vec momentum nesterov s_start s_stride select_params spec clip_kind clip clip_value ws "
                                "ws_bytes stream",
                                dict(grad=PTR, mmt=PTR, vec=PTR, momentum=0.9, s_stride=1, select_params=None, clip_kind=SCALE,
                                     clip=PTR, ws=PTR, ws_bytes=1 << 24)),
    # select_params / batch: built per call (_params, _batch); a row changes a field as "p.<field>" / "b.<field>"
    "dgc_select": ("vec mmt thr0 select_params values indices count info ws ws_bytes sync_mode stream",
                   dict(vec=PTR, mmt=PTR, thr0=PTR, values=PTR, indices=PTR, ws=PTR, ws_bytes=1 << 24)),
    "dgc_compress_finish": ("vec mmt s_start s_stride top_k_samples select_params spec spec_margin values indices count info "
                            "ws ws_bytes sync_mode stream",
                            dict(vec=PTR, mmt=PTR, s_stride=1, top_k_samples=50, values=PTR, indices=PTR, ws=PTR,
                                 ws_bytes=1 << 24)),
    "dgc_batch_init": ("batch ws ws_bytes stream", dict(ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_compress": ("batch grad mmt vec sample_starts payload info ws ws_bytes sync_mode stream",
                           dict(grad=PTR, mmt=PTR, vec=PTR, sample_starts=_i64(0, 0), payload=PTR, ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_compress_begin": ("batch grad mmt vec sample_starts ws ws_bytes stream",
                                 dict(grad=PTR, mmt=PTR, vec=PTR, sample_starts=_i64(0, 0), ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_compress_begin_ptrs": ("batch grads mmt vec sample_starts ws ws_bytes stream",
                                      dict(grads=_ptrs(PTR, PTR), mmt=PTR, vec=PTR, sample_starts=_i64(0, 0), ws=PTR,
                                           ws_bytes=1 << 24)),
    "dgc_batch_compress_begin_clip": ("batch grad mmt vec sample_starts clip_kind clip clip_value ws ws_bytes stream",
                                      dict(grad=PTR, mmt=PTR, vec=PTR, sample_starts=_i64(0, 0), clip_kind=SCALE, clip=PTR,
                                           ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_compress_begin_ptrs_clip": ("batch grads mmt vec sample_starts clip_kind clip clip_value ws ws_bytes stream",
                                           dict(grads=_ptrs(PTR, PTR), mmt=PTR, vec=PTR, sample_starts=_i64(0, 0),
                                                clip_kind=SCALE, clip=PTR, ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_compress_finish": ("batch mmt vec payload info ws ws_bytes sync_mode stream",
                                  dict(mmt=PTR, vec=PTR, payload=PTR, ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_select": ("batch vec32 mmt32 sample_starts payload info ws ws_bytes sync_mode stream",
                         dict(vec32=PTR, mmt32=PTR, sample_starts=_i64(0, 0), payload=PTR, ws=PTR, ws_bytes=1 << 24)),
    "dgc_batch_flush": ("batch mmt vec ws ws_bytes stream", dict(mmt=PTR, vec=PTR, ws=PTR, ws_bytes=1 << 24)),
}
for _alias in ("dgc_decompress_packed", "dgc_scatter_packed", "dgc_scatter_packed_cleared"):
    names, base = FUNCS["dgc_decompress_packed_over"]
    FUNCS[_alias] = (names.replace(" prev", ""), {k: v for k, v in base.items() if k != "prev"})

PACKED32 = ("dgc_decompress_packed", "dgc_scatter_packed", "dgc_scatter_packed_cleared", "dgc_decompress_packed_over",
            "dgc_clear_packed")
SPLIT32 = ("dgc_scatter_split", "dgc_clear_split")

# (entry point, what is wrong, the arguments that differ from the accepted call)
ROWS = []
for fn in PACKED32 + SPLIT32 + ("dgc_apply_packed", "dgc_apply_packed_multi", "dgc_decompress"):
    ROWS += [(fn, "bad value dtype", dict(vdtype=7)), (fn, "bf16 wire to an fp32 receiver", dict(vdtype=BF16)),
             (fn, "bad index dtype", dict(idtype=2)), (fn, "bad value and index dtype", dict(vdtype=-1, idtype=9))]
for fn in PACKED32 + SPLIT32 + ("dgc_decompress", "dgc_scatter_split16"):
    ROWS += [(fn, "null workspace", dict(ws=None)), (fn, "short workspace", dict(ws_bytes=255)),
             (fn, "misaligned workspace", dict(ws=PTR + 128)), (fn, "null grad", dict(grad=None)), (fn, "n = 0", dict(n=0)),
             (fn, "bad dtype and short workspace", dict(idtype=5, ws_bytes=0))]
for fn in PACKED32 + ("dgc_apply_packed", "dgc_apply_packed_multi", "dgc_decompress_packed16"):
    ROWS += [(fn, "short rank_stride", dict(rank_stride=STRIDE - 1)), (fn, "zero rank_stride", dict(rank_stride=0))]
for fn in PACKED32:
    ROWS += [(fn, "null payload", dict(prev=None) if fn == "dgc_clear_packed" else dict(payload=None)),
             (fn, "capacity < 0", dict(capacity=-1)), (fn, "world = 65", dict(world=65)),
             (fn, "short rank_stride and short workspace", dict(rank_stride=8, ws_bytes=64))]
ROWS += [("dgc_decompress_packed_over", "null prev", dict(prev=None)),
         ("dgc_decompress_packed_over", "prev is the payload", dict(prev=PTR))]
for fn in SPLIT32 + ("dgc_scatter_split16",):
    ROWS += [(fn, "null gathered", dict(prev=None) if fn == "dgc_clear_split" else dict(gathered=None)),
             (fn, "parts = 1", dict(parts=1)), (fn, "parts = 9", dict(parts=9)), (fn, "world * parts = 72", dict(world=9, parts=8)),
             (fn, "parts = 1 and bad value dtype", dict(parts=1, vdtype=5))]
ROWS += [("dgc_scatter_split", "part = parts", dict(part=PARTS)), ("dgc_scatter_split16", "part = -1", dict(part=-1)),
         ("dgc_scatter_split16", "fp32 grad", dict(dtype=F32)), ("dgc_scatter_split16", "bad grad dtype", dict(dtype=3)),
         ("dgc_scatter_split16", "bad value dtype", dict(vdtype=3)), ("dgc_scatter_split16", "bad index dtype", dict(idtype=-1)),
         ("dgc_scatter_split16", "odd grad address", dict(grad=PTR + 1)),
         ("dgc_scatter_split16", "fp32 grad and bad value dtype", dict(dtype=F32, vdtype=3))]
ROWS += [("dgc_payload_split", "bad value dtype", dict(vdtype=3)), ("dgc_payload_split", "bad index dtype", dict(idtype=2)),
         ("dgc_payload_split", "null payload", dict(payload=None)), ("dgc_payload_split", "null split", dict(split=None)),
         ("dgc_payload_split", "parts = 9", dict(parts=9)), ("dgc_payload_split", "misaligned split", dict(split=PTR + 64)),
         ("dgc_payload_split", "bad dtype and null payload", dict(vdtype=3, payload=None))]
ROWS += [("dgc_decompress", "null values", dict(values=None)), ("dgc_decompress", "65 runs", dict(nruns=65))]
for fn in ("dgc_apply_packed", "dgc_apply_packed_multi"):
    ROWS += [(fn, "null payload", dict(payload=None)), (fn, "null acc", dict(acc=None)), (fn, "world = 0", dict(world=0)),
             (fn, "capacity < 0", dict(capacity=-1)), (fn, "null workspace", dict(ws=None)), (fn, "short workspace", dict(ws_bytes=8)),
             (fn, "world = 0 and bad value dtype", dict(world=0, vdtype=4))]
ROWS += [("dgc_apply_packed", "misaligned workspace", dict(ws=PTR + 2)), ("dgc_apply_packed", "negative lr", dict(lr=-0.1)),
         ("dgc_apply_packed", "momentum without buf", dict(buf=None)),
         ("dgc_apply_packed_multi", "misaligned workspace", dict(ws=PTR + 64)),
         ("dgc_apply_packed_multi", "nine groups", dict(groups=9)), ("dgc_apply_packed_multi", "null table", dict(table=None))]
for fn in ("dgc_compensate16", "dgc_compensate16_clip", "dgc_compensate16_multi_clip", "dgc_widen16", "dgc_sgd_step16",
           "dgc_grad_stats16", "dgc_clip_coefs16", "dgc_compress_begin16_clip"):
    ROWS += [(fn, "fp32 to a 16-bit entry point", dict(dtype=F32)), (fn, "bad dtype", dict(dtype=3))]
for fn in ("dgc_decompress16", "dgc_decompress_packed16"):
    ROWS += [(fn, "fp32 grad", dict(dtype=F32)), (fn, "bad value dtype", dict(vdtype=3)), (fn, "bad index dtype", dict(idtype=2)),
             (fn, "null grad", dict(grad=None)), (fn, "null bad_flag", dict(bad_flag=None)),
             (fn, "fp32 grad and bad value dtype", dict(dtype=F32, vdtype=3)),
             (fn, "bad value and index dtype", dict(vdtype=3, idtype=2))]
ROWS += [("dgc_decompress16", "descending run offsets", dict(run_offsets=_i64(0, CAP, CAP - 1))),
         ("dgc_decompress16", "null values", dict(values=None)),
         ("dgc_decompress_packed16", "null payload", dict(payload=None)), ("dgc_decompress_packed16", "world = 0", dict(world=0)),
         ("dgc_decompress_packed16", "bad index dtype and short rank_stride", dict(idtype=2, rank_stride=0)),
         ("dgc_mask_packed16", "bad index dtype", dict(idtype=2)), ("dgc_mask_packed16", "null payload", dict(payload=None)),
         ("dgc_mask_packed16", "null vec", dict(vec=None)), ("dgc_mask_packed16", "null vec and bad index dtype", dict(vec=None, idtype=2))]
for fn in ("dgc_mask_indices16", "dgc_mask_indices"):
    ROWS += [(fn, "bad index dtype", dict(idtype=2)), (fn, "null vec", dict(vec=None)), (fn, "null indices", dict(indices=None)),
             (fn, "null vec and bad index dtype", dict(vec=None, idtype=-1))]
for fn in ("dgc_compensate16_clip", "dgc_compensate16_multi_clip", "dgc_compensate_clip", "dgc_compensate_multi_clip",
           "dgc_clip_apply", "dgc_compress_begin16_clip", "dgc_compress_begin_clip"):
    kind = "kind" if fn == "dgc_clip_apply" else "clip_kind"
    ROWS += [(fn, "bad clip kind", {kind: 3}), (fn, "negative clip kind", {kind: -1}),
             (fn, "DGC_CLIP_SCALE without a table", {kind: SCALE, "clip": None})]
ROWS += [("dgc_clip_apply", "DGC_CLIP_NONE", dict(kind=NONE)), ("dgc_clip_apply", "null tensors", dict(tensors=None)),
         ("dgc_clip_apply", "null tensors and bad clip kind", dict(tensors=None, kind=3)),
         ("dgc_compensate16_clip", "bad dtype and bad clip kind", dict(dtype=F32, clip_kind=3)),
         ("dgc_compensate16_clip", "bad clip kind and null grad", dict(clip_kind=3, grad=None)),
         ("dgc_compensate16_clip", "null grad", dict(grad=None)), ("dgc_compensate16_clip", "n < 0", dict(n=-1)),
         ("dgc_compensate16", "accumulate without vec", dict(vec=None)),
         ("dgc_compensate16", "dense branch without out", dict(accumulate=0)),
         ("dgc_compensate16_multi_clip", "null numels", dict(numels=None)),
         ("dgc_compensate16_multi_clip", "offset not a multiple of 1024", dict(offsets=_i64(0, 1000))),
         ("dgc_compensate16_multi_clip", "tensor past flat_numel", dict(flat_numel=1024)),
         ("dgc_compensate16_multi_clip", "bad clip kind and null numels", dict(clip_kind=9, numels=None)),
         ("dgc_compensate_clip", "null grad", dict(grad=None)), ("dgc_compensate_clip", "n < 0 and bad clip kind", dict(n=-1, clip_kind=3)),
         ("dgc_compensate_multi_clip", "bad round_to", dict(round_to=BF16)),
         ("dgc_compensate_multi_clip", "bad round_to and bad clip kind", dict(round_to=BF16, clip_kind=3)),
         ("dgc_compensate_multi_clip", "null mmt", dict(mmt=None)),
         ("dgc_gather_cast", "bad dtype", dict(dtype=3)), ("dgc_gather_cast", "null dst", dict(dst=None)),
         ("dgc_widen16", "null x", dict(x=None)), ("dgc_sgd_step16", "null params", dict(params=None)),
         ("dgc_grad_stats16", "short workspace", dict(ws_bytes=8)), ("dgc_grad_stats16", "misaligned workspace", dict(ws=PTR + 8)),
         ("dgc_grad_stats16", "sum of squares", dict(kind=0)), ("dgc_grad_stats16", "odd tensor address", dict(srcs=_ptrs(PTR, PTR + 1))),
         ("dgc_clip_coefs16", "null stats", dict(stats=None)),
         ("dgc_compress_begin16_clip", "null vec32", dict(vec32=None)),
         ("dgc_compress_begin16_clip", "thr_dtype is not the dtype", dict(dtype=F16)),
         ("dgc_compress_begin16_clip", "misaligned grad", dict(grad=PTR + 8)),
         ("dgc_compress_begin16_clip", "short workspace", dict(ws_bytes=256)),
         ("dgc_compress_begin16_clip", "bad dtype and bad clip kind", dict(dtype=F32, clip_kind=3)),
         ("dgc_compress_begin_clip", "null grad", dict(grad=None)), ("dgc_compress_begin_clip", "short workspace", dict(ws_bytes=256))]
for fn in ("dgc_rank_sum", "dgc_compensate_ranks"):
    ROWS += [(fn, "bad wire dtype", dict(dtype=3)), (fn, "short rank_stride", dict(rank_stride=2 * N - 2)),
             (fn, "odd source address", dict(src=PTR + 1)), (fn, "null src", dict(src=None)),
             (fn, "bad wire dtype and short rank_stride", dict(dtype=3, rank_stride=0))]
ROWS += [("dgc_compensate_ranks", "bf16 wire to fp32 parameters", dict(dtype=BF16, rank_stride=2 * N)),
         ("dgc_compensate_ranks", "null mmt", dict(mmt=None)), ("dgc_rank_sum", "null dst", dict(dst=None))]
for fn in ("dgc_select", "dgc_compress_finish"):   # validate_select
    ROWS += [(fn, "bad value dtype", {"p.vdtype": 3}), (fn, "bad threshold dtype", {"p.thr_dtype": 3}),
             (fn, "negative threshold dtype", {"p.thr_dtype": -1}), (fn, "bad index dtype", {"p.idtype": 2}),
             (fn, "bad value and index dtype", {"p.vdtype": 7, "p.idtype": 2}),
             (fn, "bad threshold and index dtype", {"p.thr_dtype": 3, "p.idtype": -1}),
             (fn, "bad index dtype and null outputs", {"p.idtype": 2, "values": None}),
             (fn, "num_selects > numel and bad value dtype", {"p.num_selects": N + 1, "p.vdtype": 3}),
             (fn, "null outputs", dict(indices=None))]
BATCH = [fn for fn in FUNCS if fn.startswith("dgc_batch_")]
for fn in BATCH:   # batch_layout
    ROWS += [(fn, "bad dtype", {"b.dtype": 3}), (fn, "negative dtype", {"b.dtype": -1}),
             (fn, "tensor past flat_numel and bad dtype", {"b.flat_numel": 5000, "b.dtype": 3}),
             (fn, "empty table", {"b.count": 0})]
for fn in ("dgc_batch_compress_begin_clip", "dgc_batch_compress_begin_ptrs_clip"):   # check_clip comes first
    ROWS += [(fn, "bad clip kind", dict(clip_kind=3)), (fn, "negative clip kind", dict(clip_kind=-1)),
             (fn, "DGC_CLIP_SCALE without a table", dict(clip=None)),
             (fn, "bad clip kind and bad dtype", {"clip_kind": 3, "b.dtype": 3}),
             (fn, "DGC_CLIP_SCALE without a table and short workspace", dict(clip=None, ws_bytes=8))]
ROWS += [("dgc_batch_compress_begin_ptrs_clip", "null gradient table and bad clip kind", dict(grads=None, clip_kind=3)),
         ("dgc_batch_compress_begin_ptrs", "null gradient table and bad dtype", {"grads": None, "b.dtype": 3})]

IDS = ["%s: %s" % (fn, what) for fn, what, _ in ROWS]


def refuse(L, fn, change):
    """(status, dgc_last_error()) of the accepted call of `fn` with `change` applied."""
    names, base = FUNCS[fn]
    args = dict(base, **{k: v for k, v in change.items() if "." not in k})
    unknown = set(args) - set(names.split())
    assert not unknown, (fn, unknown)
    if "select_params" in names.split():
        args["select_params"] = _params(thr_dtype=BF16 if fn == "dgc_compress_begin16_clip" else F32,
                                        update_memory=0 if fn == "dgc_compress_begin16_clip" else 1)
    if "batch" in names.split():
        args["batch"] = _batch()
    for k, v in change.items():   # "p.vdtype": a field of the dgc_select_params, "b.dtype": of the dgc_batch_desc
        if "." in k:
            struct = args["select_params" if k[0] == "p" else "batch"].contents
            assert hasattr(struct, k[2:]), k
            setattr(struct, k[2:], v)
    from dgc import _lib
    # an argument the accepted call does not name is 0 / null
    types = _lib._SIGNATURES[fn][1]
    assert len(types) == len(names.split()), fn
    zero = [0 if t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float) else None for t in types]
    status = getattr(L, fn)(*[args.get(a, z) for a, z in zip(names.split(), zero)])
    return [int(status), L.dgc_last_error().decode()]


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "abi_refusals.json")) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(recorded):
    assert len(set(IDS)) == len(IDS)
    assert sorted(recorded) == sorted(IDS)


@pytest.mark.parametrize("fn, what, change", ROWS, ids=IDS)
def test_refusal(L, recorded, fn, what, change):
    status, message = refuse(L, fn, change)
    assert status not in (OK, HIP), (status, message)   # refused, and before anything reached HIP
    assert message.startswith("dgc_")
    assert [status, message] == recorded["%s: %s" % (fn, what)]
