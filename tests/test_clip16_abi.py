"""The 16-bit clipping entry points (dgc_grad_stats16, dgc_clip_coefs16, dgc_compensate16_clip,
dgc_compensate16_multi_clip, dgc_compress_begin16_clip): exported, declared, and every
argument check answers with the right DGC_ERR_* and a message before anything is launched.
No GPU needed: no pointer given here is ever dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO

OK, INVALID, DTYPE, WORKSPACE = 0, 1, 2, 5
F32, F16, BF16 = 0, 1, 2
SUMSQ, NORM2, ABSMAX = 0, 1, 2
NONE, SCALE, CLAMP = 0, 1, 2
PTR = ctypes.c_void_p(4096)   # non-null, 256-B aligned
ENTRY = {"dgc_grad_stats16": 9, "dgc_clip_coefs16": 6, "dgc_compensate16_clip": 14,
         "dgc_compensate16_multi_clip": 15, "dgc_compress_begin16_clip": 17}


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


def refused(L, rc, code, who, *words):
    err = L.dgc_last_error()
    assert rc == code, (who, rc, err)
    assert who.encode() in err and all(w.encode() in err for w in words), (who, err)


@pytest.mark.parametrize("name", list(ENTRY))
def test_exported_and_declared(L, name):
    assert hasattr(L, name)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, f"include/dgc_hip.h does not declare {name}"
    assert len(m.group(1).split(",")) == ENTRY[name]
    from dgc import _lib
    assert len(_lib._SIGNATURES[name][1]) == ENTRY[name]


def stats16(L, srcs=(4096,), numels=(1000,), kind=NORM2, dtype=BF16, stats=PTR, ws=PTR, ws_bytes=1 << 20, null=()):
    n = len(numels)
    ps = (ctypes.c_void_p * n)(*srcs)
    ns = (ctypes.c_int64 * n)(*numels)
    return L.dgc_grad_stats16(None if "srcs" in null else ps, None if "numels" in null else ns, n, kind, dtype, stats,
                              ws, ws_bytes, None)


def test_grad_stats16_refusals(L):
    who = "dgc_grad_stats16"
    refused(L, stats16(L, null=("srcs",)), INVALID, who, "null")
    refused(L, stats16(L, null=("numels",)), INVALID, who, "null")
    refused(L, stats16(L, stats=None), INVALID, who, "null")
    refused(L, stats16(L, srcs=(None,)), INVALID, who, "pointer")
    refused(L, stats16(L, dtype=F32), DTYPE, who, "dtype")
    refused(L, stats16(L, dtype=3), DTYPE, who, "dtype")
    refused(L, stats16(L, kind=SUMSQ), INVALID, who, "SUMSQ")
    refused(L, stats16(L, kind=7), INVALID, who, "kind")
    refused(L, stats16(L, srcs=(4097,)), INVALID, who, "aligned")            # 1-B aligned
    refused(L, stats16(L, srcs=(4096, 4099), numels=(10, 10)), INVALID, who, "tensor 1", "aligned")
    refused(L, stats16(L, numels=(-1,)), INVALID, who, "numel")
    refused(L, stats16(L, ws=None), WORKSPACE, who, "workspace")
    refused(L, stats16(L, ws_bytes=8), WORKSPACE, who, "workspace")          # short
    refused(L, stats16(L, ws=ctypes.c_void_p(4096 + 8)), WORKSPACE, who, "workspace")   # misaligned
    # a 70-tensor table whose last tensor is bad is refused whole (the first 64 are not launched)
    refused(L, stats16(L, srcs=(4096,) * 69 + (4097,), numels=(10,) * 70), INVALID, who, "tensor 69")
    assert stats16(L, srcs=(), numels=()) == OK                             # an empty table is a no-op


def test_workspace_is_grad_stats_workspace(L):
    ns = (ctypes.c_int64 * 2)(4097, 1)
    need = L.dgc_grad_stats_workspace(ns, 2)
    assert need >= 3 * 8
    ps = (ctypes.c_void_p * 2)(4096, 8192)
    rc = L.dgc_grad_stats16(ps, ns, 2, NORM2, BF16, PTR, PTR, need - 1, None)
    refused(L, rc, WORKSPACE, "dgc_grad_stats16", str(need))


def test_clip_coefs16_refusals(L):
    who = "dgc_clip_coefs16"
    refused(L, L.dgc_clip_coefs16(None, 1, 1.0, BF16, PTR, None), INVALID, who, "null")
    refused(L, L.dgc_clip_coefs16(PTR, 1, 1.0, BF16, None, None), INVALID, who, "null")
    refused(L, L.dgc_clip_coefs16(PTR, 1, 1.0, F32, PTR, None), DTYPE, who, "dtype")
    refused(L, L.dgc_clip_coefs16(PTR, -1, 1.0, F16, PTR, None), INVALID, who)
    assert L.dgc_clip_coefs16(None, 0, 1.0, F16, None, None) == OK


def comp16(L, fn="dgc_compensate16_clip", grad=PTR, mmt=PTR, vec=PTR, out=None, n=100, acc=1, dtype=BF16, kind=SCALE,
           clip=PTR):
    return getattr(L, fn)(grad, mmt, vec, out, None, n, 0.9, 1, acc, dtype, kind, clip, 1.0, None)


def test_compensate16_clip_refusals(L):
    who = "dgc_compensate16_clip"
    refused(L, comp16(L, dtype=F32), DTYPE, who, "dtype")
    refused(L, comp16(L, kind=3), INVALID, who, "clip kind")
    refused(L, comp16(L, kind=-1), INVALID, who, "clip kind")
    refused(L, comp16(L, kind=SCALE, clip=None), INVALID, who, "DGC_CLIP_SCALE")
    refused(L, comp16(L, grad=None), INVALID, who, "null")
    refused(L, comp16(L, mmt=None), INVALID, who, "null")
    refused(L, comp16(L, vec=None), INVALID, who, "vec")
    refused(L, comp16(L, acc=0, out=None), INVALID, who, "out")
    refused(L, comp16(L, n=-1), INVALID, who, "n < 0")
    assert comp16(L, n=0, kind=CLAMP, clip=None) == OK


def multi16(L, grad=PTR, mmt=PTR, vec=PTR, numels=(1000, 5), offsets=(0, 1024), flat=2048, dtype=BF16, kind=SCALE,
            clip=PTR, null=()):
    n = len(numels)
    ns = (ctypes.c_int64 * n)(*numels)
    os_ = (ctypes.c_int64 * n)(*offsets)
    return L.dgc_compensate16_multi_clip(grad, mmt, vec, None, None if "numels" in null else ns,
                                         None if "offsets" in null else os_, n, flat, 0.9, 0, dtype, kind, clip, 1.0,
                                         None)


def test_compensate16_multi_clip_refusals(L):
    who = "dgc_compensate16_multi_clip"
    refused(L, multi16(L, dtype=F32), DTYPE, who, "dtype")
    refused(L, multi16(L, kind=5), INVALID, who, "clip kind")
    refused(L, multi16(L, clip=None), INVALID, who, "DGC_CLIP_SCALE")
    for arg in ("grad", "mmt", "vec"):
        refused(L, multi16(L, **{arg: None}), INVALID, who, "null")
    refused(L, multi16(L, null=("numels",)), INVALID, who, "null")
    refused(L, multi16(L, null=("offsets",)), INVALID, who, "null")
    refused(L, multi16(L, offsets=(0, 1000)), INVALID, who, "tensor 1")        # not at a 1024-element offset
    refused(L, multi16(L, numels=(1000, 1025)), INVALID, who, "tensor 1")      # past flat_numel
    refused(L, multi16(L, numels=(-1, 5)), INVALID, who, "tensor 0")
    refused(L, multi16(L, numels=(5,) * 69 + (-2,), offsets=tuple(1024 * i for i in range(70)), flat=70 * 1024),
            INVALID, who, "tensor 69")
    assert multi16(L, numels=(), offsets=()) == OK
    # DGC_CLIP_NONE is allowed, with or without a table: the clip check passes and the next
    # refusal is the table's (a tensor past flat_numel)
    for clip in (None, PTR):
        refused(L, multi16(L, kind=NONE, clip=clip, numels=(1000, 1025)), INVALID, who, "tensor 1")
    refused(L, multi16(L, kind=CLAMP, clip=None, numels=(1000, 1025)), INVALID, who, "tensor 1")


def params(dtype=BF16):
    from dgc import _lib
    p = _lib.SelectParams()
    p.numel, p.num_selects, p.num_samples = 100000, 100, 1000
    p.max_iters, p.resample, p.masking = 10, 1, 1
    p.vdtype = p.thr_dtype = dtype
    p.update_memory = 0
    return p


def begin16(L, p, dtype=BF16, grad=PTR, mmt=PTR, vec=PTR, vec32=PTR, kind=SCALE, clip=PTR):
    return L.dgc_compress_begin16_clip(grad, mmt, vec, vec32, 0.9, 1, 3, 100, ctypes.byref(p), None, kind, clip, 1.0,
                                       None, 0, dtype, None)


def test_compress_begin16_clip_refusals(L):
    who = "dgc_compress_begin16_clip"   # the refusal names the function that was called
    refused(L, begin16(L, params(F32), dtype=F32), INVALID, who, "dtype")
    for arg in ("grad", "mmt", "vec", "vec32"):
        refused(L, begin16(L, params(), **{arg: None}), INVALID, who, "null")
    refused(L, begin16(L, params(), kind=3), INVALID, who, "clip kind")
    refused(L, begin16(L, params(), kind=SCALE, clip=None), INVALID, who, "DGC_CLIP_SCALE")
    refused(L, begin16(L, params(), grad=ctypes.c_void_p(4098)), INVALID, who, "aligned")
    p = params()
    p.update_memory = 2
    refused(L, begin16(L, p), INVALID, who, "update_memory")
    # everything valid, for every clip kind: the next refusal is the missing workspace (no launch)
    for dt in (BF16, F16):
        for kind, clip in ((NONE, None), (SCALE, PTR), (CLAMP, None), (CLAMP, PTR)):
            refused(L, begin16(L, params(dt), dtype=dt, kind=kind, clip=clip), WORKSPACE, "workspace")
    # the unclipped entry point still answers under its own name
    rc = L.dgc_compress_begin16(None, PTR, PTR, PTR, 0.9, 1, 3, 100, ctypes.byref(params()), None, None, 0, BF16, None)
    assert rc == INVALID and b"dgc_compress_begin16:" in L.dgc_last_error(), L.dgc_last_error()
