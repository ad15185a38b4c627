"""dgc_compress_begin16 (K1-16 of the flat bucket): exported, declared, and its argument
checks answer before anything is launched. No GPU needed."""
import ctypes
import os
import re

import pytest

from conftest import REPO

INVALID = 1
F32, F16, BF16 = 0, 1, 2
PTR = ctypes.c_void_p(4096)   # non-null, 16-B aligned; never dereferenced on these paths


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


def params(dtype=BF16, update_memory=0):
    from dgc import _lib
    p = _lib.SelectParams()
    p.numel, p.num_selects, p.num_samples = 100000, 100, 1000
    p.max_iters, p.resample, p.masking = 10, 1, 1
    p.vdtype = p.thr_dtype = dtype
    p.update_memory = update_memory
    return p


def begin16(L, p, dtype=BF16, grad=PTR, mmt=PTR, vec=PTR, vec32=PTR, ws=None, ws_bytes=0):
    return L.dgc_compress_begin16(grad, mmt, vec, vec32, 0.9, 1, 3, 100, ctypes.byref(p), None, ws, ws_bytes, dtype,
                                  None)


def test_exported_and_declared(L):
    assert hasattr(L, "dgc_compress_begin16")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dgc_compress_begin16\s*\(([^;]*)\)\s*;", text)
    assert m, "include/dgc_hip.h does not declare dgc_compress_begin16"
    # grad, mmt, vec, vec32, momentum, nesterov, start, stride, params, spec, ws, ws_bytes, dtype, stream
    assert len(m.group(1).split(",")) == 14


@pytest.mark.parametrize("what, kwargs, message", [
    ("dtype = DGC_F32", dict(dtype=F32), b"dtype"),
    ("null grad", dict(grad=None), b"null"),
    ("null mmt", dict(mmt=None), b"null"),
    ("null vec32", dict(vec32=None), b"null"),
])
def test_refuses_before_any_launch(L, what, kwargs, message):
    p = params(kwargs.get("dtype", BF16))
    rc = begin16(L, p, **kwargs)
    assert rc == INVALID, (what, L.dgc_last_error())
    err = L.dgc_last_error()
    assert b"dgc_compress_begin16" in err and message in err, (what, err)


def test_refuses_update_memory_and_thr_dtype(L):
    rc = begin16(L, params(update_memory=1))
    assert rc == INVALID and b"update_memory" in L.dgc_last_error(), L.dgc_last_error()
    rc = begin16(L, params(update_memory=2))
    assert rc == INVALID and b"update_memory" in L.dgc_last_error(), L.dgc_last_error()
    p = params(BF16)
    rc = begin16(L, p, dtype=F16)                      # thr_dtype bf16 on an fp16 call
    assert rc == INVALID and b"thr_dtype" in L.dgc_last_error(), L.dgc_last_error()
    rc = begin16(L, params(), grad=ctypes.c_void_p(4098))   # an 8-B vector load needs the alignment
    assert rc == INVALID and b"aligned" in L.dgc_last_error(), L.dgc_last_error()


def test_valid_arguments_reach_the_workspace_check(L):
    """Everything above passed: the next refusal is the missing workspace (still no launch)."""
    WORKSPACE = 5
    for dt in (BF16, F16):
        rc = begin16(L, params(dt), dtype=dt)
        assert rc == WORKSPACE, (dt, rc, L.dgc_last_error())


def test_algorithmic_bytes_default_unchanged():
    from dgc.bucket import algorithmic_bytes
    N, k, S, W = 10 ** 9, 10 ** 6, 10 ** 7, 8
    assert algorithmic_bytes(N, k, S, W) == 28 * N + 4 * S + 8 * k + (1 + W) * k * 12 + 8 * W * k
    # 16-bit state: K1-16 14N + the image re-read 4N + the 2N decompress write
    assert algorithmic_bytes(N, k, S, W, vbytes=2, sbytes=2) == 20 * N + 4 * S + 4 * k + (1 + W) * k * 10 + 4 * W * k
