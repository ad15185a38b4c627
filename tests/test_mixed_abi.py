"""dgc_compress_begin_g16 (K1 of the flat bucket with fp32 state and a bf16 / fp16 gradient):
exported, declared, bound, and every refusal answers with its status and a message before
anything is launched. No GPU needed: the pointers are never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO

OK, INVALID, DTYPE, WORKSPACE = 0, 1, 2, 5
F32, F16, BF16 = 0, 1, 2
PTR = ctypes.c_void_p(4096)   # non-null, 256-B aligned
NAME = "dgc_compress_begin_g16"


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


def params(numel=100000, num_samples=1000):
    from dgc import _lib
    p = _lib.SelectParams()
    p.numel, p.num_selects, p.num_samples = numel, 100, num_samples
    p.max_iters, p.resample, p.masking = 10, 1, 1
    p.vdtype = p.thr_dtype = F32
    p.update_memory = 2
    return p


def begin(L, p="default", grad_dtype=BF16, grad=PTR, mmt=PTR, vec=PTR, start=3, stride=100, ws=None, ws_bytes=0):
    p = params() if p == "default" else p
    return L.dgc_compress_begin_g16(grad, grad_dtype, mmt, vec, 0.9, 1, start, stride,
                                    ctypes.byref(p) if p is not None else None, None, ws, ws_bytes, None)


def test_exported_declared_and_bound(L):
    from dgc import _lib
    assert hasattr(L, NAME)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m, "include/dgc_hip.h does not declare " + NAME
    # grad, grad_dtype, mmt, vec, momentum, nesterov, start, stride, params, spec, ws, ws_bytes, stream
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[NAME][1]) == 13


def test_header_comment_cites_the_reference():
    text = open(os.path.join(REPO, "include", "dgc_hip.h")).read()
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "dgc/memory.py:50-63" in comment and "dgc/compression.py:113-121" in comment


@pytest.mark.parametrize("what, kwargs, status, message", [
    ("fp32 gradient", dict(grad_dtype=F32), DTYPE, b"grad_dtype"),
    ("unknown gradient dtype", dict(grad_dtype=3), DTYPE, b"grad_dtype"),
    ("negative gradient dtype", dict(grad_dtype=-1), DTYPE, b"grad_dtype"),
    ("bad dtype wins over a null pointer", dict(grad_dtype=F32, grad=None), DTYPE, b"grad_dtype"),
    ("null grad", dict(grad=None), INVALID, b"null"),
    ("null mmt", dict(mmt=None), INVALID, b"null"),
    ("null vec", dict(vec=None), INVALID, b"null"),
    ("null params", dict(p=None), INVALID, b"null"),
    ("grad 2-B aligned", dict(grad=ctypes.c_void_p(4098)), INVALID, b"8-B aligned"),
    ("grad 4-B aligned", dict(grad=ctypes.c_void_p(4100)), INVALID, b"8-B aligned"),
    ("mmt 8-B aligned", dict(mmt=ctypes.c_void_p(4104)), INVALID, b"16-B aligned"),
    ("vec 4-B aligned", dict(vec=ctypes.c_void_p(4100)), INVALID, b"16-B aligned"),
    ("stride 2", dict(stride=2, start=1), INVALID, b"stride"),
    ("stride 3", dict(stride=3), INVALID, b"stride"),
    ("stride 2^30", dict(stride=1 << 30), INVALID, b"stride"),
    ("start = stride", dict(start=100), INVALID, b"sample_start"),
    ("start < 0", dict(start=-1), INVALID, b"sample_start"),
])
def test_refuses_before_any_launch(L, what, kwargs, status, message):
    rc = begin(L, **kwargs)
    err = L.dgc_last_error()
    assert rc == status, (what, rc, err)
    assert message in err and b"dgc_compress" in err, (what, err)


def test_accepts_an_8_byte_aligned_gradient_and_both_dtypes(L):
    """Everything above passed: the next refusal is the missing workspace (still no launch).
    The gradient needs 8-B alignment only, the unsampled tensor no stride."""
    for dt in (BF16, F16):
        rc = begin(L, grad_dtype=dt, grad=ctypes.c_void_p(4104))
        assert rc == WORKSPACE, (dt, rc, L.dgc_last_error())
        assert b"workspace" in L.dgc_last_error()
    for stride in (4, (1 << 30) - 1):
        assert begin(L, stride=stride) == WORKSPACE, (stride, L.dgc_last_error())
    assert begin(L, p=params(5000, 5000), stride=1, start=0) == WORKSPACE, L.dgc_last_error()
    # a short or misaligned workspace
    assert begin(L, ws=PTR, ws_bytes=256) == WORKSPACE
    need = L.dgc_compress_workspace(100000, 100, 1000)
    assert begin(L, ws=ctypes.c_void_p(4096 + 128), ws_bytes=need) == WORKSPACE


def test_replay_width_is_compress_checks(L):
    """What dgc_compress_begin refuses is refused here: a resample whose candidates do not fit K5's width."""
    p = params(1 << 40, 1 << 30)
    p.num_selects = 1 << 33
    rc = begin(L, p=p, stride=1 << 10)
    assert rc == 3 and b"resample replay" in L.dgc_last_error(), (rc, L.dgc_last_error())


def test_algorithmic_bytes_gradient_size():
    from dgc.bucket import algorithmic_bytes
    N, k, S, W = 10 ** 9, 10 ** 6, 10 ** 7, 8
    rest = 4 * S + 8 * k + (1 + W) * k * 12 + 8 * W * k
    assert algorithmic_bytes(N, k, S, W) == 28 * N + rest == algorithmic_bytes(N, k, S, W, gbytes=4)
    assert algorithmic_bytes(N, k, S, W, gbytes=2) == 26 * N + rest   # K1 18N
    assert algorithmic_bytes(N, k, S, W, vbytes=2, sbytes=2) == 20 * N + 4 * S + 4 * k + (1 + W) * k * 10 + 4 * W * k
