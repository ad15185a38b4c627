"""dgc_apply_packed / dgc_apply_packed_workspace (the sparse DGCSGD step of the flat bucket):
exported, declared, and every argument check answers before anything is launched. No GPU
needed."""
import ctypes
import os
import re

import pytest

from conftest import REPO

INVALID, DTYPE, WORKSPACE = 1, 2, 5
F32, F16 = 0, 1
I64, I32 = 0, 1
PTR = ctypes.c_void_p(4096)   # non-null, 256-B aligned; never dereferenced on these paths
WORLD, CAP, N = 4, 1000, 100_000


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


def layout(L, cap=CAP, vd=F32, idt=I64):
    return L.dgc_payload_layout(cap, vd, idt, None, None)


def apply(L, payload=PTR, world=WORLD, stride=None, cap=CAP, vd=F32, idt=I64, acc=PTR, param=PTR, buf=PTR, first=0,
          n=N, lr=0.1, mom=0.0, damp=0.0, wd=0.0, nesterov=0, ws=None, ws_bytes=0):
    stride = layout(L, cap, vd if vd in (F32, F16) else F32, idt if idt in (I64, I32) else I64) if stride is None \
        else stride
    return L.dgc_apply_packed(payload, world, stride, cap, vd, idt, acc, param, buf, first, n, lr, mom, damp, wd,
                              nesterov, ws, ws_bytes, None)


def test_codes_match_the_header():
    text = open(os.path.join(REPO, "include", "dgc_hip.h")).read()
    for name, value in (("DGC_ERR_INVALID", INVALID), ("DGC_ERR_DTYPE", DTYPE), ("DGC_ERR_WORKSPACE", WORKSPACE)):
        m = re.search(rf"\b{name}\s*=?\s*(-?\d+)", text)
        assert m and int(m.group(1)) == value, name


def test_exported_and_declared(L):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)
    assert hasattr(L, "dgc_apply_packed") and hasattr(L, "dgc_apply_packed_workspace")
    m = re.search(r"\bint\s+dgc_apply_packed\s*\(([^;]*)\)\s*;", text)
    assert m, "include/dgc_hip.h does not declare dgc_apply_packed"
    # payload, world, rank_stride, capacity, vdtype, idtype, acc, param, buf, first, n, lr, momentum, dampening,
    # weight_decay, nesterov, ws, ws_bytes, stream
    assert len(m.group(1).split(",")) == 19
    m = re.search(r"\bsize_t\s+dgc_apply_packed_workspace\s*\(([^;]*)\)\s*;", text)
    assert m and len(m.group(1).split(",")) == 2, "include/dgc_hip.h does not declare dgc_apply_packed_workspace"
    from dgc import _lib
    assert len(_lib._SIGNATURES["dgc_apply_packed"][1]) == 19
    assert len(_lib._SIGNATURES["dgc_apply_packed_workspace"][1]) == 2


def test_workspace_holds_a_word_per_gathered_slot(L):
    assert L.dgc_apply_packed_workspace(8, 1000) >= 8 * 1000 * 4
    assert L.dgc_apply_packed_workspace(8, 1000) % 256 == 0
    assert L.dgc_apply_packed_workspace(1, 7) % 256 == 0 and L.dgc_apply_packed_workspace(1, 7) >= 28


@pytest.mark.parametrize("what, kwargs, code", [
    ("null payload", dict(payload=None), INVALID),
    ("null acc", dict(acc=None), INVALID),
    ("null param", dict(param=None), INVALID),
    ("world 0", dict(world=0), INVALID),
    ("world -1", dict(world=-1), INVALID),
    ("bad idtype", dict(idt=7), DTYPE),
    ("bad vdtype", dict(vd=9), DTYPE),
    ("rank_stride below the layout", dict(stride=256), INVALID),
    ("negative lr", dict(lr=-0.1), INVALID),
    ("null buf with weight decay and momentum", dict(buf=None, wd=1e-4, mom=0.9, ws=PTR, ws_bytes=1 << 20), INVALID),
    ("null ws with weight decay", dict(wd=1e-4, ws=None, ws_bytes=1 << 20), WORKSPACE),
    ("small ws with weight decay", dict(wd=1e-4, ws=PTR, ws_bytes=WORLD * CAP * 4 - 1), WORKSPACE),
    ("small ws with weight decay and momentum", dict(wd=1e-4, mom=0.9, ws=PTR, ws_bytes=16), WORKSPACE),
])
def test_refuses_before_any_launch(L, what, kwargs, code):
    rc = apply(L, **kwargs)
    err = L.dgc_last_error()
    assert rc == code, (what, rc, err)
    assert b"dgc_apply_packed" in err, (what, err)


def test_the_layout_stride_is_the_smallest_accepted(L):
    """One byte below dgc_payload_layout's stride is refused for every wire format (the
    refusal names both strides); the layout's own stride passes that check and meets the
    next one (the missing workspace), still before any launch."""
    for vd, idt in ((F32, I64), (F16, I32), (F32, I32), (F16, I64)):
        s = layout(L, CAP, vd, idt)
        rc = apply(L, vd=vd, idt=idt, stride=s - 1)
        assert rc == INVALID and b"rank_stride" in L.dgc_last_error(), (vd, idt, L.dgc_last_error())
        rc = apply(L, vd=vd, idt=idt, stride=s, wd=1e-4)
        assert rc == WORKSPACE, (vd, idt, rc, L.dgc_last_error())
