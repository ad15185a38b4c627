"""dgc_apply_packed_multi / dgc_apply_packed_multi_workspace (the sparse DGCSGD step of a
batch's tensors): exported, declared, the row mirrored by ``_lib``, and every argument check
answers before anything is launched. No GPU needed."""
import ctypes
import os
import re

import pytest

from conftest import REPO

INVALID, DTYPE, WORKSPACE = 1, 2, 5
F32, F16 = 0, 1
I64, I32 = 0, 1
PTR = ctypes.c_void_p(4096)   # non-null, 256-B aligned; never dereferenced on these paths
WORLD, CAP, N, T = 4, 1000, 100_000, 5
NAME = b"dgc_apply_packed_multi"


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


def hypers(*sets):
    """(lr, momentum, dampening, weight_decay, nesterov) per group as a dgc_apply_hyper array."""
    from dgc import _lib
    return (_lib.ApplyHyper * len(sets))(*[_lib.ApplyHyper(*s) for s in sets])


WD0 = (0.1, 0.0, 0.0, 0.0, 0)
WD = (0.1, 0.9, 0.0, 1e-4, 1)
DEFAULT = object()


def apply(L, payload=PTR, world=WORLD, stride=None, cap=CAP, vd=F32, idt=I64, acc=PTR, n=N, table=PTR, count=T,
          dense_blocks=0, hs=DEFAULT, groups=None, ws=None, ws_bytes=0):
    if stride is None:
        stride = L.dgc_payload_layout(cap, vd if vd in (F32, F16) else F32, idt if idt in (I64, I32) else I64, None,
                                      None)
    if hs is DEFAULT:
        hs = hypers(WD0)
    groups = (len(hs) if hs is not None else 1) if groups is None else groups
    return L.dgc_apply_packed_multi(payload, world, stride, cap, vd, idt, acc, n, table, count, dense_blocks, hs,
                                    groups, ws, ws_bytes, None)


def test_exported_and_declared(L):
    from dgc import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)
    assert hasattr(L, "dgc_apply_packed_multi") and hasattr(L, "dgc_apply_packed_multi_workspace")
    m = re.search(r"\bint\s+dgc_apply_packed_multi\s*\(([^;]*)\)\s*;", text)
    assert m, "include/dgc_hip.h does not declare dgc_apply_packed_multi"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["dgc_apply_packed_multi"][1]) == 16
    m = re.search(r"\bsize_t\s+dgc_apply_packed_multi_workspace\s*\(([^;]*)\)\s*;", text)
    assert m, "include/dgc_hip.h does not declare dgc_apply_packed_multi_workspace"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["dgc_apply_packed_multi_workspace"][1]) == 2


def test_row_and_hyper_mirror_the_header():
    """_lib.ApplyRow / ApplyHyper list the header's fields in the header's order, and the row
    is the 48 bytes the library asserts."""
    from dgc import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)
    for struct, mirror in (("dgc_apply_row", _lib.ApplyRow), ("dgc_apply_hyper", _lib.ApplyHyper)):
        m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), text, flags=re.S)
        assert m, struct
        names = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if decl:   # "float lr, momentum" declares two
                first, *rest = decl.split(",")
                names += [re.findall(r"\w+", first)[-1]] + [re.findall(r"\w+", r)[-1] for r in rest]
        assert names == [f[0] for f in mirror._fields_], (struct, names)
    assert ctypes.sizeof(_lib.ApplyRow) == 48 and ctypes.sizeof(_lib.ApplyHyper) == 20


def test_workspace_grows_with_the_gathered_slots(L):
    ws = L.dgc_apply_packed_multi_workspace
    assert ws(8, 1000) >= 8 * 1000 * 4 and ws(8, 1000) % 256 == 0
    assert ws(1, 7) >= 28 and ws(1, 7) % 256 == 0
    assert ws(8, 1000) > ws(4, 1000) > ws(4, 500) > ws(1, 7)
    assert ws(16, 1 << 20) >= 16 * (1 << 20) * 4 and ws(16, 1 << 20) % 256 == 0


@pytest.mark.parametrize("what, kwargs, code", [
    ("null payload", dict(payload=None), INVALID),
    ("null acc", dict(acc=None), INVALID),
    ("null table", dict(table=None), INVALID),
    ("null hypers", dict(hs=None), INVALID),
    ("world 0", dict(world=0), INVALID),
    ("world 65", dict(world=65), INVALID),
    ("world -1", dict(world=-1), INVALID),
    ("bad idtype", dict(idt=7), DTYPE),
    ("bad vdtype", dict(vd=9), DTYPE),
    ("bf16 values", dict(vd=2), DTYPE),
    ("rank_stride below the layout", dict(stride=256), INVALID),
    ("no tensor", dict(count=0), INVALID),
    ("flat_numel 0", dict(n=0), INVALID),
    ("nine groups", dict(hs=hypers(*[WD0] * 9)), INVALID),
    ("no group", dict(groups=0), INVALID),
    ("negative lr", dict(hs=hypers((-0.1, 0.0, 0.0, 0.0, 0))), INVALID),
    ("NaN lr", dict(hs=hypers((float("nan"), 0.0, 0.0, 0.0, 0))), INVALID),
    ("negative lr in the second group", dict(hs=hypers(WD0, (-1.0, 0.9, 0.0, 1e-4, 0)), ws=PTR, ws_bytes=1 << 20),
     INVALID),
    ("negative dense_blocks", dict(dense_blocks=-1), INVALID),
    ("dense_blocks 2^31", dict(dense_blocks=1 << 31), INVALID),
    ("null ws with weight decay", dict(hs=hypers(WD), ws=None, ws_bytes=1 << 20), WORKSPACE),
    ("small ws with weight decay", dict(hs=hypers(WD), ws=PTR, ws_bytes=WORLD * CAP * 4 - 1), WORKSPACE),
    ("small ws, weight decay in the second group", dict(hs=hypers(WD0, WD), ws=PTR, ws_bytes=16), WORKSPACE),
    ("misaligned ws", dict(hs=hypers(WD), ws=ctypes.c_void_p(4096 + 4), ws_bytes=1 << 20), WORKSPACE),
])
def test_refuses_before_any_launch(L, what, kwargs, code):
    rc = apply(L, **kwargs)
    err = L.dgc_last_error()
    assert rc == code, (what, rc, err)
    assert NAME in err, (what, err)


def test_the_layout_stride_is_the_smallest_accepted(L):
    """One byte below dgc_payload_layout's stride is refused for every wire format; the
    layout's own stride — and a larger one, the batched step's dense tail — passes that check
    and meets the next one (the missing workspace), still before any launch."""
    for vd, idt in ((F32, I64), (F16, I32), (F32, I32), (F16, I64)):
        s = L.dgc_payload_layout(CAP, vd, idt, None, None)
        rc = apply(L, vd=vd, idt=idt, stride=s - 1)
        assert rc == INVALID and b"rank_stride" in L.dgc_last_error(), (vd, idt, L.dgc_last_error())
        for stride in (s, s + 4096):
            rc = apply(L, vd=vd, idt=idt, stride=stride, hs=hypers(WD))
            assert rc == WORKSPACE, (vd, idt, rc, L.dgc_last_error())
