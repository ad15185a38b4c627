"""The 16-bit split exchange's C ABI (dgc_decompress_split16_workspace, dgc_scatter_split16,
dgc_fill_zero16): declared, exported, bound, and every refusal answers with its status and a
message before anything is launched. No GPU needed."""
import ctypes
import os
import re

import pytest

from conftest import REPO

OK, INVALID, DTYPE, WORKSPACE = 0, 1, 2, 5
F32, F16, BF16 = 0, 1, 2
I64, I32 = 0, 1
PTR = ctypes.c_void_p(4096)   # non-null, 256-B aligned; never dereferenced on these paths
N, W, PARTS, CAP = 100_000, 4, 2, 100


@pytest.fixture(scope="module")
def L():
    from dgc import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    return _lib.lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dgc_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name, ret, nargs", [
    ("dgc_decompress_split16_workspace", "size_t", 4),
    ("dgc_scatter_split16", "int", 14),
    ("dgc_fill_zero16", "int", 3),
])
def test_declared_exported_and_bound(L, name, ret, nargs):
    from dgc import _lib
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), header())
    assert m, f"include/dgc_hip.h does not declare {name}"
    assert len(m.group(1).split(",")) == nargs
    assert hasattr(L, name)
    assert len(_lib._SIGNATURES[name][1]) == nargs


def test_declarations_cite_the_reference():
    """Each declaration carries a comment with the reference's lines, as the others do."""
    text = open(os.path.join(REPO, "include", "dgc_hip.h")).read()
    for name in ("dgc_decompress_split16_workspace", "dgc_scatter_split16", "dgc_fill_zero16"):
        decl = re.search(r"\n[a-z_0-9]+\s+%s\s*\(" % name, text).start()
        comment = text[text.rfind("/*", 0, decl): decl]
        assert comment.rstrip().endswith("*/"), name        # the comment sits right above the declaration
        assert re.search(r"dgc/compression\.py:\d+", comment), name


def test_workspace_size(L):
    wsz = L.dgc_decompress_split16_workspace(N, W, PARTS, CAP)
    assert wsz > 0 and wsz % 256 == 0
    assert wsz == L.dgc_decompress_split_workspace(N, W, PARTS, CAP)   # one layout
    assert L.dgc_decompress_split16_workspace(N, 8, 8, CAP) > 0        # 64 runs: the most
    assert L.dgc_decompress_split16_workspace(N, 16, 8, CAP) == 0      # 128 runs > 64
    assert L.dgc_decompress_split16_workspace(N, 9, 8, CAP) == 0
    assert L.dgc_decompress_split16_workspace(N, 2, 9, CAP) == 0


def scatter(L, gathered=PTR, world=W, parts=PARTS, part=0, cap=CAP, vd=BF16, idt=I64, grad=PTR, dtype=BF16, n=N,
            ws=PTR, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.dgc_decompress_split16_workspace(n, min(world, 8), min(max(parts, 1), 8), cap) or (1 << 20)
    return L.dgc_scatter_split16(gathered, world, parts, part, cap, vd, idt, grad, dtype, n, 0.25, ws, ws_bytes, None)


@pytest.mark.parametrize("what, kwargs, status, message", [
    ("null gathered", dict(gathered=None), INVALID, b"null"),
    ("null grad", dict(grad=None), INVALID, b"null"),
    ("odd grad address", dict(grad=ctypes.c_void_p(4097)), INVALID, b"2-B aligned"),
    ("parts = 1", dict(parts=1), INVALID, b"parts outside 2..8"),
    ("parts = 0", dict(parts=0), INVALID, b"parts outside 2..8"),
    ("parts = 9", dict(parts=9, world=2), INVALID, b"parts outside 2..8"),
    ("world * parts = 72", dict(world=9, parts=8), INVALID, b"world * parts > 64"),
    ("part = parts", dict(part=PARTS), INVALID, b"part 2 outside 0..1"),
    ("part < 0", dict(part=-1), INVALID, b"part -1 outside 0..1"),
    ("n = 0", dict(n=0), INVALID, b"n < 1"),
    ("fp32 gradient", dict(dtype=F32), DTYPE, b"grad dtype"),
    ("unknown gradient dtype", dict(dtype=3), DTYPE, b"grad dtype"),
    ("unknown wire dtype", dict(vd=3), DTYPE, b"dtype"),
    ("unknown index dtype", dict(idt=2), DTYPE, b"dtype"),
    ("null workspace", dict(ws=None), WORKSPACE, b"workspace"),
    ("unaligned workspace", dict(ws=ctypes.c_void_p(4096 + 16)), WORKSPACE, b"workspace"),
    ("workspace one byte short", dict(ws_bytes=-1), WORKSPACE, b"workspace"),
])
def test_scatter_refuses_before_any_launch(L, what, kwargs, status, message):
    if kwargs.get("ws_bytes") == -1:
        kwargs = dict(kwargs, ws_bytes=L.dgc_decompress_split16_workspace(N, W, PARTS, CAP) - 1)
    rc = scatter(L, **kwargs)
    err = L.dgc_last_error()
    assert rc == status, (what, rc, err)
    assert message in err, (what, err)
    if status != WORKSPACE:   # (the workspace check is the decompress family's shared one)
        assert b"dgc_scatter_split16" in err, (what, err)


@pytest.mark.parametrize("vd", [F32, F16, BF16])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("idt", [I64, I32])
def test_every_dtype_combination_reaches_the_workspace_check(L, vd, dtype, idt):
    """All three wire dtypes onto both gradient dtypes pass the argument checks: the next
    refusal is the missing workspace (still no launch)."""
    rc = scatter(L, vd=vd, dtype=dtype, idt=idt, ws=None)
    assert rc == WORKSPACE, (rc, L.dgc_last_error())


def test_fp32_split_still_refuses_a_bf16_wire(L):
    rc = L.dgc_scatter_split(PTR, W, PARTS, 0, CAP, BF16, I64, PTR, N, 0.25, 0, PTR, 1 << 20, None)
    assert rc == DTYPE, (rc, L.dgc_last_error())


@pytest.mark.parametrize("what, args, message", [
    ("null buffer", (None, 10), b"null"),
    ("n < 0", (PTR, -1), b"n < 0"),
    ("odd address", (ctypes.c_void_p(4097), 10), b"2-B aligned"),
])
def test_fill_zero16_refuses_before_any_launch(L, what, args, message):
    rc = L.dgc_fill_zero16(*args, None)
    err = L.dgc_last_error()
    assert rc == INVALID and b"dgc_fill_zero16" in err and message in err, (what, rc, err)


def test_fill_zero16_of_nothing_is_a_no_op(L):
    assert L.dgc_fill_zero16(PTR, 0, None) == OK
