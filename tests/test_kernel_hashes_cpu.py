"""tools/kernel_hashes.py on a hand-written assembly text (no compiler, no GPU): a function's
hash does not depend on its own name, does depend on every instruction and on every line of its
kernel descriptor, and --diff reports a function that only changed its name as renamed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_hashes  # noqa: E402

FUNC = """\
\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_mov_b32 s4, 0
\tv_mov_b32_e32 v1, 0
.LBB{no}_1:                               ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v1, {inc}, v1
\ts_add_u32 s4, s4, 1
\ts_cmp_lt_u32 s4, 8
\ts_cbranch_scc1 .LBB{no}_1
; %bb.2:
\tv_mul_f32_e32 v0, v0, v1
\ts_endpgm
.Lfunc_end{no}:
\t.size\t{name}, .Lfunc_end{no}-{name}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
"""


def asm(*funcs):
    """One translation unit: (name, emission-order number, increment, vgprs) per function."""
    return "\t.text\n" + "".join(FUNC.format(name=n, no=no, inc=inc, vgpr=vg) for n, no, inc, vg in funcs)


OLD, NEW, OTHER = "_Z6kernelILi0EEvPf", "_Z6kernelILi0ELi0EEvPf", "_Z5otherv"


def test_hash_ignores_the_functions_own_name():
    a = kernel_hashes.functions(asm((OLD, 0, 1, 2), (OTHER, 1, 1, 2)))
    b = kernel_hashes.functions(asm((OTHER, 0, 1, 2), (NEW, 1, 1, 2)))   # renamed, and emitted in another order
    assert set(a) == {OLD, OTHER} and set(b) == {NEW, OTHER}
    assert a[OLD] == b[NEW] == a[OTHER] == b[OTHER]


@pytest.mark.parametrize("inc, vgpr", [(2, 2), (1, 3)], ids=["instruction", "amdhsa line"])
def test_hash_sees_a_changed_instruction_and_a_changed_descriptor(inc, vgpr):
    a = kernel_hashes.functions(asm((OLD, 0, 1, 2)))
    b = kernel_hashes.functions(asm((OLD, 0, inc, vgpr)))
    assert a[OLD] != b[OLD]


def listing(path, text):
    rows = sorted("unit.hip  %s  %s" % kv for kv in kernel_hashes.functions(text).items())
    path.write_text("\n".join(rows) + "\n")
    return str(path)


def test_diff_reports_renamed_and_exits_1(tmp_path, capsys, monkeypatch):
    old = listing(tmp_path / "old.txt", asm((OLD, 0, 1, 2), (OTHER, 1, 1, 2), ("_Z4gonev", 2, 3, 2)))
    new = listing(tmp_path / "new.txt", asm((NEW, 0, 1, 2), (OTHER, 1, 2, 2), ("_Z4camev", 2, 4, 2)))
    monkeypatch.setattr(sys, "argv", ["kernel_hashes.py", "--diff", old, new])
    assert kernel_hashes.main() == 1
    out = capsys.readouterr().out.splitlines()
    assert out == ["removed  unit.hip  _Z4gonev", "added    unit.hip  _Z4camev", "changed  unit.hip  " + OTHER,
                   "renamed  unit.hip  %s -> %s" % (OLD, NEW)]
    # a rename alone is still a difference; two equal listings are none
    only = listing(tmp_path / "only.txt", asm((NEW, 0, 1, 2), (OTHER, 1, 1, 2), ("_Z4gonev", 2, 3, 2)))
    assert kernel_hashes.diff(old, only) == 1
    assert capsys.readouterr().out.splitlines() == ["renamed  unit.hip  %s -> %s" % (OLD, NEW)]
    assert kernel_hashes.diff(old, old) == 0


def test_diff_pairs_equal_hashes_in_sorted_order(tmp_path, capsys):
    old = listing(tmp_path / "old.txt", asm(("_Z1bv", 0, 1, 2), ("_Z1av", 1, 1, 2)))
    new = listing(tmp_path / "new.txt", asm(("_Z1yv", 0, 1, 2), ("_Z1xv", 1, 1, 2)))
    assert kernel_hashes.diff(old, new) == 1
    assert capsys.readouterr().out.splitlines() == ["renamed  unit.hip  _Z1av -> _Z1xv", "renamed  unit.hip  _Z1bv -> _Z1yv"]
