#!/usr/bin/env python3
"""What the compiler made of K1 (k_compensate_list), of K1-16 (k_compensate_list16), of K1-mixed
(k_compensate_list with a 16-bit GD: fp32 state, 16-bit gradient) and of the plain compensate kernels.

Host only, no GPU: compiles a .hip file of adam-compression_amd/csrc to gfx950 assembly
with the Makefile's flags (read from the Makefile) and prints, per kernel instantiation,

  vgpr / occ / scratch   registers, waves per SIMD, scratch bytes (the compiler's own figures)
  launched               waves per SIMD a flat bucket's launch really holds: select.hip asks for
                         kK1FlatLds bytes of unused LDS per workgroup (one wave per SIMD each) of
                         a CU's 160 KB, past the write-through size (48M elements): printed as
                         `past it / up to it`; every other launch holds `occ`
  flat                   flat_ loads in the kernel's text (a load whose address space the
                         compiler could not prove)
  walks                  the walks through the kernel that the figures below range over (+: cut off)
  stream                 non-temporal streaming loads on a walk, a wave's 12: 16-B ones in K1,
                         8-B ones in K1-16, eight 16-B and four 8-B ones in K1-mixed
  before-vm-wait         how many of them are issued before the first wait on the vector
                         memory counter that waits for one of them
  waits-before / mem     waits in front of the first streaming load / those of them that
                         wait for a read of memory other than the kernel arguments
  mem-to-last            such memory-dependent waits in front of the LAST streaming load

A walk takes every lane as active (a branch on an empty exec mask is not taken, so the
one-thread sections are walked too) and goes both ways at every forward branch on a scalar
condition, once through every loop, up to the wave's twelfth streaming load; a figure that
differs between the walks prints as min-max. It is a reading of the compiler's output, not
a measurement, and it rests on heuristics that fit today's assembly. What would miscount
without a warning:
  - a streaming load is any (global|flat)_load_dwordx4 whose operands include `nt`; another
    16-B non-temporal load in the kernel (none today) would be counted as one, and a
    streaming load the compiler emitted without `nt`, or split into narrower loads, would not;
  - K1-16's streaming load is any (global|flat)_load_dwordx2 with `nt`. The 8-B form is also
    what a plain 64-bit read compiles to (a pointer, an int64 table entry): one that carried
    `nt` would be counted, and two streaming loads of a lane that the compiler merged into one
    dwordx4 would not. The gradient's partial last group (ld_tail16) is 2-B loads without
    `nt`, so counts as `mem`, never as a streaming load. K1-mixed counts both widths;
  - a vmcnt wait that finds nothing outstanding on the walk is taken for the wait of a loop
    whose load stands below it in the text (task_first's search) and counted as
    memory-dependent; a redundant wait would be counted the same way;
  - a scalar load counts as a kernel-argument read only while its base is s[0:1] or a copy
    made by s_add / s_addc / s_mov that the walk saw; a base computed any other way (a
    dynamic index into an argument array) counts as memory;
  - loads and stores retire in issue order on their counter (true of gfx9 vector memory;
    scalar loads are only ever waited for with lgkmcnt(0) here).

  tools/k1_isa.py                      # K1's twelve instantiations, K1-16's twelve and K1-mixed's four, as a markdown table
  tools/k1_isa.py --compensate         # k_compensate4 / k_compensate_mt (compensate.hip)
  tools/k1_isa.py --asm FILE.s         # read an assembly file instead of compiling
  tools/k1_isa.py --trace 'ILb1ELb1ELi0E'   # the memory operations and waits of one kernel
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

kSegLoads = 12   # a wave's streaming loads (three arrays x kSegTiles)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adam-compression_amd", "csrc")


def makefile_vars(csrc=CSRC):
    """The variables of csrc/Makefile as written (continuation lines joined)."""
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    return dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M))


def makefile_flags(csrc=CSRC):
    """CXXFLAGS of csrc/Makefile with its variables filled in (ARCH default, no EXTRA)."""
    var = makefile_vars(csrc)
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"].strip()).replace("$(EXTRA)", "")
    return var["HIPCC"].strip(), flags.split()


def compile_asm(src, csrc=CSRC):
    hipcc, flags = makefile_flags(csrc)
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
    out.close()
    cmd = [hipcc] + flags + ["-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", out.name]
    subprocess.run(cmd, cwd=csrc, check=True)
    text = open(out.name).read()
    os.unlink(out.name)
    return text


def kernels(text, name_re):
    """(mangled name, body lines, trailer comment lines) of every matching function."""
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m and re.search(name_re, m.group(1)):
            j = i + 1
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            k = j
            while k < len(lines) and not re.match(r"^; Occupancy:", lines[k]):
                k += 1
            yield m.group(1), lines[i + 1:j], lines[j:k + 1]
            i = k
        i += 1


def trailer(tr, key):
    for ln in tr:
        m = re.match(r"^; %s: (\d+)" % key, ln)
        if m:
            return int(m.group(1))
    return -1


def regs(op):
    """SGPR numbers named by an operand such as s3 or s[4:7]."""
    m = re.match(r"^s\[(\d+):(\d+)\]$", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^s(\d+)$", op)
    return {int(m.group(1))} if m else set()


class Path:
    """One walk through a kernel: what is outstanding, and what it has counted."""

    def __init__(self, stream_op="dwordx4"):
        self.stream_op = stream_op   # the width of the kernel's streaming load
        self.pc = 0
        self.karg = {0, 1}     # SGPRs that hold the kernel-argument pointer or an offset copy of it
        self.vm = []           # outstanding vector memory operations, oldest first: 'mem' | 'stream' | 'store'
        self.lgkm = []         # outstanding scalar (and flat) loads: 'arg' | 'mem'
        self.stream = 0
        self.before_vm_wait = None
        self.waits_before = self.mem_before = 0
        self.mem_to_last = self.mem_pending = 0
        self.log = []
        self.looped = set()

    def fork(self):
        q = Path()
        q.__dict__.update({k: (v.copy() if isinstance(v, (set, list)) else v) for k, v in self.__dict__.items()})
        return q

    def key(self):
        return (self.pc, tuple(self.vm), tuple(self.lgkm), frozenset(self.karg), self.stream, self.before_vm_wait,
                self.waits_before, self.mem_before, self.mem_to_last, self.mem_pending)

    def step(self, ins, op, args):
        if op.startswith("s_load_"):
            base = regs(args[1])
            kind = "arg" if base and base <= self.karg else "mem"
            self.lgkm.append(kind)
            self.karg -= regs(args[0])
            self.log.append("%-6s %s" % (kind, ins))
        elif re.match(r"^(global|flat|buffer|scratch)_load", op):
            if op.startswith("flat_"):
                self.lgkm.append("mem")
            if re.match(r"^(global|flat)_load_%s$" % self.stream_op, op) and "nt" in args:
                self.stream += 1
                self.mem_to_last += self.mem_pending
                self.mem_pending = 0
                self.vm.append("stream")
                self.log.append("stream %s" % ins)
            else:
                self.vm.append("mem")
                self.log.append("mem    %s" % ins)
        elif re.match(r"^(global|flat|buffer|scratch)_(store|atomic)", op):
            self.vm.append("store")
        elif op == "s_waitcnt":
            dep = False
            m = re.search(r"vmcnt\((\d+)\)", ins)
            if m:
                keep = int(m.group(1))
                gone = self.vm[:len(self.vm) - keep] if keep < len(self.vm) else []
                # nothing outstanding on this walk: the wait of a loop whose load stands below it
                if any(g != "store" for g in gone) or not self.vm:
                    dep = True
                if keep < len(self.vm):
                    self.vm = self.vm[len(self.vm) - keep:]
                if "stream" in gone and self.before_vm_wait is None:
                    self.before_vm_wait = self.stream
            m = re.search(r"lgkmcnt\((\d+)\)", ins)
            if m:
                keep = int(m.group(1))
                gone = self.lgkm[:len(self.lgkm) - keep] if keep < len(self.lgkm) else []
                if keep < len(self.lgkm):
                    self.lgkm = self.lgkm[len(self.lgkm) - keep:]
                if any(g == "mem" for g in gone):
                    dep = True
            if self.stream == 0:
                self.waits_before += 1
                self.mem_before += dep
            self.mem_pending += dep
            self.log.append("%-6s %s" % ("WAIT*" if dep else "wait", ins))
        else:
            # address arithmetic on the kernel-argument pointer keeps it one; any other write ends it
            dst = regs(args[0]) if args else set()
            src_karg = len(args) > 1 and regs(args[1]) and regs(args[1]) <= self.karg
            if op in ("s_add_u32", "s_addc_u32", "s_mov_b64", "s_mov_b32") and src_karg:
                self.karg |= dst
            elif not op.startswith(("s_cmp", "s_nop", "v_cmp")) and not (dst & {0, 1}):
                self.karg -= dst


def scan(body, nstream=None, max_paths=20000, stream_op="dwordx4"):
    """Every walk through the kernel up to its nstream-th streaming load (None: to its end).

    All lanes are taken as active: a branch on an empty exec mask is not taken, one on a
    non-empty mask is. A branch on a scalar condition is walked both ways, except backwards
    (a loop is walked once). Returns the finished walks and whether the search was cut off.
    """
    prog, label = [], {}
    for ln in body:
        ins = ln.split(";")[0].strip()
        m = re.match(r"^(\.\w+):", ins)
        if m:
            label[m.group(1)] = len(prog)
        elif ins and not ins.startswith("."):
            prog.append(ins)
    done, todo, seen = [], [Path(stream_op)], set()
    while todo and len(done) + len(todo) < max_paths:
        p = todo.pop()
        while True:
            if p.pc >= len(prog):
                break
            if nstream and p.stream >= nstream:
                done.append(p)
                break
            ins = prog[p.pc]
            parts = ins.replace(",", " ").split()
            op, args = parts[0], parts[1:]
            p.pc += 1
            if op == "s_endpgm":
                if not nstream:
                    done.append(p)
                break
            if op.startswith(("s_branch", "s_cbranch")):
                tgt = label.get(args[0])
                if tgt is None or op == "s_cbranch_execz":
                    continue
                if op in ("s_branch", "s_cbranch_execnz"):
                    if tgt < p.pc:
                        if p.pc in p.looped:
                            continue
                        p.looped.add(p.pc)
                    p.pc = tgt
                    continue
                if tgt < p.pc:      # a loop's back edge on a scalar condition: fall out of it
                    continue
                q = p.fork()
                q.pc = tgt
                if q.key() not in seen:
                    seen.add(q.key())
                    todo.append(q)
                continue
            p.step(ins, op, args)
    return done, bool(todo)


CU_LDS = 160 << 10   # bytes of LDS per CU (gfx950)


def flat_launch_waves():
    """Waves per SIMD that kK1FlatLds (select.hip) leaves a one-tensor launch; None: no limit found."""
    m = re.search(r"kK1FlatLds\s*=\s*(\d+)u?\s*<<\s*(\d+)", open(os.path.join(CSRC, "select.hip")).read())
    return CU_LDS // (int(m.group(1)) << int(m.group(2))) if m else None


# K1-mixed: k_compensate_list<NEST, true, DGC_CLIP_NONE, GD> with GD = DGC_BF16 (1) or DGC_F16 (2)
MIXED = r"k_compensate_listILb(\d)ELb1ELi0ELi([12])E"


def pretty(name):
    m = re.search(MIXED, name)
    if m:
        return "K1-mixed GD=%s NEST=%s" % (m.group(2), m.group(1))
    m = re.search(r"k_compensate_listILb(\d)ELb(\d)ELi(\d)E", name)
    if m:
        return "K1 NEST=%s ONE=%s CLIP=%s" % m.groups()
    m = re.search(r"k_compensate_list16ILi(\d)ELb(\d)ELi(\d)E", name)
    if m:
        return "K1-16 DT=%s NEST=%s CLIP=%s" % m.groups()
    m = re.search(r"\d+(k_compensate\w*?)I(\w+?)EEv", name)
    return "%s<%s>" % m.groups() if m else name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="an assembly file to read instead of compiling")
    ap.add_argument("--compensate", action="store_true", help="compensate.hip's k_compensate4 / k_compensate_mt")
    ap.add_argument("--trace", metavar="REGEX", help="print the memory operations and waits of the kernels matching it")
    a = ap.parse_args()
    src, name_re = ("compensate.hip", r"k_compensate(4|_mt)I") if a.compensate else ("select.hip", r"k_compensate_list(16)?I")
    text = open(a.asm).read() if a.asm else compile_asm(src)
    print("| kernel | vgpr | occ | launched | scratch | flat | walks | stream | before-vm-wait | waits-before / mem | mem-to-last |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    out = []
    cap = None if (a.asm or a.compensate) else flat_launch_waves()   # an --asm file's launch is not known
    for name, body, tr in kernels(text, name_re):
        occ = trailer(tr, "Occupancy")
        one = re.search(r"k_compensate_listILb\dELb1E", name)
        launched = "%d" % occ if not (cap and one) else "%d / %d" % (min(occ, cap), occ)
        # K1-16 streams 8-B loads and has no LDS-bounded launch (`one` does not match it);
        # K1-mixed streams both widths under K1's launch
        width = "dwordx2" if "k_compensate_list16I" in name else "dwordx[24]" if re.search(MIXED, name) else "dwordx4"
        walks, cut = scan(body, nstream=None if a.compensate else kSegLoads, stream_op=width)
        if a.trace:
            if re.search(a.trace, name) and walks:
                for what, w in (("fewest", min(walks, key=lambda w: w.mem_to_last)), ("most", max(walks, key=lambda w: w.mem_to_last))):
                    print("## %s: the walk with the %s memory-dependent waits up to its last streaming load" % (pretty(name), what))
                    print("\n".join(w.log))
            continue
        flat = sum(1 for ln in body if re.match(r"^\s+flat_load", ln))
        if not walks:
            out.append("| %s | %d | %d | %s | %d | %d | 0%s | - | - | - | - |" % (
                pretty(name), trailer(tr, "NumVgprs"), occ, launched, trailer(tr, "ScratchSize"), flat, "+" if cut else ""))
            continue
        for w in walks:
            if w.before_vm_wait is None:
                w.before_vm_wait = w.stream
        rng = lambda f: ("%d" % min(map(f, walks))) if min(map(f, walks)) == max(map(f, walks)) else "%d-%d" % (min(map(f, walks)), max(map(f, walks)))
        out.append("| %s | %d | %d | %s | %d | %d | %d%s | %s | %s | %s / %s | %s |" % (
            pretty(name), trailer(tr, "NumVgprs"), occ, launched, trailer(tr, "ScratchSize"), flat, len(walks),
            "+" if cut else "", rng(lambda w: w.stream), rng(lambda w: w.before_vm_wait), rng(lambda w: w.waits_before),
            rng(lambda w: w.mem_before), rng(lambda w: w.mem_to_last)))
    print("\n".join(sorted(out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
