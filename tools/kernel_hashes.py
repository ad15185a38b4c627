#!/usr/bin/env python3
"""One hash per device function of the library: did a change of host code leave every kernel alone?

Host only, no GPU. For each of the Makefile's SRCS it compiles device-only gfx950 assembly with
the Makefile's own flags (read as tools/k1_isa.py reads them) and prints one line per function,
sorted:

  file  mangled-name  sha256

The hash covers the function's text, without comments, with local labels (`.L...`, which
carry the function's emission-order number) renamed by order of first appearance and with the
function's own symbol (its label, its `.amdhsa_kernel NAME` line) replaced by a placeholder, and
the kernel's `.amdhsa_kernel ... .end_amdhsa_kernel` block (registers, LDS, scratch). Two listings
are equal exactly when the same functions were emitted with the same instructions and the same
resources; a function that only changed its name (a new template parameter, say) keeps its hash,
and --diff pairs it with its old name: a removed and an added function of one file with equal
hashes print as `renamed  FILE  OLD -> NEW` (several with one hash: paired in sorted order).

  tools/kernel_hashes.py > new.txt                 # this tree
  tools/kernel_hashes.py --root OLD > old.txt      # another checkout of the repository
  tools/kernel_hashes.py --diff old.txt new.txt    # exit 1 on any added, removed, changed or renamed function

Both listings of a --diff are made by the same version of this tool: listings of an earlier
version hashed the name too.
"""
import argparse
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k1_isa  # noqa: E402  (the Makefile reader and the compile step)


def functions(text):
    """{mangled name: sha256} of every function of one translation unit's assembly."""
    lines = text.split("\n")
    names = [m.group(1) for m in (re.match(r"^\s*\.type\s+(\S+),@function", ln) for ln in lines) if m]
    start = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"^[\w.$]+:", ln)}
    desc = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = lines[i:j + 1]
    out = {}
    for name in names:
        i = j = start[name]
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        local = {}
        # comments go: the compiler's loop notes name blocks by the same emission-order number
        body = "\n".join(ln.split(";")[0].rstrip() for ln in lines[i:j] + desc.get(name, []))
        body = re.sub(r"\.L\w+", lambda m: local.setdefault(m.group(0), ".L%d" % len(local)), body)
        body = body.replace(name, "SELF")   # (also inside `.text.NAME`, its section)
        out[name] = hashlib.sha256(body.encode()).hexdigest()
    return out


def listing(root, srcs=None):
    csrc = os.path.join(root, "adam-compression_amd", "csrc")
    rows = []
    for src in srcs or k1_isa.makefile_vars(csrc)["SRCS"].split():
        for name, h in functions(k1_isa.compile_asm(src, csrc)).items():
            rows.append("%s  %s  %s" % (src, name, h))
    return sorted(rows)


def read_listing(path):
    return {tuple(ln.split()[:2]): ln.split()[2] for ln in open(path) if ln.strip()}


def diff(old, new):
    a, b = read_listing(old), read_listing(new)
    gone, came = sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys())
    renamed = []
    for k in list(gone):
        twin = next((c for c in came if c[0] == k[0] and b[c] == a[k]), None)
        if twin:
            renamed.append((k[0], k[1], twin[1]))
            gone.remove(k)
            came.remove(twin)
    changed = [k for k in sorted(a.keys() & b.keys()) if a[k] != b[k]]
    out = ["removed  %s  %s" % k for k in gone] + ["added    %s  %s" % k for k in came]
    out += ["changed  %s  %s" % k for k in changed] + ["renamed  %s  %s -> %s" % r for r in renamed]
    print("\n".join(out), end="\n" if out else "")
    print("%d functions, %d removed, %d added, %d changed, %d renamed" % (
        len(a), len(gone), len(came), len(changed), len(renamed)), file=sys.stderr)
    return 1 if out else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=k1_isa.ROOT, help="the checkout to compile (default: this one)")
    ap.add_argument("--diff", nargs=2, metavar=("OLD", "NEW"), help="compare two listings instead of compiling")
    ap.add_argument("srcs", nargs="*", metavar="FILE.hip", help="only these translation units (default: the Makefile's SRCS)")
    a = ap.parse_args()
    if a.diff:
        return diff(*a.diff)
    print("\n".join(listing(a.root, a.srcs)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
