"""Records tests/golden/abi_refusals.json: the (status, message) of every row of
tests/test_abi_refusals.py, from the library DGC_HIP_LIB names (default: the built one).

The committed file was recorded from a library built from the commit BEFORE csrc/dispatch.hpp and
csrc/payload.hpp (make -C <that commit's csrc> OUT_DIR=<dir>; DGC_HIP_LIB=<dir>/libdgc_hip.so
python tests/golden/make_abi_refusals.py), so the test pins the refusals those headers must keep.
Re-record only for a row that is new, from a library in which the entry point's checks are known
good. No GPU needed: a row that is accepted or reaches HIP is an error here too.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the package on the path)
import test_abi_refusals as t  # noqa: E402
from dgc import _lib  # noqa: E402


def main():
    L = _lib.lib()
    out = {}
    for (fn, what, change), key in zip(t.ROWS, t.IDS):
        status, message = t.refuse(L, fn, change)
        if status in (t.OK, t.HIP):
            sys.exit("%s: not refused before HIP: %d %s" % (key, status, message))
        out[key] = [status, message]
    with open(os.path.join(HERE, "abi_refusals.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d refusals recorded from %s" % (len(out), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
