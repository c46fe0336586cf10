"""Compares the gfx950 kernels of two builds of libigs_rast.so instruction by instruction (llvm-objdump -d of the code objects,
tools/audit_barriers.py).  Branch targets are compared as offsets from the kernel's start; kernels are matched by name, and a kernel
whose name changed only by a template flag added with its default (`<true>` -> `<true, false>`) is matched to its old name.

usage: python tools/compare_kernels.py OLD.so NEW.so      (exit status 1 if any kernel present in OLD differs in NEW)
"""
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_barriers as A  # noqa: E402


def streams(lib):
    tmp, cos = A.code_objects(lib)
    try:
        out = {}
        for co in cos:
            for f, insns in A.parse(co).items():
                if insns:
                    base = insns[0][0]
                    out[f] = [mn + " " + ("->%d" % (t - base) if t is not None and t >= 0 else ops) for _, mn, ops, t in insns]
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def main(old_lib, new_lib):
    old, new = streams(old_lib), streams(new_lib)
    dem = demangle(list(old) + list(new))
    key = lambda n: re.sub(r"\(.*", "", dem[n]).replace(", false>", ">")      # name without parameter list / defaulted flag
    by_key = {key(n): n for n in new}
    bad = 0
    for n, ins in old.items():
        m = n if n in new else by_key.get(key(n))
        if m is None:
            print("MISSING  ", dem[n]); bad += 1
        elif new[m] != ins:
            print("CHANGED  ", dem[n]); bad += 1
    added = [dem[n] for n in new if n not in old and n not in {by_key.get(key(o)) for o in old}]
    print("%d kernels compared, %d differ; new: %s" % (len(old), bad, ", ".join(sorted(added)) or "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
