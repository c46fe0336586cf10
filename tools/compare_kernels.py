"""Compares the gfx950 kernels of two builds of libigs_rast.so instruction by instruction (llvm-objdump -d of the code objects,
tools/audit_barriers.py).  Branch targets are compared as offsets from the kernel's start; kernels are matched by name, and a kernel
whose name changed only by a template flag added with its default (`<true>` -> `<true, false>`) is matched to its old name.

usage: python tools/compare_kernels.py OLD.so NEW.so [--fp]      (exit status 1 if any kernel present in OLD differs in NEW)

--fp: for every CHANGED kernel, the floating-point arithmetic opcodes whose count per class and type differs (fp_class below) -- none
when only the schedule, the addressing or the register allocation moved; a mul + add that became an fma, or the reverse, shows here.
"""
import collections
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


FP_OP = re.compile(r"^v_(pk_)?(fmac|fmamk|fmaak|fma_mixlo|fma_mixhi|fma_mix|fma|add|subrev|sub|mul|div_scale|div_fmas|div_fixup|rcp|rsq|sqrt|exp|log"
                   r"|ldexp|rndne|min3|max3|med3|min|max)(?:_legacy)?_(f16|f32|f64)$")
FP_CLASS = {"fmac": "fma", "fmamk": "fma", "fmaak": "fma", "subrev": "add", "sub": "add",      # the register allocator picks between these
            "fma_mix": "fma", "fma_mixlo": "fma", "fma_mixhi": "fma", "min3": "min", "max3": "max", "med3": "minmax3",
            "div_scale": "div", "div_fmas": "div", "div_fixup": "div"}


def fp_class(mnemonic):
    """Class and type of a floating-point arithmetic opcode, e.g. "fma_f32", "cvt_f32_f64"; None for anything else.  Compares
    (v_cmp*) are left out: the compiler swaps their operands and predicates freely."""
    mn = re.sub(r"(_e32|_e64|_sdwa|_dpp)+$", "", mnemonic)
    m = FP_OP.match(mn)
    if m:
        return (m.group(1) or "") + FP_CLASS.get(m.group(2), m.group(2)) + "_" + m.group(3)
    return mn[2:] if re.match(r"^v_cvt_.*(f16|f32|f64)", mn) else None


def fp_counts(insns):
    return collections.Counter(c for c in (fp_class(i.split(" ", 1)[0]) for i in insns) if c)


def main(old_lib, new_lib, fp=False):
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
            if fp:
                a, b = fp_counts(ins), fp_counts(new[m])
                diff = ["%s %d -> %d" % (c, a[c], b[c]) for c in sorted(set(a) | set(b)) if a[c] != b[c]]
                print("    fp:", ", ".join(diff) or "every class equal (%d opcodes)" % sum(a.values()))
    added = [dem[n] for n in new if n not in old and n not in {by_key.get(key(o)) for o in old}]
    print("%d kernels compared, %d differ; new: %s" % (len(old), bad, ", ".join(sorted(added)) or "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*[x for x in sys.argv[1:] if x != "--fp"], fp="--fp" in sys.argv))
