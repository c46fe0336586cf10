"""Static figures of the fused blend kernel's instances in a built libigs_rast.so (gfx950 code objects; runs without a GPU):

  * resources of every blend_step_kernel instance from the code object's metadata: VGPRs, scratch bytes, LDS bytes;
  * how often each instance names a given instruction (ds_bpermute_b32: the LDS crossbar);
  * the length, in instructions, of its ROW LOOPS: the innermost loops that evaluate a splat (they hold a v_exp_f32).  The forward's
    loop (blend_fwd_tile.h: blend_row) has no ds_write_addtid_b32; the backward's (blend_bwd_tile.h: process_row + reduce_row, one copy
    per 64-splat word of a round) has the column writes of the transpose.  A loop is the span from the lowest target of a backward
    branch to the last branch back to it, so the loop's own control instructions count.

  python tools/row_loops.py [lib.so]          prints one JSON object
"""
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_barriers as A

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
BENCH_INSTANCE = "_Z17blend_step_kernelILb1ELb1ELb1ELb0ELb0EEv12BlendFwdArgs12BlendBwdArgs"       # what bench.py (cfg3) launches


def resources(co):
    """{kernel symbol: {vgpr, scratch, lds}} from the AMDGPU metadata note"""
    txt = subprocess.run([READELF, "--notes", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    out, cur = {}, {}
    for line in txt.splitlines():
        m = re.match(r"^\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if line.lstrip().startswith("- ."):          # a new kernel's map begins
            cur = {}
        cur[k] = v
        if k == "vgpr_count" and "name" in cur:      # (keys are sorted: name comes before vgpr_count)
            out[cur["name"]] = dict(vgpr=int(v), scratch=int(cur.get("private_segment_fixed_size", -1)),
                                    lds=int(cur.get("group_segment_fixed_size", -1)), spill=-1)
        if k == "vgpr_spill_count" and cur.get("name") in out:
            out[cur["name"]]["spill"] = int(v)
    return out


def loops(insns):
    """[(first index, last index)] of the innermost loops of one kernel"""
    index = {a: i for i, (a, _, _, _) in enumerate(insns)}
    ext = {}
    for i, (a, mn, ops, tgt) in enumerate(insns):
        if tgt is not None and tgt in index and index[tgt] <= i:
            h = index[tgt]
            ext[h] = max(ext.get(h, h), i)
    spans = sorted(ext.items())
    return [(h, e) for h, e in spans if not any(h2 != h and h <= h2 <= e for h2, _ in spans)]


def row_loops(insns):
    """{'fwd': [lengths], 'bwd': [lengths]}"""
    out = {"fwd": [], "bwd": []}
    for h, e in loops(insns):
        body = [mn for _, mn, _, _ in insns[h:e + 1]]
        if not any(mn.startswith("v_exp_f32") for mn in body):
            continue
        out["bwd" if any(mn.startswith("ds_write_addtid_b32") for mn in body) else "fwd"].append(e + 1 - h)
    return out


def figures(lib):
    tmp, cos = A.code_objects(lib)
    try:
        res = {}
        for co in cos:
            meta = resources(co)
            for f, insns in A.parse(co).items():
                if "blend_step_kernel" not in f or not insns:
                    continue
                r = dict(meta.get(f, {}))
                r["instructions"] = len(insns)
                r["ds_bpermute_b32"] = sum(1 for _, mn, _, _ in insns if mn.startswith("ds_bpermute"))
                r["row_loops"] = row_loops(insns)
                res[f] = r
        return res
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    print(json.dumps(figures(sys.argv[1] if len(sys.argv) > 1 else A.LIB), indent=1, sort_keys=True))
