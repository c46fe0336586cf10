"""Residency guard of the two front-end kernels of the step, read from the built gfx950 code objects (no GPU needed).

preprocess_fwd_kernel<true, false> and tile_sort_kernel are latency chains: every wave of the launch is resident at once or starts late
(the late starters are the last to finish), so neither may lose a wave per SIMD or start to spill.  gfx950 allocates
VGPRs in steps of 8 out of 512 per lane: up to 72 allocated registers leave 7 waves per SIMD, the class both kernels are in
(profiles/front_end_split.json records the figures of this build next to its parent's: 68 and 67 VGPRs, no scratch).
"""
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = "_Z21preprocess_fwd_kernelILb1ELb0EE"      # preprocess_fwd_kernel<SPLIT = true, VANILLA = false>
SORT = "_Z16tile_sort_kernel"
VGPR_CLASS = 72                                  # allocation of the 7-waves-per-SIMD class


def front_end_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = A.code_objects(build.LIB)
    try:
        found = {}
        for co in cos:
            for name, md in kernel_metadata(co).items():
                for key in (PRE, SORT):
                    if name.startswith(key):
                        found.setdefault(key, []).append(md)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_front_end_kernels_keep_their_occupancy_class_and_do_not_spill():
    found = front_end_kernels()
    assert sorted(found) == sorted([PRE, SORT]) and all(len(v) == 1 for v in found.values()), {k: len(v) for k, v in found.items()}
    with open(os.path.join(ROOT, "profiles", "front_end_split.json")) as f:
        recorded = json.load(f)["kernels"]
    for key, label in ((PRE, "preprocess_fwd_kernel<true, false>"), (SORT, "tile_sort_kernel")):
        md = found[key][0]
        vgpr, scratch = int(md[".vgpr_count"]), int(md[".private_segment_fixed_size"])
        parent = recorded[label]["parent"]
        assert (parent["vgpr"] + 7) // 8 * 8 <= VGPR_CLASS and parent["scratch"] == 0, (label, parent)      # (the class is the parent's)
        assert (vgpr + 7) // 8 * 8 <= VGPR_CLASS, (label, "VGPRs", vgpr)
        assert scratch == 0, (label, "scratch bytes per lane", scratch)
