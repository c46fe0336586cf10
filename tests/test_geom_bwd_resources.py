"""Residency guard of the fused per-Gaussian backward + Adam (geom_bwd.hip), read from the built gfx950 code objects (no GPU needed).

The bench grid (200k Gaussians, one 64-thread workgroup per 64 of them = 3,125 workgroups) fits the chip in one round only if the
colour-only instances run 4 waves per SIMD (<= 128 VGPRs, SGPR spills included, no scratch) and a workgroup's LDS stays at or below
10 KiB (16 workgroups per CU).  At 2 waves per SIMD and 15.6 KiB the kernel ran in two rounds, the second repeating the latency-bound
per-Gaussian phase with the HBM half idle.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
# geom_bwd_kernel<FUSED = true, NT = 64, COLOUR_ONLY = true, PARTIAL = *>
COLOUR_ONLY = re.compile(r"^_Z15geom_bwd_kernelILb1ELi64ELb1ELb[01]EEv6GBArgs$")


def kernel_metadata(code_object):
    """{kernel symbol: {metadata key: value}} from the NT_AMDGPU_METADATA note (top-level scalar keys of each amdhsa.kernels entry)."""
    txt = subprocess.run([READELF, "--notes", code_object], stdout=subprocess.PIPE, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^  - (\.\w+):\s*(.*)$", line)             # a new entry of amdhsa.kernels
        if m:
            cur = {m.group(1): m.group(2).strip()}
        else:
            m = re.match(r"^    (\.\w+):\s*(\S.*)$", line)
            if m is None or cur is None:
                continue
            cur[m.group(1)] = m.group(2).strip()
        if ".name" in cur:
            kernels[cur[".name"]] = cur
    return kernels


def geom_bwd_instances():
    """{kernel symbol: metadata} of every geom_bwd_kernel instance in the built library"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    tmp, cos = A.code_objects(build.LIB)
    try:
        found = {}
        for co in cos:
            for name, md in kernel_metadata(co).items():
                if name.startswith("_Z15geom_bwd_kernelI"):
                    found[name] = md
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_no_geom_bwd_instance_uses_scratch():
    """The kernel's phases hand their values on in small structs: none of them may end up in private memory (a runtime-indexed local
    array would), in any instance: unfused, and fused general / colour-only with and without frozen groups."""
    found = geom_bwd_instances()
    assert len(found) == 5, sorted(found)
    for name, md in found.items():
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane", md[".private_segment_fixed_size"])


def test_colour_only_geom_bwd_fits_the_bench_grid_in_one_round():
    from igs_amd import _cabi
    found = {name: md for name, md in geom_bwd_instances().items() if COLOUR_ONLY.match(name)}
    assert len(found) == 2, sorted(found)            # the unmasked and the masked (PARTIAL) instance
    fn = _cabi.lib().igs_geom_bwd_adam_dyn_lds
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int]
    dyn = fn(16)                                     # SH degree 3: M = 16 coefficient rows
    for name, md in found.items():
        vgpr, scratch, lds = int(md[".vgpr_count"]), int(md[".private_segment_fixed_size"]), int(md[".group_segment_fixed_size"])
        assert vgpr <= 128, (name, "VGPRs (SGPR-spill lanes included)", vgpr)
        assert scratch == 0, (name, "scratch bytes per lane", scratch)
        assert lds + dyn <= 10 * 1024, (name, "LDS per workgroup: static + dynamic for M = 16", lds, dyn)
