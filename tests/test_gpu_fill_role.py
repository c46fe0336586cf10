"""The accumulator zero-fill of igs_refine_step, stored coalesced by the binning role of preprocess: the 64 rows of a wave are one span,
lane l of store k writes the 16-byte unit 64 k + l if the row it belongs to is that of a Gaussian the view sees (preprocess.hip).  What
can go wrong is the mapping of units to rows: a wave whose 64 rows are partly culled, partly beyond P, or partly in front of the first
row of a masked step; rows of 128 and of 256 bytes; the frame redone after a slab overflow (the first attempt's blend has added to
the rows by then); the one-kernel tile sort of slabs above 1024 slots.

Scenes as in tests/test_gpu_zero_fill_visible.py (tests/fill_role_case.py): steps on a workspace of 0xFF bytes (NaN as double and as
float) against the same steps on a zeroed one -- bit for bit on images, radii, parameters and both Adam moments.

A fill role in the tile-sort launch was measured against this and dropped (profiles/front_end_fill.txt), and with it its A/B switch
and a test of one placement against the other: there is one placement.  The radix-binning path is not selected
here: igs_refine_step reaches it only through a tile of more than TILE_SORT_BIG instances or slabs beyond SLAB_MAX_BYTES (IGS_BINNING=
radix is read by the stand-alone forward alone), neither of which is a test of a few seconds; the fill is the same code on both paths.
"""
import functools

import numpy as np
import pytest

import fill_role_case as F
from test_gpu_parity import dev  # noqa: F401

pytestmark = pytest.mark.gpu

PLAIN_SORT_SLAB = 1024          # TILE_SORT_WAVE_ALONE (csrc/common.h): slabs up to this size are sorted by the plain tile_sort_kernel


def same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert np.isfinite(b[k].astype(np.float64)).all(), (what, k)
        differ = F.bytes_that_differ(a[k], b[k])
        assert differ == 0, (what, k, "bytes that differ: %d" % differ)


@functools.lru_cache(maxsize=None)
def clean_run(case, n, w, h, scale_shift):
    """The reference of a scene: the steps on a zeroed workspace.  Computed once, never written to."""
    import torch
    out = F.run(case, 0, torch.device("cuda", 0), n, w, h, scale_shift)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("hint", [2048, 64])
@pytest.mark.parametrize("case", sorted(F.CASES))
def test_poisoned_workspace_on_the_one_kernel_sort_and_through_a_redone_frame(dev, case, hint):  # noqa: F811
    """Slab hint 2048: tile_sort_one_kernel follows the preprocess launch.  Hint 64: the first step overflows its slabs, the frame is
    redone with larger ones and both attempts fill (the first attempt's blend has added to the rows by then)."""
    from igs_amd import _cabi
    L = _cabi.lib()
    clean = clean_run(case, F.P, F.W, F.H, 1.5)
    old = L.igs_rast_get_slab_hint()
    try:
        L.igs_rast_set_slab_hint(hint)
        poisoned = F.run(case, 0xFF, dev)
        after = L.igs_rast_get_slab_hint()
    finally:
        L.igs_rast_set_slab_hint(old)
    print("case %s hint %d -> %d" % (case, hint, after))
    assert after >= 2048 if hint == 2048 else after > 64, (hint, after)       # (64: a tile overflowed and the frame was redone)
    same_bits(clean, poisoned, (case, hint))
    assert float(np.abs(clean["exp_avg_sq"]).max()) > 0.0 and float(np.abs(clean["images_2"][0:3]).max()) > 0.05      # the steps did something


# P = 20 011 at 32 x 32: 79 binning workgroups over four tiles, the last wave partial (20 011 = 312 * 64 + 43); masked: 13 340 rows, the
# first one not at a multiple of 64 Gaussians, so one wave's span starts in front of the accumulator.  Scales shifted down (footprints of
# a pixel or two: the ~1200 Gaussians a view sees land in one tile each), so that the four tiles hold what 1024-slot slabs carry and no
# frame is redone.  P = 129 and P = 1: a third wave with one row, and fewer rows than one wave has lanes (P = 1 masked has no trainable
# Gaussian at all and is left out).
SIZES = [(20011, 32, 32, -1.5, c) for c in sorted(F.CASES)] + [(129, 32, 32, 1.5, c) for c in sorted(F.CASES)] + [(1, 32, 32, 1.5, "l1"), (1, 32, 32, 1.5, "depth_normal")]


@pytest.mark.parametrize("n,w,h,shift,case", SIZES, ids=["P%d-%s" % (s[0], s[4]) for s in SIZES])
def test_partial_waves_and_a_first_row_inside_a_wave(dev, n, w, h, shift, case):  # noqa: F811
    from igs_amd import _cabi
    L = _cabi.lib()
    old = L.igs_rast_get_slab_hint()
    try:
        L.igs_rast_set_slab_hint(0)
        clean = clean_run(case, n, w, h, shift)
        poisoned = F.run(case, 0xFF, dev, n, w, h, shift)
        after = L.igs_rast_get_slab_hint()
    finally:
        L.igs_rast_set_slab_hint(old)
    seen = [int((clean["radii_%d" % s] > 0).sum()) for s in range(F.STEPS)]
    print("P %d case %s: visible per step %s, slab hint afterwards %d" % (n, case, seen, after))
    assert after <= PLAIN_SORT_SLAB, ("no frame was to be redone with larger slabs", after)
    if n > 1:
        assert min(seen) > 0, seen
    same_bits(clean, poisoned, (n, case))
