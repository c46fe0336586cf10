"""The radix sort's calling protocol (igs_amd/csrc/radix_sort.h) without a GPU: the scratch layouts its callers build with
radix_layout_append, seen through the C ABI's scratch-size queries, and the one rule for the buffer pair a sort's result lands in."""
import os
import re

import motion_restatement as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igs_amd", "csrc")
SIZES = (0, 1, 63, 64, 2049)


def test_scratch_sizes_are_those_of_the_hand_written_layouts():
    """Every caller's layout once spelled the sort's five regions out by hand.  The literals below were recorded from that build: the
    shared helper must give every size byte for byte (other arguments as in test_anchors_host / test_motion_host / test_lift_host)."""
    from igs_amd import _cabi
    L = _cabi.lib()
    assert [L.igs_morton_order_scratch_bytes(n) for n in SIZES] == [1311232, 1312256, 1312256, 1312256, 1345024]
    assert [L.igs_knn_scratch_bytes(n) for n in SIZES] == [2654976, 2657536, 2657536, 2657536, 2724096]
    assert [L.igs_fps_scratch_bytes(1, n, n) for n in SIZES] == [2656768, 2657792, 2659072, 2659072, 2733056]
    assert [L.igs_fps_scratch_bytes(3, n, n) for n in SIZES] == [2659328, 2660352, 2661632, 2661632, 2735616]
    assert [L.igs_anchor_interp_index_bytes(n, 8, 8192, 128) for n in SIZES] == [5571584, 5573120, 5583872, 5583872, 5966336]
    assert [L.igs_anchor_lift_scratch_bytes(5, 4, n, 128, 128, 128, 0) for n in SIZES] == [512, 1280, 15872, 15872, 492800]
    assert [L.igs_anchor_lift_bwd_scratch_bytes(5, 4, n, 128, 128, 128, 0) for n in SIZES] == [2622208, 2625024, 2718464, 2719488, 5737984]


def test_one_rule_for_where_the_result_lands():
    """8 key bits per pass, one swap of the buffer pairs per pass: in (kb, vb) after 1 or 3 passes, in (ka, va) after 0, 2 or 4."""
    got = {bits: MR.radix_lands_in_b(bits) for bits in (0, 1, 8, 9, 16, 17, 24, 25, 30, 31, 32)}
    assert got == {0: False, 1: True, 8: True, 9: False, 16: False, 17: True, 24: True, 25: False, 30: False, 31: False, 32: False}
    header = open(os.path.join(CSRC, "radix_sort.h")).read()
    assert "static inline bool radix_lands_in_b(int bits) { return (((bits + 7) / 8) & 1) != 0; }" in header
    # the sort itself: one swap per pass of 8 bits, and nobody else restates the rule
    sort = open(os.path.join(CSRC, "radix_sort.hip")).read()
    assert "for (int lo = bit_lo; lo < bit_hi; lo += 8, pass++)" in sort and sort.count("t = vin; vin = vout; vout = t;") == 1
    for name in os.listdir(CSRC):
        text = open(os.path.join(CSRC, name)).read()
        if name != "radix_sort.h":
            assert not re.search(r"\+ 7\) / 8\) (&|%) ?[12]|passes % 2|sorted_in_b", text), name
            assert "atomicAdd(&hist0[" not in text, name
        if name not in ("radix_sort.h", "radix_sort.hip"):
            assert "SORT_MAX_PASSES" not in text, name
