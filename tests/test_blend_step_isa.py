"""Static checks of the fused blend kernel's instances in the built library (tools/row_loops.py; no GPU needed), and of the hand-placed
scenes of tests/blend_step_case.py on the CPU oracle.

Every blend_step_kernel instance: at most 64 VGPRs, no scratch, at most 20 KB of LDS (eight workgroups per CU), and no ds_bpermute_b32
(the wave reductions of the backward prologue run in the vector ALU: blend_common.h, wave_sum_lane0 / wave_max_lane0).  The instance
bench.py launches: its three row loops -- the forward's, and the backward's two copies, one per 64-splat word -- are each shorter than
in the parent commit, whose figures profiles/blend_step_row_loops.json records next to this build's; the counts below are upper bounds.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# instructions per row of the bench instance, loop control included (the parent: forward 74, backward 104 and 105)
FWD_ROW_MAX = 69
BWD_ROW_MAX = (101, 102)


@pytest.fixture(scope="module")
def figures():
    from igs_amd import build
    build.build()
    import row_loops as RL
    return RL, RL.figures(build.LIB)


def test_every_instance_keeps_its_resources_and_uses_no_lds_crossbar(figures):
    RL, fig = figures
    assert len(fig) == 6, sorted(fig)          # <geometry, colour-only> x <plain, |gradient|, masked>
    for name, f in fig.items():
        assert 0 < f["vgpr"] <= 64, (name, f)
        assert f["scratch"] == 0 and f["spill"] == 0, (name, f)
        assert 0 < f["lds"] <= 20 * 1024, (name, f)
        assert f["ds_bpermute_b32"] == 0, (name, f)
        assert len(f["row_loops"]["fwd"]) == 1 and len(f["row_loops"]["bwd"]) == 2, (name, f)      # (the loops were recognised)


def test_row_loops_of_the_bench_instance_are_shorter_than_the_parents(figures):
    RL, fig = figures
    with open(os.path.join(ROOT, "profiles", "blend_step_row_loops.json")) as fh:
        rec = json.load(fh)
    parent = rec["parent"][RL.BENCH_INSTANCE]["row_loops"]
    now = fig[RL.BENCH_INSTANCE]["row_loops"]
    print("row loops of the bench instance: parent", parent, "now", now)
    assert now["fwd"][0] <= FWD_ROW_MAX < parent["fwd"][0]
    for n, bound, p in zip(sorted(now["bwd"]), BWD_ROW_MAX, sorted(parent["bwd"])):
        assert n <= bound < p
    assert rec["branch"][RL.BENCH_INSTANCE]["row_loops"]["fwd"][0] <= FWD_ROW_MAX           # (the record is of a build that met the bounds)
    assert tuple(sorted(rec["branch"][RL.BENCH_INSTANCE]["row_loops"]["bwd"])) <= BWD_ROW_MAX


def test_loop_finder_on_a_hand_written_stream():
    import row_loops as RL
    ins = [(0, "s_mov_b32", "", None), (4, "v_exp_f32_e32", "", None), (8, "s_cbranch_scc1", "", 4),            # forward-like loop 4..8
           (12, "s_nop", "", None), (16, "v_exp_f32_e32", "", None), (20, "s_cbranch_vccz", "", 12),               # early exit to the latch ...
           (24, "ds_write_addtid_b32", "", None), (28, "s_branch", "", 12), (32, "s_endpgm", "", None)]           # ... and the branch back
    assert RL.loops(ins) == [(1, 2), (3, 7)]
    assert RL.row_loops(ins) == {"fwd": [2], "bwd": [5]}


@pytest.mark.parametrize("name", ["counts_a", "counts_b", "saturate"])
def test_hand_placed_scenes_hold_the_instance_counts_they_claim(name):
    """The oracle's binning of the layouts the GPU test runs: every tile's list has the length the layout names; in the counting
    layouts some pixel takes the very last element of every list, in `saturate` no pixel of any tile gets past 70 % of its list."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import blend_step_case as B
    from igs_amd.scenes import activate
    from oracle import c_oracle as co
    raw, bg, gt, tiles = B.scene(name)
    assert raw["xyz"].shape[0] % 4 == 0
    cam, a = B.camera(), activate(raw)
    nr, out, st = co.rasterize_forward(bg, a["means3D"], None, a["opacities"], a["scales"], a["rotations"], 1.0, None,
                                       cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, 0.0,
                                       cam.height, cam.width, a["shs"], 3, cam.camera_center)
    im = st.intermediates()
    rg, nc = im["ranges"].astype(np.int64), im["n_contrib"][0]
    assert (rg[:, 1] - rg[:, 0]).tolist() == tiles and nr == sum(tiles)
    deepest = [int(nc[(t // 3) * 16:(t // 3) * 16 + 16, (t % 3) * 16:(t % 3) * 16 + 16].max()) for t in range(6)]
    if name == "saturate":
        assert all(0 < d <= 0.7 * n for d, n in zip(deepest, tiles)), (deepest, tiles)
        T = 1.0 - np.asarray(out["alpha"]).reshape(B.H, B.W)
        assert float(T.max()) < 1e-2          # (every pixel finished: T (1 - alpha) < 1e-4 with alpha <= 0.99 means T < 0.01)
    else:
        assert deepest == tiles
        assert set(tiles) >= ({0, 1, 64, 65, 128, 129} if name == "counts_a" else {192, 193, 260})
