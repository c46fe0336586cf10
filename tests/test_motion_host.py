"""Anchor feature interpolation and the Gaussian deform without a GPU: the float64 restatement (tests/motion_restatement.py) against hand
evaluations and gradcheck, and the argument refusals of the compiled module and the C ABI (igs_amd/csrc/motion.hip)."""
import ctypes as C
import os

import pytest
import torch

import motion_restatement as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROWS = 1 << 24        # IGS_INTERP_MAX_ROWS (include/igs_rast.h)
MAX_ANCHORS = 1 << 24     # IGS_INTERP_MAX_ANCHORS
MAX_POINTS = 1 << 26      # IGS_DEFORM_MAX_POINTS
NAMES = ("igs_anchor_interp_fwd", "igs_anchor_interp_index_bytes", "igs_anchor_interp_index", "igs_anchor_interp_bwd",
         "igs_gaussian_deform_fwd", "igs_gaussian_deform_bwd")


# ---------------------------------------------------------------- the restatement
def test_interp_restatement_by_hand():
    F = torch.tensor([[1., 2.], [3., 4.], [5., 6.]], dtype=torch.float64)
    w = torch.tensor([[2., 1.], [1., 0.5]], dtype=torch.float64).unsqueeze(-1)
    col = torch.tensor([0, 2, 1, -1])                       # row 1's second slot is knn padding: nothing
    out = MR.interp_restate(F, w, col)
    assert out.tolist() == [[2 * 1 + 5, 2 * 2 + 6], [3., 4.]]
    parts = MR.split_by_batch(out, torch.tensor([0., 1.]))
    assert [p.shape[0] for p in parts] == [1, 1]


def test_qmul_restatement_by_hand():
    i = torch.tensor([[0., 1., 0., 0.]], dtype=torch.float64)
    j = torch.tensor([[0., 0., 1., 0.]], dtype=torch.float64)
    k = torch.tensor([[0., 0., 0., 1.]], dtype=torch.float64)
    assert MR.qmul_restate(i, j).tolist() == k.tolist()               # i j = k (Hamilton)
    assert MR.qmul_restate(j, i).tolist() == (-k).tolist()            # j i = -k
    two = torch.tensor([[2., 0., 0., 0.]], dtype=torch.float64)       # normalised first: 2 -> 1
    assert MR.qmul_restate(two, 3 * i).tolist() == i.tolist()
    z = torch.zeros(1, 4, dtype=torch.float64)                        # |q| < eps: q / eps = 0
    assert MR.qmul_restate(z, i).tolist() == z.tolist()


def test_deform_restatement_by_hand():
    class G:
        xyz = torch.tensor([[0., 0., 0.], [1., 1., 1.], [2., 2., 2.]], dtype=torch.float64)
        rotation = torch.tensor([[1., 0., 0., 0.]] * 3, dtype=torch.float64)
        opacity = torch.zeros(3, 1, dtype=torch.float64)
        scaling = torch.ones(3, 3, dtype=torch.float64)
        shs = torch.zeros(3, 16, 3, dtype=torch.float64)
    mask = torch.tensor([2, 0])
    res = {"xyz": torch.tensor([[1., 2., 3.], [4., 5., 6.]], dtype=torch.float64),
           "rotation": torch.tensor([[0., 2., 0., 0.], [1., 0., 0., 0.]], dtype=torch.float64)}
    d = MR.deform_restate(G, res, mask)
    assert d["xyz"].tolist() == [[4., 5., 6.], [1., 1., 1.], [3., 4., 5.]]
    assert d["rotation"].tolist() == [[1., 0., 0., 0.], [1., 0., 0., 0.], [0., 1., 0., 0.]]
    assert sorted(d) == sorted(["xyz", "opacity", "rotation", "scaling", "shs", "resi_xyz", "resi_rotation", "mask"])


def test_restatement_gradcheck():
    g = torch.Generator().manual_seed(0)
    F = torch.randn(6, 5, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.rand(4, 3, dtype=torch.float64, generator=g, requires_grad=True)
    col = torch.tensor([[0, 5, 2], [1, -1, 1], [3, 4, 0], [2, 2, 9]])
    assert torch.autograd.gradcheck(lambda F, w: MR.interp_restate(F, w, col), (F, w))
    xyz = torch.randn(5, 3, dtype=torch.float64, generator=g, requires_grad=True)
    rot = torch.randn(5, 4, dtype=torch.float64, generator=g, requires_grad=True)
    mask = torch.tensor([4, 1, 2])
    dx = torch.randn(3, 3, dtype=torch.float64, generator=g, requires_grad=True)
    dr = torch.randn(3, 4, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda *a: MR.deform_xyz_rotation_restate(a[0], a[1], mask, a[2], a[3]), (xyz, rot, dx, dr))


# ---------------------------------------------------------------- the compiled module
def test_compiled_module_refusals():
    from igs_amd import _cabi
    E = _cabi.ext()
    F = torch.zeros(8, 4)
    col = torch.zeros(3, 2, dtype=torch.long)
    w = torch.zeros(3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_interp_fwd(F, col, w)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.motion_interp_fwd(F.double(), col, w)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.motion_interp_fwd(F.bfloat16(), col, w)
    with pytest.raises(NotImplementedError, match="col must be"):
        E.motion_interp_fwd(F, col.int(), w)
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_interp_fwd(F, col, torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="out of range"):
        E.motion_interp_fwd(torch.zeros(8, 1025), col, w)
    with pytest.raises(RuntimeError, match="out of range"):
        E.motion_interp_fwd(F, torch.zeros(3, 101, dtype=torch.long), torch.zeros(3, 101))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_interp_index(col, 8, 4)
    with pytest.raises(RuntimeError, match="out of range"):
        E.motion_interp_index(col, 0, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_interp_bwd(F, w, torch.zeros(3, 4), torch.zeros(10, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_interp_bwd(F, w, torch.zeros(3, 5), torch.zeros(10, dtype=torch.uint8))
    xyz, rot, mask = torch.zeros(5, 3), torch.zeros(5, 4), torch.tensor([1, 3])
    dx, dr = torch.zeros(2, 3), torch.zeros(2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_deform_fwd(xyz, rot, mask, dx, dr)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.motion_deform_fwd(xyz, rot, mask, dx.double(), dr.double())
    with pytest.raises(NotImplementedError, match="xyz must be"):
        E.motion_deform_fwd(xyz.double(), rot, mask, dx, dr)
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_deform_fwd(xyz, rot, mask, torch.zeros(3, 3), dr)
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_deform_fwd(torch.zeros(5, 4), rot, mask, dx, dr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_deform_bwd(rot, mask, dx, dr, xyz, rot)


def test_python_layer_refusals():
    from igs_amd import motion
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        motion.interpolate_anchor_features(torch.zeros(1, 8, 4, dtype=torch.float64), torch.zeros(3, 2, 1), torch.zeros(6, dtype=torch.long))
    with pytest.raises(ValueError, match="col has"):
        motion.interpolate_anchor_features(torch.zeros(1, 8, 4), torch.zeros(3, 2, 1), torch.zeros(5, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.interpolate_anchor_features(torch.zeros(1, 8, 4), torch.zeros(3, 2, 1), torch.zeros(6, dtype=torch.long))

    class G:
        xyz, rotation = torch.zeros(5, 3), torch.zeros(5, 4)
        opacity, scaling, shs = torch.zeros(5, 1), torch.zeros(5, 3), torch.zeros(5, 16, 3)
    with pytest.raises(NotImplementedError, match="shs"):
        motion.deform(G, {"xyz": torch.zeros(2, 3), "rotation": torch.zeros(2, 4), "shs": torch.zeros(2, 48)}, torch.tensor([0, 1]))


# ---------------------------------------------------------------- the C ABI
def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1), not IGS_RAST_E_HIP (-2): on a machine without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    for name in NAMES:
        assert name in _cabi.EXPORTS and hasattr(L, name)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = _cabi.last_error
    # index sizes
    assert L.igs_anchor_interp_index_bytes(-1, 8, 100, 4) == 0 and L.igs_anchor_interp_index_bytes(10, 0, 100, 4) == 0
    assert L.igs_anchor_interp_index_bytes(10, 101, 100, 4) == 0 and L.igs_anchor_interp_index_bytes(10, 8, 0, 4) == 0
    assert L.igs_anchor_interp_index_bytes(10, 8, 100, 1025) == 0 and L.igs_anchor_interp_index_bytes(10, 8, MAX_ANCHORS + 1, 4) == 0
    assert L.igs_anchor_interp_index_bytes(100000, 8, 8192, 128) >= 100000 * 8 * 16
    # forward: sizes, dtype, NULLs
    for (N, K, D, A), what in (((-1, 8, 4, 10), "N out of range"), ((MAX_ROWS + 1, 8, 4, 10), "N out of range"),
                               ((5, 0, 4, 10), "K out of range"), ((5, 101, 4, 10), "K out of range"),
                               ((5, 8, 0, 10), "D out of range"), ((5, 8, 1025, 10), "D out of range"),
                               ((5, 8, 4, 0), "A_total out of range"), ((5, 8, 4, MAX_ANCHORS + 1), "A_total out of range")):
        assert L.igs_anchor_interp_fwd(None, N, K, D, A, 0, p, p, p, p) == -1 and what in err(), (N, K, D, A, err())
        assert L.igs_anchor_interp_index(None, N, K, A, D, p, p) == -1 and what in err()
        assert L.igs_anchor_interp_bwd(None, N, K, D, A, 0, p, p, p, p, p, p) == -1 and what in err()
    assert L.igs_anchor_interp_fwd(None, 5, 8, 4, 10, 2, p, p, p, p) == -1 and "dtype" in err()
    assert L.igs_anchor_interp_bwd(None, 5, 8, 4, 10, -1, p, p, p, p, p, p) == -1 and "dtype" in err()
    for i in range(4):
        args = [p] * 4
        args[i] = None
        assert L.igs_anchor_interp_fwd(None, 5, 8, 4, 10, 0, *args) == -1 and "NULL" in err()
    for i in range(2):
        args = [p] * 2
        args[i] = None
        assert L.igs_anchor_interp_index(None, 5, 8, 10, 4, *args) == -1 and "NULL" in err()
    for i in range(4):                       # F (needed for dw), w, dout, scratch
        args = [p] * 4
        args[i] = None
        assert L.igs_anchor_interp_bwd(None, 5, 8, 4, 10, 0, *args, p, p) == -1 and "NULL" in err()
    # zero-size calls launch nothing
    assert L.igs_anchor_interp_fwd(None, 0, 8, 4, 10, 0, None, None, None, None) == 0
    assert L.igs_anchor_interp_index(None, 0, 8, 10, 4, None, None) == 0
    assert L.igs_anchor_interp_bwd(None, 5, 8, 4, 10, 0, p, p, p, p, None, None) == 0
    # deform
    for fn, extra in ((L.igs_gaussian_deform_fwd, 7), (L.igs_gaussian_deform_bwd, 9)):
        assert fn(None, -1, 0, 0, *[p] * extra) == -1 and "P out of range" in err()
        assert fn(None, MAX_POINTS + 1, 0, 0, *[p] * extra) == -1 and "P out of range" in err()
        assert fn(None, 5, 6, 0, *[p] * extra) == -1 and "M out of range" in err()
        assert fn(None, 5, -1, 0, *[p] * extra) == -1 and "M out of range" in err()
        assert fn(None, 5, 2, 3, *[p] * extra) == -1 and "dtype" in err()
        assert fn(None, 0, 0, 0, *[None] * extra) == 0
    for i in range(7):
        args = [p] * 7
        args[i] = None
        assert L.igs_gaussian_deform_fwd(None, 5, 2, 0, *args) == -1 and "NULL" in err(), i
    for i in range(3):                       # rot, mask, drot (with d_rot asked for)
        args = [p] * 3
        args[i] = None
        assert L.igs_gaussian_deform_bwd(None, 5, 2, 0, *args, p, p, p, p, p, p) == -1 and "NULL" in err(), i
    assert L.igs_gaussian_deform_bwd(None, 5, 2, 0, p, p, p, p, p, None, None, None, None) == 0


def test_header_states_the_limits():
    h = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    for s in ("#define IGS_INTERP_MAX_ROWS (1 << 24)", "#define IGS_INTERP_MAX_K 100", "#define IGS_INTERP_MAX_D 1024",
              "#define IGS_INTERP_MAX_ANCHORS (1 << 24)", "#define IGS_INTERP_MAX_EDGES (1 << 30)", "#define IGS_DEFORM_MAX_POINTS (1 << 26)",
              "#define IGS_DTYPE_F32 0", "#define IGS_DTYPE_F16 1"):
        assert s in h
    for name in NAMES:
        assert name + "(" in h


# ---------------------------------------------------------------- the case builders of tests/test_gpu_motion_edges.py
# Each GPU edge test names the launch branch it is there for; these restate the launch code (tests/motion_restatement.py cites the
# lines) and fail if a size stops landing in its branch.
def test_launch_geometry_restated_from_the_source():
    src = open(os.path.join(ROOT, "igs_amd", "csrc", "motion.hip")).read()
    for line in ("while (c < 512 && (uint64_t)c * 4 * 16 * 256 < E) c *= 2;", "while (((uint64_t)1 << bits) <= (uint64_t)A) bits++;",
                 "return D <= 64 ? 1 : D <= 128 ? 2 : D <= 256 ? 4 : D <= 512 ? 8 : 16;", "radix_sort_pairs(s, E, r, 0, L.bits)"):
        assert line in src, line
    header = open(os.path.join(ROOT, "igs_amd", "csrc", "radix_sort.h")).read()
    assert "#define SORT_MAX_BLOCKS 256" in header and "#define SORT_TILE (256 * SORT_ITEMS)" in header and "#define SORT_ITEMS 8" in header
    assert "for (int lo = bit_lo; lo < bit_hi; lo += 8, pass++)" in open(os.path.join(ROOT, "igs_amd", "csrc", "radix_sort.hip")).read()
    assert [MR.interp_chunk(e) for e in (1, 1 << 20, (1 << 20) + 1, 1 << 21, (1 << 21) + 1, 1 << 22, (1 << 22) + 1, 1 << 30)] == \
        [64, 64, 128, 128, 256, 256, 512, 512]
    assert [MR.interp_index_bits(a) for a in (1, 255, 256, 65535, 65536, MAX_ANCHORS)] == [1, 8, 9, 16, 17, 25]
    assert [MR.interp_dv(d) for d in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert MR.sort_geometry(1) == (1, 2048) and MR.sort_geometry(2049) == (2, 2048) and MR.sort_geometry(256 * 2048) == (256, 2048)
    assert MR.sort_geometry(256 * 2048 + 1) == (129, 4096)


def test_edge_cases_land_in_the_branches_their_tests_name():
    # what tests/test_gpu_motion.py already runs: chunk 64 and one or two index passes only
    assert MR.interp_chunk(150000) == 64 and MR.interp_chunk(15000 * 8) == 64
    # the shipped backward: chunk 128, a sort capped at 256 blocks whose slices span several sort tiles
    E = 200000 * 8
    assert MR.interp_chunk(E) == 128 and (E + MR.SORT_TILE - 1) // MR.SORT_TILE > MR.SORT_MAX_BLOCKS
    assert MR.sort_geometry(E) == (196, 8192) and MR.interp_index_passes(8192) == 2 and MR.interp_dv(128) == 2
    # the chunk-length cases
    for chunk, (N, K, D) in MR.CHUNK_SHAPES.items():
        assert MR.interp_chunk(N * K) == chunk, chunk
    assert sorted(MR.CHUNK_SHAPES) == [128, 256, 512]
    for c in (64, 128, 256, 512):
        assert {c - 1, c, c + 1} <= set(MR.CHUNK_DEGREES)
    assert {0, 1, 1025, 150000} <= set(MR.CHUNK_DEGREES)
    # the index's pass-count boundaries
    assert [MR.interp_index_passes(a) for a in MR.INDEX_PASS_ANCHORS] == [1, 2, 2, 3]
    # wide rows: both wide instantiations, at both ends of their ranges
    assert [MR.interp_dv(d) for d in (257, 512, 513, 1024)] == [8, 8, 16, 16] and MR.INTERP_MAX_D == 1024
    # the gradient-subset case: every anchor's list has many chunks
    F, w, col, dout = MR.exact_interp_case(4000, 8, 16, 40, pad=0.02, seed=4)
    assert int(MR.in_degrees(col, 16).min()) > 10 * MR.interp_chunk(4000 * 8)


@pytest.mark.parametrize("chunk", [128, 256, 512])
def test_exact_case_builder_degrees_and_exactness(chunk):
    N, K, D = MR.CHUNK_SHAPES[chunk]
    F, w, col, dout = MR.exact_interp_case(N, K, 300, D, degrees=MR.CHUNK_DEGREES, pad=0.02, seed=chunk)
    assert col.shape == (N, K) and F.shape == (300, D) and w.shape == (N, K) and dout.shape == (N, D)
    deg = MR.in_degrees(col, 300)
    assert deg[:len(MR.CHUNK_DEGREES)].tolist() == list(MR.CHUNK_DEGREES)
    pad = (col == -1).sum().item() / col.numel()
    assert 0.01 < pad < 0.03 and int(col.max()) < 300
    assert (F == F.round()).all() and (dout == dout.round()).all() and F.abs().max() <= 50 and dout.abs().max() <= 4
    assert set(w.unique().tolist()) == {1.0, 0.5, 0.25}
    m = MR.exact_margin(F, w, col, dout)
    assert m < 2 ** 24                                  # 4 * max sum |w g| < 2^24: every partial sum is an exact float32
    # the float32 evaluation of the restatement, in any order, equals the float64 one
    out32 = MR.interp_restate(F, w, col)
    assert torch.equal(out32.double(), MR.interp_restate(F.double(), w.double(), col))


def test_exact_case_builder_out_of_range_slots_and_margin_trips():
    F, w, col, dout = MR.exact_interp_case(3000, 8, 65536, 3, pad=0.05, oob=9, seed=65536)
    assert (col == 65536 + 7).sum().item() == 9 and 0.03 < (col == -1).float().mean().item() < 0.07
    big = dout * 2.0 ** 22                              # the condition is a real one: scaled gradients break it
    assert MR.exact_margin(F, w, col, big) >= 2 ** 24


def test_blocked_truth_equals_autograd_of_the_restatement():
    g = torch.Generator().manual_seed(3)
    N, K, A, D = 70, 5, 11, 6
    F = torch.randn(A, D, generator=g).double()
    w = torch.rand(N, K, generator=g).double()
    col = torch.randint(-2, A + 2, (N, K), generator=g)
    dout = torch.randn(N, D, generator=g).double()
    Fr, wr = F.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = MR.interp_restate(Fr, wr, col)
    ref.backward(dout)
    t = MR.interp_truth_blocked(F, w, col, dout, block=16)
    torch.testing.assert_close(t["out"], ref.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(t["dF"], Fr.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(t["dw"], wr.grad, rtol=1e-13, atol=1e-13)
    bad = (col < 0) | (col >= A)
    assert (t["dw"][bad] == 0).all() and (t["dw_abs"][bad] == 0).all() and t["deg"] == int(MR.in_degrees(col, A).max())
    torch.testing.assert_close(t["out_abs"], MR.interp_restate(F.abs(), w.abs(), col), rtol=1e-13, atol=1e-13)
    tol_F, tol_w = MR.interp_backward_bounds(t, K, D, True)
    assert (tol_F >= t["deg"] * MR.U * t["dF_abs"]).all() and (tol_F >= MR.U16 * t["dF"].abs()).all() and (tol_w[bad] <= 1e-30).all()


def test_ratio_helpers():
    ref = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    assert MR.worst_ratio(ref.float(), ref, torch.zeros_like(ref)) == 0.0                 # a zero bound admits a zero error
    assert MR.worst_ratio(ref.float() + 1, ref, torch.zeros_like(ref)) == float("inf")
    assert abs(MR.worst_ratio(ref.float() + 0.5, ref, torch.ones_like(ref)) - 0.5) < 1e-12
    gb = torch.tensor([[1.0, 100.0], [1e6, 0.0]], dtype=torch.float64)
    assert MR.deform_grad_ratio(gb.float(), gb, False) == 0.0
    assert MR.deform_grad_ratio(gb.float() + torch.tensor([[2e-3, 0.0], [0.0, 0.0]]), gb, False) > 1      # 1e-5 of the row's largest
    ga = gb.clone()
    ga[1, 0] = float("inf")                             # a float16 row beyond 65504 must hold an inf, and is then left out
    assert MR.deform_grad_ratio(ga.half(), gb, True) <= 1
    with pytest.raises(AssertionError):
        MR.deform_grad_ratio(gb.clamp(max=60000).half(), gb, True)
