"""The anchor-graph drop-ins without a GPU: the reference's import lines, the argument refusals of torch_cluster / fpsample / the
compiled module / the C ABI, and the restatements of tests/anchors_restatement.py against each other."""
import ast
import ctypes as C
import os

import numpy as np
import pytest
import torch

import anchors_restatement as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS = 1 << 26           # IGS_ANCHOR_MAX_POINTS (include/igs_rast.h)
MAX_EXAMPLES = 1 << 16         # IGS_ANCHOR_MAX_EXAMPLES
MAX_EXAMPLE_POINTS = 1 << 22   # IGS_FPS_MAX_EXAMPLE_POINTS


def test_reference_import_lines_resolve_to_this_repository():
    import fpsample                                   # igs/models/gs.py:14
    import torch_cluster                              # igs/models/grid_encoder.py:13, main.py:34
    from torch_cluster import fps, knn                # igs/models/gs.py:41
    for m in (fpsample, torch_cluster):
        assert os.path.dirname(os.path.dirname(os.path.abspath(m.__file__))) == ROOT
    assert callable(fps) and callable(knn) and callable(fpsample.bucket_fps_kdline_sampling)
    assert sorted(torch_cluster.__all__) == ["fps", "knn"]


def test_packages_import_nothing_from_oracle():
    for pkg in ("torch_cluster", "fpsample"):
        for f in os.listdir(os.path.join(ROOT, pkg)):
            if f.endswith(".py"):
                tree = ast.parse(open(os.path.join(ROOT, pkg, f)).read())
                for node in ast.walk(tree):
                    names = [a.name for a in node.names] if isinstance(node, ast.Import) else \
                        [node.module or ""] if isinstance(node, ast.ImportFrom) else []
                    assert not any(n.split(".")[0] == "oracle" for n in names), (pkg, f)
    tree = ast.parse(open(os.path.join(ROOT, "igs_amd", "anchors.py")).read())
    for node in ast.walk(tree):
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [a.name for a in node.names] + [getattr(node, "module", None) or ""]
            assert not any(n.split(".")[0] == "oracle" for n in names)


def test_torch_cluster_knn_refusals():
    from torch_cluster import knn
    x = torch.zeros(8, 3)
    with pytest.raises(NotImplementedError, match="cosine"):
        knn(x, x, 2, cosine=True)
    with pytest.raises(NotImplementedError, match="3-D"):
        knn(torch.zeros(8, 2), torch.zeros(8, 2), 2)
    with pytest.raises(NotImplementedError, match="float32"):
        knn(x.double(), x.double(), 2)
    for k in (0, 101, -1):
        with pytest.raises(ValueError, match="k must be in"):
            knn(x, x, k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn(x, x, 2)


def test_torch_cluster_fps_refusals():
    from torch_cluster import fps
    x = torch.zeros(8, 3)
    for r in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="ratio"):
            fps(x, ratio=r)
    with pytest.raises(NotImplementedError, match="3-D"):
        fps(torch.zeros(8, 4))
    with pytest.raises(NotImplementedError, match="float32"):
        fps(x.half())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fps(x, ratio=0.5)


def test_fpsample_refusals():
    import fpsample
    pc = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="n_samples"):
        fpsample.bucket_fps_kdline_sampling(pc, 11, h=5)
    for h in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match="h must be"):
            fpsample.bucket_fps_kdline_sampling(pc, 4, h=h)
    with pytest.raises(ValueError, match="start_idx"):
        fpsample.bucket_fps_kdline_sampling(pc, 4, h=5, start_idx=10)
    with pytest.raises(NotImplementedError, match="float32"):
        fpsample.bucket_fps_kdline_sampling(pc.astype(np.float64), 4, h=5)
    with pytest.raises(NotImplementedError, match=r"\[N, 3\]"):
        fpsample.bucket_fps_kdline_sampling(np.zeros((10, 2), np.float32), 4, h=5)
    assert fpsample.bucket_fps_kdline_sampling(pc, 0, h=5).shape == (0,)


def test_compiled_module_refusals():
    from igs_amd import _cabi
    E = _cabi.ext()
    x = torch.zeros(8, 3)
    p = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.anchors_knn(x, x, p, p, 4)
    with pytest.raises(RuntimeError, match="k must be in"):
        E.anchors_knn(x, x, p, p, 101)
    with pytest.raises(RuntimeError, match="float32"):
        E.anchors_knn(x.double(), x, p, p, 4)
    with pytest.raises(RuntimeError, match=r"shape \[N, 3\]"):
        E.anchors_fps(torch.zeros(8, 2), p, p[:1], p, 4, 8, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.anchors_fps(x, p, p[:1], p, 4, 8, 1.0)
    with pytest.raises(RuntimeError, match="more than the supported"):
        E.anchors_fps(x, p, p[:1], p, 4, MAX_EXAMPLE_POINTS + 1, 1.0)
    with pytest.raises(RuntimeError, match="init_d2"):
        E.anchors_fps(x, p, p[:1], p, 4, 8, -1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.anchors_bbox_select(x, p, torch.zeros(1, 2, 3))
    with pytest.raises(RuntimeError, match="box must be"):
        E.anchors_bbox_select(x, p, torch.zeros(2, 2, 3))


def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1), not IGS_RAST_E_HIP (-2): on a machine without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    for name in ("igs_bbox_select_scratch_bytes", "igs_bbox_select", "igs_fps_scratch_bytes", "igs_fps", "igs_knn_query"):
        assert name in _cabi.EXPORTS and hasattr(L, name)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # scratch sizes
    assert L.igs_bbox_select_scratch_bytes(-1) == 0 and L.igs_bbox_select_scratch_bytes(MAX_POINTS + 1) == 0
    assert L.igs_bbox_select_scratch_bytes(1000) > 0
    assert L.igs_fps_scratch_bytes(0, 10, 10) == 0 and L.igs_fps_scratch_bytes(1, -1, 10) == 0
    assert L.igs_fps_scratch_bytes(1, 10, MAX_EXAMPLE_POINTS + 1) == 0 and L.igs_fps_scratch_bytes(MAX_EXAMPLES + 1, 10, 10) == 0
    assert L.igs_fps_scratch_bytes(1, 200000, 200000) >= 200000 * 16
    # bbox select
    assert L.igs_bbox_select(None, 0, 5, p, p, p, p, p, p, p) == -1 and "out of range" in _cabi.last_error()
    assert L.igs_bbox_select(None, 1, MAX_POINTS + 1, p, p, p, p, p, p, p) == -1
    for i in range(7):
        args = [p] * 7
        args[i] = None
        assert L.igs_bbox_select(None, 1, 5, *args) == -1 and "NULL" in _cabi.last_error()
    # fps
    assert L.igs_fps(None, 0, 5, 5, p, p, p, p, 4, 1.0, p, p) == -1 and "out of range" in _cabi.last_error()
    assert L.igs_fps(None, 1, 5, MAX_EXAMPLE_POINTS + 1, p, p, p, p, 4, 1.0, p, p) == -1
    assert L.igs_fps(None, 1, 5, 5, p, p, p, p, -1, 1.0, p, p) == -1 and "total" in _cabi.last_error()
    assert L.igs_fps(None, 1, 5, 5, p, p, p, p, 4, -1.0, p, p) == -1 and "init_d2" in _cabi.last_error()
    assert L.igs_fps(None, 1, 5, 5, p, p, p, p, 4, float("nan"), p, p) == -1
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert L.igs_fps(None, 1, 5, 5, *args[:4], 4, 1.0, *args[4:]) == -1 and "NULL" in _cabi.last_error()
    assert L.igs_fps(None, 1, 5, 5, None, None, None, None, 0, 1.0, None, None) == 0
    # knn
    for k in (0, 101):
        assert L.igs_knn_query(None, 1, 5, 5, p, p, p, p, k, 0.0, p, None, None) == -1 and "k out of range" in _cabi.last_error()
    assert L.igs_knn_query(None, 0, 5, 5, p, p, p, p, 8, 0.0, p, None, None) == -1
    assert L.igs_knn_query(None, 1, -1, 5, p, p, p, p, 8, 0.0, p, None, None) == -1
    for i in range(5):
        args = [p] * 5
        args[i] = None
        assert L.igs_knn_query(None, 1, 5, 5, *args[:4], 8, 0.0, args[4], None, None) == -1 and "NULL" in _cabi.last_error()
    assert L.igs_knn_query(None, 1, 5, 0, None, None, None, None, 8, 0.0, None, None, None) == 0


def test_header_states_the_limits():
    h = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    for s in ("#define IGS_ANCHOR_MAX_POINTS (1 << 26)", "#define IGS_ANCHOR_MAX_EXAMPLES (1 << 16)",
              "#define IGS_FPS_MAX_EXAMPLE_POINTS (1 << 22)", "#define IGS_KNN_QUERY_MAX_K 100"):
        assert s in h


# ---------------------------------------------------------------- the restatements against each other
def test_fps_restatement_equals_float64_loop_on_integer_clouds():
    g = np.random.default_rng(0)
    for n, s in ((60, 30), (150, 50), (200, 40)):
        x = g.integers(0, 50, (n, 3)).astype(np.float32)
        start = int(g.integers(n))
        np.testing.assert_array_equal(AR.fps_restate(x, s, start, np.inf), AR.fps_f64(x, s, start))


def test_fps_restatement_passes_its_certificate_on_float_clouds():
    g = np.random.default_rng(1)
    x = g.random((400, 3)).astype(np.float32)
    AR.fps_certificate(x, AR.fps_restate(x, 100, 5, np.inf))
    np.testing.assert_array_equal(AR.fps_restate(x, 100, 5, np.inf), AR.fps_f64(x, 100, 5))


def test_fps_tie_rules_on_a_lattice():
    x = AR.lattice(2)                                  # the unit cube's corners, index = 4 x + 2 y + z
    # 7 is the one corner at 3; after 0 and 7 the other six are all at 1 of a pick, so they come in index order
    np.testing.assert_array_equal(AR.fps_restate(x, 8, 0, np.inf), [0, 7, 1, 2, 3, 4, 5, 6])
    # once every point is picked, the lowest index with cur 0 repeats
    s = AR.fps_restate(x, 10, 0, np.inf)
    assert list(s[8:]) == [0, 0]
    # the initial distance caps cur: with init 0.5 every point starts below any distance >= 1, so picks go in index order
    np.testing.assert_array_equal(AR.fps_restate(x, 4, 5, 0.5), [5, 0, 1, 2])


def test_fps_restatement_non_finite_points():
    x = AR.lattice(3)
    x[4, 1] = np.nan
    x[20, 0] = np.inf
    s = AR.fps_restate(x, 25, 0, np.inf)
    assert 4 not in s and 20 not in s and np.unique(s).size == 25


def test_knn_restatement_equals_float64_truth_on_integer_clouds():
    g = np.random.default_rng(2)
    x = g.integers(0, 30, (300, 3)).astype(np.float32)
    y = g.integers(0, 30, (100, 3)).astype(np.float32)
    for k in (1, 8, 16):
        ri, rd = AR.knn_restate(x, y, k, [0, 120, 300], [0, 60, 100])
        fi, fd = AR.knn_f64(x, y, k, [0, 120, 300], [0, 60, 100])
        np.testing.assert_array_equal(ri, fi)
        np.testing.assert_array_equal(rd, fd[:, :k].astype(np.float32))


def test_knn_restatement_tie_rule_and_padding():
    x = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 2], [3e5, 0, 0], [np.nan, 0, 0]], np.float32)
    y = np.zeros((1, 3), np.float32)
    idx, d2 = AR.knn_restate(x, y, 6)
    np.testing.assert_array_equal(idx[0], [0, 1, 2, 3, -1, -1])    # equal distances: lower index first; d2 >= 1e10 and NaN never count
    np.testing.assert_array_equal(d2[0], [1, 1, 1, 4, np.inf, np.inf])


def test_select_restatement():
    x = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 1, 1], [1, 1, 1.5]], np.float32)
    out = AR.select_restate([x, x], [[[0, 0, 0], [1, 1, 1]], [[1, 1, 1], [2, 2, 2]]])
    np.testing.assert_array_equal(out[0], [0, 1])
    np.testing.assert_array_equal(out[1], [1, 2, 4])


# ---------------------------------------------------------------- the case builders of tests/test_gpu_anchors_edges.py
# Each GPU edge test names the launch branch it is there for; these restate the launch code (tests/anchors_restatement.py cites the
# lines) and fail if a size stops landing in its branch.
def test_fps_geometry_restated_and_the_classes_of_the_edge_cases():
    assert AR.fps_geometry(1) == (64, 1) and AR.fps_geometry(65536) == (64, 1) and AR.fps_geometry(65537) == (64, 2)
    assert AR.fps_geometry(131072) == (64, 2) and AR.fps_geometry(131073) == (64, 4) and AR.fps_geometry(262144) == (64, 4)
    assert AR.fps_geometry(262145) == (128, 4) and AR.fps_geometry(524288) == (128, 4) and AR.fps_geometry(524289) == (256, 4)
    assert AR.fps_geometry(MAX_EXAMPLE_POINTS) == (1024, 4)
    src = open(os.path.join(ROOT, "igs_amd", "csrc", "anchors.hip")).read()
    for line in ("#define FPS_WAVES 16", "#define FPS_MAX_SLOTS 4", "#define KNNQ_THREADS 256", "#define KNNQ_TILE 2048",
                 "while ((long long)max_n > (long long)FPS_WAVES * 64 * FPS_MAX_SLOTS * 64 * m) m *= 2;",
                 "while ((long long)FPS_WAVES * 64 * r < leaves) r *= 2;", "while ((1 << bits) < B) bits++;",
                 "if (k <= 8) knnq_launch<8>", "else if (k <= 16) knnq_launch<16>", "else if (k <= 32) knnq_launch<32>",
                 "else knnq_launch<100>"):
        assert line in src, line
    seen = set()
    for name, (side, samples, start, cls) in AR.FPS_CLASS_CASES.items():
        assert AR.fps_geometry(side ** 3) == cls, name
        assert 0 < start < side ** 3 and samples < side ** 3
        assert 3 * (side - 1) ** 2 < 2 ** 24              # every squared distance of the lattice is an exact float32
        seen.add(cls)
    assert seen == {(64, 2), (64, 4), (128, 4), (256, 4)}
    assert AR.fps_geometry(AR.FPS_CERT_R2[0]) == (64, 2)
    assert AR.fps_geometry(40 ** 3) == (64, 1)            # (what test_gpu_anchors.py's large lattice runs: one slot)


def test_fps_batch_builders():
    xs = AR.fps_batch_case()
    assert [len(x) for x in xs] == [512, 64, 1000, 27]
    full = [s == len(x) for s, x in zip(AR.FPS_BATCH_SAMPLES, xs)]
    assert full == [False, True, False, True]
    assert all(0 <= s < len(x) for s, x in zip(AR.FPS_BATCH_STARTS, xs)) and AR.FPS_BATCH_STARTS[1] == 63 and AR.FPS_BATCH_STARTS[2] == 999
    bad = [int((~np.isfinite(x).all(1)).sum()) for x in xs]
    assert bad == [0, 0, 5, 0] and np.isfinite(xs[2][AR.FPS_BATCH_STARTS[2]]).all()
    assert AR.FPS_BATCH_SAMPLES[2] <= 1000 - 5            # the non-finite rows are never reached
    # a fully sampled lattice: a permutation
    s = AR.fps_restate(xs[3], 27, 0, np.inf)
    np.testing.assert_array_equal(np.sort(s), np.arange(27))
    B, side, samples = AR.FPS_MANY
    assert AR.fps_example_bits(B) == 9 and (AR.fps_example_bits(B) + 7) // 8 == 2 and samples < side ** 3
    assert AR.fps_example_bits(256) == 8 and AR.fps_example_bits(257) == 9 and AR.fps_example_bits(4) == 2 and AR.fps_example_bits(1) == 0
    # the 70 000-point example under max_n = 1000: more leaves than the launch's slots hold, while the scratch (sized by N) has its rows
    LS, R = AR.fps_geometry(1000)
    assert (LS, R) == (64, 1) and (70000 + LS - 1) // LS > AR.FPS_WAVES * 64 * R
    # the 100-point example beside the 65^3 lattice: one leaf of 128 rows
    assert AR.fps_geometry(65 ** 3)[0] == 128 and (100 + 127) // 128 == 1


def test_select_builders():
    for n in (1, 63, 64, 65, 255, 256, 257, 1025, 300000):
        x, box = AR.select_case(n, seed=n)
        assert x.shape == (n, 3) and x.dtype == np.float32
        assert (x[np.isfinite(x)] * 2 == np.round(x[np.isfinite(x)] * 2)).all()              # half-integers
        if n >= 63:
            fin = np.isfinite(x).all(1)
            assert (~fin).sum() >= max(3, n // 100)
            assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
            assert ((x[fin] == box[0]).any(1)).any() and ((x[fin] == box[1]).any(1)).any()      # points exactly on both faces
            assert (x[fin] < box[0]).any() and (x[fin] > box[1]).any()                          # and points outside
            kept = AR.select_restate([x], [box])[0]
            assert 0 < kept.size < n
    assert AR.select_scan_per_thread(300000) == 2 and (300000 + 255) // 256 == 1172
    assert AR.select_scan_per_thread(262144) == 1 and AR.select_scan_per_thread(1025) == 1
    xs, boxes = AR.select_batch_case()
    assert tuple(len(x) for x in xs) == AR.SELECT_BATCH_SIZES == (100, 0, 37, 1, 300)
    ptr = np.concatenate([[0], np.cumsum(AR.SELECT_BATCH_SIZES)])
    inside = [p for p in ptr[1:-1] if p % 64 != 0 and p < 256]
    assert sorted(set(inside)) == [100, 137, 138]         # example boundaries inside waves of the first workgroup
    want = AR.select_restate(xs, boxes)
    assert want[0].size == 100 and want[1].size == 0 and want[3].size == 0 and 0 < want[2].size < 37 and 0 < want[4].size < 300


def test_knn_builders():
    assert [AR.knn_slot_class(k) for k in (1, 8, 9, 16, 17, 32, 33, 100)] == [8, 8, 16, 16, 32, 32, 100, 100]
    x, y, px, py = AR.knn_masked_case()
    assert list(np.diff(px)) == [2049, 40, 300] and list(np.diff(py)) == [250, 20, 330]
    assert AR.knn_straddling_workgroups(py) == [True, True, False]
    assert px[1] - px[0] > AR.KNNQ_TILE                   # example 0 spans two LDS tiles
    assert 32 < px[2] - px[1] < 100                       # example 1 (40 points): padded slots at k = 100, full rows at 16 and 32
    assert (x >= 0).all() and (x < 12).all() and (x == np.round(x)).all()
    assert AR.knn_straddling_workgroups([0, 256, 512]) == [False, False] and AR.knn_straddling_workgroups([0, 255, 512]) == [True, False]
    # the cut: 99 999^2 rounds below 1e10 in float32, 100 000^2 is 1e10 exactly
    x, y = AR.knn_cut_case()
    d = AR.d2_f32(y[0], x[:2])
    assert d[0] < np.float32(AR.KNN_NONE) and d[1] == np.float32(AR.KNN_NONE) and float(np.float32(1e10)) == 1e10
    idx, d2 = AR.knn_restate(x, y, 16)
    assert list(idx[0][:5]) == [8, 9, 3, 5, 0] and (idx[0][5:] == -1).all() and (idx[1] == -1).all()
    w = AR.knn_weights_f64(d2, idx, 0.001)
    assert (w[1] == 0).all() and (w[0][5:] == 0).all() and abs(w[0].sum() - 1) < 1e-12 and abs(w[2].sum() - 1) < 1e-12
    ref = torch.softmax(-0.001 * torch.from_numpy(d2[0, :5]).double().sqrt(), -1).numpy()
    np.testing.assert_allclose(w[0, :5], ref, rtol=1e-12)
