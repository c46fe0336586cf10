"""simple_knn drop-in without a GPU: the reference import line, the argument checks of distCUDA2 and of the C ABI, the closed forms of
the restatement (tests/knn_restatement.py), and the COLMAP point-cloud reader."""
import ast
import ctypes as C
import os

import numpy as np
import pytest
import torch

import knn_restatement as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_POINTS = 1 << 25          # IGS_KNN_MAX_POINTS (include/igs_rast.h)


def test_reference_import_line_gives_the_compiled_builtin():
    from simple_knn._C import distCUDA2           # RaDe-GS scene/gaussian_model.py:20, IGS igs/models/gaussian_model.py:19
    from igs_amd import _cabi
    assert type(distCUDA2).__name__ == "builtin_function_or_method"
    assert distCUDA2 is _cabi.ext().distCUDA2 or distCUDA2.__self__ is _cabi.ext().distCUDA2.__self__


def test_distcuda2_rejects_cpu_dtype_and_shape():
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distCUDA2(torch.zeros(8, 3))
    for dt in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(RuntimeError, match="float32"):
            distCUDA2(torch.zeros(8, 3, dtype=dt))
    for shape in ((8, 4), (8,), (8, 3, 1), (3, 8)):
        with pytest.raises(RuntimeError, match=r"shape \[N, 3\]"):
            distCUDA2(torch.zeros(*shape))
    with pytest.raises(RuntimeError, match="more than the supported"):
        distCUDA2(torch.zeros(1, 3).expand(MAX_POINTS + 1, 3))


def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1), not IGS_RAST_E_HIP (-2): on a machine without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    for name in ("igs_knn_scratch_bytes", "igs_knn_mean_dist2"):
        assert name in _cabi.EXPORTS and hasattr(L, name)
    assert L.igs_knn_scratch_bytes(-1) == 0 and L.igs_knn_scratch_bytes(MAX_POINTS + 1) == 0
    assert L.igs_knn_scratch_bytes(1000) >= 1000 * 16 and L.igs_knn_scratch_bytes(MAX_POINTS) > L.igs_knn_scratch_bytes(1000)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.igs_knn_mean_dist2(None, -1, p, p, p) == -1 and "out of range" in _cabi.last_error()
    assert L.igs_knn_mean_dist2(None, MAX_POINTS + 1, p, p, p) == -1 and "out of range" in _cabi.last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.igs_knn_mean_dist2(None, 5, *args) == -1 and "NULL" in _cabi.last_error()
    assert L.igs_knn_mean_dist2(None, 0, None, None, None) == 0


def test_restatement_unit_lattice():
    x = KR.lattice(4)
    np.testing.assert_array_equal(KR.restate_f32(x), np.ones(64, np.float32))        # every point: three neighbours at 1 (corners too)
    x = KR.lattice(3, dims=2)
    r = KR.restate_f32(x).reshape(3, 3)
    assert r[1, 1] == 1.0 and r[0, 1] == 1.0                                            # interior, edge: four / three at 1
    assert r[0, 0] == np.float32(np.float32(1 + 1) + np.float32(2)) / np.float32(3)    # corner: 1, 1, then the diagonal 2
    x = KR.lattice(5, dims=1)
    r = KR.restate_f32(x)
    assert r[2] == np.float32(1 + 1 + 4) / np.float32(3) and r[0] == np.float32(1 + 4 + 9) / np.float32(3)


def test_restatement_small_n():
    inf, fmax = np.float32(np.inf), np.float32(KR.FLT_MAX)
    assert KR.restate_f32(np.zeros((1, 3)))[0] == inf
    np.testing.assert_array_equal(KR.restate_f32([[0, 0, 0], [1, 0, 0]]), [inf, inf])
    r = KR.restate_f32([[0, 0, 0], [1, 0, 0], [0, 2, 0]])
    assert r.dtype == np.float32 and np.all(r == fmax / np.float32(3)) and np.all(np.isfinite(r))
    r = KR.restate_f32([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]])
    assert r[0] == np.float32(1 + 4 + 9) / np.float32(3) and r[1] == np.float32(1 + 5 + 10) / np.float32(3)


def test_restatement_duplicates_and_f64_agree():
    x = np.array([[0.5, 0.5, 0.5]] * 4 + [[2, 2, 2]], np.float32)
    r = KR.restate_f32(x)
    assert np.all(r[:4] == 0)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(300, 3, generator=g)
    np.testing.assert_allclose(KR.restate_f32(x.numpy()), KR.brute_f64(x).numpy(), rtol=2e-6)


def test_simple_knn_imports_nothing_from_oracle():
    for f in ("__init__.py", "_C.py"):
        tree = ast.parse(open(os.path.join(ROOT, "simple_knn", f)).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not any(a.name.split(".")[0] == "oracle" for a in node.names), f
            elif isinstance(node, ast.ImportFrom):
                assert node.level > 0 or (node.module or "").split(".")[0] != "oracle", f


def _write_points3d(path, xyz, rgb, normals, fmt="binary_little_endian"):
    names = [("x", "f4"), ("y", "f4"), ("z", "f4")] + ([("nx", "f4"), ("ny", "f4"), ("nz", "f4")] if normals else []) + \
            [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    a = np.zeros(len(xyz), dtype=[(n, "<" + t) for n, t in names])
    a["x"], a["y"], a["z"] = xyz.T
    a["red"], a["green"], a["blue"] = rgb.T
    with open(path, "wb") as f:
        f.write(("ply\nformat %s 1.0\nelement vertex %d\n" % (fmt, len(xyz))).encode())
        for n, t in names:
            f.write(("property %s %s\n" % ("float" if t == "f4" else "uchar", n)).encode())
        f.write(b"end_header\n")
        if fmt == "ascii":
            for row in a:
                f.write((" ".join(repr(v.item()) if isinstance(v, np.floating) else str(int(v)) for v in row) + "\n").encode())
        else:
            f.write(a.tobytes())


@pytest.mark.parametrize("normals,fmt", [(True, "binary_little_endian"), (False, "binary_little_endian"), (False, "ascii")])
def test_load_point_cloud_ply(tmp_path, normals, fmt):
    from igs_amd.io import load_point_cloud_ply
    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((37, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    path = str(tmp_path / "points3D.ply")
    _write_points3d(path, xyz, rgb, normals, fmt)
    p, c = load_point_cloud_ply(path)
    assert p.dtype == torch.float32 and c.dtype == torch.float32 and p.shape == (37, 3) and c.shape == (37, 3)
    np.testing.assert_array_equal(p.numpy(), xyz)
    np.testing.assert_array_equal(c.numpy(), (rgb / 255.0).astype(np.float32))        # fetchPly: uint8 / 255.0
