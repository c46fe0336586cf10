"""The compress rasterizer drop-in (diff_gaussian_rasterization_compress) without a GPU: the package's surface and argument checks, the
compiled count_gaussians, the C ABI's argument validation, and the count-pass restatement (tests/compress_restatement.py) against
closed forms."""
import ast
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import compress_restatement as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diff_gaussian_rasterization_compress")


def test_reference_import_line():
    # RaDe-GS gaussian_renderer/__init__.py:15, verbatim
    from diff_gaussian_rasterization_compress import GaussianRasterizationSettings as GaussianRasterizationSettings_compress, GaussianRasterizer as GaussianRasterizer_compress  # noqa: E501,F401
    import diff_gaussian_rasterization_compress as m
    for name in ("GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "_RasterizeGaussians", "cpu_deep_copy_tuple", "_C"):
        assert hasattr(m, name), name
    assert callable(m._RasterizeGaussians.forward_count)
    assert callable(m._C.count_gaussians) and callable(m._C.mark_visible)


def test_settings_field_order():
    from diff_gaussian_rasterization_compress import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
                                                     "viewmatrix", "projmatrix", "sh_degree", "campos", "prefiltered", "debug", "f_count")


def _settings(f_count=True, dev="cpu", W=32, H=32):
    from diff_gaussian_rasterization_compress import GaussianRasterizationSettings
    from igs_amd.camera import Camera
    c2w = torch.eye(4)
    c2w[2, 3] = -5.0
    cam = Camera.from_c2w(c2w, (math.radians(50.0), math.radians(50.0)), (H, W))
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                         bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev),
                                         projmatrix=cam.full_proj_transform.to(dev), sh_degree=0, campos=cam.camera_center.to(dev),
                                         prefiltered=False, debug=False, f_count=f_count)


def _inputs(P=4):
    g = torch.Generator().manual_seed(0)
    return dict(means3D=torch.rand(P, 3, generator=g), means2D=torch.zeros(P, 3), opacities=torch.rand(P, 1, generator=g),
                shs=torch.rand(P, 1, 3, generator=g), scales=torch.rand(P, 3, generator=g) * 0.1,
                rotations=torch.nn.functional.normalize(torch.rand(P, 4, generator=g), dim=1))


def test_rasterizer_argument_messages():
    from diff_gaussian_rasterization_compress import GaussianRasterizer
    r = GaussianRasterizer(_settings())
    x = _inputs()
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        r(means3D=x["means3D"], means2D=x["means2D"], opacities=x["opacities"], scales=x["scales"], rotations=x["rotations"])
    with pytest.raises(Exception, match="Please provide excatly one of either SHs or precomputed colors!"):
        r(means3D=x["means3D"], means2D=x["means2D"], opacities=x["opacities"], shs=x["shs"], colors_precomp=torch.rand(4, 3),
          scales=x["scales"], rotations=x["rotations"])
    with pytest.raises(Exception, match="Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"):
        r(means3D=x["means3D"], means2D=x["means2D"], opacities=x["opacities"], shs=x["shs"], scales=x["scales"])
    with pytest.raises(Exception, match="Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"):
        r(means3D=x["means3D"], means2D=x["means2D"], opacities=x["opacities"], shs=x["shs"], scales=x["scales"],
          rotations=x["rotations"], cov3D_precomp=torch.rand(4, 6))


def test_cpu_tensors_raise_loudly():
    from diff_gaussian_rasterization_compress import GaussianRasterizer
    x = _inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianRasterizer(_settings())(**x)


def test_training_path_is_not_built():
    import diff_gaussian_rasterization_compress as m
    x = _inputs()
    with pytest.raises(NotImplementedError, match="diff_gaussian_rasterization_rade"):
        m.GaussianRasterizer(_settings(f_count=False))(**x)
    with pytest.raises(NotImplementedError, match="diff_gaussian_rasterization_rade"):
        m._C.rasterize_gaussians()
    with pytest.raises(NotImplementedError, match="diff_gaussian_rasterization_rade"):
        m._C.rasterize_gaussians_backward()
    with pytest.raises(NotImplementedError, match="diff_gaussian_rasterization_rade"):
        m._RasterizeGaussians.backward(None, None)


def test_count_gaussians_is_compiled():
    from diff_gaussian_rasterization_compress import _C
    from igs_amd import _cabi
    assert type(_C.count_gaussians).__name__ == "builtin_function_or_method"
    assert _C.count_gaussians is _cabi.ext().count_gaussians
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs = _settings()
        x = _inputs()
        _C.count_gaussians(rs.bg, x["means3D"], torch.Tensor([]), x["opacities"], x["scales"], x["rotations"], 1.0, torch.Tensor([]),
                           rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, 32, 32, x["shs"], 0, rs.campos, False, False, True)


def test_c_abi_validates_before_any_hip_call():
    from igs_amd import _cabi
    L = _cabi.lib()
    assert "igs_rast_count_gaussians" in _cabi.EXPORTS and hasattr(L, "igs_rast_count_gaussians")
    assert L.igs_rast_version() == 4

    @_cabi.ALLOC_FN
    def never(user, n):                 # a scratch request would mean the call went past its checks
        raise AssertionError("scratch requested")

    buf = (C.c_float * 64)()
    ibuf = (C.c_int * 64)()
    p = C.cast(buf, C.c_void_p)
    ip = C.cast(ibuf, C.c_void_p)

    def call(P=4, W=16, H=16, color=p, count=ip, score=p, radii=ip):
        return L.igs_rast_count_gaussians(None, never, None, never, None, never, None, P, 0, 1, p, W, H, p, p, None, p, p, 1.0, p, None,
                                          p, p, p, 0.5, 0.5, 0, color, count, score, radii, 0)

    for kw in (dict(P=-1), dict(W=0), dict(H=-3), dict(color=None), dict(count=None), dict(score=None), dict(radii=None)):
        assert call(**kw) == -1, kw                                  # IGS_RAST_E_INVALID
        assert L.igs_rast_last_error()
    assert call(P=0, color=None, count=None, score=None, radii=None) == 0      # nothing to do, nothing launched


def test_c_abi_forward_and_backward_validate_before_any_hip_call():
    from igs_amd import _cabi
    L = _cabi.lib()

    @_cabi.ALLOC_FN
    def never(user, n):                 # a scratch request would mean the call went past its checks
        raise AssertionError("scratch requested")

    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fwd_names = ["stream", "geom", "geom_user", "binning", "binning_user", "image", "image_user", "P", "D", "M", "background", "W", "H",
                 "means3D", "shs", "colors_precomp", "opacities", "scales", "scale_modifier", "rotations", "cov3D_precomp",
                 "viewmatrix", "projmatrix", "cam_pos", "tan_fovx", "tan_fovy", "kernel_size", "prefiltered",
                 "color", "coord", "mcoord", "depth", "mdepth", "alpha", "normal", "radii", "require_coord", "require_depth", "debug"]
    fwd_ok = dict(stream=None, geom=never, geom_user=None, binning=never, binning_user=None, image=never, image_user=None,
                  P=4, D=0, M=1, background=p, W=16, H=16, means3D=p, shs=p, colors_precomp=None, opacities=p, scales=p,
                  scale_modifier=1.0, rotations=p, cov3D_precomp=None, viewmatrix=p, projmatrix=p, cam_pos=p, tan_fovx=0.5,
                  tan_fovy=0.5, kernel_size=0.0, prefiltered=0, color=p, coord=p, mcoord=p, depth=p, mdepth=p, alpha=p, normal=p,
                  radii=p, require_coord=1, require_depth=1, debug=0)
    null_fn = _cabi.ALLOC_FN()
    fwd_bad = [dict(P=-1), dict(W=0), dict(H=-3), dict(geom=null_fn), dict(binning=null_fn), dict(image=null_fn), dict(D=1, M=1), dict(D=4, M=25)]
    fwd_bad += [{k: None} for k in ("means3D", "opacities", "viewmatrix", "projmatrix", "cam_pos", "background", "radii",
                                    "color", "coord", "mcoord", "depth", "mdepth", "alpha", "normal")]
    fwd_bad += [dict(shs=None), dict(scales=None), dict(rotations=None)]

    def fwd(fn, **kw):
        a = dict(fwd_ok, **kw)
        return fn(*[a[k] for k in fwd_names])

    for fn in (L.igs_rast_forward, L.igs_rast_forward_async, L.igs_rast_forward_nowait):
        for kw in fwd_bad:
            assert fwd(fn, **kw) == -1, (fn.__name__, kw)                 # IGS_RAST_E_INVALID
            assert L.igs_rast_last_error(), (fn.__name__, kw)
    # (igs_rast_forward_nowait looks for its pinned status slot first: without a forward before it, even P == 0 is refused)
    for fn in (L.igs_rast_forward, L.igs_rast_forward_async):
        assert fwd(fn, P=0, geom=null_fn, means3D=None, color=None, radii=None) == 0, fn.__name__      # nothing to do, nothing launched
    assert L.igs_rast_forward_finish() == -1                            # no refused call above latched a pending forward

    bwd_names = ["stream", "P", "D", "M", "R", "background", "W", "H", "means3D", "shs", "colors_precomp", "alphas", "scales",
                 "scale_modifier", "rotations", "cov3D_precomp", "viewmatrix", "projmatrix", "campos", "tan_fovx", "tan_fovy",
                 "kernel_size", "radii", "normalmap", "geom_buffer", "binning_buffer", "image_buffer", "dL_dpix", "dL_dcoord",
                 "dL_dmcoord", "dL_ddepth", "dL_dmdepth", "dL_dalpha", "dL_dnormal", "workspace", "dL_dmean2D", "dL_dcolor",
                 "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot", "require_coord", "require_depth", "debug"]
    bwd_ok = dict(stream=None, P=4, D=0, M=1, R=8, background=p, W=16, H=16, means3D=p, shs=p, colors_precomp=None, alphas=p, scales=p,
                  scale_modifier=1.0, rotations=p, cov3D_precomp=None, viewmatrix=p, projmatrix=p, campos=p, tan_fovx=0.5, tan_fovy=0.5,
                  kernel_size=0.0, radii=p, normalmap=p, geom_buffer=p, binning_buffer=p, image_buffer=p, dL_dpix=p, dL_dcoord=None,
                  dL_dmcoord=None, dL_ddepth=None, dL_dmdepth=None, dL_dalpha=None, dL_dnormal=None, workspace=p, dL_dmean2D=p,
                  dL_dcolor=p, dL_dopacity=p, dL_dmean3D=p, dL_dcov3D=p, dL_dsh=p, dL_dscale=p, dL_drot=p, require_coord=1,
                  require_depth=1, debug=0)
    bwd_bad = [dict(P=-1), dict(R=-1), dict(W=0), dict(H=-3), dict(P=1 << 24)]
    bwd_bad += [{k: None} for k in ("geom_buffer", "binning_buffer", "image_buffer", "workspace", "means3D", "alphas", "viewmatrix",
                                    "projmatrix", "campos", "background", "radii", "normalmap", "dL_dmean2D", "dL_dcolor", "dL_dopacity",
                                    "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")]

    def bwd(**kw):
        a = dict(bwd_ok, **kw)
        return L.igs_rast_backward(*[a[k] for k in bwd_names])

    for kw in bwd_bad:
        assert bwd(**kw) == -1, kw
        assert L.igs_rast_last_error(), kw
    assert bwd(P=0, geom_buffer=None, workspace=None, means3D=None, dL_dcolor=None) == 0


def test_package_does_not_import_oracle():
    for f in os.listdir(PKG):
        if not f.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(PKG, f)).read())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n == "oracle" or n.startswith("oracle.") for n in names), (f, names)


# ---- the restatement against closed forms ----------------------------------------------------------------------------------
def _splat(x, y, sigma, opacity, depth):
    conic = torch.tensor([1.0 / sigma ** 2, 0.0, 1.0 / sigma ** 2])
    return x, y, conic, opacity, depth, math.ceil(3.0 * sigma)


def _g(splats):
    xy = torch.tensor([[s[0], s[1]] for s in splats], dtype=torch.float32)
    return dict(valid=torch.ones(len(splats), dtype=torch.bool), xy=xy, conic=torch.stack([s[2] for s in splats]).float(),
                opacity=torch.tensor([s[3] for s in splats], dtype=torch.float32), rgb=torch.ones(len(splats), 3),
                depth=torch.tensor([s[4] for s in splats], dtype=torch.float32),
                radius=torch.tensor([float(s[5]) for s in splats]))


def test_restatement_single_isotropic_gaussian():
    W, H = 48, 40
    s = _splat(20.3, 17.6, 3.0, 0.8, 1.0)
    count, color, _ = CR.count_blend(_g([s]), W, H, torch.zeros(3))
    want = CR.closed_form_single((s[0], s[1]), s[2].tolist(), s[3], W, H)
    assert int(count[0]) == int(want.sum()) > 50
    # analytic size of the alpha >= 1/255 disc: power >= ln(1 / (255 o)) <=> r^2 <= 2 sigma^2 ln(255 o)
    r2 = 2 * 9.0 * math.log(255 * 0.8)
    assert abs(int(count[0]) - math.pi * r2) < 2 * math.pi * math.sqrt(r2) + 4


def test_restatement_stacked_opaque_gaussians_stop_at_t_1e4():
    W, H = 32, 32
    front = _splat(16.0, 16.0, 4.0, 0.995, 1.0)
    back = _splat(16.0, 16.0, 4.0, 0.995, 2.0)
    count, _, _ = CR.count_blend(_g([front, back]), W, H, torch.zeros(3))
    alone, _, _ = CR.count_blend(_g([back]), W, H, torch.zeros(3))
    # closed form: the back splat is blended at a pixel iff it passes alone and (1 - a_front)(1 - a_back) >= 1e-4
    py, px = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    d2 = (np.float32(16.0) - px) ** 2 + (np.float32(16.0) - py) ** 2
    power = np.float32(-0.5) * (d2 / np.float32(16.0))
    a = np.minimum(np.float32(0.99), np.float32(0.995) * np.exp(power))
    passes = a >= np.float32(1.0 / 255.0)
    t_front = np.where(passes, np.float32(1.0) - a, np.float32(1.0))
    back_blended = passes & ~((t_front * (np.float32(1.0) - a)) < np.float32(1e-4))
    assert int(count[0]) == int(passes.sum())
    assert int(count[1]) == int(back_blended.sum())
    assert int(count[1]) < int(alone[0]) == int(passes.sum())        # the centre pixels are saturated by the front splat


def test_restatement_flat_gaussian_counts_at_full_opacity():
    """A flat Gaussian (a needle seen side-on: the undilated 2-D determinant is ~4e-10, which RaDe-GS clamps to det0 = 1e-6 and then
    zeroes the opacity for): the vanilla preprocess dilates it and renders it at its full opacity."""
    from igs_amd.camera import Camera
    W = H = 64
    c2w = torch.eye(4)
    c2w[2, 3] = -5.0
    fov = math.radians(50.0)
    cam = Camera.from_c2w(c2w, (fov, fov), (H, W))
    means = torch.tensor([[0.0, 0.0, 0.0]])
    cov3D = torch.tensor([[0.01, 0.0, 0.0, 1e-12, 0.0, 0.01]])      # a needle along x (depth variance: invisible on the axis)
    op = torch.tensor([[0.9]])
    args = (means, None, torch.ones(1, 3), op, None, None, cov3D, 1.0, cam.world_view_transform, cam.full_proj_transform,
            cam.camera_center, cam.tanfovx, cam.tanfovy)
    from oracle.torch_oracle import per_gaussian
    g0 = per_gaussian(*args, 0.3, W, H, 0)
    a, b, c = g0["cov2"][0].tolist()
    assert abs(a * c - b * b) < 1e-6 and float(g0["coef"][0]) == 0.0        # RaDe-GS: opacity x 0
    count, score, color, radii, g = CR.count_pass(*args, W, H, 0, torch.zeros(3))
    assert float(g["opacity"][0]) == pytest.approx(0.9) and int(radii[0]) > 0
    want = CR.closed_form_single(g["xy"][0].tolist(), g["conic"][0].tolist(), 0.9, W, H)
    assert int(count[0]) == int(want.sum()) > 0
    assert float(score[0]) == float(count[0]) * float(torch.tensor(0.9))
