"""Host-side checks of the multi-view entry points (igs_rast_forward_views / igs_rast_backward_views, rasterizer.rasterize_views): what is
exported and declared, what is refused before any GPU work, the restatement the GPU tests certify against, and the new kernel's
code object.  No GPU needed."""
import ctypes as C
import math
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("igs_rast_views_max", "igs_rast_forward_views", "igs_rast_backward_views")


def test_entry_points_are_exported_declared_and_bound():
    from igs_amd import _cabi
    L = _cabi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "igs_rast.h")).read(), flags=re.S)
    for n in NAMES:
        assert getattr(L, n) is not None
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert n in _cabi.SIGNATURES and n in _cabi.EXPORTS
    assert L.igs_rast_views_max() >= 16


def _forward_views(L, V, cams=True, users=True, P=1):
    """igs_rast_forward_views with never-dereferenced placeholder addresses everywhere but where a test puts a NULL"""
    from igs_amd import _cabi
    one = C.c_void_p(0x1000)
    cb = _cabi.ALLOC_FN(lambda user, n: None)
    users_arr = (C.c_void_p * 32)(*([0x1000] * 32)) if users else None
    cam = one if cams else None
    return L.igs_rast_forward_views(None, V, cb, users_arr, cb, users_arr, cb, users_arr, P, 0, 1, one, 8, 8, one, one, None, one, one, 1.0, one,
                                    None, cam, cam, cam, 1.0, 1.0, 0.0, 0, one, one, one, one, one, one, one, one, (C.c_int * 32)(), 1, 1, 0)


def _backward_views(L, V, cams=True, scratch=True, P=1):
    one = C.c_void_p(0x1000)
    cam = one if cams else None
    bufs = (C.c_void_p * 32)(*([0x1000] * 32)) if scratch else None
    return L.igs_rast_backward_views(None, V, P, 0, 1, (C.c_int * 32)(), one, 8, 8, one, one, None, one, one, 1.0, one, None, cam, cam, cam, 1.0, 1.0,
                                     0.0, one, one, bufs, bufs, bufs, one, None, None, None, None, None, None, one if scratch else None,
                                     one, one, one, one, one, one, one, one, 1, 1, 0)


def test_c_abi_refuses_bad_view_counts_and_null_arrays_before_any_hip_call():
    """None of these may reach HIP: there is no device here, and the placeholder addresses must never be read."""
    from igs_amd import _cabi
    L = _cabi.lib()
    vmax = L.igs_rast_views_max()
    for call in (_forward_views, _backward_views):
        for V in (0, -1, vmax + 1):
            assert call(L, V) == E_INVALID, (call.__name__, V)
            assert b"igs_rast_views_max" in L.igs_rast_last_error()
        assert call(L, 3, cams=False) == E_INVALID
        assert b"camera" in L.igs_rast_last_error()
    assert _forward_views(L, 3, users=False) == E_INVALID
    assert b"scratch" in L.igs_rast_last_error()
    assert _backward_views(L, 3, scratch=False) == E_INVALID
    assert b"scratch" in L.igs_rast_last_error()
    # a NULL entry inside the per-view arrays
    one = C.c_void_p(0x1000)
    holes = (C.c_void_p * 32)(*([0x1000, 0] + [0x1000] * 30))
    rc = L.igs_rast_backward_views(None, 3, 1, 0, 1, (C.c_int * 32)(), one, 8, 8, one, one, None, one, one, 1.0, one, None, one, one, one, 1.0, 1.0,
                                   0.0, one, one, holes, holes, holes, one, None, None, None, None, None, None, one,
                                   one, one, one, one, one, one, one, one, 1, 1, 0)
    assert rc == E_INVALID and b"scratch" in L.igs_rast_last_error()
    # P == 0: nothing to do, num_rendered zeroed
    nr = (C.c_int * 4)(7, 7, 7, 7)
    users = (C.c_void_p * 4)()
    cb = _cabi.ALLOC_FN(lambda user, n: None)
    assert L.igs_rast_forward_views(None, 3, cb, users, cb, users, cb, users, 0, 0, 1, one, 8, 8, one, one, None, one, one, 1.0, one, None, one, one,
                                    one, 1.0, 1.0, 0.0, 0, one, one, one, one, one, one, one, one, nr, 1, 1, 0) == 0
    assert list(nr) == [0, 0, 0, 7]


def _settings(R, H=8, W=8):
    return R.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, kernel_size=0.0, bg=torch.zeros(3),
                                           scale_modifier=1.0, viewmatrix=torch.Tensor([]), projmatrix=torch.Tensor([]), sh_degree=0,
                                           campos=torch.Tensor([]), prefiltered=False, require_depth=True, require_coord=True, debug=False)


def test_python_layer_refusals():
    from igs_amd import rasterizer as R
    E = torch.Tensor([])
    P, V = 5, 3
    good = dict(means3D=torch.zeros(P, 3), sh=torch.zeros(P, 1, 3), colors_precomp=E, opacities=torch.ones(P, 1), scales=torch.ones(P, 3),
                rotations=torch.ones(P, 4), cov3Ds_precomp=E, settings=_settings(R), viewmatrices=torch.eye(4).repeat(V, 1, 1),
                projmatrices=torch.eye(4).repeat(V, 1, 1), camposes=torch.zeros(V, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # CPU tensors, everything else in order
        R.rasterize_views(**good)
    bad = [dict(viewmatrices=torch.eye(4).repeat(0, 1, 1)),                               # V = 0
           dict(viewmatrices=torch.eye(4).repeat(R.views_max() + 1, 1, 1)),               # V = max + 1
           dict(projmatrices=torch.eye(4).repeat(V + 1, 1, 1)),                           # V differs between the arguments
           dict(camposes=torch.zeros(V - 1, 3)),
           dict(opacities=torch.ones(P + 1, 1)),                                          # P differs
           dict(sh=torch.zeros(P - 1, 1, 3)),
           dict(means2D=torch.zeros(V, P + 1, 3)),
           dict(means2D=torch.zeros(V + 1, P, 3)),
           dict(means3D=torch.zeros(P, 3, dtype=torch.float64)),                          # not float32
           dict(viewmatrices=torch.eye(4, dtype=torch.float16).repeat(V, 1, 1))]
    for change in bad:
        with pytest.raises(ValueError):
            R.rasterize_views(**{**good, **change})
    # the compiled module states the same as RuntimeError (RasterizerError), CPU tensors included
    def c_call(**change):
        g = {**good, **change}
        return R._C._views.rasterize_views(torch.zeros(3), g["means3D"], E, g["opacities"], g["scales"], g["rotations"], 1.0, E, g["viewmatrices"],
                                    g["projmatrices"], 1.0, 1.0, 0.0, 8, 8, g["sh"], 0, g["camposes"], False, True, True, False,
                                    scratch=[R.ScratchSet(torch.device("cpu"), False) for _ in range(g["viewmatrices"].size(0))])
    for change in (dict(viewmatrices=torch.eye(4).repeat(R.views_max() + 1, 1, 1)), dict(camposes=torch.zeros(V - 1, 3)),
                   dict(opacities=torch.ones(P + 1, 1)), dict(means3D=torch.zeros(P, 3, dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            c_call(**change)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        c_call()


def test_oracle_views_equals_float64_autograd_of_the_summed_loss(monkeypatch):
    """Pins the restatement itself: on 40 Gaussians at 32 x 32 under 3 cameras, the float64 sum of `oracle_views` is the gradient that
    float64 autograd gives for the summed loss through oracle/torch_oracle.render -- to the agreement test_oracle_autograd.py asks of one
    view, under its conditions: world scaled x30 (the eigen-solver's absolute threshold) and the d(coef)/d(cov2D) terms left out on
    both sides (oracle flag 1, detach_coef): the reference evaluates them with dL_dconic.w in place of the opacity, which no autograd
    reproduces.  `oracle_all` sets the oracle's flags itself, so flag 1 is OR-ed into whatever it sets for the length of this test."""
    from oracle import c_oracle
    set_flags = c_oracle.set_flags
    monkeypatch.setattr(c_oracle, "set_flags", lambda f: set_flags(f | 1))
    try:
        _pin_oracle_views()
    finally:
        set_flags(0)


def _pin_oracle_views():
    from igs_amd.camera import Camera
    from igs_amd.scenes import activate
    from oracle import torch_oracle as to
    import test_oracle_autograd as oa
    from views_restatement import oracle_views
    dt, size, scale = torch.float64, 32, 30.0
    raw, _ = oa._scene(40, size, dt, world_scale=scale, tilt=0.2)
    # Footprints x3: at 32 x 32 the scene's Gaussians are otherwise under a pixel wide, where the absolute epsilons of the reference's conic
    # backward (1e-7 in pixels^4, 1e-6 beside the determinants) are no longer small -- ONE view's oracle is then 1e-2 from autograd on
    # scales and rotations (measured; at x3 every view below is within 2e-4, the frustum clamp's edge cases avoided by the camera choice).
    raw["scaling"] = raw["scaling"] + math.log(3.0)
    fov = math.radians(50.0)
    cams = []
    for tilt, dx in ((0.2, 0.3), (-0.15, -0.1), (0.0, 0.0)):
        c2w = torch.eye(4, dtype=dt)
        c2w[2, 3], c2w[0, 3] = -5.0 * scale, dx * scale
        c, s = math.cos(tilt), math.sin(tilt)
        c2w[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=dt)
        cams.append(Camera.from_c2w(c2w, (fov, fov), (size, size)))
    bg = torch.tensor([0.3, 0.5, 0.7], dtype=dt)
    grads = [oa._grads(size, np.float64, seed=v) for v in range(3)]
    a = {k: v.detach() for k, v in activate(raw).items()}
    ob = oracle_views(a, cams, bg, grads, samples=1, exp_samples=1)
    assert min(ob["nr"]) > 0
    g_c = oa._chain_to_raw(raw, ob["g64"])
    leaf = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    al = activate(leaf)
    loss = 0.0
    for cam, g in zip(cams, grads):
        out = to.render(al["means3D"], al["shs"], None, al["opacities"], al["scales"], al["rotations"], None, 1.0, cam.world_view_transform,
                        cam.full_proj_transform, cam.camera_center, cam.tanfovx, cam.tanfovy, 0.0, cam.width, cam.height, 3, bg,
                        require_coord=True, require_depth=True, detach_coef=True)
        loss = loss + sum((out[k] * torch.from_numpy(g[k])).sum() for k in oa.KEYS)
    loss.backward()
    for k, v in leaf.items():
        r = oa._rel(v.grad.numpy(), g_c[k])
        print("oracle_views against autograd, %s: worst %.3g, beyond 1e-4 %.4f" % (k, r.max(), (r > 1e-4).mean()))
        assert r.max() < 2e-3 and (r > 1e-4).mean() < 0.02, (k, r.max(), (r > 1e-4).mean())
    # and the clamp is applied per view, before the sum
    big = max(float(np.abs(o["g64"]["sh"]).max()) for o in ob["views"])
    ob_c = oracle_views(a, cams, bg, grads, clamp=0.5 * big, samples=1, exp_samples=1)
    want = sum(np.clip(o["g64"]["sh"], -0.5 * big, 0.5 * big) for o in ob["views"])
    np.testing.assert_array_equal(ob_c["g64"]["sh"], want)
    np.testing.assert_array_equal(ob_c["g64"]["colors"], ob["g64"]["colors"])


def test_views_kernel_uses_no_scratch():
    """geom_bwd_views_kernel's code object, read the way tests/test_geom_bwd_resources.py reads geom_bwd_kernel's: no private memory (the
    48 SH sums and the per-view structs must stay in registers).  VGPRs and LDS are printed for DESIGN.md, not bounded."""
    from test_geom_bwd_resources import kernel_metadata
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    tmp, cos = A.code_objects(build.LIB)
    try:
        found = {n: md for co in cos for n, md in kernel_metadata(co).items() if "geom_bwd_views_kernel" in n}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(found) == 1, sorted(found)
    for name, md in found.items():
        print("%s: %s VGPRs, %s SGPRs, %s bytes of LDS, %s bytes of scratch per lane"
              % (name, md[".vgpr_count"], md[".sgpr_count"], md[".group_segment_fixed_size"], md[".private_segment_fixed_size"]))
        assert int(md[".private_segment_fixed_size"]) == 0, (name, md[".private_segment_fixed_size"])
