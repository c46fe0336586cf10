"""The compress rasterizer's count pass on the GPU (diff_gaussian_rasterization_compress, igs_rast_count_gaussians) against the
restatement of tests/compress_restatement.py, across the binning paths, and in compress.py's pruning flow."""
import math

import pytest
import torch

import compress_restatement as CR
from igs_amd.camera import Camera
from igs_amd.scenes import activate, cfg1_scene, sear_steak_like_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _gpu_count(a, cam, bg, degree=3, colors=False, cov=False, scale_modifier=1.0, prefiltered=False):
    from diff_gaussian_rasterization_compress import _C
    e = torch.Tensor([])
    d = lambda t: t.to(DEV)
    cols = d(a["colors"]) if colors else e
    cov3D = d(a["cov3D"]) if cov else e
    sh = e if colors else d(a["shs"])
    sc, rot = (e, e) if cov else (d(a["scales"]), d(a["rotations"]))
    out = _C.count_gaussians(d(bg), d(a["means3D"]), cols, d(a["opacities"]), sc, rot, scale_modifier, cov3D,
                             d(cam.world_view_transform), d(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, cam.height, cam.width,
                             sh, degree, d(cam.camera_center), prefiltered, False, True)
    torch.cuda.synchronize()
    count, score, R, color, radii = out[:5]
    return dict(count=count.cpu(), score=score.cpu(), R=R, color=color.cpu(), radii=radii.cpu())


def _restated(a, cam, bg, degree=3, colors=False, cov=False, scale_modifier=1.0):
    count, score, color, radii, g = CR.count_pass(
        a["means3D"], None if colors else a["shs"], a["colors"] if colors else None, a["opacities"],
        None if cov else a["scales"], None if cov else a["rotations"], a["cov3D"] if cov else None, scale_modifier,
        cam.world_view_transform.cpu(), cam.full_proj_transform.cpu(), cam.camera_center.cpu(), cam.tanfovx, cam.tanfovy,
        cam.width, cam.height, degree, bg)
    return dict(count=count, score=score, color=color, radii=radii)


def _activated(raw, seed=5):
    a = {k: v.detach() for k, v in activate(raw).items()}
    g = torch.Generator().manual_seed(seed)
    P = a["means3D"].shape[0]
    a["colors"] = torch.rand(P, 3, generator=g)
    # the 3-D covariance the preprocess would build from scale / rotation (upper triangle, row-major)
    q = torch.nn.functional.normalize(a["rotations"], dim=1)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Mm = R * a["scales"][:, None, :]
    S = Mm @ Mm.transpose(1, 2)
    a["cov3D"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()
    a["opacities"] = a["opacities"].reshape(-1, 1)
    return a


def _check_parity(got, ref, opac):
    assert torch.equal(got["radii"], ref["radii"]), int((got["radii"] != ref["radii"]).sum())
    dc = (got["count"].long() - ref["count"]).abs()
    total = int(ref["count"].sum())
    assert total > 0
    assert int(dc.sum()) <= max(4, 1e-4 * total), (int(dc.sum()), total)
    vis = ref["radii"] > 0
    exact = float((dc[vis] == 0).float().mean())
    assert exact >= 0.995, exact
    assert torch.equal(got["score"], got["count"].float() * opac.reshape(-1).float())      # bitwise: count x opacity, rounded once
    # image: 1e-4 except where a splat flipped at a threshold (alpha vs 1/255, T vs 1e-4: __expf against exp).  At most 0.01 % of the
    # pixels -- or, in a scene dense enough to have more, as many as the count says flipped (each flip moves one count by one); a flip
    # moves a pixel by at most alpha T < 1/255 per channel
    err = (got["color"] - ref["color"]).abs().amax(0)
    n_bad = int((err > 1e-4).sum())
    assert n_bad <= max(1, int(1e-4 * err.numel()), int(dc.sum())), (n_bad, int(dc.sum()), float(err.max()))
    assert float(err.max()) < 1.0 / 255.0, float(err.max())


def _cfg1(P, size):
    raw, cams, _ = cfg1_scene(P=P, size=size)
    return _activated(raw), cams[0]


@pytest.mark.parametrize("variant", ["deg0", "deg1", "deg2", "deg3", "colors_precomp", "cov3D_precomp", "scale_modifier"])
def test_parity_cfg1_small(variant):
    a, cam = _cfg1(2000, 128)
    bg = torch.zeros(3)
    kw = dict(degree=3)
    if variant.startswith("deg"):
        kw["degree"] = int(variant[3])
    elif variant == "colors_precomp":
        kw["colors"] = True
    elif variant == "cov3D_precomp":
        kw["cov"] = True
    else:
        kw["scale_modifier"] = 0.7
    got = _gpu_count(a, cam, bg, **kw)
    _check_parity(got, _restated(a, cam, bg, **kw), a["opacities"])


def test_parity_cfg1_10k():
    a, cam = _cfg1(10000, 256)
    bg = torch.zeros(3)
    _check_parity(_gpu_count(a, cam, bg), _restated(a, cam, bg), a["opacities"])


def test_parity_ragged_image_with_background():
    a, cam0 = _cfg1(4000, 128)
    fov = math.radians(50.0)
    cam = Camera(cam0.world_view_transform.t().contiguous(), fov, fov * 173 / 240, (173, 240))
    bg = torch.tensor([0.25, 0.5, 0.75])
    got = _gpu_count(a, cam, bg)
    ref = _restated(a, cam, bg)
    _check_parity(got, ref, a["opacities"])
    assert float(got["color"][2, 172, 239]) > 0.0


def test_prefiltered():
    from igs_amd.rasterizer import RasterizerError
    a, cam = _cfg1(2000, 128)
    bg = torch.zeros(3)
    _check_parity(_gpu_count(a, cam, bg, prefiltered=True), _restated(a, cam, bg), a["opacities"])      # nothing culled: same result
    b = {k: v.clone() for k, v in a.items()}
    b["means3D"][7] = torch.tensor([0.0, 0.0, -20.0])          # behind the camera
    with pytest.raises(RasterizerError, match="Point is filtered although prefiltered is set. This shouldn't happen!"):
        _gpu_count(b, cam, bg, prefiltered=True)


def _same(x, y):
    for k in ("count", "score", "color", "radii"):
        assert torch.equal(x[k], y[k]), k
    assert x["R"] == y["R"]


def test_binning_paths_bit_identical(monkeypatch):
    from igs_amd import _cabi
    L = _cabi.lib()
    a, cam = _cfg1(10000, 256)
    bg = torch.tensor([0.1, 0.2, 0.3])
    L.igs_rast_set_slab_hint(0)
    slab = _gpu_count(a, cam, bg)
    L.igs_rast_set_slab_hint(128)
    try:
        over = _gpu_count(a, cam, bg)
        assert L.igs_rast_get_slab_hint() > 128                  # a tile overflowed its slab and the frame was redone
    finally:
        L.igs_rast_set_slab_hint(0)
    monkeypatch.setenv("IGS_BINNING", "radix")
    radix = _gpu_count(a, cam, bg)
    monkeypatch.delenv("IGS_BINNING")
    _same(slab, over)
    _same(slab, radix)
    assert int(slab["count"].sum()) > 0


def test_deterministic():
    a, cam = _cfg1(10000, 256)
    bg = torch.zeros(3)
    _same(_gpu_count(a, cam, bg), _gpu_count(a, cam, bg))


def test_empty_and_all_culled():
    from diff_gaussian_rasterization_compress import _C
    a, cam = _cfg1(2000, 128)
    e = torch.Tensor([])
    bg = torch.tensor([0.5, 0.25, 0.125], device=DEV)
    z3 = torch.zeros(0, 3, device=DEV)
    out = _C.count_gaussians(bg, z3, e, torch.zeros(0, 1, device=DEV), z3, torch.zeros(0, 4, device=DEV), 1.0, e,
                             cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), cam.tanfovx, cam.tanfovy, 128, 128,
                             torch.zeros(0, 16, 3, device=DEV), 3, cam.camera_center.to(DEV), False, False, True)
    assert out[0].shape == (0,) and out[1].shape == (0,) and out[2] == 0 and out[4].shape == (0,)
    assert out[0].dtype == torch.int32 and out[4].dtype == torch.int32
    assert float(out[3].abs().sum()) == 0.0 and out[3].shape == (3, 128, 128)
    b = {k: v.clone() for k, v in a.items()}
    b["means3D"][:, 2] = -30.0                                     # everything behind the camera
    got = _gpu_count(b, cam, bg.cpu())
    assert got["R"] == 0 and int(got["count"].abs().sum()) == 0 and float(got["score"].abs().sum()) == 0.0
    assert int(got["radii"].abs().sum()) == 0
    assert torch.equal(got["color"], bg.cpu().reshape(3, 1, 1).expand(3, 128, 128))


def test_full_size_scene():
    from igs_amd import _cabi
    raw, cams, bg = sear_steak_like_scene()
    a = _activated(raw)
    cam = cams[0]
    _cabi.lib().igs_rast_set_slab_hint(0)
    first = _gpu_count(a, cam, bg)
    _same(first, _gpu_count(a, cam, bg))
    import os
    os.environ["IGS_BINNING"] = "radix"
    try:
        radix = _gpu_count(a, cam, bg)
    finally:
        del os.environ["IGS_BINNING"]
    _same(first, radix)
    assert first["R"] > 100000
    # parity on a 4x downscaled copy of that camera
    small = Camera(cam.world_view_transform.t().contiguous(), cam.FoVx, cam.FoVy, (cam.height // 4, cam.width // 4))
    _check_parity(_gpu_count(a, small, bg), _restated(a, small, bg), a["opacities"])


def test_prune_flow_end_to_end():
    """compress.py: prune_list over the training views through GaussianRasterizer(f_count=True), calculate_v_imp_score(v_pow=0.1),
    prune_gaussians(0.45) -- against the same flow on the restatement's scores."""
    from diff_gaussian_rasterization_compress import GaussianRasterizationSettings, GaussianRasterizer
    raw, cams, bg = sear_steak_like_scene(P=20000, n_cams=10, width=338, height=253, focal=182.5)
    a = _activated(raw)
    d = {k: v.to(DEV) for k, v in a.items()}
    gaussian_list = imp_list = None
    ref_count = ref_imp = None
    for cam in reversed(cams):                                     # prune_list pops from the end
        rs = GaussianRasterizationSettings(image_height=cam.height, image_width=cam.width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                           bg=bg.to(DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(DEV),
                                           projmatrix=cam.full_proj_transform.to(DEV), sh_degree=3, campos=cam.camera_center.to(DEV),
                                           prefiltered=False, debug=False, f_count=True)
        means2D = torch.zeros_like(d["means3D"], requires_grad=True)
        gaussians_count, important_score, color, radii = GaussianRasterizer(rs)(
            means3D=d["means3D"], means2D=means2D, shs=d["shs"], colors_precomp=None, opacities=d["opacities"], scales=d["scales"],
            rotations=d["rotations"], cov3D_precomp=None)
        gaussian_list = gaussians_count.detach() if gaussian_list is None else gaussian_list + gaussians_count.detach()
        imp_list = important_score.detach() if imp_list is None else imp_list + important_score.detach()
        ref = _restated(a, cam, bg)
        ref_count = ref["count"] if ref_count is None else ref_count + ref["count"]
        ref_imp = ref["score"] if ref_imp is None else ref_imp + ref["score"]
    torch.cuda.synchronize()
    v = CR.calculate_v_imp_score(d["scales"], imp_list, 0.1).cpu()
    v_ref = CR.calculate_v_imp_score(a["scales"], ref_imp, 0.1)
    mask, pv = CR.prune_mask(v, 0.45)
    mask_ref, pv_ref = CR.prune_mask(v_ref, 0.45)
    near = ((v - pv).abs() <= 1e-6 * pv.abs()) | ((v_ref - pv_ref).abs() <= 1e-6 * pv_ref.abs())
    counted_apart = gaussian_list.cpu().long() != ref_count        # (the parity tolerance of the count itself)
    assert int(counted_apart.sum()) <= max(4, 1e-4 * int(ref_count.sum()))
    differ = (mask != mask_ref) & ~near & ~counted_apart
    assert int(differ.sum()) == 0, int(differ.sum())
    assert 0.3 < float(mask.float().mean()) < 0.9
