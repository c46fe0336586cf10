"""V views of one Gaussian set in one call (rasterizer.rasterize_views, igs_rast_forward_views / igs_rast_backward_views) on the GPU.

Forward: every view's images, radii and instance count are the single-view call's, bit for bit.  Backward: the summed gradients carry
the every-element certificate of tests/certificate.py against `views_restatement.oracle_views` -- the per-view oracle results added up,
each clamped first in the clamp variant -- with the parameters `certify_grads` uses for the feature branches; the per-view
dL_dmeans2D is certified against each view's own oracle.  Scene: cfg1_scene(P=1500, size=96), whose one camera is joined by two more
of the same size and field of view looking at the scene from the side, and by `away`, the first camera turned round."""
import math

import numpy as np
import pytest
import torch

import certificate as cert
from views_restatement import oracle_views, sum_views, certify_views
from igs_amd.camera import Camera, look_at_c2w, render_views
from igs_amd.scenes import cfg1_scene, activate

pytestmark = pytest.mark.gpu

KEYS = cert.KEYS
E = torch.Tensor([])
BAR = dict(max_allowance_frac=0.05, oracle_factor=2.0, allowance_floor=50)      # (test_gpu_parity.certify_grads)
ORACLE = dict(samples=12, exp_samples=2)
P, SIZE = 1500, 96


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cameras(size=(SIZE, SIZE)):
    fov = math.radians(50.0)
    c2w0 = torch.eye(4)
    c2w0[2, 3] = -5.0
    turned = c2w0.clone()
    turned[0, 0], turned[2, 2] = -1.0, -1.0           # half a turn about y: looks along -z, away from the scene
    mk = lambda c2w: Camera.from_c2w(c2w, (fov, fov), size)
    return [mk(c2w0), mk(look_at_c2w((1.5, 0.5, -4.7), (0.0, 0.0, 0.0))), mk(look_at_c2w((-1.2, -0.8, -4.8), (0.0, 0.0, 0.0)))], mk(turned)


def rand_grads(shapes, seed, only=None):
    rng = np.random.default_rng(seed)
    g = {k: rng.standard_normal(shapes[k]).astype(np.float32) for k in KEYS}
    return {k: (v if only is None or k in only else None) for k, v in g.items()}


def _shapes(cam):
    return {k: ((1 if k in ("depth", "mdepth", "alpha") else 3), cam.height, cam.width) for k in KEYS}


@pytest.fixture(scope="module")
def scene():
    """The scene, the cameras and every oracle result the tests share (the CPU oracle runs once per view and set of upstream gradients)."""
    raw, _, bg = cfg1_scene(P=P, size=SIZE)
    bg = torch.tensor([0.2, 0.4, 0.6])
    cams, away = _cameras()
    a = activate(raw)
    s = dict(a=a, bg=bg, cams=cams, away=away)
    s["g_full"] = [rand_grads(_shapes(c), 10 + v) for v, c in enumerate(cams)]
    s["g_colour"] = [rand_grads(_shapes(c), 20 + v, only=("color",)) for v, c in enumerate(cams)]
    s["g_away"] = rand_grads(_shapes(away), 30)
    s["o_full"] = [cert.oracle_all(a, c, bg, g, **ORACLE) for c, g in zip(cams, s["g_full"])]
    s["o_colour"] = [cert.oracle_all(a, c, bg, g, **ORACLE) for c, g in zip(cams, s["g_colour"])]
    s["o_away"] = cert.oracle_all(a, away, bg, s["g_away"], **ORACLE)
    return s


def _mats(cams, dev):
    return (torch.stack([c.world_view_transform for c in cams]).to(dev), torch.stack([c.full_proj_transform for c in cams]).to(dev),
            torch.stack([c.camera_center for c in cams]).to(dev))


def views_forward(a, cams, bg, dev, req=(True, True), deg=3):
    """_C._views.rasterize_views with fresh scratch sets: (the module's tuple, device inputs, camera stacks, scratch sets)"""
    from igs_amd import rasterizer as R
    ad = {k: v.to(dev) for k, v in a.items()}
    Vm, Pm, Cc = _mats(cams, dev)
    ss = [R.ScratchSet(dev, True) for _ in cams]
    out = R._C._views.rasterize_views(bg.to(dev), ad["means3D"], E, ad["opacities"], ad["scales"], ad["rotations"], 1.0, E, Vm, Pm, cams[0].tanfovx,
                               cams[0].tanfovy, 0.0, cams[0].height, cams[0].width, ad["shs"], deg, Cc, False, req[0], req[1], False, scratch=ss)
    return out, ad, (Vm, Pm, Cc), ss


def views_backward(fwd, cams, bg, dev, grads, req=(True, True), deg=3, clamp=0.0, nan_report=0):
    """_C._views.rasterize_views_backward on the result of views_forward: the eight gradients in GNAMES order (means2D [V, P, 3])"""
    from igs_amd import rasterizer as R
    out, ad, (Vm, Pm, Cc), ss = fwd
    nr, color, coord, mcoord, alpha, normal, depth, mdepth, radii = out
    up = [None if grads[0][k] is None else torch.from_numpy(np.stack([g[k] for g in grads])).to(dev) for k in KEYS]
    res = R._C._views.rasterize_views_backward(bg.to(dev), ad["means3D"], radii, E, ad["scales"], ad["rotations"], 1.0, E, Vm, Pm, cams[0].tanfovx,
                                        cams[0].tanfovy, 0.0, *up, normal, ad["shs"], deg, Cc, ss, nr, alpha, req[0], req[1], False,
                                        want_means2D=True, nan_report=nan_report, clamp=clamp)
    return res


def single_forward(a, cam, bg, dev, req=(True, True)):
    from igs_amd import rasterizer as R
    ad = {k: v.to(dev) for k, v in a.items()}
    return R.rasterize_gaussians(bg.to(dev), ad["means3D"], E, ad["opacities"], ad["scales"], ad["rotations"], 1.0, E,
                                 cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), cam.tanfovx, cam.tanfovy, 0.0, cam.height,
                                 cam.width, ad["shs"], 3, cam.camera_center.to(dev), False, req[0], req[1], False)


def assert_views_equal_single(a, cams, bg, dev):
    """every image, radii and num_rendered of every view == the single-view call with that camera, bit for bit"""
    out = views_forward(a, cams, bg, dev)[0]
    nr, color, coord, mcoord, alpha, normal, depth, mdepth, radii = out
    stacks = dict(color=color, coord=coord, mcoord=mcoord, alpha=alpha, normal=normal, depth=depth, mdepth=mdepth)
    assert len(nr) == len(cams) and radii.shape == (len(cams), a["means3D"].shape[0])
    for v, cam in enumerate(cams):
        one = single_forward(a, cam, bg, dev)
        n1, c1, co1, mc1, al1, no1, de1, md1, ra1 = one[:9]
        assert nr[v] == n1, (v, nr[v], n1)
        np.testing.assert_array_equal(radii[v].cpu().numpy(), ra1.cpu().numpy())
        for k, t in dict(color=c1, coord=co1, mcoord=mc1, alpha=al1, normal=no1, depth=de1, mdepth=md1).items():
            assert stacks[k][v].shape == t.shape, (k, stacks[k].shape, t.shape)
            np.testing.assert_array_equal(stacks[k][v].cpu().numpy(), t.cpu().numpy(), err_msg="view %d %s" % (v, k))
    return nr


# ---- 1. forward identity ----
@pytest.mark.parametrize("V", [1, 3])
def test_forward_is_the_single_view_forward_bit_for_bit(dev, scene, V):
    nr = assert_views_equal_single(scene["a"], scene["cams"][:V], scene["bg"], dev)
    assert list(nr) == [o["nr"] for o in scene["o_full"][:V]]


def test_forward_identity_on_a_ragged_image(dev, scene):
    cams, _ = _cameras(size=(72, 100))          # 100 x 72: neither side a multiple of the 16-pixel tile
    assert_views_equal_single(scene["a"], cams, scene["bg"], dev)


def test_forward_identity_through_the_global_sort(dev, scene, monkeypatch):
    """IGS_BINNING=radix: the views run one after the other through the fallback binning (and, unset again, through the slabs)"""
    monkeypatch.setenv("IGS_BINNING", "radix")
    assert_views_equal_single(scene["a"], scene["cams"], scene["bg"], dev)
    monkeypatch.delenv("IGS_BINNING")
    assert_views_equal_single(scene["a"], scene["cams"], scene["bg"], dev)


def test_overflowing_views_are_redone_and_the_slab_hint_grows(dev, scene):
    """Slabs of 256 slots: the densest tile of every view here holds more (294 .. 297 instances on the CPU oracle), so the views
    overflow, are redone with grown slabs, and the hint has grown once the call returns."""
    from igs_amd import _cabi
    L = _cabi.lib()
    ranges = [o["state"].intermediates()["ranges"] for o in scene["o_full"]]
    assert max(int((r[:, 1] - r[:, 0]).max()) for r in ranges) > 256
    before = L.igs_rast_get_slab_hint()
    try:
        L.igs_rast_set_slab_hint(256)
        assert_views_equal_single(scene["a"], scene["cams"], scene["bg"], dev)      # (its single-view calls run after the views call)
        L.igs_rast_set_slab_hint(256)
        views_forward(scene["a"], scene["cams"], scene["bg"], dev)
        assert L.igs_rast_get_slab_hint() > 256, L.igs_rast_get_slab_hint()
    finally:
        L.igs_rast_set_slab_hint(before)


# ---- 2. summed gradients ----
@pytest.mark.parametrize("V", [3, 1])
def test_summed_gradients_all_outputs(dev, scene, V):
    cams, grads = scene["cams"][:V], scene["g_full"][:V]
    fwd = views_forward(scene["a"], cams, scene["bg"], dev)
    gout = views_backward(fwd, cams, scene["bg"], dev, grads)[0]
    assert tuple(gout[0].shape) == (V, P, 3)
    certify_views(gout, sum_views(scene["o_full"][:V]), "%d views, all outputs" % V, **BAR)


def test_summed_gradients_colour_only_runs_the_compact_instance(dev, scene):
    from igs_amd import rasterizer as R
    cams, grads = scene["cams"], scene["g_colour"]
    fwd = views_forward(scene["a"], cams, scene["bg"], dev)
    gout = views_backward(fwd, cams, scene["bg"], dev, grads)[0]
    inst = R.last_backward_instance()
    assert not (inst["coord"] or inst["depth"] or inst["normal"]), inst          # the colour-only blend instance: compact accumulator rows
    certify_views(gout, sum_views(scene["o_colour"]), "3 views, colour only", **BAR)


# ---- 3. partial visibility ----
def test_a_view_that_sees_nothing_and_gaussians_no_view_sees(dev, scene):
    cams = [scene["cams"][0], scene["away"], scene["cams"][1]]
    grads = [scene["g_full"][0], scene["g_away"], scene["g_full"][1]]
    # a few Gaussians far off to the side, outside every frustum: no view sees them
    a = {k: v.clone() for k, v in scene["a"].items()}
    a["means3D"][:7] = torch.tensor([60.0, 0.0, 0.0]) + a["means3D"][:7]
    obs = [cert.oracle_all(a, c, scene["bg"], g, **ORACLE) for c, g in zip(cams, grads)]
    fwd = views_forward(a, cams, scene["bg"], dev)
    radii = fwd[0][8].cpu().numpy()
    assert (radii[1] == 0).all() and fwd[0][0][1] == 0                     # `away` sees nothing
    unseen = (radii == 0).all(0)
    assert unseen[:7].all() and (~unseen).sum() > 1000
    gout = views_backward(fwd, cams, scene["bg"], dev, grads)[0]
    certify_views(gout, sum_views(obs), "[cam0, away, cam1]", **BAR)
    m2d = gout[0].cpu().numpy()
    assert not m2d[1].any() and not np.signbit(m2d[1]).any()
    for n, t in zip(cert.GNAMES[1:], gout[1:]):
        rows = t.cpu().numpy().reshape(P, -1)[unseen]
        assert not rows.any() and not np.signbit(rows).any(), n            # exactly +0


# ---- 4. clamp before the sum ----
def test_clamp_is_applied_per_view_before_the_sum(dev, scene):
    CL = 15.0
    # the oracle first: scale the colour-only upstream gradients by a power of two until at least 1 % of the per-view sh elements are
    # beyond +-15 in float64.  dL_dsh is linear in them, so the factor can be read off the unscaled results; the oracle then runs on
    # the scaled gradients themselves (the geometry gradients are NOT linear: the reference's coef backward multiplies two of them)
    s = 1.0
    frac = lambda obs_, s_: np.mean([(np.abs(o["g64"]["sh"]) * s_ > CL).mean() for o in obs_])
    while frac(scene["o_colour"], s) < 0.01:
        s *= 2.0
        assert s < 2.0 ** 40
    grads = [{k: (None if v is None else v * np.float32(s)) for k, v in g.items()} for g in scene["g_colour"]]
    obs = [cert.oracle_all(scene["a"], c, scene["bg"], g, **ORACLE) for c, g in zip(scene["cams"], grads)]
    assert frac(obs, 1.0) >= 0.01, frac(obs, 1.0)
    ob = sum_views(obs, clamp=CL)
    # ... and the order matters there by more than the bar: clamp(sum) is outside plain + allowance of sum(clamp) somewhere
    wrong = np.clip(sum(o["g64"]["sh"] for o in obs), -CL, CL).reshape(P, -1)
    G, G32 = ob["g64"]["sh"].reshape(P, -1), ob["g32"]["sh"].reshape(P, -1)
    bar = cert.REL * np.abs(G) + cert.FLOOR * np.abs(G).max() + cert.K * np.abs(G32 - G).max(1, keepdims=True) + cert.K * ob["shift"]["sh"].reshape(P, 1)
    assert (np.abs(wrong - G) > bar).sum() > 10
    fwd = views_forward(scene["a"], scene["cams"], scene["bg"], dev)
    gout = views_backward(fwd, scene["cams"], scene["bg"], dev, grads, clamp=CL)[0]
    certify_views(gout, ob, "3 views, clamp 15 before the sum", **BAR)


# ---- 5. autograd ----
def _autograd_case(scene, dev, plant_nan=False, seed=40):
    raw, _, _ = cfg1_scene(P=P, size=SIZE)
    leaf = {k: v.to(dev).requires_grad_(True) for k, v in raw.items()}
    a = activate(leaf)
    for t in a.values():
        t.retain_grad()
    c2ws = torch.stack([torch.inverse(c.world_view_transform.transpose(0, 1)) for c in scene["cams"]]).to(dev)
    fov = math.radians(50.0)
    m2d = torch.zeros(3, P, 3, device=dev, requires_grad=True)
    out = render_views(a, c2ws, (fov, fov), (SIZE, SIZE), scene["bg"].to(dev), 3, clamp=True, means2D=m2d)
    grads = [rand_grads(_shapes(c), seed + v, only=("color", "depth")) for v, c in enumerate(scene["cams"])]
    gc = torch.from_numpy(np.stack([g["color"] for g in grads])).to(dev)
    gd = torch.from_numpy(np.stack([g["depth"] for g in grads])).to(dev)
    if plant_nan:
        gc[1, 0, SIZE // 2, SIZE // 2] = float("nan")
    loss = (out["images_pred"] * gc).sum() + (out["depth_pred"] * gd).sum()
    return leaf, a, m2d, out, grads, loss


def test_autograd_through_render_views(dev, scene):
    leaf, a, m2d, out, grads, loss = _autograd_case(scene, dev)
    assert tuple(out["images_pred"].shape) == (3, 3, SIZE, SIZE) and tuple(out["depth_pred"].shape) == (3, 1, SIZE, SIZE)
    assert tuple(out["bg_color"].shape) == (3, 3)
    loss.backward()
    assert tuple(m2d.grad.shape) == (3, P, 3)
    assert all(v.grad is not None and torch.isfinite(v.grad).all() for v in leaf.values())
    # the cameras render_views builds from the c2ws are the scene's cameras up to the rounding of two matrix inversions: the oracle gets
    # the cameras as render_views builds them
    fov = math.radians(50.0)
    c2ws = torch.stack([torch.inverse(c.world_view_transform.transpose(0, 1)) for c in scene["cams"]])
    cams = [Camera.from_c2w(c2w, (fov, fov), (SIZE, SIZE)) for c2w in c2ws]
    ob = oracle_views(scene["a"], cams, scene["bg"], grads, clamp=15.0, **ORACLE)
    for n in ("colors", "cov3D"):                                          # (no such inputs: autograd has no gradient for them)
        ob["g32"][n] = np.zeros((0,))
    gout = [m2d.grad, None, a["opacities"].grad, a["means3D"].grad, None, a["shs"].grad, a["scales"].grad, a["rotations"].grad]
    certify_views(gout, ob, "render_views, colour + depth loss", **BAR)


def test_autograd_raises_on_a_nan_in_one_views_gradient(dev, scene):
    leaf, a, m2d, out, grads, loss = _autograd_case(scene, dev, plant_nan=True)
    with pytest.raises(AssertionError):
        loss.backward()


def test_no_grad_returns_the_same_images_and_saves_nothing(dev, scene):
    from igs_amd import rasterizer as R
    ad = {k: v.to(dev) for k, v in scene["a"].items()}
    Vm, Pm, Cc = _mats(scene["cams"], dev)
    c0 = scene["cams"][0]
    st = R.GaussianRasterizationSettings(image_height=c0.height, image_width=c0.width, tanfovx=c0.tanfovx, tanfovy=c0.tanfovy, kernel_size=0.0,
                                         bg=scene["bg"].to(dev), scale_modifier=1.0, viewmatrix=E, projmatrix=E, sh_degree=3, campos=E,
                                         prefiltered=False, require_depth=True, require_coord=True, debug=False)
    leaves = {k: v.clone().requires_grad_(True) for k, v in ad.items()}
    with torch.no_grad():
        out = R.rasterize_views(leaves["means3D"], leaves["shs"], E, leaves["opacities"], leaves["scales"], leaves["rotations"], E, st, Vm, Pm, Cc)
    assert all(t.grad_fn is None and not t.requires_grad for t in out)
    ref = views_forward(scene["a"], scene["cams"], scene["bg"], dev)[0]
    _, color, coord, mcoord, alpha, normal, depth, mdepth, radii = ref
    for got, want in zip(out, (color, radii, coord, mcoord, depth, mdepth, alpha, normal)):
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    # the V scratch sets went straight back to the pool
    key = (P, SIZE, SIZE, dev, torch._C._cuda_getCurrentRawStream(dev.index))
    assert len(R._POOL.free.get(key, [])) >= 3
    # ... and with gradients enabled one node covers all views
    out = R.rasterize_views(leaves["means3D"], leaves["shs"], E, leaves["opacities"], leaves["scales"], leaves["rotations"], E, st, Vm, Pm, Cc)
    assert out[0].grad_fn is not None and out[0].grad_fn is out[4].grad_fn
    with pytest.raises(R.RasterizerError):
        R.rasterize_views(ad["means3D"].cpu(), ad["shs"].cpu(), E, ad["opacities"].cpu(), ad["scales"].cpu(), ad["rotations"].cpu(), E, st,
                          Vm.cpu(), Pm.cpu(), Cc.cpu())


def test_refused_on_a_capturing_stream(dev, scene):
    """Capture is out of scope in this version: the call says so before it launches anything (the capture itself holds one unrelated node)."""
    from igs_amd import rasterizer as R
    ad = {k: v.to(dev) for k, v in scene["a"].items()}
    Vm, Pm, Cc = _mats(scene["cams"], dev)
    c0 = scene["cams"][0]
    st = R.GaussianRasterizationSettings(image_height=c0.height, image_width=c0.width, tanfovx=c0.tanfovx, tanfovy=c0.tanfovy, kernel_size=0.0,
                                         bg=scene["bg"].to(dev), scale_modifier=1.0, viewmatrix=E, projmatrix=E, sh_degree=3, campos=E,
                                         prefiltered=False, require_depth=True, require_coord=True, debug=False)
    x = torch.zeros(8, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = x + 1.0
        with pytest.raises(R.RasterizerError, match="capture"):
            R.rasterize_views(ad["means3D"], ad["shs"], E, ad["opacities"], ad["scales"], ad["rotations"], E, st, Vm, Pm, Cc)
    torch.cuda.synchronize()
    assert y.shape == x.shape
