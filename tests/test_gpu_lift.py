"""The multi-view anchor feature lift on the MI355X (igs_amd.motion.lift_anchor_features / grid_encoder_lift over lift.hip) against the
float64 restatement of tests/lift_restatement.py.

Tolerances are derived (lift_restatement.forward_bound / backward_bound state the operation counts), never measured.  No sample is left
out of a comparison; the generator keeps |p_cam.z| >= 0.25 (resampling the few points that violate it, negative z included), which
bounds the conditioning.  The restatement is given the float32 inverse of the poses that the product computes (torch.linalg.inv), so
the inversion error is not part of the comparison."""
import math

import pytest
import torch

import lift_restatement as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(B=1, V=4, C=128, H=128, W=128, A=8192, seed=0, dtype=torch.float32, behind=0.02):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B * V, C, H, W, generator=g).to(dtype).to(DEV)
    c2w = torch.eye(4).repeat(B * V, 1, 1)
    c2w[:, :3, :3] += 0.15 * torch.randn(B * V, 3, 3, generator=g)
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, -3.0]) + 0.3 * torch.randn(B * V, 3, generator=g)
    c2w = c2w.to(DEV)
    w2c = torch.linalg.inv(c2w)
    pts = torch.rand(B, A, 3, generator=g) * 3.0 - 1.5
    nb = int(A * behind)
    pts[:, :nb, 2] -= 5.0                                                # behind the cameras
    pts = pts.to(DEV)
    for _ in range(50):
        pc = pts.double().repeat_interleave(V, 0) @ w2c.double()[:, :3, :3].transpose(1, 2) + w2c.double()[:, :3, 3].unsqueeze(1)
        bad = (pc[..., 2].abs() < 0.25).reshape(B, V, A).any(1)
        n = int(bad.sum())
        if n == 0:
            break
        pts[bad] = (torch.rand(n, 3, generator=g) * 3.0 - 1.5).to(DEV)
    assert n == 0
    return feat, pts, c2w, w2c


def _intr(BV, H, W, fov=0.9):
    """[B*V, 4] with the true names: fx from the width."""
    fx, fy = W / (2 * math.tan(fov / 2)), H / (2 * math.tan(fov / 2))
    return torch.tensor([fx, fy, W / 2.0, H / 2.0], dtype=torch.float32, device=DEV).repeat(BV, 1)


def _check_forward(out, feat, pts, w2c, intr, reject=True):
    ref = LR.lift_restate(feat.double(), pts.double(), w2c.double(), intr.double())
    bound = LR.forward_bound(feat, pts, w2c, intr)
    err = (out.double() - ref).abs()
    print("forward: max err %.3e, max err / bound %.3f, max |ref| %.3f" % (err.max().item(), (err / bound).max().item(), ref.abs().max().item()))
    assert out.dtype == torch.float32 and out.shape == ref.shape
    assert (err <= bound).all()
    if reject:          # the bound is not vacuous: it rejects the same restatement with align_corners=True
        wrong = LR.lift_restate(feat.double(), pts.double(), w2c.double(), intr.double(), align_corners=True)
        assert not ((wrong - ref).abs() <= bound).all()
    return ref


@pytest.mark.parametrize("B", [1, 5])
def test_forward_shipped_shape(B):
    from igs_amd.motion import lift_anchor_features
    feat, pts, c2w, w2c = _case(B=B, seed=B)
    intr = _intr(B * 4, 128, 128)
    with torch.no_grad():
        out = lift_anchor_features(feat, pts, c2w, intr)
    assert out.shape == (B, 8192, 128) and out.permute(0, 2, 1).is_contiguous()          # a view of a [B, C, A] buffer
    ref = _check_forward(out, feat, pts, w2c, intr)
    assert (ref != 0).double().mean() > 0.3
    K = torch.zeros(B * 4, 3, 3, device=DEV)                                             # the 3 x 3 form gives the same bits
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1.0
    with torch.no_grad():
        assert torch.equal(lift_anchor_features(feat, pts, c2w.reshape(B, 4, 4, 4), K), out)
    K[0, 0, 1] = 0.5
    with pytest.raises(NotImplementedError, match="intrinsics must be"):
        lift_anchor_features(feat, pts, c2w, K)


@pytest.mark.parametrize("C", [1, 3, 127, 128, 256])
def test_forward_channel_counts(C):
    from igs_amd.motion import lift_anchor_features
    feat, pts, c2w, w2c = _case(B=2, V=3, C=C, H=40, W=56, A=5000, seed=C)
    intr = _intr(6, 40, 56)
    with torch.no_grad():
        out = lift_anchor_features(feat, pts, c2w, intr)
    _check_forward(out, feat, pts, w2c, intr)


def test_grid_encoder_lift_on_a_banded_non_square_map():
    """136 x 200 is larger than one LDS plane (two bands) and not square: GridEncoder's swapped names (fx from shape[-2]) are visible."""
    from igs_amd.motion import grid_encoder_lift
    B, V, H, W = 2, 4, 136, 200
    feat, pts, c2w, w2c = _case(B=B, V=V, C=16, H=H, W=W, A=6000, seed=7)
    fovx, fovy = 0.9, 0.7
    FOV = torch.tensor([[fovx, fovy], [0.3, 0.3]], device=DEV)                           # FOV[0] serves every example
    intr = LR.grid_encoder_intr(feat.shape, fovx, fovy, B * V).to(DEV)
    assert intr[0, 2].item() == H / 2.0 and intr[0, 3].item() == W / 2.0                 # cx from the height: the swap
    with torch.no_grad():
        out_host = grid_encoder_lift(feat, pts, None, c2w.reshape(B, V, 4, 4), fov=(fovx, fovy))
        out_dev = grid_encoder_lift(feat, pts, FOV, c2w.reshape(B, V, 4, 4))
    ref = _check_forward(out_host, feat, pts, w2c, intr.float())
    # the device path evaluates fov2focal's tensor branch in float32 where FOV lies: the same operations here give its focal lengths
    focal = torch.tensor([float(H), float(W)], device=DEV) / (2 * torch.tan(FOV[0] / 2))
    intr_dev = torch.cat([focal, torch.tensor([H / 2.0, W / 2.0], device=DEV)]).repeat(B * V, 1)
    _check_forward(out_dev, feat, pts, w2c, intr_dev, reject=False)
    true_names = LR.lift_restate(feat.double(), pts.double(), w2c.double(), _intr(B * V, H, W).double())
    assert not ((true_names - ref).abs() <= LR.forward_bound(feat, pts, w2c, intr.float())).all()


def test_forward_half_strided_channels_last_side_stream_and_empty():
    from igs_amd.motion import lift_anchor_features
    feat, pts, c2w, w2c = _case(B=2, V=4, C=24, H=64, W=48, A=3000, seed=3, dtype=torch.float16)
    intr = _intr(8, 64, 48)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        out = lift_anchor_features(feat, pts, c2w, intr)
    s.synchronize()
    _check_forward(out, feat, pts, w2c, intr)
    with torch.no_grad():
        big = torch.randn(8, 40, 64, 48, device=DEV).half()
        big[:, 5:29] = feat
        view = big[:, 5:29]                                                              # a slice of c: read in place
        assert not view.is_contiguous()
        assert torch.equal(lift_anchor_features(view, pts, c2w, intr), out)
        wide = torch.zeros(8, 24, 64, 50, device=DEV).half()
        wide[..., :48] = feat
        assert torch.equal(lift_anchor_features(wide[..., :48], pts, c2w, intr), out)    # rows not contiguous: copied, same bits
        cl = feat.contiguous(memory_format=torch.channels_last)
        assert cl.stride(1) == 1
        assert torch.equal(lift_anchor_features(cl, pts, c2w, intr), out)                # channels-last: copied to NCHW (no own kernels)
        e = lift_anchor_features(feat, pts[:, :0], c2w, intr)
        assert e.shape == (2, 0, 24)


def test_outside_behind_and_non_finite_samples():
    from igs_amd.motion import lift_anchor_features
    V, H, W = 2, 32, 32
    feat = torch.randn(V, 4, H, W, device=DEV)
    c2w = torch.eye(4, device=DEV).repeat(V, 1, 1)
    intr = torch.tensor([16.0, 16.0, 16.0, 16.0], device=DEV).repeat(V, 1)               # ix = 16 x / z + 15.5
    far = torch.tensor([[[40.0, 0.0, 1.0], [0.0, -40.0, 1.0], [3.0, 3.0, 1.0], [-1.04, 0.0, 1.0]]], device=DEV)     # ix = -1.14: outside
    with torch.no_grad():
        assert (lift_anchor_features(feat, far, c2w, intr) == 0).all()                   # exact zeros
        # z < 0: divided like any other; (0.5, 0.25, -1) lands where (-0.5, -0.25, 1) does
        a = lift_anchor_features(feat, torch.tensor([[[0.5, 0.25, -1.0]]], device=DEV), c2w, intr)
        b = lift_anchor_features(feat, torch.tensor([[[-0.5, -0.25, 1.0]]], device=DEV), c2w, intr)
        assert torch.equal(a, b) and (a != 0).any()
        # z = 0, NaN and overflow: zero from that view; a finite view still counts (mean over both)
        c2 = c2w.clone()
        c2[1, 2, 3] = 1.0                                                                # view 1 sees z + 1
        pts = torch.tensor([[[0.1, 0.1, 0.0], [float("nan"), 0.0, 1.0], [1e38, 1e38, 1e-38], [0.0, 0.0, -1.0]]], device=DEV)
        w2 = torch.linalg.inv(c2)
        out = lift_anchor_features(feat, pts, c2, intr)
        assert torch.isfinite(out).all()
        ref = LR.lift_restate(feat[1:].double(), pts[:, :1].double(), w2[1:].double(), intr[1:].double()) / 2
        bound = LR.forward_bound(feat[1:], pts[:, :1], w2[1:], intr[1:])                 # (of the one finite view, not halved)
        assert ((out[:, :1].double() - ref).abs() <= bound).all() and (out[:, 0] != 0).any()     # view 0: z = 0 adds zero; view 1 counts
        assert (out[:, 1] == 0).all() and (out[:, 2] == 0).all()


def test_bit_equality_on_exact_inputs():
    """Identity poses, dyadic focal lengths, coordinates and features: every sample is a pixel centre or a cell midpoint, every product
    and partial sum is exact in float32, V = 2 divides exactly: bit-equal to float64, forward and backward."""
    from igs_amd.motion import lift_anchor_features
    g = torch.Generator().manual_seed(5)
    V, C, H, W, A = 2, 6, 16, 16, 4000
    feat = (torch.randint(-64, 64, (V, C, H, W), generator=g).float() / 8).to(DEV).requires_grad_(True)
    c2w = torch.eye(4, device=DEV).repeat(V, 1, 1)
    intr = torch.tensor([8.0, 8.0, 8.0, 8.0], device=DEV).repeat(V, 1)                   # ix = 8 x + 7.5 at z = 1
    pts = torch.cat([torch.randint(-20, 20, (1, A, 2), generator=g).float() / 16, torch.ones(1, A, 1)], -1).to(DEV)
    gout = (torch.randint(-8, 8, (1, A, C), generator=g).float() / 4).to(DEV)
    out = lift_anchor_features(feat, pts, c2w, intr)
    out.backward(gout)
    f64 = feat.detach().double().requires_grad_(True)
    ref = LR.lift_restate(f64, pts.double(), c2w.double(), intr.double())
    ref.backward(gout.double())
    assert torch.equal(out.double(), ref) and (ref != 0).any()
    assert torch.equal(feat.grad.double(), f64.grad)


def _backward(feat, pts, c2w, intr, gout):
    from igs_amd.motion import lift_anchor_features
    x = feat.detach().clone().requires_grad_(True)
    lift_anchor_features(x, pts, c2w, intr).backward(gout)
    return x.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_backward_against_float64_twice(dtype):
    # (A > 8192: d out read from global memory; 8192 is the last A that stages it in LDS, 8193 the first that does not)
    for (B, V, C, H, W, A) in ((1, 4, 128, 128, 128, 8192), (2, 3, 7, 136, 200, 9000), (1, 2, 3, 24, 20, 8193)):
        feat, pts, c2w, w2c = _case(B=B, V=V, C=C, H=H, W=W, A=A, seed=11 + C, dtype=dtype)
        intr = _intr(B * V, H, W)
        gout = torch.randn(B, A, C, generator=torch.Generator().manual_seed(1)).to(DEV)
        with torch.no_grad():                                                            # (the banded forward of either dtype: 136 x 200)
            from igs_amd.motion import lift_anchor_features
            _check_forward(lift_anchor_features(feat, pts, c2w, intr), feat, pts, w2c, intr, reject=False)
        d1 = _backward(feat, pts, c2w, intr, gout)
        d2 = _backward(feat, pts, c2w, intr, gout)
        assert d1.dtype == dtype and d1.shape == feat.shape
        assert torch.equal(d1, d2)                                                       # fixed summation order: bitwise reproducible
        d3 = _backward(feat, pts, c2w, intr, gout.permute(0, 2, 1).contiguous().permute(0, 2, 1))    # d out laid out [B, C, A]
        assert torch.equal(d1, d3)
        f64 = feat.detach().double().requires_grad_(True)
        LR.lift_restate(f64, pts.double(), w2c.double(), intr.double()).backward(gout.double())
        tol = LR.backward_bound(gout, pts, w2c, intr, H, W, half=dtype == torch.float16, ref=f64.grad)
        err = (d1.double() - f64.grad).abs()
        worst = (err / tol).argmax()
        print("backward %s: max err %.3e, max err / bound %.3f (there: native %.6e, float64 %.6e, bound %.3e)" % (
            dtype, err.max().item(), (err / tol).max().item(), d1.flatten()[worst].item(), f64.grad.flatten()[worst].item(),
            tol.flatten()[worst].item()))
        assert (err <= tol).all()
        assert (f64.grad != 0).double().mean() > 0.2


def test_backward_writes_every_element():
    """d feat comes from torch.empty: poison the allocator's block first; pixels no sample touches must read exactly zero."""
    from igs_amd import _cabi
    E = _cabi.ext()
    B, V, C, H, W, A = 1, 2, 5, 64, 64, 50                                               # 50 samples on 4096 pixels: almost all untouched
    feat, pts, c2w, w2c = _case(B=B, V=V, C=C, H=H, W=W, A=A, seed=2)
    intr = _intr(V, H, W)
    gout = torch.randn(B, A, C, device=DEV)
    for _ in range(3):
        poison = torch.full((V, C, H, W), float("nan"), device=DEV)
        del poison
        d = E.motion_lift_bwd(gout.permute(0, 2, 1), pts, w2c, intr, H, W, False)
        assert torch.isfinite(d).all()
        assert (d == 0).double().mean() > 0.8 and (d != 0).any()
    z = E.motion_lift_bwd(gout[:, :0].permute(0, 2, 1), pts[:, :0], w2c, intr, H, W, False)        # A = 0: all zero
    assert z.shape == (V, C, H, W) and (z == 0).all()
    far = pts.clone()
    far[..., 0] = 1e4                                                                    # every sample outside: all zero, and quickly
    assert (E.motion_lift_bwd(gout.permute(0, 2, 1), far, w2c, intr, H, W, False) == 0).all()


def test_no_grad_saves_nothing_and_point_gradients_are_refused():
    from igs_amd.motion import lift_anchor_features
    feat, pts, c2w, w2c = _case(B=1, V=2, C=4, H=16, W=16, A=100, seed=4)
    intr = _intr(2, 16, 16)
    x = feat.clone().requires_grad_(True)
    with torch.no_grad():
        assert lift_anchor_features(x, pts, c2w, intr).grad_fn is None
    assert lift_anchor_features(x, pts, c2w, intr).grad_fn is not None
    with pytest.raises(NotImplementedError, match="anchor_points"):
        lift_anchor_features(x, pts.clone().requires_grad_(True), c2w, intr)
    with pytest.raises(NotImplementedError, match="c2ws"):
        lift_anchor_features(x, pts, c2w.clone().requires_grad_(True), intr)


def test_chain_anchor_graph_lift_to_rasterizer():
    """anchor_graph -> grid_encoder_lift -> Linear -> query_ir_grid -> MLP -> deform -> rasterizer -> L1: the gradient arriving at the
    lift's output is captured with a hook, and motion_feature.grad is compared with the restatement's backward of that same gradient."""
    import diff_gaussian_rasterization_rade_clamp as DC
    from igs_amd import motion
    from igs_amd.anchors import anchor_graph
    from igs_amd.scenes import cfg1_scene
    raw, cams, bg = cfg1_scene(P=10000, size=128)
    cam = cams[0].to(DEV)
    xyz = raw["xyz"].to(DEV)
    bbox = torch.tensor([[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]], device=DEV)
    anchors, masks, weights, nb, _ = anchor_graph([xyz], bbox, anchor_size=512, k=8, start_idx=[0])
    g = torch.Generator().manual_seed(0)
    V, C, H, W = 4, 16, 32, 32
    mf = (torch.randn(V, C, H, W, generator=g) * 0.5).to(DEV).requires_grad_(True)
    c2w = torch.eye(4).repeat(V, 1, 1)
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, -4.0]) + 0.2 * torch.randn(V, 3, generator=g)
    c2w = c2w.to(DEV)
    fov = (0.8, 0.8)
    W0 = (torch.randn(C, 32, generator=g) / C ** 0.5).to(DEV)
    W1 = (torch.randn(32, 64, generator=g) / 32 ** 0.5).to(DEV)
    W2 = (torch.randn(64, 7, generator=g) * 0.02).to(DEV)
    grids = motion.grid_encoder_lift(mf, anchors, None, c2w.reshape(1, V, 4, 4), fov=fov)
    caught = []
    grids.register_hook(lambda t: caught.append(t.detach().clone()))
    feats = grids @ W0                                                                   # the Linear standing in for the anchor transformer
    (f,) = motion.query_ir_grid(feats, weights, nb, counts=[masks[0].numel()])
    h = torch.nn.functional.silu(f @ W1) @ W2
    rot = raw["rotation"].to(DEV)
    xo, ro = motion.deform_xyz_rotation(xyz, rot, masks[0], h[:, :3] * 0.05, h[:, 3:] + torch.tensor([1.0, 0, 0, 0], device=DEV))
    st = DC.GaussianRasterizationSettings(image_height=cam.height, image_width=cam.width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                          kernel_size=0.0, bg=bg.to(DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                                          projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False,
                                          require_depth=True, require_coord=True, debug=False)
    m2d = torch.zeros_like(xo, requires_grad=True)
    out = DC.GaussianRasterizer(raster_settings=st)(means3D=xo, means2D=m2d, opacities=torch.sigmoid(raw["opacity"].to(DEV)),
                                                    shs=raw["shs"].to(DEV), scales=torch.exp(raw["scaling"].to(DEV)),
                                                    rotations=torch.nn.functional.normalize(ro))
    (out[0] - 0.25).abs().mean().backward()
    assert len(caught) == 1 and mf.grad is not None and (mf.grad != 0).any()
    gout = caught[0]
    w2c = torch.linalg.inv(c2w)
    intr = LR.grid_encoder_intr(mf.shape, fov[0], fov[1], V).float().to(DEV)
    f64 = mf.detach().double().requires_grad_(True)
    ref = LR.lift_restate(f64, anchors.double(), w2c.double(), intr.double())
    ref.backward(gout.double())
    assert ((grids.detach().double() - ref.detach()).abs() <= LR.forward_bound(mf.detach(), anchors, w2c, intr)).all()
    tol = LR.backward_bound(gout, anchors, w2c, intr, H, W)
    assert ((mf.grad.double() - f64.grad).abs() <= tol).all()
