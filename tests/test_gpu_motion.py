"""Anchor feature interpolation and the Gaussian deform on the MI355X (igs_amd/motion.py over motion.hip) against the float64
restatement of tests/motion_restatement.py, and the chain anchor_graph -> query_ir_grid -> MLP -> deform -> rasterizer -> L1."""
import pytest
import torch

import motion_restatement as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -23


def _case(N, K, A, D, B=1, seed=0, dtype=torch.float32, pad=0.0):
    """IGS's layout for B examples: features [B, A, D], example i's columns offset by i * A, softmax weights [N, K, 1]."""
    g = torch.Generator().manual_seed(seed)
    F = torch.randn(B, A, D, generator=g).to(dtype)
    ex = torch.randint(0, B, (N,), generator=g).sort().values
    col = torch.randint(0, A, (N, K), generator=g) + ex[:, None] * A
    if pad:
        col[torch.rand(N, K, generator=g) < pad] = -1
    w = torch.softmax(torch.randn(N, K, generator=g), dim=1).unsqueeze(-1)
    return F.to(DEV), w.to(DEV), col.reshape(-1).to(DEV)


def _fwd_bound(F, w, col):
    return MR.interp_forward_bound(F, w, col)


@pytest.mark.parametrize("D", [1, 3, 4, 127, 128, 256])
@pytest.mark.parametrize("K", [1, 8, 100])
def test_forward_against_float64(D, K):
    from igs_amd.motion import interpolate_anchor_features
    for B in (1, 5):
        F, w, col = _case(700, K, 150, D, B=B, seed=D * 1000 + K + B)
        out = interpolate_anchor_features(F, w, col)
        ref = MR.interp_restate(F.reshape(-1, D).double(), w.double(), col)
        assert out.dtype == torch.float32 and out.shape == (700, D)
        assert ((out.double() - ref).abs() <= _fwd_bound(F, w, col)).all()


def test_forward_half_noncontiguous_side_stream_and_empty():
    from igs_amd.motion import interpolate_anchor_features
    F, w, col = _case(900, 8, 300, 128, B=5, seed=3, dtype=torch.float16)
    ref = MR.interp_restate(F.reshape(-1, 128).double(), w.double(), col)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = interpolate_anchor_features(F, w, col)
    s.synchronize()
    assert ((out.double() - ref).abs() <= _fwd_bound(F, w, col)).all()
    Ft = F.reshape(-1, 128).t().contiguous().t()                         # a transposed (strided) view of the same values
    wt = w.squeeze(-1).t().contiguous().t()
    ct = col.reshape(900, 8).t().contiguous().t()
    assert not Ft.is_contiguous() and not wt.is_contiguous() and not ct.is_contiguous()
    assert torch.equal(interpolate_anchor_features(Ft, wt, ct), out)
    e = interpolate_anchor_features(F, w[:0], col[:0])
    assert e.shape == (0, 128)


def test_padding_and_out_of_range_slots_contribute_nothing():
    from igs_amd.motion import interpolate_anchor_features
    F, w, col = _case(500, 8, 64, 32, seed=5)
    bad = col.clone().reshape(500, 8)
    bad[:, 3] = -1
    bad[:, 5] = 64 + 7
    bad[::7, 0] = -12345
    w2 = w.clone()
    w2[:, 3] = float("nan")                                              # a padded slot's weight is never read
    out = interpolate_anchor_features(F, w2, bad)
    ref = MR.interp_restate(F.reshape(-1, 32).double(), w.double(), bad)
    assert torch.isfinite(out).all()
    assert ((out.double() - ref).abs() <= _fwd_bound(F, w, bad)).all()
    F.requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    interpolate_anchor_features(F, wg, bad).sum().backward()
    assert (wg.grad.squeeze(-1)[:, 3] == 0).all() and (wg.grad.squeeze(-1)[:, 5] == 0).all()


def _backward_pair(F, w, col, seed=0):
    from igs_amd.motion import interpolate_anchor_features
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(w.shape[0], F.shape[-1], generator=g).to(DEV)
    Fn = F.detach().clone().requires_grad_(True)
    wn = w.detach().clone().requires_grad_(True)
    interpolate_anchor_features(Fn, wn, col).backward(dout)
    return Fn.grad, wn.grad, dout


def test_backward_against_float64():
    for (N, K, A, D, B, dt) in ((3000, 8, 200, 128, 1, torch.float32), (2000, 8, 100, 3, 5, torch.float32),
                                (1500, 100, 400, 127, 1, torch.float32), (2500, 8, 300, 64, 5, torch.float16)):
        F, w, col = _case(N, K, A, D, B=B, seed=N + D, dtype=dt, pad=0.05)
        dF, dw, dout = _backward_pair(F, w, col)
        F64 = F.detach().double().requires_grad_(True)
        w64 = w.detach().double().requires_grad_(True)
        MR.interp_restate(F64.reshape(-1, D), w64, col).backward(dout.double())
        assert dF.dtype == dt and dF.shape == F.shape and dw.shape == w.shape
        tol_F, tol_w = MR.interp_backward_bounds(MR.interp_truth_blocked(F.detach(), w.detach(), col, dout), K, D, dt == torch.float16)
        assert ((dF.double() - F64.grad).abs() <= tol_F.reshape(F.shape)).all(), (N, K, D, B)
        assert ((dw.double() - w64.grad).abs() <= tol_w.reshape(w.shape)).all(), (N, K, D, B)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("D", [64, 65, 128, 129, 256, 257, 512, 513, 1024])
def test_every_lane_group_count_at_both_ends_forward_and_backward(D, dtype):
    """interp_dv (motion.hip) gives a lane 1, 2, 4, 8 or 16 features for D up to 64, 128, 256, 512 and 1024: the row kernel and the chunk
    kernel of every count at the smallest and the largest D it serves (1 is above), in both feature dtypes, against the same bounds as the
    tests above.  Few rows and anchors: what changes with D is the lane mapping, not the lists."""
    N, K, A, B = 300, 8, 40, 2
    F, w, col = _case(N, K, A, D, B=B, seed=D + 7, dtype=dtype, pad=0.05)
    dF, dw, dout = _backward_pair(F, w, col, seed=D)
    from igs_amd.motion import interpolate_anchor_features
    out = interpolate_anchor_features(F, w, col)
    truth = MR.interp_truth_blocked(F.detach(), w.detach(), col, dout)
    tol_F, tol_w = MR.interp_backward_bounds(truth, K, D, dtype == torch.float16)
    assert out.shape == (N, D) and dF.dtype == dtype and dF.shape == F.shape and dw.shape == w.shape
    ratios = (MR.worst_ratio(out, truth["out"], _fwd_bound(F, w, col)), MR.worst_ratio(dF.reshape(-1, D), truth["dF"], tol_F),
              MR.worst_ratio(dw.reshape(N, K), truth["dw"], tol_w))
    print("D %d (%d per lane) %s: max |err| / bound forward %.3f, dF %.3f, dw %.3f" % ((D, MR.interp_dv(D), str(dtype)[6:]) + ratios))
    assert max(ratios) <= 1.0, ratios


def test_bit_equality_on_exact_inputs():
    """Integer features, power-of-two weights: every product and partial sum is exact in float32."""
    from igs_amd.motion import interpolate_anchor_features
    g = torch.Generator().manual_seed(9)
    N, K, A, D = 4000, 8, 256, 40
    F = torch.randint(-50, 50, (A, D), generator=g).float().to(DEV).requires_grad_(True)
    col = torch.randint(0, A, (N, K), generator=g).to(DEV)
    w = (2.0 ** -torch.randint(0, 6, (N, K), generator=g).float()).to(DEV).requires_grad_(True)
    dout = torch.randint(-8, 8, (N, D), generator=g).float().to(DEV)
    out = interpolate_anchor_features(F, w, col)
    out.backward(dout)
    F64, w64 = F.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    ref = MR.interp_restate(F64, w64, col)
    ref.backward(dout.double())
    assert torch.equal(out.double(), ref)
    assert torch.equal(F.grad.double(), F64.grad) and torch.equal(w.grad.double(), w64.grad)


def test_skewed_in_degree_and_reproducibility():
    """Anchor 0 receives 120 000 edges (the chunk split), the rest spread thinly; two backward runs are bit-identical."""
    N, K, A, D = 15000, 8, 1024, 128
    F, w, col = _case(N, K, A, D, seed=11)
    col = col.reshape(N, K).clone()
    col[:, :7] = 0
    col[::3, 7] = torch.randint(0, A, (col[::3].shape[0],), device=DEV)
    assert (col == 0).sum() >= 100000
    dF1, dw1, dout = _backward_pair(F, w, col, seed=1)
    dF2, dw2, _ = _backward_pair(F, w, col, seed=1)
    assert torch.equal(dF1, dF2) and torch.equal(dw1, dw2)
    F64 = F.detach().double().requires_grad_(True)
    MR.interp_restate(F64.reshape(-1, D), w.double(), col).backward(dout.double())
    flat = col.reshape(-1)
    absF = torch.zeros(A, D, dtype=torch.float64, device=DEV)
    absF.index_add_(0, flat, w.double().abs().reshape(-1, 1) * dout.double().abs().repeat_interleave(K, 0))
    deg = torch.bincount(flat, minlength=A).max().item()
    assert ((dF1.double() - F64.grad.reshape(A, D)).abs() <= deg * U * absF.reshape(A, D) + 1e-30).all()


def test_no_grad_forward_allocates_only_its_output():
    from igs_amd.motion import interpolate_anchor_features
    F, w, col = _case(100000, 8, 8192, 128, seed=2)
    with torch.no_grad():
        interpolate_anchor_features(F, w, col)                           # warm-up (module load, allocator pools)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = interpolate_anchor_features(F, w, col)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
    assert grown <= out.numel() * 4 + (1 << 20), grown


# ---------------------------------------------------------------- deform
def _deform_case(P, M, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    xyz = (torch.rand(P, 3, generator=g) * 4 - 2).to(DEV)
    rot = torch.randn(P, 4, generator=g).to(DEV)
    mask = torch.randperm(P, generator=g)[:M].to(DEV)
    dx = (torch.randn(M, 3, generator=g) * 0.01).to(dtype).to(DEV)
    dr = (torch.tensor([1.0, 0, 0, 0]) + torch.randn(M, 4, generator=g) * 0.1).to(dtype).to(DEV)
    return xyz, rot, mask, dx, dr


def test_deform_forward_backward_against_float64():
    from igs_amd.motion import deform_xyz_rotation
    for dt in (torch.float32, torch.float16):
        xyz, rot, mask, dx, dr = _deform_case(50000, 20000, seed=1, dtype=dt)
        rot[5] = 0.0                                                     # unmasked zero quaternion: copied as is
        dr[7] = torch.tensor([1e-14, -2e-14, 0.0, 0.0], dtype=torch.float32).to(dt)   # (fp16: underflows to zero -- still |q| < eps)
        rot[mask[9]] = torch.tensor([3e-13, 0.0, -1e-13, 0.0], device=DEV)            # a masked quaternion below eps
        leaves = [t.clone().requires_grad_(True) for t in (xyz, rot, dx, dr)]
        xo, ro = deform_xyz_rotation(leaves[0], leaves[1], mask, leaves[2], leaves[3])
        l64 = [t.detach().double().requires_grad_(True) for t in (xyz, rot, dx, dr)]
        xr, rr = MR.deform_xyz_rotation_restate(l64[0], l64[1], mask, l64[2], l64[3])
        rx, rq = MR.deform_forward_ratios(xo, ro, xyz, mask, dx, xr.detach(), rr.detach())
        assert rx <= 1 and rq <= 1
        unm = torch.ones(50000, dtype=torch.bool, device=DEV)
        unm[mask] = False
        assert torch.equal(xo[unm], xyz[unm]) and torch.equal(ro[unm], rot[unm])
        gx, gr = torch.randn_like(xo), torch.randn_like(ro)
        torch.autograd.backward((xo, ro), (gx, gr))
        torch.autograd.backward((xr, rr), (gx.double(), gr.double()))
        for a, b, name in zip(leaves, l64, ("xyz", "rotation", "res_xyz", "res_rotation")):
            assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
            # (a residual below eps has a gradient of g / 1e-12: beyond float16, as in the reference -- MR.deform_grad_ratio asserts the inf)
            assert MR.deform_grad_ratio(a.grad, b.grad, a.dtype == torch.float16) <= 1, (dt, name)


def test_deform_returns_the_reference_fields():
    from igs_amd.motion import deform
    xyz, rot, mask, dx, dr = _deform_case(3000, 1000, seed=4)

    class G:
        pass
    gs = G()
    gs.xyz, gs.rotation = xyz, rot
    gs.opacity, gs.scaling, gs.shs = torch.randn(3000, 1, device=DEV), torch.randn(3000, 3, device=DEV), torch.randn(3000, 16, 3, device=DEV)
    res = {"xyz": dx, "rotation": dr}
    d = deform(gs, res, mask)
    r = MR.deform_restate(gs, res, mask)
    assert sorted(d) == sorted(r)
    for k in ("opacity", "scaling", "shs", "resi_xyz", "resi_rotation", "mask"):
        assert torch.equal(d[k], r[k]), k
    assert d["opacity"].data_ptr() != gs.opacity.data_ptr()
    torch.testing.assert_close(d["xyz"], r["xyz"], rtol=0, atol=1e-6)
    torch.testing.assert_close(d["rotation"], r["rotation"], rtol=0, atol=1e-6)


# ---------------------------------------------------------------- end to end
def _chain(native, seed=0):
    import diff_gaussian_rasterization_rade_clamp as DC
    from igs_amd import motion
    from igs_amd.anchors import anchor_graph
    from igs_amd.scenes import cfg1_scene
    raw, cams, bg = cfg1_scene(P=10000, size=128)
    cam = cams[0].to(DEV)
    xyz = raw["xyz"].to(DEV)
    bbox = torch.tensor([[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]], device=DEV)
    anchors, masks, weights, nb, _ = anchor_graph([xyz], bbox, anchor_size=512, k=8, start_idx=[0])
    g = torch.Generator().manual_seed(seed)
    feats = (torch.randn(1, 512, 32, generator=g) * 0.5).to(DEV)
    W1 = (torch.randn(32, 64, generator=g) / 32 ** 0.5).to(DEV).requires_grad_(True)
    W2 = (torch.randn(64, 7, generator=g) * 0.02).to(DEV).requires_grad_(True)
    if native:
        (f,) = motion.query_ir_grid(feats, weights, nb, counts=[masks[0].numel()])
    else:
        (f,) = MR.split_by_batch(MR.interp_restate(feats.reshape(-1, 32), weights, nb[1]), nb[3])
    h = torch.nn.functional.silu(f @ W1) @ W2
    res = {"xyz": h[:, :3] * 0.05, "rotation": h[:, 3:] + torch.tensor([1.0, 0, 0, 0], device=DEV)}
    rot = raw["rotation"].to(DEV)
    if native:
        xo, ro = motion.deform_xyz_rotation(xyz, rot, masks[0], res["xyz"], res["rotation"])
    else:
        xo, ro = MR.deform_xyz_rotation_restate(xyz, rot, masks[0], res["xyz"], res["rotation"])
    st = DC.GaussianRasterizationSettings(image_height=cam.height, image_width=cam.width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                                          kernel_size=0.0, bg=bg.to(DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
                                          projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False,
                                          require_depth=True, require_coord=True, debug=False)
    ras = DC.GaussianRasterizer(raster_settings=st)
    m2d = torch.zeros_like(xo, requires_grad=True)
    out = ras(means3D=xo, means2D=m2d, opacities=torch.sigmoid(raw["opacity"].to(DEV)), shs=raw["shs"].to(DEV),
              scales=torch.exp(raw["scaling"].to(DEV)), rotations=torch.nn.functional.normalize(ro))
    img = out[0]
    loss = (img - 0.25).abs().mean()
    gW1, gW2 = torch.autograd.grad(loss, (W1, W2))
    return img.detach(), gW1, gW2


def test_chain_anchor_graph_to_rasterizer_matches_restatement():
    img, g1, g2 = _chain(True)
    img_r, g1_r, g2_r = _chain(False)
    assert (img - img_r).abs().max().item() <= 1e-4
    for a, b in ((g1, g1_r), (g2, g2_r)):
        assert ((a - b).abs() <= 1e-3 * b.abs() + 1e-3 * b.abs().max()).all()
