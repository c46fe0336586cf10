"""The fused condition3D forward on the MI355X (igs_amd.motion.condition3d_fused / use_native_condition3d over cond_fused.hip) against the
float64 restatement and its derived bound (tests/condition3d_fused_restatement.py).  Every element is compared; every float test prints
its worst |error| / bound.  The shapes are the smallest at which the kernel can still go wrong: widths off the 32-channel tile grid, images
whose pixel count is no multiple of a wave's 32 pixels (so the last group is partial and the next image starts a new group), one pixel."""
import os
import types

import numpy as np
import pytest
import torch

import condition3d_fused_restatement as FR
import condition3d_restatement as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16 = torch.float32, torch.float16


def _rays_depth(B, V, H, W, Hd, Wd, seed, depth_top=6.0):
    g = torch.Generator().manual_seed(seed)
    rays = torch.cat([torch.randn(B, V, H, W, 3, generator=g) * 1.5,
                      torch.randn(B, V, H, W, 3, generator=g) * (0.5 + 2.0 * torch.rand(B, V, H, W, 1, generator=g))], -1)   # not unit vectors
    depth = 1.0 + (depth_top - 1.0) * torch.rand(B, V, Hd, Wd, generator=g)
    return rays.to(DEV), depth.to(DEV)


def _module(C, hidden=128, seed=0):
    torch.manual_seed(seed)
    m = CR.AdaLNModule(C, hidden=hidden)
    with torch.no_grad():
        m.norm.weight.copy_(1.0 + 0.5 * torch.randn(C))
        m.norm.bias.copy_(0.4 * torch.randn(C))
    return m.to(DEV)


def _x(N, C, H, W, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (3.0 + 0.5 * torch.randn(N, C, H, W, generator=g)).to(dtype).to(DEV)


def _check(x, rays, depth, module, mlp_dtype, tag):
    from igs_amd.motion import condition3d_fused
    with torch.no_grad():
        out = condition3d_fused(x, rays, depth, module, mlp_dtype=mlp_dtype)
    r = FR.restate(x, rays, depth, module, half=mlp_dtype == F16)
    ratio = FR.worst(out, r["out64"], r["bound"])
    print("%s: max |out - out64| / bound %.4f, max |out64| %.3f" % (tag, ratio, r["out64"].abs().max().item()))
    assert out.dtype == F32 and out.shape == x.shape and out.is_contiguous()
    assert ratio <= 1.0
    return out, r


def _fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_condition3d.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_fixture_inputs():
    """N = 4, C = 8, hidden = 128, 6 x 10, depth 15 x 23, float32 MLP: within the derived bound of the restatement, and within
    bound + the fixture's own bound + the float64 distance of the two restatements of the reference's stored out (the triangle inequality
    of test_condition3d_against_the_reference_fixture)."""
    fx = _fixture()
    module = CR.AdaLNModule.from_arrays(fx).to(DEV)
    out, r = _check(fx["x"].to(DEV), fx["rays"].to(DEV), fx["depth"].to(DEV), module, F32, "fixture")
    w, b, eps = fx["norm_weight"], fx["norm_bias"], float(fx["eps"])
    stored64 = CR.modln_restate(fx["x"].double(), fx["mod"].double(), w.double(), b.double(), eps)
    slack = (r["out64"] - stored64).abs()
    err = (out.cpu().double() - fx["out"].double()).abs()
    print("fixture: max |native - reference| %.3e, max |reference| %.3e" % (err.max().item(), fx["out"].abs().max().item()))
    assert (err <= r["bound"] + CR.modln_forward_bound(fx["x"], fx["mod"], w, b, eps) + slack).all()
    # not vacuous: the bound rejects the swapped halves and the unbiased variance
    for kw in (dict(swap_halves=True), dict(unbiased=True)):
        wrong = CR.modln_restate(fx["x"].double(), r["mod64"], w.double(), b.double(), eps, **kw)
        assert FR.worst(out, wrong, r["bound"]) > 1.0, kw


@pytest.mark.parametrize("x_dtype", [F32, F16])
@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_shipped_widths_on_a_small_image(x_dtype, mlp_dtype):
    """C = 128, hidden = 128 on 9 x 7 = 63 pixels per image: a partial last group, and the next image starts its own group."""
    B, V, C, H, W = 1, 2, 128, 9, 7
    rays, depth = _rays_depth(B, V, H, W, 5, 11, seed=1)
    _check(_x(B * V, C, H, W, 2, x_dtype), rays, depth, _module(C, seed=3), mlp_dtype, "x %s mlp %s" % (x_dtype, mlp_dtype))


@pytest.mark.parametrize("C,hidden", [(7, 5), (33, 65), (96, 32), (128, 1), (65, 48)])         # (65, 48): the one count of hidden tiles, 2, not above
@pytest.mark.parametrize("H,W", [(1, 1), (5, 13), (33, 2)])
@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_widths_off_the_tile_grid(C, hidden, H, W, mlp_dtype):
    B, V = 1, 3
    rays, depth = _rays_depth(B, V, H, W, 4, 9, seed=C + H)
    _check(_x(B * V, C, H, W, hidden + W), rays, depth, _module(C, hidden, seed=C * hidden), mlp_dtype, "C %d hidden %d %dx%d %s" % (C, hidden, H, W, mlp_dtype))


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_large_depth_values(mlp_dtype):
    """Depth up to 1e4: pre-activations of the order of 1e3, where SiLU's exponent is clamped: finite and within the bound."""
    B, V, C, H, W = 1, 2, 128, 9, 7
    rays, depth = _rays_depth(B, V, H, W, 5, 11, seed=11, depth_top=1e4)
    assert depth.max() > 9e3
    out, _ = _check(_x(B * V, C, H, W, 12), rays, depth, _module(C, seed=13), mlp_dtype, "depth 1e4 %s" % mlp_dtype)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_nan_stays_in_its_pixel(mlp_dtype):
    from igs_amd.motion import condition3d_fused
    B, V, C, H, W = 1, 2, 33, 9, 7
    module = _module(C, 65, seed=21)
    x = _x(B * V, C, H, W, 22)
    rays, depth = _rays_depth(B, V, H, W, 5, 11, seed=23)
    bits = lambda t: t.contiguous().view(torch.int32)                    # noqa: E731
    with torch.no_grad():
        base = condition3d_fused(x, rays, depth, module, mlp_dtype=mlp_dtype)
        assert torch.isfinite(base).all()
        rays2 = rays.clone()
        rays2[0, 1, 4, 3, 4] = float("nan")                              # one component of one pixel's direction
        x2 = x.clone()
        x2[1, 5, 4, 3] = float("nan")                                    # one channel of one pixel
        for got in (condition3d_fused(x, rays2, depth, module, mlp_dtype=mlp_dtype), condition3d_fused(x2, rays, depth, module, mlp_dtype=mlp_dtype)):
            assert torch.isnan(got[1, :, 4, 3]).all()
            hit = torch.zeros_like(got, dtype=torch.bool)
            hit[1, :, 4, 3] = True
            assert torch.equal(bits(got)[~hit], bits(base)[~hit]) and int(torch.isnan(got).sum()) == C


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_reproducible_and_independent_of_the_batch(mlp_dtype):
    from igs_amd.motion import condition3d_fused
    C, H, W = 96, 9, 7
    module = _module(C, 32, seed=31)
    x = _x(3, C, H, W, 32)
    rays, depth = _rays_depth(3, 1, H, W, 5, 11, seed=33)
    with torch.no_grad():
        a = condition3d_fused(x, rays, depth, module, mlp_dtype=mlp_dtype)
        b = condition3d_fused(x, rays, depth, module, mlp_dtype=mlp_dtype)
        alone = condition3d_fused(x[1:2], rays[1:2], depth[1:2], module, mlp_dtype=mlp_dtype)
    assert torch.equal(a, b)
    assert torch.equal(alone[0], a[1])


def test_layouts_side_stream_and_empty():
    from igs_amd.motion import condition3d_fused
    C, H, W = 16, 8, 10
    module = _module(C, 128, seed=41)
    big = _x(6, 24, H, W, 42)
    rays, depth = _rays_depth(2, 2, H, W, 5, 11, seed=43)
    view = big[1:5, 3:19]                                                # a batch slice and a channel slice: read in place
    assert not view.is_contiguous()
    with torch.no_grad():
        base = condition3d_fused(view.contiguous(), rays, depth, module)
        assert torch.equal(condition3d_fused(view, rays, depth, module), base)
        cl = view.contiguous(memory_format=torch.channels_last)          # goes through the copy
        assert not cl.is_contiguous()
        assert torch.equal(condition3d_fused(cl, rays, depth, module), base)
        h = view.half()
        assert torch.equal(condition3d_fused(big.half()[1:5, 3:19], rays, depth, module), condition3d_fused(h.contiguous(), rays, depth, module))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            side = condition3d_fused(view, rays, depth, module)
        s.synchronize()
        assert torch.equal(side, base)
        empty = condition3d_fused(big[:0, :16], rays[:0], depth[:0], module)
        assert empty.shape == (0, C, H, W) and empty.dtype == F32
    _check(view, rays, depth, module, F32, "slice")


def test_in_a_captured_graph():
    from igs_amd.motion import condition3d_fused, pack_condition_mlp
    B, V, C, H, W = 1, 2, 128, 9, 7
    module = _module(C, seed=51)
    x = _x(B * V, C, H, W, 52)
    rays, depth = _rays_depth(B, V, H, W, 20, 30, seed=53)
    depth2 = depth * 0.5 + 1.0
    with torch.no_grad():
        packed = pack_condition_mlp(module.mlp)
        eager1 = condition3d_fused(x, rays, depth, module, packed=packed).clone()
        eager2 = condition3d_fused(x, rays, depth2, module, packed=packed).clone()
        static_depth = depth.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                condition3d_fused(x, rays, static_depth, module, packed=packed)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = condition3d_fused(x, rays, static_depth, module, packed=packed)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager1)
        static_depth.copy_(depth2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager2)
        assert not torch.equal(eager1, eager2)


def _model(C):
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = types.SimpleNamespace(local_ray=False, use_condition3d=True)
            self.ModLN = CR.AdaLNModule(C)
    return Model().to(DEV)


def test_binder():
    from igs_amd.motion import condition3d, condition3d_fused, use_native_condition3d
    B, V, C, H, W = 1, 2, 128, 9, 7
    torch.manual_seed(61)
    model = _model(C)
    assert use_native_condition3d(model) is model
    x = _x(B * V, C, H, W, 62)
    rays, depth = _rays_depth(B, V, H, W, 5, 11, seed=63)
    with torch.no_grad():
        got = model.condition3D(x, rays, depth)
        assert torch.equal(got, condition3d_fused(x, rays, depth, model.ModLN))
    # with a gradient: today's path, forward and every gradient bit for bit
    gout = torch.randn(B * V, C, H, W, device=DEV)
    params = list(model.ModLN.parameters())
    xa = x.clone().requires_grad_(True)
    out_a = model.condition3D(xa, rays, depth)
    ga = torch.autograd.grad(out_a, [xa] + params, gout)
    xb = x.clone().requires_grad_(True)
    out_b = condition3d(xb, rays, depth, model.ModLN)
    gb = torch.autograd.grad(out_b, [xb] + params, gout)
    assert torch.equal(out_a, out_b)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)
    # an in-place update is followed
    with torch.no_grad():
        model.ModLN.mlp[2].weight.mul_(2)
        after = model.condition3D(x, rays, depth)
        assert torch.equal(after, condition3d_fused(x, rays, depth, model.ModLN)) and not torch.equal(after, got)


def test_feeds_the_lift_in_place():
    """The result is NCHW-contiguous, so grid_encoder_lift takes its no-copy branch; the lift of a channels-last copy of the same values
    goes through the copy branch and the same kernel: equal bits."""
    from igs_amd.motion import condition3d_fused, grid_encoder_lift
    B, V, C, H, W = 1, 4, 128, 16, 16
    g = torch.Generator().manual_seed(71)
    module = _module(C, seed=72)
    x = _x(B * V, C, H, W, 73)
    rays, depth = _rays_depth(B, V, H, W, 50, 67, seed=74)
    with torch.no_grad():
        out = condition3d_fused(x, rays, depth, module)
        assert out.is_contiguous() and out.shape == x.shape
        pts = (torch.rand(B, 512, 3, generator=g) * 2 - 1).to(DEV)
        c2w = torch.eye(4).repeat(B, V, 1, 1)
        c2w[..., 2, 3] = -3.0
        c2w = c2w.to(DEV)
        fov = torch.tensor([[0.9, 0.9]], device=DEV)
        a = grid_encoder_lift(out, pts, fov, c2w)
        cl = out.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not cl.is_contiguous()
        assert torch.equal(grid_encoder_lift(cl, pts, fov, c2w), a)
        assert (a != 0).any()
