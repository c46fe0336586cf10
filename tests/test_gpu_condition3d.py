"""IGS.condition3D's native parts on the MI355X (igs_amd.motion.ray_condition / modln / condition3d over cond.hip) against the float64
restatements of tests/condition3d_restatement.py.

Tolerances are derived (ray_condition_bound / modln_forward_bound / modln_backward_bounds state the operation counts), never measured.
Every element is compared.  Float16 inputs are widened exactly before the float64 restatement sees them; a float16 output adds one
rounding to half (half_rounding)."""
import os

import numpy as np
import pytest
import torch

import condition3d_restatement as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6


def _rays_depth(B, V, H, W, Hd, Wd, seed):
    g = torch.Generator().manual_seed(seed)
    rays = torch.cat([torch.randn(B, V, H, W, 3, generator=g) * 1.5,
                      torch.randn(B, V, H, W, 3, generator=g) * (0.5 + 2.0 * torch.rand(B, V, H, W, 1, generator=g))], -1)   # not unit vectors
    depth = 1.0 + 5.0 * torch.rand(B, V, Hd, Wd, generator=g)
    return rays.to(DEV), depth.to(DEV)


def _check_cond(cond, rays, depth, reject=True):
    ref = CR.ray_condition_restate(rays.double(), depth.double())
    bound = CR.ray_condition_bound(rays, depth)
    err = (cond.double() - ref).abs()
    print("cond: max err %.3e, max err / bound %.3f, max |ref| %.3f" % (err.max().item(), (err / bound).max().item(), ref.abs().max().item()))
    assert cond.dtype == torch.float32 and cond.shape == ref.shape and cond.is_contiguous()
    assert (err <= bound).all()
    if reject:          # not vacuous: the same bound rejects the wrong variants
        for kw in (dict(align_corners=True), dict(normalise=False), dict(swap_cross=True)):
            wrong = CR.ray_condition_restate(rays.double(), depth.double(), **kw)
            assert not ((wrong - ref).abs() <= bound).all(), kw


@pytest.mark.parametrize("B", [1, 5])
def test_ray_condition_shipped_shape(B):
    from igs_amd.motion import ray_condition
    rays, depth = _rays_depth(B, 4, 128, 128, 1014, 1352, seed=B)
    cond = ray_condition(rays, depth, (128, 128))
    assert cond.shape == (B * 4, 128, 128, 33)
    _check_cond(cond, rays, depth)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1, 1), (2, 3, 7, 5, 3, 11), (1, 2, 6, 10, 15, 23), (1, 1, 33, 257, 8, 8), (1, 1, 3, 300, 700, 2)])
def test_ray_condition_odd_sizes(shape):
    from igs_amd.motion import ray_condition
    B, V, H, W, Hd, Wd = shape
    rays, depth = _rays_depth(B, V, H, W, Hd, Wd, seed=H + W)
    _check_cond(ray_condition(rays, depth, (H, W)), rays, depth, reject=False)


def test_ray_condition_by_hand():
    """Axis-aligned rays: the harmonics are known constants; a zero direction gives d = 0; a depth map resized to its own size comes back
    bit for bit."""
    from igs_amd.motion import ray_condition
    H, W = 4, 8
    rays = torch.zeros(1, 3, H, W, 6, device=DEV)
    rays[0, 0, ..., 5] = 2.0                                             # direction +z (not unit), origin 0
    rays[0, 1, ..., 3] = -3.0                                            # direction -x, origin (0, 1, 0): moment (0, 0, 1)
    rays[0, 1, ..., 1] = 1.0
    rays[0, 2, ..., 0] = 5.0                                             # zero direction: d = 0 / 1e-12 = 0, moment 0
    depth = torch.rand(1, 3, H, W, device=DEV) * 7
    cond = ray_condition(rays, depth, (H, W))
    assert torch.equal(cond[..., 32], depth.reshape(3, H, W))
    f = lambda v: torch.tensor(v, dtype=torch.float64)                   # noqa: E731
    K0, K1, K20, K30 = CR.K0, CR.K1, CR.K20, CR.K30
    up = f([K0, 0, K1, 0, 0, 0, 2 * K20, 0, 0, 0, 0, 0, 2 * K30, 0, 0, 0])
    zero = f([K0, 0, 0, 0, 0, 0, -K20, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    mx = f([K0, 0, 0, K1, 0, 0, -K20, 0, 0.5 * CR.K2, 0, 0, 0, 0, -CR.K3C, 0, CR.K3A])        # d = (-1, 0, 0)
    tol = 8 * CR.u * 3
    for v, (sd, sm) in enumerate(((up, zero), (mx, up), (zero, zero))):
        got = cond[v].double().cpu()
        assert (got[..., :16] - sd).abs().max() <= tol, v
        assert (got[..., 16:32] - sm).abs().max() <= tol, v


def _modln_case(N, C, H, W, seed, x_dtype=torch.float32, mod_dtype=torch.float32, offset=3.0, spread=0.5):
    g = torch.Generator().manual_seed(seed)
    x = (offset + spread * torch.randn(N, C, H, W, generator=g)).to(x_dtype).to(DEV)
    mod = (0.7 * torch.randn(N, H, W, 2 * C, generator=g)).to(mod_dtype).to(DEV)
    w = (1.0 + 0.5 * torch.randn(C, generator=g)).to(DEV)
    b = (0.4 * torch.randn(C, generator=g)).to(DEV)
    gout = torch.randn(N, C, H, W, generator=g).to(DEV)
    return x, mod, w, b, gout


def _check_modln(x, mod, w, b, gout, backward=True, reject=False, tag=""):
    """Forward and all four gradients of igs_amd.motion.modln against float64 on the widened inputs; returns the native results."""
    from igs_amd.motion import modln
    xd, md, wd, bd = x.detach().double(), mod.detach().double(), w.detach().double(), b.detach().double()
    ref = CR.modln_restate(xd, md, wd, bd, EPS)
    bound = CR.modln_forward_bound(x.detach().float(), mod.detach().float(), w, b, EPS)
    xg, mg, wg, bg = (t.detach().requires_grad_(backward) for t in (x, mod, w, b))          # (views stay views: read in place)
    out = modln(xg, mg, wg, bg, EPS)
    err = (out.detach().double() - ref).abs()
    print("%s forward: max err %.3e, max err / bound %.3f, max |ref| %.3f" % (tag, err.max().item(), (err / bound).max().item(), ref.abs().max().item()))
    assert out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    assert (err <= bound).all()
    if reject:
        for kw in (dict(unbiased=True), dict(swap_halves=True)):
            assert not ((CR.modln_restate(xd, md, wd, bd, EPS, **kw) - ref).abs() <= bound).all(), kw
    if not backward:
        return out, None
    out.backward(gout)
    want = CR.modln_backward_restate(xd, md, wd, bd, EPS, gout.double())
    bounds = CR.modln_backward_bounds(x.detach().float(), mod.detach().float(), w, b, EPS, gout, half_x=x.dtype == torch.float16,
                                      half_mod=mod.dtype == torch.float16)
    got = (xg.grad, mg.grad, wg.grad, bg.grad)
    assert xg.grad.dtype == x.dtype and mg.grad.dtype == mod.dtype and wg.grad.dtype == torch.float32
    for name, gv, wv in zip(("dx", "dmod", "dweight", "dbias"), got, want):
        e = (gv.double() - wv).abs()
        print("%s %s: max err %.3e, max err / bound %.3f, max |ref| %.3f" % (tag, name, e.max().item(), (e / bounds[name]).max().item(), wv.abs().max().item()))
        assert gv.shape == wv.shape
        assert (e <= bounds[name]).all(), name
    return out, got


@pytest.mark.parametrize("B", [1, 5])
def test_modln_shipped_shape(B):
    x, mod, w, b, gout = _modln_case(B * 4, 128, 128, 128, seed=10 + B)
    _check_modln(x, mod, w, b, gout, reject=True, tag="B=%d" % B)


@pytest.mark.parametrize("x_dtype,mod_dtype", [(torch.float16, torch.float32), (torch.float32, torch.float16), (torch.float16, torch.float16)])
def test_modln_half(x_dtype, mod_dtype):
    x, mod, w, b, gout = _modln_case(4, 128, 128, 128, seed=21, x_dtype=x_dtype, mod_dtype=mod_dtype)
    _check_modln(x, mod, w, b, gout, tag="%s/%s" % (x_dtype, mod_dtype))
    x, mod, w, b, gout = _modln_case(2, 7, 5, 3, seed=22, x_dtype=x_dtype, mod_dtype=mod_dtype)           # the scalar paths
    _check_modln(x, mod, w, b, gout, tag="small %s/%s" % (x_dtype, mod_dtype))


@pytest.mark.parametrize("shape", [(3, 1, 9, 7), (2, 7, 12, 10), (2, 129, 17, 16), (1, 1024, 9, 8), (2, 1024, 3, 5), (5, 16, 33, 1), (1, 244, 8, 24),
                                   (1, 248, 8, 24), (2, 480, 4, 20), (1, 64, 1, 1)] + [
    # the last and the first C of every tile size that modln_tile_log2 (cond.hip) picks from the 64 KB of LDS: the forward holds 64 pixels
    # up to C = 240, 32 up to 477, 16 up to 929, then 8; the backward (two operand tiles) 32 up to 238, 16 up to 464, 8 up to 880, then 4.
    # 72 and 35 pixels: more than one tile with a part tile at every size, the four-element and the scalar form
    (1, 238, 9, 8), (1, 239, 5, 7), (1, 240, 9, 8), (1, 241, 5, 7), (1, 464, 9, 8), (1, 465, 5, 7), (1, 477, 5, 7), (1, 478, 9, 8),
    (1, 880, 9, 8), (1, 881, 5, 7), (1, 929, 5, 7), (1, 930, 9, 8)])
def test_modln_odd_sizes(shape):
    N, C, H, W = shape
    x, mod, w, b, gout = _modln_case(N, C, H, W, seed=sum(shape))
    _check_modln(x, mod, w, b, gout, reject=1 < C <= 129, tag=str(shape))


def test_modln_planes_read_in_place_and_unaligned():
    """A slice of n and of c is read in place; a plane that does not start on a 16-byte boundary takes the scalar path; a channels-last
    tensor is copied by the Python layer.  All give the bits of a contiguous copy."""
    from igs_amd.motion import modln
    big, mod, w, b, gout = _modln_case(6, 24, 16, 20, seed=31)
    mod, w, b = mod[1:5, :, :, :32].contiguous(), w[:16].contiguous(), b[:16].contiguous()
    view = big[1:5, 3:19]
    assert not view.is_contiguous()
    with torch.no_grad():
        base = modln(view.contiguous(), mod, w, b, EPS)
        assert torch.equal(modln(view, mod, w, b, EPS), base)
        assert torch.equal(modln(view.contiguous(memory_format=torch.channels_last), mod, w, b, EPS), base)
        flat = torch.zeros(view.numel() + 1, device=DEV)
        flat[1:] = view.reshape(-1)
        off = flat[1:].view(view.shape)                                  # 4 bytes past a 16-byte boundary
        assert off.data_ptr() % 16 == 4
        assert torch.equal(modln(off, mod, w, b, EPS), base)
    _check_modln(view, mod, w, b, gout[1:5, :16].contiguous(), tag="slice")
    h = torch.zeros(view.numel() + 1, device=DEV, dtype=torch.float16)
    h[1:] = view.reshape(-1).half()
    _check_modln(h[1:].view(view.shape), mod, w, b, gout[1:5, :16].contiguous(), tag="unaligned half")


@pytest.mark.parametrize("C", [8, 128])
def test_modln_offset_input_needs_the_centred_variance(C):
    """x = 4096 + 2 randn: E[x^2] - mu^2 in float32 loses the variance; the kernel's centred sum stays within the bound."""
    x, mod, w, b, gout = _modln_case(2, C, 32, 64, seed=41, offset=4096.0, spread=2.0)
    _check_modln(x, mod, w, b, gout, tag="offset C=%d" % C)
    ref = CR.modln_restate(x.double(), mod.double(), w.double(), b.double(), EPS)
    bound = CR.modln_forward_bound(x, mod, w, b, EPS)
    var = (x * x).mean(1, keepdim=True) - x.mean(1, keepdim=True) ** 2                    # float32, the formula the kernel must not use
    xh = (x - x.mean(1, keepdim=True)) * torch.rsqrt(var.clamp_min(0) + EPS)
    naive = (xh * w.view(1, C, 1, 1) + b.view(1, C, 1, 1)) * (1 + mod[..., C:].permute(0, 3, 1, 2)) + mod[..., :C].permute(0, 3, 1, 2)
    assert ((naive.double() - ref).abs() > bound).double().mean() > 0.5


def test_modln_equal_channels_and_constant_pixel():
    """A pixel whose channels are all equal: xhat = 0, so out = bias (1 + scale) + shift up to the bound."""
    from igs_amd.motion import modln
    x, mod, w, b, _ = _modln_case(2, 128, 8, 8, seed=51)
    x[:] = x[:, :1]
    with torch.no_grad():
        out = modln(x, mod, w, b, EPS)
    want = b.double().view(1, -1, 1, 1) * (1 + mod[..., 128:].double().permute(0, 3, 1, 2)) + mod[..., :128].double().permute(0, 3, 1, 2)
    assert ((out.double() - want).abs() <= CR.modln_forward_bound(x, mod, w, b, EPS)).all()


def test_modln_side_stream_empty_and_bitwise_backward():
    from igs_amd.motion import modln
    x, mod, w, b, gout = _modln_case(4, 128, 64, 64, seed=61)
    _, first = _check_modln(x, mod, w, b, gout, tag="main")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _, second = _check_modln(x, mod, w, b, gout, tag="side stream")
    s.synchronize()
    for a, c in zip(first, second):
        assert torch.equal(a, c)                                         # d weight and d bias included: no float atomics
    # only some gradients wanted
    xg = x.clone().requires_grad_(True)
    modln(xg, mod, w, b, EPS).backward(gout)
    assert torch.equal(xg.grad, first[0])
    wg = w.clone().requires_grad_(True)
    modln(x, mod, wg, b, EPS).backward(gout)
    assert torch.equal(wg.grad, first[2])
    # N = 0
    e = modln(x[:0].requires_grad_(True), mod[:0], w.clone().requires_grad_(True), b, EPS)
    assert e.shape == (0, 128, 64, 64)
    e.sum().backward()


@pytest.mark.parametrize("H,W,T", [(9, 8, 3), (80, 80, 200), (512, 513, 8208)])
def test_modln_parameter_gradients_are_the_partial_rows_added_in_the_documented_order(H, W, T):
    """igs_modln_bwd through the C ABI, float32, N = 1, C = 4 (backward tiles of 32 pixels): rows 0 .. T - 1 of the scratch (from its
    pointer rounded up to 256 bytes, [2][C] floats each) are the tiles' partial sums and the next 64 rows the staged group sums.  Round one
    gives group g the g-th contiguous share of ceil(T / 64) rows, round two reduces the 64 staged rows; each as param_rows_sum states it.
    The staged rows, d weight and d bias bit for bit.  T = 3: most groups empty; 200: group shares of 4, wave shares of 1; 8208: group
    shares of 129, wave shares of 9 (the eight-load loop and its remainder)."""
    import token_ops_restatement as TR
    from igs_amd import _cabi
    L, C, G = _cabi.lib(), 4, 64
    lp = 5                                                               # the launcher's tile: the largest 2^lp <= 32 pixels within 64 KB of LDS
    while lp > 2 and (2 * C * ((1 << lp) + 1) + 2 * 256 + 4 * (1 << lp)) * 4 > 65536:
        lp -= 1
    assert -(-H * W // (1 << lp)) == T
    nbytes = L.igs_modln_bwd_scratch_bytes(1, C, H, W)
    assert nbytes == -(-(T + G) * 2 * C * 4 // 256) * 256 + 512
    x, mod, w, b, gout = _modln_case(1, C, H, W, seed=H + W)
    out, mean, rstd = torch.empty_like(x), torch.empty(H * W, device=DEV), torch.empty(H * W, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.igs_modln_fwd(stream, 1, C, H, W, 0, x.data_ptr(), C * H * W, H * W, W, 1, 0, mod.data_ptr(), w.data_ptr(), b.data_ptr(), EPS,
                         out.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    assert rc == 0, _cabi.last_error()
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    dw, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    rc = L.igs_modln_bwd(stream, 1, C, H, W, 0, x.data_ptr(), C * H * W, H * W, W, 1, 0, mod.data_ptr(), w.data_ptr(), b.data_ptr(), mean.data_ptr(),
                         rstd.data_ptr(), gout.data_ptr(), None, None, dw.data_ptr(), db.data_ptr(), scratch.data_ptr())
    assert rc == 0, _cabi.last_error()
    torch.cuda.synchronize()
    at = -scratch.data_ptr() % 256
    rows = scratch[at:at + (T + G) * 2 * C * 4].view(torch.float32).view(T + G, 2 * C).cpu()
    share = -(-T // G)
    staged = torch.stack([TR.param_rows_sum(rows[min(g * share, T):min(g * share + share, T)]) for g in range(G)])
    want = TR.param_rows_sum(staged)
    print("%d x %d: T %d, max |dweight| %.3e" % (H, W, T, dw.abs().max().item()))
    bits = lambda t: t.contiguous().view(torch.int32)                    # noqa: E731
    assert torch.equal(bits(rows[T:]), bits(staged))
    assert torch.equal(bits(dw.cpu()), bits(want[:C])) and torch.equal(bits(db.cpu()), bits(want[C:]))


def _fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_condition3d.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_fixture_inputs_through_the_kernels():
    """The reference's stored inputs through ray_condition and modln: both sides are float32 evaluations of the same float64 value, each
    within the bound (the reference's side is asserted by the generator and the host test), so they differ by at most twice the bound."""
    from igs_amd.motion import modln, ray_condition
    fx = {k: v.to(DEV) for k, v in _fixture().items()}
    cond = ray_condition(fx["rays"], fx["depth"], (6, 10))
    _check_cond(cond, fx["rays"], fx["depth"])
    assert ((cond.double() - fx["cond"].double()).abs() <= 2 * CR.ray_condition_bound(fx["rays"], fx["depth"])).all()
    out, grads = _check_modln(fx["x"], fx["mod"], fx["norm_weight"], fx["norm_bias"], fx["gout"], reject=True, tag="fixture")
    assert ((out.detach().double() - fx["out"].double()).abs() <= 2 * CR.modln_forward_bound(fx["x"], fx["mod"], fx["norm_weight"], fx["norm_bias"], EPS)).all()
    bb = CR.modln_backward_bounds(fx["x"], fx["mod"], fx["norm_weight"], fx["norm_bias"], EPS, fx["gout"])
    for name, gv in zip(("dx", "dmod", "dweight", "dbias"), grads):
        assert ((gv.double() - fx[name].double()).abs() <= 2 * bb[name]).all(), name


def test_condition3d_against_the_reference_fixture():
    """condition3d with the fixture's module rebuilt from its stored parameters, against the reference's out and autograd gradients.
    The MLP (PyTorch on both sides) sees a cond that differs by float32 rounding, so its output `mod` differs slightly from the stored
    one; with f the float64 restatement, |native - stored| <= bound(mod) + bound(mod_stored) + |f(mod) - f(mod_stored)|, the last term
    evaluated in float64: the triangle inequality, nothing measured."""
    from igs_amd.motion import condition3d
    fx = {k: v.to(DEV) for k, v in _fixture().items()}
    module = CR.AdaLNModule.from_arrays(fx).to(DEV)
    x = fx["x"].clone().requires_grad_(True)
    rays, depth, gout = fx["rays"], fx["depth"], fx["gout"]
    kept = {}

    def keep(_m, _i, o):
        kept["mod"] = o
        o.retain_grad()

    h = module.mlp.register_forward_hook(keep)
    out = condition3d(x, rays, depth, module)
    h.remove()
    assert out.shape == fx["out"].shape and out.dtype == torch.float32 and out.is_contiguous()
    out.backward(gout)
    mod, w, b = kept["mod"].detach(), module.norm.weight.detach(), module.norm.bias.detach()
    xd, wd, bd = fx["x"].double(), w.double(), b.double()
    got = dict(out=out.detach(), dx=x.grad, dmod=kept["mod"].grad, dweight=module.norm.weight.grad, dbias=module.norm.bias.grad)
    f, bound = {}, {}
    for tag, m in (("used", mod), ("stored", fx["mod"])):
        f[tag] = dict(zip(("dx", "dmod", "dweight", "dbias"), CR.modln_backward_restate(xd, m.double(), wd, bd, EPS, gout.double())))
        f[tag]["out"] = CR.modln_restate(xd, m.double(), wd, bd, EPS)
        bound[tag] = CR.modln_backward_bounds(fx["x"], m, w, b, EPS, gout)
        bound[tag]["out"] = CR.modln_forward_bound(fx["x"], m, w, b, EPS)
    for name, gv in got.items():
        assert ((gv.double() - f["used"][name]).abs() <= bound["used"][name]).all(), name
        slack = (f["used"][name] - f["stored"][name]).abs()
        err = (gv.double() - fx[name].double()).abs()
        print("%s: max |native - reference| %.3e, max |reference| %.3e" % (name, err.max().item(), fx[name].abs().max().item()))
        assert (err <= bound["used"][name] + bound["stored"][name] + slack).all(), name
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in module.mlp.parameters())


def test_condition3d_feeds_the_lift_in_place():
    """The result is NCHW-contiguous, so grid_encoder_lift reads it without a copy; the lift of a channels-last copy of the same values
    (what the reference hands over) goes through the copy branch and the same kernel: equal bits."""
    from igs_amd.motion import condition3d, grid_encoder_lift
    B, V, C, H, W = 1, 4, 128, 128, 128
    g = torch.Generator().manual_seed(71)
    module = CR.AdaLNModule(C).to(DEV)
    x = torch.randn(B * V, C, H, W, generator=g).to(DEV)
    rays, depth = _rays_depth(B, V, H, W, 507, 676, seed=72)
    with torch.no_grad():
        out = condition3d(x, rays, depth, module)
        assert out.is_contiguous() and out.shape == x.shape
        ref = CR.reference_composition(x, rays, depth, module)
        assert ref.stride() == (C * H * W, 1, W * C, C)                  # what the reference returns: channels-last strides
        pts = (torch.rand(B, 4096, 3, generator=g) * 2 - 1).to(DEV)
        c2w = torch.eye(4).repeat(B, V, 1, 1)
        c2w[..., 2, 3] = -3.0
        c2w = c2w.to(DEV)
        fov = torch.tensor([[0.9, 0.9]], device=DEV)
        a = grid_encoder_lift(out, pts, fov, c2w)
        cl = out.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert cl.stride() == ref.stride() and not cl.is_contiguous()
        assert torch.equal(grid_encoder_lift(cl, pts, fov, c2w), a)
        assert (a != 0).any()


def test_condition3d_in_a_captured_graph():
    from igs_amd.motion import condition3d
    B, V, C, H, W = 1, 4, 128, 64, 64
    module = CR.AdaLNModule(C).to(DEV)
    x = torch.randn(B * V, C, H, W, device=DEV)
    rays, depth = _rays_depth(B, V, H, W, 200, 300, seed=81)
    depth2 = depth * 0.5 + 1.0
    with torch.no_grad():
        eager1 = condition3d(x, rays, depth, module).clone()
        eager2 = condition3d(x, rays, depth2, module).clone()
        static_depth = depth.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                condition3d(x, rays, static_depth, module)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = condition3d(x, rays, static_depth, module)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager1)
        static_depth.copy_(depth2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager2)
        assert not torch.equal(eager1, eager2)


def test_refusals_on_the_gpu():
    from igs_amd.motion import modln, ray_condition
    x, mod, w, b, _ = _modln_case(2, 8, 4, 4, seed=91)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        modln(x.bfloat16(), mod, w, b)
    with pytest.raises(ValueError, match="mod must be"):
        modln(x, mod[..., :8], w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        modln(x, mod.cpu(), w, b)
    rays, depth = _rays_depth(1, 2, 4, 4, 8, 8, seed=92)
    with pytest.raises(NotImplementedError, match="gradients"):
        ray_condition(rays.requires_grad_(True), depth, (4, 4))
