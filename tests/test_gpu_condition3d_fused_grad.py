"""The fused condition3D backward on the MI355X (igs_amd.motion.condition3d_fused_autograd / use_native_condition3d(training=True) over
cond_fused_bwd.hip) against the float64 restatement of the gradients and its derived bound (tests/condition3d_fused_grad_restatement.py).
Every element of all seven gradients is compared; every float test prints its worst |error| / bound.  The shapes are the smallest at which
the kernels can still go wrong: widths off the 32-channel tile grid, images whose pixel count is no multiple of a wave's 32 pixels, one
pixel, a pixel count just above the chunk, more than one weight-gradient slice."""
import gc

import pytest
import torch

import condition3d_fused_grad_restatement as GR
import condition3d_fused_restatement as FR
import condition3d_restatement as CR
from test_gpu_condition3d_fused import _fixture, _module, _rays_depth, _x

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
CHUNK = GR.CHUNK_ROWS                                                    # IGS_COND_BWD_CHUNK_ROWS, mirrored


@pytest.fixture(autouse=True)
def _leave_the_allocator_as_found():
    """These tests free blocks of unusual sizes (the scratch, the chunk's slots, autograd graphs that only a collection releases).  Left
    in PyTorch's cache they would be handed out, unsplit, to later tests that assert exact allocation sizes; so every test here returns
    what it cached."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _gout(x, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(x.shape, generator=g).to(DEV)


def _params(module):
    m = module.mlp
    return dict(mlp=[m[0].weight, m[0].bias, m[2].weight, m[2].bias], ln=[module.norm.weight, module.norm.bias])


def _run(x, rays, depth, module, gout, mlp_dtype, req=("x", "mlp", "ln"), packed=None):
    """The gradients condition3d_fused_autograd leaves (GR.NAMES; None where not asked for), and the output."""
    from igs_amd.motion import condition3d_fused_autograd
    module.zero_grad(set_to_none=True)
    for kind, ps in _params(module).items():
        for p in ps:
            p.requires_grad_(kind in req)
    xg = x.detach().clone().requires_grad_("x" in req)
    out = condition3d_fused_autograd(xg, rays, depth, module, mlp_dtype=mlp_dtype, packed=packed)
    out.backward(gout)
    torch.cuda.synchronize()
    got = GR.module_grads(xg, module)
    for ps in _params(module).values():
        for p in ps:
            p.requires_grad_(True)
    return got, out


def _check(x, rays, depth, module, mlp_dtype, tag, seed=5):
    gout = _gout(x, seed)
    got, out = _run(x, rays, depth, module, gout, mlp_dtype)
    grads, bounds = GR.restate(x, rays, depth, module, gout, half=mlp_dtype == F16)
    ratios = GR.worst_ratios(got, grads, bounds)
    print("%s: max |grad - grad64| / bound %s" % (tag, {k: round(v, 4) for k, v in ratios.items()}))
    assert got["dx"].dtype == x.dtype and got["dx"].shape == x.shape
    for k in GR.NAMES[1:]:
        assert got[k].dtype == F32 and got[k].shape == grads[k].shape, k
    assert all(torch.isfinite(got[k]).all() for k in GR.NAMES)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    return got, grads, bounds, gout


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_fixture_inputs(mlp_dtype):
    """N = 4, C = 8, hidden = 128, 6 x 10, depth 15 x 23 and the fixture's own upstream gradient."""
    fx = _fixture()
    module = CR.AdaLNModule.from_arrays(fx).to(DEV)
    x, rays, depth, gout = (fx[k].to(DEV) for k in ("x", "rays", "depth", "gout"))
    got, _ = _run(x, rays, depth, module, gout, mlp_dtype)
    grads, bounds = GR.restate(x, rays, depth, module, gout, half=mlp_dtype == F16)
    ratios = GR.worst_ratios(got, grads, bounds)
    print("fixture %s: max |grad - grad64| / bound %s" % (mlp_dtype, {k: round(v, 4) for k, v in ratios.items()}))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("x_dtype", [F32, F16])
@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_shipped_widths_on_a_small_image(x_dtype, mlp_dtype):
    """C = 128, hidden = 128 on 9 x 7 = 63 pixels per image, N = 3: a partial last group, and the next image starts its own group."""
    B, V, C, H, W = 1, 3, 128, 9, 7
    rays, depth = _rays_depth(B, V, H, W, 5, 11, seed=1)
    _check(_x(B * V, C, H, W, 2, x_dtype), rays, depth, _module(C, seed=3), mlp_dtype, "x %s mlp %s" % (x_dtype, mlp_dtype))


@pytest.mark.parametrize("C,hidden", [(7, 5), (33, 65), (96, 32), (128, 1), (65, 48)])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 13), (33, 2)])
@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_widths_off_the_tile_grid(C, hidden, H, W, mlp_dtype):
    """One pixel; 65 and 66 pixels (a masked last group, a group boundary inside an image); two views."""
    B, V = 1, 2
    rays, depth = _rays_depth(B, V, H, W, 4, 7, seed=C + H)
    _check(_x(B * V, C, H, W, hidden + W), rays, depth, _module(C, hidden, seed=C * hidden), mlp_dtype,
           "C %d hidden %d %dx%d %s" % (C, hidden, H, W, mlp_dtype))


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_pixel_count_just_above_the_chunk(mlp_dtype):
    """Three images of (CHUNK + 2) / 3 pixels: CHUNK + 2 pixels, CHUNK + 32 rows; the third image straddles the chunk boundary and the
    second chunk is its last, masked group alone, whose partial sums continue the first chunk's."""
    assert (CHUNK + 2) % 6 == 0
    N, C, hidden, H, W = 3, 32, 32, 2, (CHUNK + 2) // 6
    assert CHUNK < N * H * W < CHUNK + 32 and GR.padded_rows(N, H, W) == CHUNK + 32 and 2 * GR.padded_rows(1, H, W) < CHUNK
    rays, depth = _rays_depth(1, N, H, W, 3, 40, seed=11)
    _check(_x(N, C, H, W, 12), rays, depth, _module(C, hidden, seed=13), mlp_dtype, "chunk boundary %s" % mlp_dtype)


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_more_than_one_weight_gradient_slice(mlp_dtype):
    """Two images of 9 x 17 = 153 pixels: 320 rows, two slices of 256, the second one partial."""
    N, C, hidden, H, W = 2, 32, 32, 9, 17
    assert GR.SLICE_ROWS < GR.padded_rows(N, H, W) < 2 * GR.SLICE_ROWS
    rays, depth = _rays_depth(1, N, H, W, 6, 9, seed=21)
    _check(_x(N, C, H, W, 22), rays, depth, _module(C, hidden, seed=23), mlp_dtype, "two slices %s" % mlp_dtype)


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_large_depth_and_pre_activations(mlp_dtype):
    """Depth up to 10^4 and W1 scaled until |z1| reaches 80: silu' runs on its clamped exponent, every gradient stays finite and within
    the bound."""
    B, V, C, hidden, H, W = 1, 2, 33, 65, 5, 13
    rays, depth = _rays_depth(B, V, H, W, 4, 7, seed=31, depth_top=1e4)
    module = _module(C, hidden, seed=32)
    r = FR.restate(_x(B * V, C, H, W, 33), rays, depth, module)
    W1, b1 = module.mlp[0].weight.detach().cpu().double(), module.mlp[0].bias.detach().cpu().double()
    z1 = r["cond64"].reshape(-1, 33) @ W1.T + b1
    with torch.no_grad():
        module.mlp[0].weight.mul_(80.0 / float(z1.abs().max()))
        module.mlp[0].bias.mul_(80.0 / float(z1.abs().max()))
    z1 = r["cond64"].reshape(-1, 33) @ module.mlp[0].weight.detach().cpu().double().T + module.mlp[0].bias.detach().cpu().double()
    assert 79.0 <= float(z1.abs().max()) <= 81.0 and float(depth.max()) > 9e3
    _check(_x(B * V, C, H, W, 33), rays, depth, module, mlp_dtype, "depth 1e4, |z1| 80 %s" % mlp_dtype)


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_the_bound_has_teeth(mlp_dtype):
    """The kernel's gradients are within the bound of the right restatement and outside it for each wrong backward."""
    B, V, C, hidden, H, W = 1, 2, 33, 65, 5, 13
    rays, depth = _rays_depth(B, V, H, W, 4, 7, seed=41)
    x, module = _x(B * V, C, H, W, 42), _module(C, hidden, seed=43)
    got, grads, bounds, gout = _check(x, rays, depth, module, mlp_dtype, "teeth %s" % mlp_dtype)
    for mut, key in (("swap_dw2_halves", "dW2"), ("silu_grad_one", "dW1"), ("unbiased_dx", "dx"), ("drop_depth_column", "dW1"),
                     ("dscale_without_n", "dW2")):
        wrong, _ = GR.restate(x, rays, depth, module, gout, half=mlp_dtype == F16, mutate=mut)
        ratio = FR.worst(got[key], wrong[key], bounds[key])
        print("  %s: %s off by %.1f bounds" % (mut, key, ratio))
        assert ratio > 1.0, mut


@pytest.mark.parametrize("mlp_dtype", [F32, F16])
def test_optional_gradients(mlp_dtype):
    """Only x, only the MLP's parameters, only the LayerNorm's, everything: what is returned has the bits of the all-gradients call, the
    rest is None."""
    B, V, C, hidden, H, W = 1, 2, 65, 48, 5, 13
    rays, depth = _rays_depth(B, V, H, W, 4, 7, seed=51)
    x, module = _x(B * V, C, H, W, 52), _module(C, hidden, seed=53)
    gout = _gout(x, 54)
    full, _ = _run(x, rays, depth, module, gout, mlp_dtype)
    assert all(full[k] is not None for k in GR.NAMES)
    kinds = dict(x=("dx",), mlp=("dW1", "db1", "dW2", "db2"), ln=("dnw", "dnb"))
    for req in (("x",), ("mlp",), ("ln",), ("x", "ln")):
        got, _ = _run(x, rays, depth, module, gout, mlp_dtype, req=req)
        asked = [k for r in req for k in kinds[r]]
        for k in GR.NAMES:
            if k in asked:
                assert torch.equal(got[k], full[k]), (req, k)
            else:
                assert got[k] is None, (req, k)


def test_reproducible_and_independent_of_the_batch():
    """Two runs agree bit for bit; d x of an image alone is its d x in a batch of three; a NaN in one pixel of x leaves every other
    pixel's d x bits unchanged and makes that pixel's d x and the parameter gradients that see x NaN."""
    B, V, C, hidden, H, W = 1, 3, 33, 65, 5, 13
    rays, depth = _rays_depth(B, V, H, W, 4, 7, seed=61)
    x, module = _x(B * V, C, H, W, 62), _module(C, hidden, seed=63)
    gout = _gout(x, 64)
    for dt in (F32, F16):
        a, _ = _run(x, rays, depth, module, gout, dt)
        b, _ = _run(x, rays, depth, module, gout, dt)
        assert all(torch.equal(a[k], b[k]) for k in GR.NAMES), dt
        one, _ = _run(x[1:2], rays[:, 1:2], depth[:, 1:2], module, gout[1:2], dt)
        assert torch.equal(one["dx"], a["dx"][1:2]), dt
        xn = x.clone()
        xn[2, 5, 3, 7] = float("nan")
        c, _ = _run(xn, rays, depth, module, gout, dt)
        hit = torch.zeros(x.shape, dtype=torch.bool, device=DEV)
        hit[2, :, 3, 7] = True
        assert torch.isnan(c["dx"][hit]).all() and torch.equal(c["dx"][~hit], a["dx"][~hit]), dt
        assert all(torch.isnan(c[k]).any() for k in ("dW1", "dW2", "dnw")), dt        # (d bias = sum g (1 + scale) does not see x)


def test_layouts_streams_and_empty_batches():
    from igs_amd import motion
    B, V, C, hidden, H, W = 1, 2, 33, 65, 5, 13
    rays, depth = _rays_depth(B, V, H, W, 4, 7, seed=71)
    x, module = _x(B * V, C, H, W, 72), _module(C, hidden, seed=73)
    gout = _gout(x, 74)
    want, _ = _run(x, rays, depth, module, gout, F32)
    # a channel slice of a wider buffer is read in place: the Function saves the view itself
    wide = torch.zeros(B * V, C + 9, H, W, device=DEV)
    wide[:, 4:4 + C] = x
    wide.requires_grad_(True)
    view = wide[:, 4:4 + C]
    module.zero_grad(set_to_none=True)
    out = motion.condition3d_fused_autograd(view, rays, depth, module, mlp_dtype=F32)
    saved = out.grad_fn.saved_tensors[0]
    assert saved.data_ptr() == view.data_ptr() and saved.stride() == view.stride()
    out.backward(gout)
    assert torch.equal(wide.grad[:, 4:4 + C], want["dx"]) and (wide.grad[:, :4] == 0).all() and (wide.grad[:, 4 + C:] == 0).all()
    assert torch.equal(module.mlp[0].weight.grad, want["dW1"])
    # channels-last x is copied once; the saved tensor is the copy
    cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    module.zero_grad(set_to_none=True)
    out = motion.condition3d_fused_autograd(cl, rays, depth, module, mlp_dtype=F32)
    assert out.grad_fn.saved_tensors[0].is_contiguous() and out.grad_fn.saved_tensors[0].data_ptr() != cl.data_ptr()
    # a non-contiguous upstream gradient
    out.backward(gout.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert torch.equal(cl.grad, want["dx"]) and torch.equal(module.mlp[2].weight.grad, want["dW2"])
    # a side stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, _ = _run(x, rays, depth, module, gout, F32)
    s.synchronize()
    assert all(torch.equal(got[k], want[k]) for k in GR.NAMES)
    # N = 0
    x0 = torch.zeros(0, C, H, W, device=DEV, requires_grad=True)
    module.zero_grad(set_to_none=True)
    out = motion.condition3d_fused_autograd(x0, rays[:, :0], depth[:, :0], module, mlp_dtype=F32)
    assert out.shape == (0, C, H, W)
    out.sum().backward()
    assert x0.grad.shape == x0.shape and all((p.grad == 0).all() for p in module.parameters())


def test_memory_contract_at_40000_pixels():
    """Forward + backward rise by the output, d x, the parameter gradients and the reported scratch (plus the slack of one [pixels, 128]
    float32 activation, test_gpu_decoder_grad's); the three-step path keeps at least mod = pixels x 2C x 4 bytes more."""
    from igs_amd import motion
    from igs_amd._cabi import ext
    N, C, hidden, H, W = 4, 128, 128, 100, 100
    P = N * H * W
    rays, depth = _rays_depth(1, N, H, W, 30, 40, seed=81)
    x, module = _x(N, C, H, W, 82), _module(C, hidden, seed=83)
    gout = _gout(x, 84)
    packed = motion.pack_condition_mlp(module.mlp, F32, transposed=True)
    scratch = ext()._cond.bwd_scratch_bytes(N, C, hidden, H, W)
    assert scratch == ext()._cond.bwd_scratch_bytes(10 * N, C, hidden, H, W) > 0
    act = P * 128 * 4

    def rise(fn):
        module.zero_grad(set_to_none=True)
        xg = x.detach().clone().requires_grad_(True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn(xg).backward(gout)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    native = rise(lambda xg: motion.condition3d_fused_autograd(xg, rays, depth, module, packed=packed, mlp_dtype=F32))
    three = rise(lambda xg: motion.condition3d(xg, rays, depth, module))
    tensors = 2 * x.numel() * 4 + sum(p.numel() * 4 for p in module.parameters())
    print("memory: native rise %.1f MB (out + dx + parameter gradients %.1f MB, scratch %.1f MB), three-step rise %.1f MB"
          % (native / 1e6, tensors / 1e6, scratch / 1e6, three / 1e6))
    assert native <= tensors + scratch + act
    assert three >= native + P * 2 * C * 4


def _bound_model(C):
    from test_condition3d_fused_host import _model
    torch.manual_seed(90)
    return _model(C).to(DEV)


def test_training_binder(monkeypatch):
    """use_native_condition3d(model, training=True) with the table forced to True: every parameter's .grad is filled and agrees with the
    three-step path within the sum of both bounds (the three-step path evaluates the same float32 sums in another order: the same
    bound); after an optimiser step the packs are rebuilt; under float16 autocast the parameter gradients are float32, d x half."""
    from igs_amd import motion
    monkeypatch.setattr(motion, "COND_FUSED_BWD_NATIVE", {F32: True, F16: True})
    C, H, W = 8, 6, 10
    model = motion.use_native_condition3d(_bound_model(C), training=True)
    module = model.ModLN
    rays, depth = _rays_depth(2, 2, H, W, 15, 23, seed=91)
    x = _x(4, C, H, W, 92)
    gout = _gout(x, 93)

    def step(fn, xin):
        module.zero_grad(set_to_none=True)
        xg = xin.detach().clone().requires_grad_(True)
        fn(xg).backward(gout)
        return GR.module_grads(xg, module)

    got = step(lambda xg: model.condition3D(xg, rays, depth), x)
    assert all(p.grad is not None for p in module.parameters()) and motion.COND_FUSED_TRAIN_CACHE in module.__dict__
    ref = step(lambda xg: motion.condition3d(xg, rays, depth, module), x)
    grads, bounds = GR.restate(x, rays, depth, module, gout)
    for k in GR.NAMES:
        ratio = FR.worst(got[k], ref[k].cpu().double(), 2 * bounds[k])
        print("binder %s: max |native - three-step| / (2 bound) %.4f" % (k, ratio))
        assert ratio <= 1.0, k
    assert GR.worst_ratios(got, grads, bounds)["dW1"] <= 1.0
    # an optimiser step changes the parameters in place: the packs follow
    old = module.__dict__[motion.COND_FUSED_TRAIN_CACHE]["pack"][0].clone()
    opt = torch.optim.SGD(module.parameters(), lr=1e-3)       # (small: the half d x below stays far inside the half range)
    opt.step()
    got2 = step(lambda xg: model.condition3D(xg, rays, depth), x)
    assert not torch.equal(module.__dict__[motion.COND_FUSED_TRAIN_CACHE]["pack"][0], old)
    grads2, bounds2 = GR.restate(x, rays, depth, module, gout)
    r2 = GR.worst_ratios(got2, grads2, bounds2)
    assert all(v <= 1.0 for v in r2.values()), r2
    # float16 autocast: the float16 instance, float32 parameter gradients, a half d x
    xh = x.half()
    with torch.autocast("cuda", dtype=F16):
        goth = step(lambda xg: model.condition3D(xg, rays, depth), xh)
    assert goth["dx"].dtype == F16 and all(goth[k].dtype == F32 for k in GR.NAMES[1:])
    assert module.__dict__[motion.COND_FUSED_TRAIN_CACHE]["pack"][0].dtype == F16
    gh, bh = GR.restate(xh, rays, depth, module, gout, half=True)
    rh = GR.worst_ratios(goth, gh, bh)
    print("binder autocast:", {k: round(v, 4) for k, v in rh.items()})
    assert all(v <= 1.0 for v in rh.values()), rh


def test_chain_from_the_upsample_to_the_lift():
    """upsample_conv_autograd -> fused condition3D -> grid_encoder_lift -> sum on 2 views of 6 x 5 -> 12 x 10: the gradients that reach the
    convolution's input and ModLN's parameters agree with the same chain through condition3d.  Both chains run the same float32
    upsample + convolution and the same lift; the condition3D stage's error on either side is within the restatement's bound at the
    upstream gradient that the lift hands it, and the convolution's backward is linear in that gradient with absolute weights |K|."""
    from igs_amd import motion
    B, V, Cin, C, h, w = 1, 2, 16, 32, 6, 5
    H, W = 2 * h, 2 * w
    torch.manual_seed(101)
    conv = torch.nn.Conv2d(Cin, C, 3, padding=1).to(DEV)
    module = _module(C, 64, seed=102)
    rays, depth = _rays_depth(B, V, H, W, 20, 17, seed=103)
    g = torch.Generator().manual_seed(104)
    f0 = torch.randn(B * V, Cin, h, w, generator=g).to(DEV)
    pts = (torch.rand(B, 256, 3, generator=g) * 2 - 1).to(DEV)
    c2w = torch.eye(4).repeat(B, V, 1, 1)
    c2w[..., 2, 3] = -3.0
    c2w = c2w.to(DEV)
    fov = torch.tensor([[0.9, 0.9]], device=DEV)

    def chain(stage):
        module.zero_grad(set_to_none=True)
        conv.zero_grad(set_to_none=True)
        fin = f0.clone().requires_grad_(True)
        mid = motion.upsample_conv_autograd(fin, conv, conv_dtype=F32)
        mid.retain_grad()
        out = stage(mid)
        out.retain_grad()
        motion.grid_encoder_lift(out, pts, fov, c2w).sum().backward()
        return fin.grad, mid.grad, out.grad, GR.module_grads(mid, module), mid.detach()

    fa, ma, ga, pa, mid = chain(lambda t: motion.condition3d_fused_autograd(t, rays, depth, module, mlp_dtype=F32))
    fb, mb, gb, pb, _ = chain(lambda t: motion.condition3d(t, rays, depth, module))
    assert (ga != 0).any() and torch.equal(ga, gb)                       # the lift's backward sees the same points on either side
    grads, bounds = GR.restate(mid, rays, depth, module, ga)
    for k in GR.NAMES[1:]:
        ratio = FR.worst(pa[k], pb[k].cpu().double(), 2 * bounds[k])
        print("chain %s: max |native - three-step| / (2 bound) %.4f" % (k, ratio))
        assert ratio <= 1.0, k
    assert FR.worst(ma, mb.cpu().double(), 2 * bounds["dx"]) <= 1.0
    # through the convolution's backward: |d f_a - d f_b| <= upsample^T conv^T_{|K|} (2 bound_dx), plus the float32 rounding of that sum
    e = (2 * bounds["dx"]).float().to(DEV)
    with torch.no_grad():
        absconv = torch.nn.Conv2d(Cin, C, 3, padding=1, bias=False).to(DEV)
        absconv.weight.copy_(conv.weight.abs())
    probe = torch.zeros_like(f0, requires_grad=True)
    absconv(torch.nn.functional.interpolate(probe, scale_factor=2, mode="bilinear", align_corners=False)).backward(e)
    mag = torch.zeros_like(f0, requires_grad=True)
    absconv(torch.nn.functional.interpolate(mag, scale_factor=2, mode="bilinear", align_corners=False)).backward(mb.abs())
    tol = probe.grad.double() * (1 + 2.0 ** -10) + 2 * (9 * C + 8) * 2.0 ** -24 * mag.grad.double()
    ratio = FR.worst(fa, fb.cpu().double(), tol.cpu())
    print("chain d input: max |native - three-step| / bound %.4f" % ratio)
    assert ratio <= 1.0
