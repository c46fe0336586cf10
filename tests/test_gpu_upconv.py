"""The fused 2x bilinear upsample + 3x3 convolution on the MI355X (igs_amd.motion.upsample_conv over upconv.hip) against the float64
restatement and its derived bound (tests/upconv_restatement.py).  Every element is compared; every float test prints its worst
|error| / bound.  The shapes are the smallest at which the kernel can still go wrong: widths off the 32-channel tile grid, a single
pixel, one-row and one-column maps where both clamps and both paddings meet, maps that are partial in and span several 8 x 32 output
tiles in both directions (the kernel's tile is no larger than 32 x 32, so no map beyond those).

Recorded on one MI355X for the widths that run every count of output tiles at both ends of its range (7 -> 33,
128 -> 64, 65 -> 48, 5 -> 96, 40 -> 97): worst |error| / bound 0.072 with a float32 and 0.285 with a float16 convolution; with a
float16 x (65 -> 48, 7 -> 5) 0.017 and 0.214."""
import pytest
import torch
import torch.nn.functional as F

import condition3d_restatement as CR
import upconv_restatement as UR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
IDS = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c).replace("torch.", "")       # noqa: E731


def _eager(x, conv):
    return conv(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))


def _run(case, x_dtype, conv_dtype):
    """(out on the GPU, x and conv on the CPU, the restatement) of a shared case."""
    from igs_amd.motion import upsample_conv
    x, conv, r = UR.reference(case, half=conv_dtype == F16, x_half=x_dtype == F16)
    dconv = torch.nn.Conv2d(case[0], case[1], 3, padding=1).to(DEV).requires_grad_(False)
    dconv.load_state_dict(conv.state_dict())
    with torch.no_grad():
        out = upsample_conv(x.to(DEV), dconv, conv_dtype=conv_dtype)
    assert out.dtype == conv_dtype and out.shape == r["out64"].shape and out.is_contiguous()
    return out, x, conv, r, dconv


def _check(case, x_dtype, conv_dtype):
    out, x, conv, r, _ = _run(case, x_dtype, conv_dtype)
    ratio = UR.worst(out, r["out64"], r["bound"])
    print("%s x %s conv %s: max |out - out64| / bound %.4f, max |out64| %.3f" % (case, x_dtype, conv_dtype, ratio, r["out64"].abs().max().item()))
    assert ratio <= 1.0
    return out, x, conv, r


@pytest.mark.parametrize("x_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_shipped_widths(x_dtype, conv_dtype):
    _check(UR.SHIPPED, x_dtype, conv_dtype)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("hw", UR.MAPS, ids=IDS)
@pytest.mark.parametrize("widths", UR.WIDTHS, ids=IDS)
def test_widths_off_the_tile_grid_on_edge_maps(widths, hw, conv_dtype):
    _check(widths + (2,) + hw, F32, conv_dtype)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_not_vacuous_on_the_gpu(conv_dtype):
    """The native result is outside the bound around the align_corners=True variant and around the variant that pads with zeros at the
    low resolution: the comparison above would tell either from the definition."""
    for case in (UR.SHIPPED, (33, 65, 2, 17, 3)):
        out, x, conv, r = _check(case, F32, conv_dtype)
        for kind in ("align_corners", "low_resolution_zero_padding"):
            ratio = UR.worst(out, UR.variant(kind, x, conv.weight, conv.bias), r["bound"])
            print("    against %s: %.3g x the bound" % (kind, ratio))
            assert ratio > 1.0, (case, kind)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("x_dtype", [F32, F16], ids=IDS)
def test_strided_views_are_read_in_place_and_channels_last_is_copied(x_dtype, conv_dtype):
    """The only test that hands the kernel a float16 x below the shipped width, so it runs one width of each other count of output tiles
    (3, 2, 1: igs_upconv_fwd's switch) and compares the contiguous result with float64 before the views are held against it."""
    from igs_amd.motion import upsample_conv
    for ci, co in ((33, 65), (65, 48), (7, 5)):
        case = (ci, co, 2, 9, 7)
        out, x, _, r, dconv = _run(case, x_dtype, conv_dtype)
        ratio = UR.worst(out, r["out64"], r["bound"])
        print("%s x %s conv %s: max |out - out64| / bound %.4f" % (case, x_dtype, conv_dtype, ratio))
        assert ratio <= 1.0, case
        x = x.to(x_dtype)
        big = torch.full((4, ci + 7, 9, 7), float("nan"), dtype=x_dtype, device=DEV)     # what the kernel must not touch is NaN
        big[1:3, 5:5 + ci] = x.to(DEV)
        view = big[1:3, 5:5 + ci]
        assert not view.is_contiguous()
        with torch.no_grad():
            assert torch.equal(upsample_conv(view, dconv, conv_dtype=conv_dtype), out)
            step = torch.full((4, ci, 9, 7), float("nan"), dtype=x_dtype, device=DEV)
            step[::2] = x.to(DEV)
            assert torch.equal(upsample_conv(step[::2], dconv, conv_dtype=conv_dtype), out)
            cl = x.to(DEV).contiguous(memory_format=torch.channels_last)
            assert not cl.is_contiguous()
            assert torch.equal(upsample_conv(cl, dconv, conv_dtype=conv_dtype), out)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_batch_independence_and_reproducibility(conv_dtype):
    from igs_amd.motion import upsample_conv
    x, conv = UR.make_case(33, 65, 3, 17, 18)
    conv, x = conv.to(DEV), x.to(DEV)
    with torch.no_grad():
        a = upsample_conv(x, conv, conv_dtype=conv_dtype)
        b = upsample_conv(x, conv, conv_dtype=conv_dtype)
        alone = upsample_conv(x[1:2], conv, conv_dtype=conv_dtype)
    assert torch.equal(a, b)
    assert torch.equal(a[1:2], alone)
    assert not torch.equal(a[0], a[1])


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_nan_containment(conv_dtype):
    """A NaN at one interior input pixel (i, j) reaches the upsampled rows 2i-1 .. 2i+2 and columns 2j-1 .. 2j+2, hence the outputs one
    further: everything else, and the other image, keeps the clean run's bits; (2i, 2j) and (2i+1, 2j+1) are NaN in every channel."""
    from igs_amd.motion import upsample_conv
    x, conv = UR.make_case(33, 65, 2, 9, 7)
    conv, x = conv.to(DEV), x.to(DEV)
    i, j = 4, 3
    bad = x.clone()
    bad[0, 20, i, j] = float("nan")
    with torch.no_grad():
        clean = upsample_conv(x, conv, conv_dtype=conv_dtype)
        out = upsample_conv(bad, conv, conv_dtype=conv_dtype)
    assert torch.isfinite(clean).all()
    inside = torch.zeros(18, 14, dtype=torch.bool, device=DEV)
    inside[2 * i - 2:2 * i + 4, 2 * j - 2:2 * j + 4] = True
    assert torch.equal(out[1], clean[1])
    assert torch.equal(out[0][:, ~inside], clean[0][:, ~inside])
    assert torch.isnan(out[0, :, 2 * i, 2 * j]).all() and torch.isnan(out[0, :, 2 * i + 1, 2 * j + 1]).all()
    print("NaN outputs: %d of the 36 x 65 in the window" % int(torch.isnan(out[0]).sum()))


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_result_feeds_condition3d_fused_without_a_copy(conv_dtype):
    from igs_amd import motion
    Cc, N, H, W = 8, 2, 5, 7
    x, conv = UR.make_case(Cc, Cc, N, H, W)
    conv, x = conv.to(DEV), x.to(DEV)
    torch.manual_seed(1)
    module = CR.AdaLNModule(Cc, hidden=128).to(DEV)
    g = torch.Generator().manual_seed(2)
    rays = torch.randn(1, N, 2 * H, 2 * W, 6, generator=g).to(DEV)
    depth = (1.0 + torch.rand(1, N, 11, 13, generator=g)).to(DEV)
    with torch.no_grad():
        out = motion.upsample_conv(x, conv, conv_dtype=conv_dtype)
        assert out.is_contiguous() and out.dtype == conv_dtype and motion._plane_contiguous(out)
        y = motion.condition3d_fused(out, rays, depth, module)
        assert torch.equal(y, motion.condition3d_fused(out.clone(), rays, depth, module)) and torch.isfinite(y).all()


def test_dispatch_native_without_grad_eager_with():
    from igs_amd import motion
    x, conv = UR.make_case(33, 65, 2, 9, 7)
    conv, x = conv.to(DEV), x.to(DEV)
    r = UR.reference((33, 65, 2, 9, 7))[2]
    assert motion.UPCONV_NATIVE[F32]
    with torch.no_grad():
        native = motion.upsample_conv(x, conv)
        eager = _eager(x, conv)
    assert conv.__dict__[motion.UPCONV_CACHE]["pack"][0].is_cuda                     # the kernel's pack was made: the native path ran
    assert UR.worst(native, r["out64"], r["bound"]) <= 1.0
    with torch.autocast("cuda", dtype=F16), torch.no_grad():
        half = motion.upsample_conv(x, conv)
        assert half.dtype == F16 == _eager(x, conv).dtype
    conv.requires_grad_(True)
    out = motion.upsample_conv(x, conv)
    assert out.grad_fn is not None and torch.equal(out, _eager(x, conv))
    out.square().mean().backward()
    assert conv.weight.grad is not None and torch.isfinite(conv.weight.grad).all() and conv.weight.grad.abs().sum() > 0
    print("native against eager float32: max |difference| %.3g" % (native - eager).abs().max().item())
