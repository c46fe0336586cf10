"""The native backward of the fused 2x bilinear upsample + 3x3 convolution on the MI355X (igs_amd.motion.upsample_conv_autograd over
upconv.hip and upconv_bwd.hip) against the float64 restatement and its derived bounds (tests/upconv_grad_restatement.py).  Every element
of dx, dW and db is compared; every test prints its worst |error| / bound.  The shapes are the smallest at which the kernels can still go
wrong: widths off the 32-channel tile grid that run every instance at both ends of its range, a single pixel, one-row and one-column
maps, maps that are partial in and span several of the 3 x 15 (dgrad) and 4 x 32 (wgrad) tiles both ways, and pixel-tile counts below,
at and above the slice count.

Recorded on one MI355X, worst |error| / bound for dx, dW, db over the width list: 0.062, 0.169, 0.178 with a float32
and 0.252, 0.446, 0.004 with a float16 convolution; with a float16 x 0.889, 0.004, 0.001 and 0.088, 0.078, 0.001."""
import pytest
import torch

import upconv_grad_restatement as G
import upconv_restatement as UR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
IDS = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c).replace("torch.", "")       # noqa: E731
REFS = ("dx64", "dw64", "db64")
BOUNDS = ("bound_dx", "bound_dw", "bound_db")


def _device_conv(conv, case, bias=True):
    d = torch.nn.Conv2d(case[0], case[1], 3, padding=1, bias=bias).to(DEV)
    d.load_state_dict({k: v for k, v in conv.state_dict().items() if bias or k != "bias"})
    return d


def _grads(xd, dconv, gd, conv_dtype, want=(True, True, True)):
    """(out, dx, dW, db) of the native call on device tensors; a gradient that is not wanted is None."""
    from igs_amd.motion import upsample_conv_autograd
    xd = xd.detach().requires_grad_(want[0])
    dconv.weight.requires_grad_(want[1])
    if dconv.bias is not None:
        dconv.bias.requires_grad_(want[2])
    dconv.zero_grad(set_to_none=True)
    out = upsample_conv_autograd(xd, dconv, conv_dtype=conv_dtype)
    assert out.dtype == conv_dtype and out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_UpsampleConv")
    out.backward(gd)
    return out.detach(), xd.grad, dconv.weight.grad, None if dconv.bias is None else dconv.bias.grad


def _check(case, x_dtype, conv_dtype, single_pixel=False):
    x, conv, g, R = G.reference(case, conv_dtype == F16, x_dtype == F16, single_pixel)
    dconv = _device_conv(conv, case)
    out, dx, dw, db = _grads(x.to(DEV), dconv, g.to(DEV), conv_dtype)
    assert dx.dtype == x_dtype and dx.shape == x.shape and dw.dtype == F32 and dw.shape == conv.weight.shape and db.dtype == F32
    ratios = [G.worst(t, R[r], R[b]) for t, r, b in zip((dx, dw, db), REFS, BOUNDS)]
    print("%s x %s conv %s%s: worst |error| / bound dx %.4f dW %.4f db %.4f" % (case, x_dtype, conv_dtype, " single pixel" if single_pixel else "", *ratios))
    assert all(r <= 1.0 for r in ratios), ratios
    return (dx, dw, db), x, conv, g, R


@pytest.mark.parametrize("x_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_shipped_widths(x_dtype, conv_dtype):
    _check(G.SHIPPED, x_dtype, conv_dtype)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("hw", G.MAPS, ids=IDS)
@pytest.mark.parametrize("widths", G.WIDTHS, ids=IDS)
def test_widths_off_the_tile_grid_on_edge_maps(widths, hw, conv_dtype):
    _check(widths + (2,) + hw, F32, conv_dtype)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("case", G.SLICE_CASES, ids=IDS)
def test_fewer_exactly_and_more_pixel_tiles_than_slices(case, conv_dtype):
    _check(case, F32, conv_dtype)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_g_zero_outside_a_single_pixel(conv_dtype):
    (dx, _, _), _, _, _, R = _check((7, 5, 2, 5, 7), F32, conv_dtype, single_pixel=True)
    assert torch.equal(dx.cpu() == 0, R["dx64"] == 0)                    # exact zeros where the pixel does not reach


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_not_vacuous_on_the_gpu(conv_dtype):
    """The native gradients are outside the bounds around the unflipped-taps dx and the replicate-padding dW (and the other variants):
    the comparison above would tell each from the definition."""
    for case in (G.SHIPPED, (33, 65, 2, 17, 3)):
        (dx, dw, _), x, conv, g, R = _check(case, F32, conv_dtype)
        for kind in G.DX_VARIANTS:
            if G.variant_applies(kind, case):
                ratio = G.worst(dx, G.dx_variant(kind, x, conv.weight, g), R["bound_dx"])
                print("    dx against %s: %.3g x the bound" % (kind, ratio))
                assert ratio > 1.0, (case, kind)
        for kind in G.DW_VARIANTS:
            ratio = G.worst(dw, G.dw_variant(kind, x, conv.weight, g), R["bound_dw"])
            print("    dW against %s: %.3g x the bound" % (kind, ratio))
            assert ratio > 1.0, (case, kind)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
@pytest.mark.parametrize("x_dtype", [F32, F16], ids=IDS)
def test_strided_views_are_read_in_place_and_other_layouts_are_copied(x_dtype, conv_dtype):
    """x strided in n and c is read in place, with NaN in the memory between; channels-last x and a non-contiguous d out are copied.
    A float16 x below the shipped width runs here, one width of each other dgrad instance."""
    for ci, co in ((33, 65), (65, 48), (7, 5)):
        case = (ci, co, 2, 9, 7)
        base, x, conv, g, R = _check(case, x_dtype, conv_dtype)
        dconv, gd = _device_conv(conv, case), g.to(DEV)
        big = torch.full((4, ci + 9, 9, 7), float("nan"), dtype=x_dtype, device=DEV)
        big[1:3, 2:2 + ci] = x.to(DEV)
        v = big[1:3, 2:2 + ci]
        assert not v.is_contiguous()
        got = _grads(v, dconv, gd, conv_dtype)[1:]
        assert all(torch.equal(a, b) for a, b in zip(got, base))
        cl = x.to(DEV).contiguous(memory_format=torch.channels_last)
        got = _grads(cl, dconv, gd, conv_dtype)[1:]
        assert all(torch.equal(a, b) for a, b in zip(got, base))
        gt = gd.transpose(2, 3).contiguous().transpose(2, 3)
        assert not gt.is_contiguous() or gd.shape[2] == 1 or gd.shape[3] == 1
        got = _grads(x.to(DEV), dconv, gt, conv_dtype)[1:]
        assert all(torch.equal(a, b) for a, b in zip(got, base))


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_two_runs_agree_bit_for_bit_and_an_image_does_not_depend_on_the_batch(conv_dtype):
    case = (40, 97, 3, 17, 18)
    x, conv, g, R = G.reference(case, conv_dtype == F16)
    dconv, xd, gd = _device_conv(conv, case), x.to(DEV), g.to(DEV)
    a = _grads(xd, dconv, gd, conv_dtype)
    b = _grads(xd, dconv, gd, conv_dtype)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    ratios = [G.worst(t, R[r], R[bd]) for t, r, bd in zip(a[1:], REFS, BOUNDS)]
    print("%s conv %s: worst |error| / bound dx %.4f dW %.4f db %.4f" % (case, conv_dtype, *ratios))
    assert all(r <= 1.0 for r in ratios)
    alone = _grads(xd[1:2], dconv, gd[1:2], conv_dtype)
    assert torch.equal(alone[1], a[1][1:2])                              # dx[1:2] of the batch = dx of image 1 alone
    # a NaN in d out of image 0 leaves image 1's dx with the clean run's bits
    gn = gd.clone()
    gn[0, 3, 5, 7] = float("nan")
    dirty = _grads(xd, dconv, gn, conv_dtype)
    assert torch.equal(dirty[1][1:], a[1][1:]) and torch.isnan(dirty[1][0]).any() and torch.isnan(dirty[3][3])


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_each_gradient_alone_has_the_full_call_s_bits(conv_dtype):
    case = (33, 65, 2, 9, 7)
    x, conv, g, _ = G.reference(case, conv_dtype == F16)
    dconv, xd, gd = _device_conv(conv, case), x.to(DEV), g.to(DEV)
    full = _grads(xd, dconv, gd, conv_dtype)[1:]
    for i in range(3):
        want = tuple(j == i for j in range(3))
        got = _grads(xd, dconv, gd, conv_dtype, want)[1:]
        assert torch.equal(got[i], full[i]) and all(got[j] is None for j in range(3) if j != i), want


def test_under_autocast_the_output_is_half_and_the_parameter_gradients_float32(monkeypatch):
    from igs_amd import motion
    from igs_amd.motion import upsample_conv_autograd
    monkeypatch.setitem(motion.UPCONV_BWD_NATIVE, F16, True)            # the default dtype goes native here whatever the routing table says
    case = G.SHIPPED
    x, conv, g, R = G.reference(case, True)
    dconv = _device_conv(conv, case).requires_grad_(True)
    xd = x.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=F16):
        out = upsample_conv_autograd(xd, dconv)
    assert out.dtype == F16 and type(out.grad_fn).__name__.startswith("_UpsampleConv")
    out.backward(g.to(DEV))
    assert xd.grad.dtype == F32 and dconv.weight.grad.dtype == F32 and dconv.bias.grad.dtype == F32
    ratios = [G.worst(t, R[r], R[b]) for t, r, b in zip((xd.grad, dconv.weight.grad, dconv.bias.grad), REFS, BOUNDS)]
    print("autocast %s: worst |error| / bound dx %.4f dW %.4f db %.4f" % (case, *ratios))
    assert all(r <= 1.0 for r in ratios)
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(NotImplementedError, match="autocast"):
        upsample_conv_autograd(xd, dconv)


@pytest.mark.parametrize("conv_dtype", [F32, F16], ids=IDS)
def test_a_conv_without_a_bias(conv_dtype):
    case = (7, 33, 2, 9, 7)
    x, conv, g, R = G.reference(case, conv_dtype == F16)
    dconv = _device_conv(conv, case, bias=False)
    out, dx, dw, db = _grads(x.to(DEV), dconv, g.to(DEV), conv_dtype)
    assert db is None
    fr = UR.restate(x, conv.weight, None, half=conv_dtype == F16)
    assert UR.worst(out, fr["out64"], fr["bound"]) <= 1.0                # the forward without a bias, by its own bound
    ratios = [G.worst(t, R[r], R[b]) for t, r, b in zip((dx, dw), REFS, BOUNDS)]
    print("%s conv %s no bias: worst |error| / bound dx %.4f dW %.4f" % (case, conv_dtype, *ratios))
    assert all(r <= 1.0 for r in ratios)
