"""The encoder's fused instance norms and position add on the MI355X (igs_amd/csrc/inorm.hip through the C ABI and through
igs_amd.backbone) against the float64 restatement of tests/encoder_norms_restatement.py on the same float32 / float16 inputs.

Every element is compared.  The allowances are derived, never measured (encoder_norms_restatement.norm_term / allowance /
position_allowance state the reasoning): per element 4 * 2^-24 * ((|x| + |mean|) * rstd + |x_hat| + 1), the same again for a normalised
skip, 2^-23 |out| for the add and 2^-11 |out| for a float16 result; 2e-6 + 2^-23 |out| (+ 2^-11 |out|) for the position add.  The worst
error-to-allowance ratio of every case is printed.

The norm cases go through the C ABI on PyTorch's current stream so that the test chooses where the operands lie: x and out start one
element past a 16-byte boundary in some cases (every plane base misaligned, odd sizes alternate), out sits between two sentinel bands of
one allocation and is pre-filled with NaN.

Recorded on one MI355X: worst |err| / allowance 0.35 in float32 and 0.99 in float16 (the output's own rounding) for
the norm modes, 0.35 / 0.998 for the position add.  Stand-in encoder, max |error| against the float64 run of the same weights (allowed:
4 x the unpatched error): [2, 3, 32, 32] unpatched PyTorch float32 4.8e-6, patched 5.9e-6; [2, 3, 40, 24] 5.7e-6 and 4.6e-6.
CLASS_PLANES (every workgroup shape of the resident path at both ends): 0.22 in float32 (0.08 with the normalised
skip) and 0.992 in float16."""
import types

import pytest
import torch

import encoder_norms_restatement as ER

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16]
CODE = {torch.float32: 0, torch.float16: 1}
SHAPES = [(1, 2), (1, 3), (7, 9), (8, 8), (5, 13), (15, 17), (64, 64)]
EDGES = ("max-1", "max", "max+1", "2max+3")                          # planes of resident_max - 1, ... elements, as (1, hw)
# Every workgroup shape of the resident path (launch_inorm in igs_amd/csrc/inorm.hip) at its smallest and its largest plane and at an odd
# size inside: (threads, vectors per thread) of the plain / relu / relu-add-relu modes | of the normalised-skip mode.  SHAPES above stays
# in (64, 4) except (64, 64), EDGES holds the top of the two largest shapes ("max-1" is their odd inside size, "max+1" the streamed
# kernel).  These follow EDGES in the parametrisation, so the offset from the 16-byte grid alternates down the list: the capacities 1024,
# 4096 and 16384 fall on offset 0 (every vector slot of the shape in use), (128, 128) on offset 1.
CLASS_PLANES = [
    (1, 1024),                                                       # (64, 4) | (64, 4): the largest
    (1, 1023),                                                       # (64, 4) | (64, 4): odd, one below
    (1, 1025),                                                       # (256, 4) | (256, 4): the smallest
    (1, 4095),                                                       # (256, 4) | (256, 4): odd, inside
    (1, 4096),                                                       # (256, 4) | (256, 4): the largest, on the grid
    (1, 4097),                                                       # (256, 16) | (1024, 4): the smallest
    (1, 9001),                                                       # (256, 16) | (1024, 4): odd, inside
    (1, 16383),                                                      # (256, 16) | (1024, 4): odd, one below the largest
    (1, 16384),                                                      # (256, 16) | (1024, 4): the largest
    (128, 128),                                                      # (256, 16) | (1024, 4): the quarter-resolution plane of a 512 x 512 input
    (1, 16385),                                                      # (1024, 16) | (1024, 8): the smallest
]
ALL_SHAPES = SHAPES + list(EDGES) + CLASS_PLANES                     # (appended: the seeds and offsets of the earlier cases stay)
INSIDE_NEW = [(1, 9001)]                                             # one plane from the (256, 16) and the (1024, 4) shape: the same size
CLASS_IDS = lambda s: "%dx%d" % s if s in CLASS_PLANES else None     # noqa: E731  (the earlier cases keep the ids they had)
BAND = 64                                                            # sentinel elements on either side of out
SENTINEL = 12345.0


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _resident_max(dtype, mode):
    return int(_lib().igs_instance_norm_resident_max(CODE[dtype], mode))


def _hw(shape, dtype, mode):
    if shape in EDGES:
        m = _resident_max(dtype, mode)
        return (1, {"max-1": m - 1, "max": m, "max+1": m + 1, "2max+3": 2 * m + 3}[shape])
    return shape


def _placed(t, offset):
    """A copy of t that starts `offset` elements into a fresh allocation (so offset 1 puts every plane base off the 16-byte grid)."""
    buf = torch.empty(t.numel() + offset + 8, dtype=t.dtype, device=t.device)
    v = buf[offset: offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _run(x, skip, mode, eps=1e-5, out=None, offset=0):
    """igs_instance_norm_fwd on the current stream.  out=None: a NaN-filled out between two sentinel bands, which are checked."""
    planes, hw = x.shape[0] * x.shape[1], x.shape[2] * x.shape[3]
    banded = out is None
    if banded:
        big = torch.full((2 * BAND + offset + x.numel(),), float("nan"), dtype=x.dtype, device=x.device)
        big[: BAND + offset] = SENTINEL
        big[BAND + offset + x.numel():] = SENTINEL
        out = big[BAND + offset: BAND + offset + x.numel()].view(x.shape)
    rc = _lib().igs_instance_norm_fwd(torch.cuda.current_stream().cuda_stream, x.data_ptr(), skip.data_ptr() if skip is not None else None,
                                      out.data_ptr(), planes, hw, CODE[x.dtype], mode, eps)
    from igs_amd import _cabi
    assert rc == 0, _cabi.last_error()
    if banded:
        assert (big[: BAND + offset] == SENTINEL).all() and (big[BAND + offset + x.numel():] == SENTINEL).all(), "a sentinel band was written"
    return out


def _inputs(planes, hw, dtype, mode, seed, constant_plane=None, offset=0):
    x = _placed(ER.plane_inputs(planes, hw[0], hw[1], dtype, DEV, seed, constant_plane), offset)
    skip = _placed(ER.plane_inputs(planes, hw[0], hw[1], dtype, DEV, seed + 5), offset) if mode in ER.HAS_SKIP else None
    return x, skip


def _compare(out, x, skip, mode, label, eps=1e-5, planes=None):
    x64, k64 = x.double(), (skip.double() if skip is not None else None)
    ref = ER.restate(x64, k64, mode, eps)
    allow = ER.allowance(x64, k64, mode, eps, out.dtype, ref)
    sel = slice(None) if planes is None else planes
    o, r, a = out[0, sel].double(), ref[0, sel], allow[0, sel]
    assert torch.isfinite(o).all(), (label, "an element was not written, or is not finite")
    err = (o - r).abs()
    worst = (err / a).max().item()
    print("%s: max |err| %.3e, max |err| / allowance %.3f" % (label, err.max().item(), worst))
    assert worst <= 1.0, (label, worst, err.max().item())
    return ref


# ---------------------------------------------------------------- every mode, dtype and plane size against float64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=CLASS_IDS)
def test_modes_against_float64(shape, mode, dtype):
    hw = _hw(shape, dtype, mode)
    index = ALL_SHAPES.index(shape)
    for planes in (1, 3) + ((700,) if shape == (8, 8) else ()):
        seed = 9 * index + planes + mode
        offset = (index + planes) % 2                                # half of the cases start one element past the 16-byte grid
        const = 1 if planes >= 3 else None
        x, skip = _inputs(planes, hw, dtype, mode, seed, const, offset)
        out = _run(x, skip, mode, offset=offset)
        label = "%s mode %d %s planes %d offset %d" % (hw, mode, str(dtype)[6:], planes, offset)
        _compare(out, x, skip, mode, label)
        if const is not None and mode in (ER.PLAIN, ER.RELU):
            assert (out[0, const] == 0).all(), (label, "a constant plane must give exactly zero")
    # a constant plane alone
    x = torch.full((1, 1) + tuple(hw), 100.37, dtype=dtype, device=DEV)
    skip = ER.plane_inputs(1, hw[0], hw[1], dtype, DEV, 77) if mode in ER.HAS_SKIP else None
    out = _run(x, skip, mode)
    _compare(out, x, skip, mode, "%s mode %d constant" % (hw, mode))
    if mode in (ER.PLAIN, ER.RELU):
        assert (out == 0).all()


def test_operands_on_different_offsets_take_the_scalar_form():
    """x, skip and out on three different offsets from the 16-byte grid: no vector load can serve all of them."""
    for dtype in DTYPES:
        for hw in ((7, 9), (64, 64), (1, 70001)):
            for mode in ER.MODES:
                x = _placed(ER.plane_inputs(3, hw[0], hw[1], dtype, DEV, 3), 1)
                skip = _placed(ER.plane_inputs(3, hw[0], hw[1], dtype, DEV, 4), 2) if mode in ER.HAS_SKIP else None
                out = _run(x, skip, mode, offset=3)
                _compare(out, x, skip, mode, "%s mode %d %s offsets 1 / 2 / 3" % (hw, mode, str(dtype)[6:]))


# ---------------------------------------------------------------- aliasing and determinism, on both paths
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("shape", [(7, 9), (64, 64), "max", "max+1"] + INSIDE_NEW, ids=CLASS_IDS)
def test_out_is_x_and_a_second_run_give_the_same_bits(shape, mode, dtype):
    hw = _hw(shape, dtype, mode)
    x, skip = _inputs(3, hw, dtype, mode, seed=21, offset=1)
    first = _run(x, skip, mode, offset=1).clone()
    second = _run(x, skip, mode, offset=1)
    assert torch.equal(first.view(torch.int32 if dtype == torch.float32 else torch.int16), second.view(torch.int32 if dtype == torch.float32 else torch.int16))
    keep = x.clone()
    aliased = _run(x, skip, mode, out=x)                            # out == x
    assert aliased.data_ptr() == x.data_ptr() and not torch.equal(x, keep)
    assert torch.equal(aliased, first)
    # the Python layer on operands of its own (aligned allocations: another summation order than at offset 1, so another baseline):
    # inplace writes into its argument, and only then
    from igs_amd import backbone as BB
    sk = skip.clone() if skip is not None else None
    base = _run(keep.clone(), sk, mode)

    def call(t, inplace):
        if mode in ER.HAS_SKIP:
            return BB.residual_tail(t, sk, norm_skip=mode == ER.RELU_ADDNORM_RELU, inplace=inplace)
        return BB.instance_norm(t, relu=mode == ER.RELU, inplace=inplace)

    y = keep.clone()
    r = call(y, True)
    assert r.data_ptr() == y.data_ptr() and torch.equal(r, base)
    y = keep.clone()
    r = call(y, False)
    assert r.data_ptr() != y.data_ptr() and torch.equal(y, keep) and torch.equal(r, base)


# ---------------------------------------------------------------- non-finite planes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ER.MODES)
@pytest.mark.parametrize("shape", [(7, 9), (64, 64), "max", "max+1"] + INSIDE_NEW, ids=CLASS_IDS)
def test_a_non_finite_plane_is_all_nan_and_its_neighbours_are_untouched(shape, mode, dtype):
    hw = _hw(shape, dtype, mode)
    x, skip = _inputs(4, hw, dtype, mode, seed=31)
    n = hw[0] * hw[1]
    x.view(4, n)[1, (2 * n) // 3] = float("nan")
    x.view(4, n)[2, n // 2] = float("inf")
    out = _run(x, skip, mode)
    assert torch.isnan(out[0, 1]).all() and torch.isnan(out[0, 2]).all(), (hw, mode)
    _compare(out, x, skip, mode, "%s mode %d %s beside non-finite planes" % (hw, mode, str(dtype)[6:]), planes=[0, 3])


def test_python_layer_copies_what_is_not_contiguous_once():
    from igs_amd import backbone as BB
    x = ER.plane_inputs(6, 9, 7, torch.float32, DEV, 2).view(2, 3, 9, 7)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    keep = cl.clone()
    ref = BB.instance_norm(x, relu=True)
    out = BB.instance_norm(cl, relu=True, inplace=True)             # copied: the argument stays as it was
    assert torch.equal(out, ref) and torch.equal(cl, keep) and out.is_contiguous()
    sl = x[:, :, :, :5]
    assert torch.equal(BB.residual_tail(sl, sl), BB.residual_tail(sl.contiguous(), sl.contiguous()))      # skip is y: still legitimate
    with pytest.raises(RuntimeError, match="one GPU"):
        BB.residual_tail(x, x.cpu())


# ---------------------------------------------------------------- feature_add_position
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(16, 6, 10, 2), (16, 6, 9, 3), (8, 5, 7, 1), (128, 8, 8, 2), (128, 64, 64, 2)])
def test_position_add_against_float64(case, dtype):
    from igs_amd import _cabi, backbone as BB
    C, h, w, K = case
    g = torch.Generator().manual_seed(C + h + w + K)
    f0, f1 = (torch.randn(2, C, h, w, generator=g, dtype=torch.float64).to(dtype).to(DEV) for _ in range(2))
    r0, r1 = ER.restate_position(f0.double(), f1.double(), K)
    o0, o1 = BB.feature_add_position(f0, f1, K, C)
    assert o0.data_ptr() != f0.data_ptr() and o1.data_ptr() != f1.data_ptr() and o0.dtype == dtype and o0.shape == f0.shape
    for o, r, name in ((o0, r0, "feature0"), (o1, r1, "feature1")):
        err = (o.double() - r).abs()
        worst = (err / ER.position_allowance(r, dtype)).max().item()
        print("%s %s %s: max |err| %.3e, max |err| / allowance %.3f" % (case, str(dtype)[6:], name, err.max().item(), worst))
        assert worst <= 1.0, (case, name, worst)
    a0, a1 = f0.clone(), f1.clone()
    i0, i1 = _cabi.ext()._encoder.position_add(a0, a1, K, True)                              # in place: the same bits
    assert i0.data_ptr() == a0.data_ptr() and i1.data_ptr() == a1.data_ptr()
    assert torch.equal(i0, o0) and torch.equal(i1, o1)
    # operands one element past the vector grid take the scalar form
    s0, s1 = _cabi.ext()._encoder.position_add(_placed(f0, 1), _placed(f1, 1), K, True)
    for o, r in ((s0, r0), (s1, r1)):
        assert ((o.double() - r).abs() <= ER.position_allowance(r, dtype)).all(), (case, "scalar form")


# ---------------------------------------------------------------- the stand-in encoder, patched with both binding calls
def _front_end(enc, ns, img, splits):
    f = enc(img)[0]
    f0, f1 = f.chunk(2, dim=0)
    return ns.feature_add_position(f0.contiguous(), f1.contiguous(), splits, f.shape[1])


@pytest.mark.parametrize("shape,splits", [((2, 3, 32, 32), 2), ((2, 3, 40, 24), 1)])
def test_stand_in_encoder_patched_against_its_float64_run(shape, splits):
    """The patched float32 run may be at most 4 x as far from the float64 run of the same weights as the unpatched float32 PyTorch run is
    (floor 1e-5): the reference path sets the scale, the factor covers another summation order through twelve convolutions."""
    from igs_amd import backbone as BB
    g = torch.Generator().manual_seed(shape[2])
    img = torch.randn(*shape, generator=g).to(DEV)
    enc = ER.make_encoder(seed=4).to(DEV)
    enc64 = ER.make_encoder(seed=4).to(DEV).double()
    plain = types.SimpleNamespace(feature_add_position=lambda a, b, k, c: ER.restate_position(a, b, k))
    with torch.no_grad():
        want = _front_end(enc64, plain, img.double(), splits)
        eager = _front_end(enc, plain, img, splits)
        keys = list(enc.state_dict().keys())
        ns = types.SimpleNamespace(feature_add_position=plain.feature_add_position)
        assert BB.use_native_encoder_norms(enc) == 15 and BB.use_native_position(ns) == 1
        assert list(enc.state_dict().keys()) == keys
        native = _front_end(enc, ns, img, splits)
    e_eager = max((a.double() - b).abs().max().item() for a, b in zip(eager, want))
    e_native = max((a.double() - b).abs().max().item() for a, b in zip(native, want))
    print("%s: max |err| against float64: unpatched PyTorch float32 %.3e, patched %.3e (allowed %.3e)" % (shape, e_eager, e_native, max(4 * e_eager, 1e-5)))
    assert all(torch.isfinite(t).all() for t in native)
    assert e_native <= max(4 * e_eager, 1e-5), (e_native, e_eager)
