"""The backward of the fused 2x upsample + 3x3 convolution without a GPU (igs_amd/csrc/upconv_bwd.hip, igs_amd/motion.py): the exports
and their declared signatures, the scratch size, the C ABI's refusals before any HIP call, the transposed pack's layout, the float64
restatement (tests/upconv_grad_restatement.py) against float64 autograd, its derived bounds against PyTorch's own float32 gradients, a CPU
emulation of the half roundings and every wrong variant, and the Python layer driven through a recorder."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upconv_grad_restatement as G
import upconv_restatement as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_upconv_bwd_scratch_bytes", "igs_upconv_bwd")
REFS = ("dx64", "dw64", "db64")
BOUNDS = ("bound_dx", "bound_dw", "bound_db")


def _eager(x, conv):
    return conv(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))


# ---------------------------------------------------------------- the C ABI
def test_exports_and_declared_signatures():
    from igs_amd import _cabi
    L = _cabi.lib()
    h = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    for name in NAMES:
        assert name in _cabi.EXPORTS and hasattr(L, name)
        m = re.search(r"\b%s\(([^;]*)\);" % name, h)
        assert m, name
        assert len(m.group(1).split(",")) == len(_cabi.SIGNATURES[name][1]), name
    assert len(_cabi.SIGNATURES["igs_upconv_bwd"][1]) == 20 and len(_cabi.SIGNATURES["igs_upconv_bwd_scratch_bytes"][1]) == 6
    assert _cabi.SIGNATURES["igs_upconv_bwd_scratch_bytes"][0] is C.c_longlong
    assert "#define IGS_UPCONV_BWD_SLICES %d" % G.SLICES in h
    assert '"upconv_bwd.hip"' in open(os.path.join(ROOT, "igs_amd", "build.py")).read()


def test_scratch_bytes():
    from igs_amd import _cabi
    f = _cabi.lib().igs_upconv_bwd_scratch_bytes
    for (ci, co, N, H, W) in G.SLICE_CASES + G.CPU_CASES + ((128, 128, 4, 64, 64), (128, 128, 32, 64, 64)):
        slices = min(G.wgrad_tiles(N, H, W), G.SLICES)
        want = slices * (9 * -(-ci // 32) * -(-co // 32) * 1024 + 128) * 4
        for dt in (0, 1):
            assert f(N, ci, co, H, W, dt) == want, (ci, co, N, H, W, dt)
    assert [G.wgrad_tiles(*c[2:]) for c in G.SLICE_CASES] == [6, 64, 96]                  # fewer than, exactly and more than the slices
    assert f(4, 128, 128, 64, 64, 0) == f(32, 128, 128, 64, 64, 0) == 64 * (144 * 1024 + 128) * 4     # it does not grow with N
    assert f(0, 8, 8, 4, 4, 0) == 0
    for N, ci, co, H, W, dt in ((-1, 8, 8, 4, 4, 0), (1, 0, 8, 4, 4, 0), (1, 129, 8, 4, 4, 0), (1, 8, 0, 4, 4, 0), (1, 8, 129, 4, 4, 0), (1, 8, 8, 0, 4, 0),
                                (1, 8, 8, 4097, 4, 0), (1, 8, 8, 4, 0, 0), (1, 8, 8, 4, 4097, 0), (5, 8, 8, 1024, 1024, 0), (1, 8, 8, 4, 4, 2), (1, 8, 8, 4, 4, -1)):
        assert f(N, ci, co, H, W, dt) == -1, (N, ci, co, H, W, dt)


def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1) with a message, never IGS_RAST_E_HIP (-2): without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    raw = C.create_string_buffer(4096 + 64)
    p = (C.addressof(raw) + 63) & ~63
    err = _cabi.last_error
    PTRS = ("x", "wpack_t", "dout", "scratch", "dx", "dw", "db")

    def bwd(N=2, ci=8, co=8, H=6, W=10, xdt=0, cdt=0, xs=None, sb=None, **ptrs):
        xs = xs or (ci * H * W, H * W, W, 1)
        q = {k: p for k in PTRS}
        q.update(ptrs)
        if sb is None:
            sb = max(L.igs_upconv_bwd_scratch_bytes(N, ci, co, H, W, cdt), 0)
        return L.igs_upconv_bwd(None, N, ci, co, H, W, xdt, q["x"], *xs, cdt, q["wpack_t"], q["dout"], q["scratch"], sb, q["dx"], q["dw"], q["db"])

    bad = ((dict(N=-1), "N out of range"), (dict(ci=0), "Cin out of range"), (dict(ci=129), "Cin out of range"), (dict(co=0), "Cout out of range"),
           (dict(co=129), "Cout out of range"), (dict(H=0), "H out of range"), (dict(H=4097), "H out of range"), (dict(W=0), "W out of range"),
           (dict(W=4097), "W out of range"), (dict(N=5, H=1024, W=1024), "N * H * W out of range"), (dict(xdt=2), "dtype"), (dict(xdt=-1), "dtype"),
           (dict(cdt=2), "dtype"), (dict(cdt=-1), "dtype"), (dict(xs=(480, 1, 80, 8)), "channels-last"),
           (dict(xs=(480, 60, 11, 1)), "plane must be contiguous"), (dict(xs=(-1, 60, 10, 1)), "negative"), (dict(xs=(480, -60, 10, 1)), "negative"))
    for kw, what in bad:
        assert bwd(**kw) == -1 and what in err() and "igs_upconv_bwd" in err(), (kw, err())
    for name in ("wpack_t", "dout", "scratch"):
        assert bwd(**{name: None}) == -1 and "NULL" in err(), name
    assert bwd(x=None) == -1 and "x is NULL" in err()                    # dw wanted
    assert bwd(x=p + 2) == -1 and "aligned" in err()                     # a float32 x on a 2-byte boundary
    assert bwd(x=p + 1, xdt=1) == -1 and "aligned" in err()
    assert bwd(dx=p + 2) == -1 and "aligned" in err()
    assert bwd(dx=p + 1, xdt=1) == -1 and "aligned" in err()
    assert bwd(dout=p + 2) == -1 and "aligned" in err()
    assert bwd(dout=p + 1, cdt=1) == -1 and "aligned" in err()
    assert bwd(dw=p + 2) == -1 and "4 bytes" in err()
    assert bwd(db=p + 2) == -1 and "4 bytes" in err()
    assert bwd(wpack_t=p + 8) == -1 and "16 bytes" in err()
    assert bwd(scratch=p + 8) == -1 and "16 bytes" in err()
    need = L.igs_upconv_bwd_scratch_bytes(2, 8, 8, 6, 10, 0)
    assert bwd(sb=need - 1) == -1 and "scratch_bytes" in err()
    assert bwd(sb=0) == -1 and "scratch_bytes" in err()
    # nothing wanted: 0 without a launch; N == 0 with nothing wanted likewise, whatever the pointers
    assert bwd(dx=None, dw=None, db=None) == 0
    assert bwd(x=None, dx=None, dw=None, db=None) == 0                   # x may be NULL when dw is
    assert bwd(N=0, **{k: None for k in PTRS}) == 0
    del raw


@pytest.mark.parametrize("ci,co", G.WIDTHS + ((128, 128),))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_transposed_pack_puts_every_weight_where_the_header_says(ci, co, dtype):
    from igs_amd import _cabi, motion
    _, conv = UR.make_case(ci, co, 1, 1, 1)
    plain = motion.pack_upsample_conv(conv, dtype)
    assert isinstance(plain, tuple) and len(plain) == 2                  # the default return value is unchanged
    wpack, bpack, wpack_t = motion.pack_upsample_conv(conv, dtype, transposed=True)
    assert torch.equal(wpack, plain[0]) and torch.equal(bpack, plain[1])
    half = dtype == torch.float16
    assert wpack_t.dtype == dtype and wpack_t.is_contiguous() and wpack_t.numel() == _cabi.lib().igs_upconv_pack_elems(co, ci, int(half))
    w = conv.weight.detach().to(dtype).numpy()
    want = G.pack_t_restate(w, half)
    assert np.array_equal(wpack_t.numpy(), want)
    assert (w != 0).all() and np.count_nonzero(want) == w.size           # every weight once, zeros everywhere else
    # and it is the forward's pack of the transposed, flipped convolution
    assert np.array_equal(want, UR.pack_restate(np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)), half))


# ---------------------------------------------------------------- the restatement and the bounds
@pytest.mark.parametrize("case", G.CPU_CASES, ids=lambda c: "x".join(map(str, c)))
def test_restatement_is_float64_autograd(case):
    x, conv, g, R = G.reference(case)
    N, H, W = case[2:]
    M = N * 4 * H * W
    sums = (R["bound_dx"] / G.gamma(9 * case[1] + 16, G.U24), R["bound_dw"] / G.gamma(M + 4, G.U24), R["bound_db"] / G.gamma(M, G.U24))
    for got, ref, S in zip(G.autograd64(x, conv.weight, g), REFS, sums):
        assert (S > 0).all()
        assert float(((got - R[ref]).abs() / S).max()) <= 1e-12, ref


@pytest.mark.parametrize("case", G.CPU_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_bounds_hold_for_torch_and_reject_every_wrong_variant(case, half):
    for x_half in ((False, True) if half else (False,)):
        x, conv, g, R = G.reference(case, half, x_half)
        got = G.emulate_half(x, conv.weight, g) if half else G.autograd32(x, conv.weight, g)
        for t, ref, b in zip(got, REFS, BOUNDS):
            w = G.worst(t, R[ref], R[b])
            print(case, "half" if half else "float32", "x_half" if x_half else "", ref, "worst |error| / bound = %.3g" % w)
            assert w <= 1.0, (ref, w)
        for kind in G.DX_VARIANTS:
            if G.variant_applies(kind, case):
                assert G.worst(G.dx_variant(kind, x, conv.weight, g), R["dx64"], R["bound_dx"]) > 1.0, kind
        for kind in G.DW_VARIANTS:
            assert G.worst(G.dw_variant(kind, x, conv.weight, g), R["dw64"], R["bound_dw"]) > 1.0, kind


def test_square_width_rejects_an_untransposed_weight_and_single_pixel_g_is_local():
    case = (33, 33, 2, 5, 7)
    x, conv, g, R = G.reference(case)
    assert G.variant_applies("weight_not_transposed", case) and not G.variant_applies("weight_not_transposed", (33, 65, 2, 5, 7))
    assert G.worst(G.dx_variant("weight_not_transposed", x, conv.weight, g), R["dx64"], R["bound_dx"]) > 1.0
    assert not G.variant_applies("align_corners", (7, 5, 2, 1, 1))
    # g zero outside one pixel (2H / 2, 2W - 1) of the last image: dx is non-zero only under its 3 x 3 taps' footprint, image 0 untouched
    x, conv, g, R = G.reference((7, 5, 2, 5, 7), single_pixel=True)
    assert int((g != 0).sum()) == 5
    dx = R["dx64"]
    assert (dx[0] == 0).all() and (dx[1, :, :, :5] == 0).all() and (dx[1, :, 1:4, 5:] != 0).all() and (dx[1, :, 0, 5:] == 0).all()


# ---------------------------------------------------------------- the Python layer
class _Recorder:
    """Stands in for the compiled module: records what the Python layer hands it."""

    def __init__(self):
        self.fwd, self.bwd = [], []
        self._upconv = self

    def upconv_fwd(self, x, wpack, bpack, Cout):
        self.fwd.append((x, wpack, bpack, Cout))
        return torch.zeros(x.shape[0], Cout, 2 * x.shape[2], 2 * x.shape[3], dtype=wpack.dtype)

    def upconv_bwd(self, x, wpack_t, dout, want_x, want_w, want_b):
        self.bwd.append((x, wpack_t, dout, want_x, want_w, want_b))
        Cout, Cin = dout.shape[1], x.shape[1]
        return (torch.zeros_like(x) if want_x else None, torch.zeros(Cout, Cin, 3, 3) if want_w else None, torch.zeros(Cout) if want_b else None)


@pytest.fixture
def rec(monkeypatch):
    from igs_amd import motion
    r = _Recorder()
    monkeypatch.setattr(motion, "_ext", lambda: r)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setitem(motion.UPCONV_BWD_NATIVE, torch.float32, True)
    monkeypatch.setitem(motion.UPCONV_BWD_NATIVE, torch.float16, True)
    return r


def test_without_grad_it_is_upsample_conv(rec):
    from igs_amd import motion
    x, conv = UR.make_case(33, 65, 2, 3, 4)
    out = motion.upsample_conv_autograd(x, conv)                         # nothing requires grad
    assert out.grad_fn is None and len(rec.fwd) == 1 and not rec.bwd
    assert rec.fwd[-1][0] is x and rec.fwd[-1][1] is conv.__dict__[motion.UPCONV_CACHE]["pack"][0]
    assert motion.UPCONV_TRAIN_CACHE not in conv.__dict__ and motion.UPCONV_TRAIN_CACHE != motion.UPCONV_CACHE
    conv.requires_grad_(True)
    with torch.no_grad():
        out = motion.upsample_conv_autograd(x, conv, conv_dtype=torch.float16)
    assert out.grad_fn is None and out.dtype == torch.float16 and len(rec.fwd) == 2 and motion.UPCONV_TRAIN_CACHE not in conv.__dict__


def test_with_grad_it_saves_x_itself_and_the_transposed_pack(rec):
    from igs_amd import motion
    x, conv = UR.make_case(33, 65, 2, 3, 4)
    conv.requires_grad_(True)
    big = torch.zeros(4, 40, 3, 4)
    v = big[1:3, 2:35].requires_grad_(True)                             # a slice of n and c: handed over, and saved, as it is
    out = motion.upsample_conv_autograd(v, conv)
    assert out.grad_fn is not None and out.shape == (2, 65, 6, 8) and out.dtype == torch.float32
    packs = conv.__dict__[motion.UPCONV_TRAIN_CACHE]["pack"]
    assert len(packs) == 3 and all(torch.equal(a, b) for a, b in zip(packs, motion.pack_upsample_conv(conv, transposed=True)))
    assert rec.fwd[-1][0] is v and rec.fwd[-1][1] is packs[0] and rec.fwd[-1][2] is packs[1]
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == v.data_ptr() and saved[0].stride() == v.stride() and saved[1].data_ptr() == packs[2].data_ptr()
    g = torch.ones(2, 65, 8, 6).transpose(2, 3)                          # a non-contiguous d out is copied once
    out.backward(g)
    xb, wt, dout, wx, ww, wb = rec.bwd[-1]
    assert xb.data_ptr() == v.data_ptr() and xb.stride() == v.stride() and wt.data_ptr() == packs[2].data_ptr()
    assert dout.is_contiguous() and torch.equal(dout, g) and (wx, ww, wb) == (True, True, True)
    assert conv.weight.grad.shape == conv.weight.shape and conv.bias.grad.shape == conv.bias.shape
    with pytest.raises(RuntimeError):                                    # once differentiable
        out2 = motion.upsample_conv_autograd(v, conv)
        (gx,) = torch.autograd.grad(out2.sum(), v, create_graph=True)
        gx.sum().backward()


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (True, True, True)])
def test_want_flags_follow_requires_grad(rec, want):
    from igs_amd import motion
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    x.requires_grad_(want[0])
    conv.weight.requires_grad_(want[1])
    conv.bias.requires_grad_(want[2])
    motion.upsample_conv_autograd(x, conv).sum().backward()
    assert rec.bwd[-1][3:] == want
    assert (x.grad is not None, conv.weight.grad is not None, conv.bias.grad is not None) == want


def test_half_parameters_get_half_gradients_and_no_bias_works(rec):
    from igs_amd import motion
    conv = torch.nn.Conv2d(7, 5, 3, padding=1, bias=False).half()
    x = torch.zeros(2, 7, 3, 4, dtype=torch.float16, requires_grad=True)
    out = motion.upsample_conv_autograd(x, conv, conv_dtype=torch.float16)
    assert out.dtype == torch.float16 and (rec.fwd[-1][2] == 0).all()
    out.sum().backward()
    assert rec.bwd[-1][3:] == (True, True, False) and rec.bwd[-1][2].dtype == torch.float16
    assert conv.weight.grad.dtype == torch.float16 and x.grad.dtype == torch.float16     # (the recorder returns float32 dw: cast once)
    # a float32 d out of an explicit float16 call is cast to the compute dtype
    conv32 = torch.nn.Conv2d(7, 5, 3, padding=1)
    out = motion.upsample_conv_autograd(x.detach().float(), conv32, conv_dtype=torch.float16)
    out.float().sum().backward()
    assert rec.bwd[-1][2].dtype == torch.float16 and conv32.weight.grad.dtype == torch.float32 and conv32.bias.grad.dtype == torch.float32


def test_train_cache_repacks_after_an_in_place_update(rec):
    from igs_amd import motion
    x, conv = UR.make_case(33, 65, 2, 3, 4)
    conv.requires_grad_(True)
    motion.upsample_conv_autograd(x, conv)
    first = conv.__dict__[motion.UPCONV_TRAIN_CACHE]["pack"]
    motion.upsample_conv_autograd(x, conv)
    assert conv.__dict__[motion.UPCONV_TRAIN_CACHE]["pack"] is first and rec.fwd[-1][1] is first[0]
    with torch.no_grad():
        conv.weight.mul_(2.0)                                            # what an optimiser step does
    out = motion.upsample_conv_autograd(x, conv)
    second = conv.__dict__[motion.UPCONV_TRAIN_CACHE]["pack"]
    assert second is not first and all(torch.equal(a, b) for a, b in zip(second, motion.pack_upsample_conv(conv, transposed=True)))
    assert out.grad_fn.saved_tensors[1].data_ptr() == second[2].data_ptr()
    assert motion.UPCONV_CACHE not in conv.__dict__                      # the forward-only cache is another key, untouched
    # an explicit pack is used as given; the forward-only pair is refused
    mine = motion.pack_upsample_conv(conv, transposed=True)
    motion.upsample_conv_autograd(x, conv, packed=mine)
    assert rec.fwd[-1][1] is mine[0]
    with pytest.raises(ValueError, match="transposed=True"):
        motion.upsample_conv_autograd(x, conv, packed=mine[:2])
    with pytest.raises(ValueError, match="packed holds"):
        motion.upsample_conv_autograd(x, conv, packed=mine, conv_dtype=torch.float16)


def test_routing_false_is_the_eager_lines_and_an_explicit_dtype_is_native(rec, monkeypatch):
    from igs_amd import motion
    assert set(motion.UPCONV_BWD_NATIVE) == {torch.float32, torch.float16}
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    conv.requires_grad_(True)
    monkeypatch.setitem(motion.UPCONV_BWD_NATIVE, torch.float32, False)
    out = motion.upsample_conv_autograd(x, conv)
    assert not rec.fwd and out.grad_fn is not None and torch.equal(out, _eager(x, conv))
    motion.upsample_conv_autograd(x, conv, conv_dtype=torch.float32)
    assert len(rec.fwd) == 1


def test_refusals_match_upsample_conv(monkeypatch):
    from igs_amd import motion
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    conv.requires_grad_(True)
    calls = ((ValueError, lambda f: f(x[0], conv)), (ValueError, lambda f: f(x[:, :5], conv)),
             (NotImplementedError, lambda f: f(x.double(), conv)), (NotImplementedError, lambda f: f(x.bfloat16(), conv)),
             (NotImplementedError, lambda f: f(x, conv, conv_dtype=torch.bfloat16)),
             (NotImplementedError, lambda f: f(x, torch.nn.Conv2d(7, 5, 3, padding=0))),
             (NotImplementedError, lambda f: f(x, torch.nn.Conv2d(7, 5, 3, padding=1, padding_mode="replicate"))),
             (NotImplementedError, lambda f: f(torch.zeros(1, 129, 2, 2), torch.nn.Conv2d(129, 5, 3, padding=1))),
             (NotImplementedError, lambda f: f(x, torch.nn.Linear(7, 5))))
    for exc, call in calls:
        with pytest.raises(exc) as a:
            call(motion.upsample_conv)
        with pytest.raises(exc) as b:
            call(motion.upsample_conv_autograd)
        assert str(b.value) == str(a.value).replace("upsample_conv:", "upsample_conv_autograd:")
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # with grad, on the CPU: no eager fall-back here
        motion.upsample_conv_autograd(x, conv, conv_dtype=torch.float32)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(NotImplementedError, match="sizes out of range"):
        motion.upsample_conv_autograd(torch.zeros(1, 7, 1, 4097), conv, conv_dtype=torch.float32)


def test_upsample_conv_under_grad_is_still_eager(rec):
    from igs_amd import motion
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    conv.requires_grad_(True)
    out = motion.upsample_conv(x, conv)
    assert out.grad_fn is not None and torch.equal(out, _eager(x, conv)) and not rec.fwd and not rec.bwd
