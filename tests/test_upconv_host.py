"""The fused 2x upsample + 3x3 convolution without a GPU (igs_amd/csrc/upconv.hip, igs_amd/motion.py): the exports and their declared
signatures, the pack's element count and layout, the float64 restatement and its derived bound (tests/upconv_restatement.py) against
PyTorch's own float32 result and against every wrong variant, the C ABI's refusals before any HIP call, the Python layer's exceptions,
the eager path under grad and the cache on the module."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upconv_restatement as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_upconv_pack_elems", "igs_upconv_fwd")


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
    assert len(_cabi.SIGNATURES["igs_upconv_fwd"][1]) == 16 and len(_cabi.SIGNATURES["igs_upconv_pack_elems"][1]) == 3
    assert "#define IGS_UPCONV_MAX_WIDTH 128" in h and "#define IGS_UPCONV_MAX_HW 4096" in h and "#define IGS_UPCONV_MAX_PIXELS (1 << 22)" in h
    assert '"upconv.hip"' in open(os.path.join(ROOT, "igs_amd", "build.py")).read()


def test_pack_elems():
    from igs_amd import _cabi, motion
    L = _cabi.lib()
    for ci, co in UR.WIDTHS + ((128, 128), (32, 33), (1, 1)):
        for dt in (0, 1):
            assert L.igs_upconv_pack_elems(ci, co, dt) == 9 * -(-ci // 32) * -(-co // 32) * 1024, (ci, co, dt)
    assert L.igs_upconv_pack_elems(128, 128, 0) == 144 * 1024
    for ci, co, dt in ((129, 128, 0), (0, 128, 0), (128, 0, 0), (128, 129, 1), (128, 128, 2), (128, 128, -1)):
        assert L.igs_upconv_pack_elems(ci, co, dt) == -1, (ci, co, dt)
    assert (motion.UPCONV_MAX_WIDTH, motion.UPCONV_MAX_HW, motion.UPCONV_MAX_PIXELS) == (128, 4096, 1 << 22)
    assert set(motion.UPCONV_NATIVE) == {torch.float32, torch.float16}


@pytest.mark.parametrize("ci,co", UR.WIDTHS + ((128, 128),))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_pack_puts_every_weight_where_the_header_says(ci, co, dtype):
    from igs_amd import _cabi, motion
    _, conv = UR.make_case(ci, co, 1, 1, 1)
    wpack, bpack = motion.pack_upsample_conv(conv, dtype)
    half = dtype == torch.float16
    assert wpack.dtype == dtype and wpack.is_contiguous() and wpack.numel() == _cabi.lib().igs_upconv_pack_elems(ci, co, int(half))
    w = conv.weight.detach().to(dtype).numpy()
    want = UR.pack_restate(w, half)
    assert np.array_equal(wpack.numpy(), want)
    assert (w != 0).all() and np.count_nonzero(want) == w.size           # every weight once, zeros everywhere else
    assert bpack.dtype == torch.float32 and bpack.shape == (128,)
    assert torch.equal(bpack[:co], conv.bias.detach()) and (bpack[co:] == 0).all()
    nb = torch.nn.Conv2d(ci, co, 3, padding=1, bias=False)
    assert (motion.pack_upsample_conv(nb, dtype)[1] == 0).all()


def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1) with a message, never IGS_RAST_E_HIP (-2): without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    raw = C.create_string_buffer(4096 + 64)
    p = (C.addressof(raw) + 63) & ~63
    err = _cabi.last_error
    PTRS = ("x", "wpack", "bpack", "out")

    def fwd(N=2, ci=8, co=8, H=6, W=10, xdt=0, cdt=0, xs=None, **ptrs):
        xs = xs or (ci * H * W, H * W, W, 1)
        q = {k: p for k in PTRS}
        q.update(ptrs)
        return L.igs_upconv_fwd(None, N, ci, co, H, W, xdt, q["x"], *xs, cdt, q["wpack"], q["bpack"], q["out"])

    bad = ((dict(N=-1), "N out of range"), (dict(ci=0), "Cin out of range"), (dict(ci=129), "Cin out of range"), (dict(co=0), "Cout out of range"),
           (dict(co=129), "Cout out of range"), (dict(H=0), "H out of range"), (dict(H=4097), "H out of range"), (dict(W=0), "W out of range"),
           (dict(W=4097), "W out of range"), (dict(N=5, H=1024, W=1024), "N * H * W out of range"), (dict(xdt=2), "dtype"), (dict(xdt=-1), "dtype"),
           (dict(cdt=2), "dtype"), (dict(cdt=-1), "dtype"), (dict(xs=(480, 1, 80, 8)), "channels-last"),
           (dict(xs=(480, 60, 11, 1)), "plane must be contiguous"), (dict(xs=(-1, 60, 10, 1)), "negative"), (dict(xs=(480, -60, 10, 1)), "negative"))
    for kw, what in bad:
        assert fwd(**kw) == -1 and what in err() and "igs_upconv_fwd" in err(), (kw, err())
    for name in PTRS:
        assert fwd(**{name: None}) == -1 and "NULL" in err(), name
    assert fwd(x=p + 2) == -1 and "aligned" in err()                     # a float32 x on a 2-byte boundary
    assert fwd(x=p + 1, xdt=1) == -1 and "aligned" in err()              # a float16 x on an odd address
    assert fwd(out=p + 2) == -1 and "aligned" in err()
    assert fwd(out=p + 1, cdt=1) == -1 and "aligned" in err()
    assert fwd(wpack=p + 8) == -1 and "16 bytes" in err()
    assert fwd(bpack=p + 4) == -1 and "16 bytes" in err()
    assert fwd(N=0, **{k: None for k in PTRS}) == 0                      # nothing to do: 0 without a launch, whatever the pointers
    del raw


# ---------------------------------------------------------------- the restatement and the bound
@pytest.mark.parametrize("case", UR.CASES, ids=lambda c: "x".join(map(str, c)))
def test_bound_holds_for_torch_and_rejects_every_wrong_variant(case):
    x, conv, r = UR.reference(case)
    rh = UR.reference(case, half=True)[2]
    assert r["out64"].shape == (case[2], case[1], 2 * case[3], 2 * case[4])
    with torch.no_grad():
        f32 = UR.worst(_eager(x, conv), r["out64"], r["bound"])
    f16 = UR.worst(UR.emulate_half(x, conv.weight, conv.bias), rh["out64"], rh["bound"])
    print("%s: torch float32 %.3f of the bound, emulated half %.3f" % (case, f32, f16))
    assert f32 <= 1.0 and f16 <= 1.0
    assert (rh["bound"] > r["bound"]).all()
    for kind in UR.VARIANTS:
        if kind in UR.UPSAMPLING_VARIANTS and case[3] * case[4] == 1:
            assert torch.equal(UR.variant(kind, x, conv.weight, conv.bias), r["out64"])
            continue
        wrong = UR.variant(kind, x, conv.weight, conv.bias)
        a, b = UR.worst(wrong, r["out64"], r["bound"]), UR.worst(wrong, rh["out64"], rh["bound"])
        print("    %-28s %.3g x the float32 bound, %.3g x the float16 bound" % (kind, a, b))
        assert a > 1.0 and b > 1.0, (kind, a, b)
    if case[1] > 1:                              # (a single channel's one draw of 0.4 randn can fall inside the float16 bound)
        nobias = UR.restate(x, conv.weight, None)["out64"]
        assert UR.worst(nobias, r["out64"], r["bound"]) > 1.0 and UR.worst(nobias, rh["out64"], rh["bound"]) > 1.0


def test_restatement_is_the_definition_at_a_pixel():
    """out64 against the issue's formula written out for a few outputs: source index (dst + 0.5) / 2 - 0.5 clamped at 0, the neighbour at
    the last row / column, zero outside the 2H x 2W map."""
    x, conv, r = UR.reference((7, 5, 2, 17, 3))
    x64, w64, b64 = x.double(), conv.weight.double(), conv.bias.double()
    H, W = x.shape[2:]

    def up(n, c, Y, X):
        if not (0 <= Y < 2 * H and 0 <= X < 2 * W):
            return 0.0
        sy, sx = max((Y + 0.5) / 2 - 0.5, 0.0), max((X + 0.5) / 2 - 0.5, 0.0)
        y0, x0 = int(sy), int(sx)
        y1, x1 = min(y0 + 1, H - 1), min(x0 + 1, W - 1)
        fy, fx = sy - y0, sx - x0
        v = x64[n, c]
        return float((1 - fy) * ((1 - fx) * v[y0, x0] + fx * v[y0, x1]) + fy * ((1 - fx) * v[y1, x0] + fx * v[y1, x1]))

    for n, o, Y, X in ((0, 0, 0, 0), (1, 4, 33, 5), (0, 2, 16, 3), (1, 1, 1, 0), (0, 3, 32, 4)):
        s = float(b64[o]) + sum(float(w64[o, c, dy, dx]) * up(n, c, Y + dy - 1, X + dx - 1) for c in range(7) for dy in range(3) for dx in range(3))
        assert abs(s - float(r["out64"][n, o, Y, X])) <= 1e-12 * float(r["S"][n, o, Y, X])


# ---------------------------------------------------------------- the Python layer
def test_python_layer_refusals():
    from igs_amd import motion
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    f = motion.upsample_conv
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, conv)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x.half(), conv, conv_dtype=torch.float16)
        with pytest.raises(ValueError, match="x must be"):
            f(x[0], conv)
        with pytest.raises(ValueError, match="x must be"):
            f(x[:, :6], conv)
        for bad in (torch.float64, torch.bfloat16):
            with pytest.raises(NotImplementedError, match="float32 or float16"):
                f(x.to(bad), conv)
        with pytest.raises(NotImplementedError, match="conv_dtype"):
            f(x, conv, conv_dtype=torch.bfloat16)
        nn = torch.nn
        for other in (nn.Conv2d(7, 5, 3, padding=0), nn.Conv2d(7, 5, 3, stride=2, padding=1), nn.Conv2d(7, 5, 5, padding=2),
                      nn.Conv2d(7, 5, 3, padding=2, dilation=2), nn.Conv2d(7, 7, 3, padding=1, groups=7), nn.Conv2d(7, 5, (3, 1), padding=1),
                      nn.Conv2d(7, 5, 3, padding=1, padding_mode="replicate"), nn.Conv2d(7, 5, 3, padding="same"), nn.Conv2d(129, 5, 3, padding=1),
                      nn.Conv2d(7, 129, 3, padding=1), nn.ConvTranspose2d(7, 5, 3, padding=1), nn.Linear(7, 5)):
            with pytest.raises(NotImplementedError, match="conv must be|must be in 1..128"):
                f(x, other)
        assert conv.__dict__.get(motion.UPCONV_CACHE) is None            # a refusal leaves the module as it was


def test_compiled_module_refusals():
    from igs_amd import _cabi, motion
    E = _cabi.ext()._upconv
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    wpack, bpack = motion.pack_upsample_conv(conv)
    assert E.pack_elems(7, 5, False) == wpack.numel() and E.pack_elems(129, 5, False) == -1 and E.pack_elems(7, 0, True) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.upconv_fwd(x, wpack, bpack, 5)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.upconv_fwd(x.double(), wpack, bpack, 5)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.upconv_fwd(x, wpack.bfloat16(), bpack, 5)
    for xx, ww, bb, co in ((x[0], wpack, bpack, 5), (x, wpack[:-1], bpack, 5), (x, wpack, bpack[:5], 5), (x, wpack, bpack, 33)):
        with pytest.raises(RuntimeError, match="shape"):
            E.upconv_fwd(xx, ww, bb, co)
    with pytest.raises(RuntimeError, match="1..128"):
        E.upconv_fwd(torch.zeros(1, 129, 1, 1), wpack, bpack, 5)
    with pytest.raises(RuntimeError, match="out of range"):
        E.upconv_fwd(torch.zeros(1, 7, 1, 4097), wpack, bpack, 5)


def test_grad_path_is_the_eager_two_lines_on_any_device():
    """With grad enabled and a parameter (or x) requiring it the call is conv(F.interpolate(...)) itself: CPU tensors are served, bit for
    bit, and the result carries the graph."""
    from igs_amd import motion
    x, conv = UR.make_case(7, 5, 2, 3, 4)
    conv.requires_grad_(True)
    out = motion.upsample_conv(x, conv)
    assert out.grad_fn is not None and torch.equal(out, _eager(x, conv))
    out.square().sum().backward()
    assert conv.weight.grad is not None and conv.weight.grad.abs().sum() > 0
    conv.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    out = motion.upsample_conv(xg, conv)
    assert out.grad_fn is not None and torch.equal(out, _eager(x, conv))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.upsample_conv(xg, conv)


class _Recorder:
    """Stands in for the compiled module: records what the Python layer hands it."""

    def __init__(self):
        self.calls = []
        self._upconv = self

    def upconv_fwd(self, x, wpack, bpack, Cout):
        self.calls.append((x, wpack, bpack, Cout))
        return torch.zeros(x.shape[0], Cout, 2 * x.shape[2], 2 * x.shape[3], dtype=wpack.dtype)


def test_cache_repacks_after_an_in_place_update_and_layouts_are_copied(monkeypatch):
    from igs_amd import motion
    x, conv = UR.make_case(33, 65, 2, 3, 4)
    rec = _Recorder()
    monkeypatch.setattr(motion, "_ext", lambda: rec)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with torch.no_grad():
        out = motion.upsample_conv(x, conv)
        assert out.shape == (2, 65, 6, 8) and out.dtype == torch.float32
        first = rec.calls[-1]
        assert first[0] is x and torch.equal(first[1], motion.pack_upsample_conv(conv)[0])
        motion.upsample_conv(x, conv)
        assert rec.calls[-1][1] is first[1] and rec.calls[-1][2] is first[2]             # the same pack, not packed again
        conv.weight.mul_(2.0)                                                           # what an optimiser step does
        motion.upsample_conv(x, conv)
        assert rec.calls[-1][1] is not first[1] and torch.equal(rec.calls[-1][1], motion.pack_upsample_conv(conv)[0])
        second = rec.calls[-1]
        conv.bias.add_(1.0)
        motion.upsample_conv(x, conv)
        assert rec.calls[-1][2] is not second[2] and torch.equal(rec.calls[-1][2][:65], conv.bias)
        conv.load_state_dict({k: v.clone() + 1 for k, v in conv.state_dict().items()})
        motion.upsample_conv(x, conv)
        assert torch.equal(rec.calls[-1][1], motion.pack_upsample_conv(conv)[0])
        # the compute dtype is part of the key, and the result has it
        out = motion.upsample_conv(x, conv, conv_dtype=torch.float16)
        assert out.dtype == torch.float16 and rec.calls[-1][1].dtype == torch.float16
        # slices of n and c are handed over as they are; channels-last and a transposed plane are copied to NCHW
        big = torch.zeros(4, 40, 3, 4)
        v = big[1:3, 2:35]
        motion.upsample_conv(v, conv)
        assert rec.calls[-1][0] is v
        cl = x.contiguous(memory_format=torch.channels_last)
        motion.upsample_conv(cl, conv)
        assert rec.calls[-1][0] is not cl and rec.calls[-1][0].is_contiguous() and torch.equal(rec.calls[-1][0], x)
        t = x.transpose(2, 3).contiguous().transpose(2, 3)
        motion.upsample_conv(t, conv)
        assert rec.calls[-1][0].is_contiguous()
        # an explicit pack is used as given; one of the other dtype is refused
        mine = motion.pack_upsample_conv(conv)
        motion.upsample_conv(x, conv, packed=mine)
        assert rec.calls[-1][1] is mine[0]
        with pytest.raises(ValueError, match="packed holds"):
            motion.upsample_conv(x, conv, packed=mine, conv_dtype=torch.float16)
        # UPCONV_NATIVE False sends the default dtype to the eager lines
        n = len(rec.calls)
        monkeypatch.setitem(motion.UPCONV_NATIVE, torch.float32, False)
        assert torch.equal(motion.upsample_conv(x, conv), _eager(x, conv)) and len(rec.calls) == n
