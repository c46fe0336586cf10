"""The encoder's fused instance norms and position add (igs_amd/csrc/inorm.hip, igs_amd/backbone.py) without a GPU: the float64
restatement against the reference-produced golden file, exports and argument counts, the refusals of the C ABI before any HIP call and of
the Python layer, the resident limit, the registers and scratch of the built gfx950 kernels, the derived allowance on a float32 emulation
of the kernel's arithmetic and on three wrong variants, and the two binding calls on a stand-in encoder."""
import os
import re
import shutil
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import encoder_norms_restatement as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_instance_norm_fwd", "igs_instance_norm_resident_max", "igs_position_add")
INVALID = -1
F32, F16 = 0, 1
POSITION_CASES = ((16, 6, 10, 2), (16, 6, 9, 3), (8, 5, 7, 1))


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_encoder.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_restated_modes_equal_the_reference_blocks(golden):
    g = golden
    assert g["ident_x"].dtype == torch.float64 and g["ident_x"].shape == (2, 6, 10, 14) and g["down_n3_in"].shape == (2, 10, 5, 7)
    for tag in ("ident_", "down_"):
        assert (ER.restate(g[tag + "n1_in"], None, ER.RELU) - g[tag + "n1_out"]).abs().max() <= 1e-12, tag
    assert (ER.restate(g["ident_n2_in"], g["ident_x"], ER.RELU_ADD_RELU) - g["ident_out"]).abs().max() <= 1e-12
    assert (ER.restate(g["down_n2_in"], g["down_n3_in"], ER.RELU_ADDNORM_RELU) - g["down_out"]).abs().max() <= 1e-12
    assert (ER.restate(g["stem_n1_in"], None, ER.RELU) - g["stem_out"]).abs().max() <= 1e-12
    # the modes are different functions on this data, and PLAIN is PyTorch's own instance norm
    assert (ER.restate(g["down_n2_in"], g["down_n3_in"], ER.RELU_ADD_RELU) - g["down_out"]).abs().max() > 1e-2
    assert (ER.restate(g["stem_n1_in"], None, ER.PLAIN) - F.instance_norm(g["stem_n1_in"], eps=1e-5)).abs().max() <= 1e-12


@pytest.mark.parametrize("case", POSITION_CASES)
def test_position_closed_form_equals_the_reference(golden, case):
    """The reference builds its embedding in float32 whatever the features' dtype (position.py:30-39), so its float64 outputs carry a
    float32 embedding: the closed form in float64 is compared within the position allowance, which is derived for exactly that float32
    arithmetic.  (The largest difference measured when the file was made: 7e-7.)"""
    C, h, w, K = case
    tag = "pos_%d_%d_%d_%d_" % case
    f0, f1 = golden[tag + "f0"], golden[tag + "f1"]
    assert f0.shape == (2, C, h, w)
    o0, o1 = ER.restate_position(f0, f1, K)
    for o, name in ((o0, "o0"), (o1, "o1")):
        err = (o - golden[tag + name]).abs()
        print(case, name, "max |closed form - reference| %.2e" % err.max().item())
        assert (err <= 2e-6).all(), (case, name, err.max().item())
    assert (o0 - f0 - (o1 - f1)).abs().max() <= 1e-15                                      # one embedding for both features
    if K > 1:                                                                              # ... periodic in the window
        pos = o0 - f0
        assert (pos[:, :, : h // K, : w // K] - pos[:, :, h // K: 2 * (h // K), w // K: 2 * (w // K)]).abs().max() <= 1e-15


# ---------------------------------------------------------------- exports and ABI
def test_exports_and_argument_counts():
    from igs_amd import _cabi, build
    L = _cabi.lib()
    hdr = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m, n
        assert len(_cabi.SIGNATURES[n][1]) == len(m.group(1).split(",")), n
    assert "inorm.hip" in build.SOURCES
    m = _cabi.ext()
    assert hasattr(m._encoder, "instance_norm_fwd") and hasattr(m._encoder, "position_add")    # (a private submodule of _C)
    from igs_amd import backbone as BB
    assert (BB.PLAIN, BB.RELU, BB.RELU_ADD_RELU, BB.RELU_ADDNORM_RELU) == ER.MODES
    for name, code in (("PLAIN", 0), ("RELU", 1), ("RELU_ADD_RELU", 2), ("RELU_ADDNORM_RELU", 3)):
        assert re.search(r"#define IGS_INORM_%s %d\b" % (name, code), hdr), name


def _norm(L, x=0x1000, skip=None, out=0x2000000, planes=3, hw=64, dt=F32, mode=0, eps=1e-5):
    return L.igs_instance_norm_fwd(None, x, skip, out, planes, hw, dt, mode, eps)


def _pos(L, f0=0x1000, f1=0x2000000, o0=0x4000000, o1=0x6000000, B=1, C=16, H=6, W=10, K=2, dt=F32):
    return L.igs_position_add(None, f0, f1, o0, o1, B, C, H, W, K, dt)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    L = _cabi.lib()
    for kw, word in ((dict(hw=1), "more than 1 spatial element"), (dict(hw=0), "more than 1 spatial element"), (dict(hw=-5), "more than 1"),
                     (dict(hw=(1 << 30) + 1), "hw out of range"), (dict(planes=-1), "planes out of range"), (dict(planes=1 << 31), "planes out of range"),
                     (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(mode=2), "needs skip"), (dict(mode=3), "needs skip"),
                     (dict(mode=4), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(dt=2), "dtype"), (dict(dt=-1), "dtype"),
                     (dict(eps=-1e-5), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"),
                     (dict(x=0x1002), "aligned to its element size"), (dict(dt=F16, out=0x2000001), "aligned to its element size"),
                     (dict(out=0x1010), "only out == x may alias"), (dict(mode=2, skip=0x2000000), "overlaps skip"),
                     (dict(mode=3, skip=0x2000100), "overlaps skip"), (dict(mode=2, skip=0x1000, out=0x1000), "overlaps skip")):
        assert _norm(L, **kw) == INVALID, kw
        assert word in _cabi.last_error() and "igs_instance_norm_fwd" in _cabi.last_error(), (kw, _cabi.last_error())
    assert _norm(L, planes=0) == 0 and _norm(L, planes=0, x=None, out=None) == 0            # nothing to do
    assert _norm(L, planes=0, hw=1) == INVALID                                              # ... but the sizes are still checked
    for kw, word in ((dict(C=6), "multiple of 4"), (dict(C=0), "out of range"), (dict(K=0), "splits"), (dict(K=-2), "splits"), (dict(K=4), "multiples of splits"),
                     (dict(H=6, W=9, K=2), "multiples of splits"), (dict(B=-1), "out of range"), (dict(H=0), "out of range"), (dict(dt=5), "dtype"),
                     (dict(f0=None), "NULL"), (dict(f1=None), "NULL"), (dict(o0=None), "NULL"), (dict(o1=None), "NULL"),
                     (dict(o0=0x1010), "overlap"), (dict(o1=0x4000000), "overlap"), (dict(o0=0x2000000), "overlap"),
                     (dict(f0=0x1001), "aligned to its element size"), (dict(H=1 << 16, W=1 << 16, K=1), "H * W out of range"),
                     (dict(B=1 << 20, C=1 << 12, H=64, W=64), "B * C * H * W out of range")):
        assert _pos(L, **kw) == INVALID, kw
        assert word in _cabi.last_error() and "igs_position_add" in _cabi.last_error(), (kw, _cabi.last_error())
    assert _pos(L, B=0) == 0


def test_resident_limit_covers_the_shipped_planes():
    from igs_amd import _cabi
    L = _cabi.lib()
    for dt in (F32, F16):
        for mode in (ER.PLAIN, ER.RELU, ER.RELU_ADD_RELU):
            assert L.igs_instance_norm_resident_max(dt, mode) >= 65536, (dt, mode)          # 256 x 256: read once
        two = L.igs_instance_norm_resident_max(dt, ER.RELU_ADDNORM_RELU)
        assert 16384 <= two <= L.igs_instance_norm_resident_max(dt, ER.RELU)                # the shipped downsample blocks: 128 x 128, 64 x 64
    assert L.igs_instance_norm_resident_max(7, 0) == 0 and L.igs_instance_norm_resident_max(F32, 9) == 0


# ---------------------------------------------------------------- the built code objects
@pytest.fixture(scope="module")
def inorm_kernels():
    """{symbol: metadata} of every kernel of inorm.hip in libigs_rast.so."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = A.code_objects(build.LIB)
    try:
        found = {}
        for co in cos:
            for name, md in kernel_metadata(co).items():
                if re.match(r"^_Z\d+(inorm_\w+_kernel|position_add_kernel)", name):
                    found[name] = md
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_resident_kernels_have_no_scratch_and_the_budgeted_waves(inorm_kernels):
    """the 1024-thread shapes need 4 waves per SIMD to be launchable at all (<= 128 registers); the 256-thread
    64-values-per-thread shape is budgeted at 4 workgroups per CU (4 waves per SIMD, <= 128), the small shapes at 8 waves per SIMD (<= 64)."""
    res = {n: md for n, md in inorm_kernels.items() if "inorm_resident_kernel" in n}
    assert len(res) == 16, sorted(res)                                                       # 2 dtypes x (4 one-plane + 4 two-plane shapes)
    assert len([n for n in inorm_kernels if "inorm_streamed_kernel" in n]) == 4 and len([n for n in inorm_kernels if "position_add" in n]) == 4
    for name, md in inorm_kernels.items():
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0 and int(md.get(".sgpr_spill_count", 0)) == 0, (name, "spills")
    for name, md in res.items():
        threads, nv, two = re.search(r"Li(\d+)ELi(\d+)ELb([01])E", name).groups()
        regs = (int(md[".vgpr_count"]) + int(md.get(".agpr_count", 0)) + 7) // 8 * 8
        values = 4 * int(nv) * (2 if two == "1" else 1)
        print(name, "threads", threads, "values per thread", values, "vgpr", md[".vgpr_count"], "lds", md[".group_segment_fixed_size"])
        assert regs <= (128 if values >= 64 else 64), (name, regs)                        # 4 waves per SIMD; 8 below 64 values
        assert int(md[".max_flat_workgroup_size"]) == int(threads), name


# ---------------------------------------------------------------- the allowance
def _ratio(y, x64, eps=1e-5):
    ref = ER.restate(x64, None, ER.PLAIN, eps)
    return ((y.double() - ref).abs() / ER.allowance(x64, None, ER.PLAIN, eps, torch.float32, ref)).max().item()


@pytest.mark.parametrize("hw", [(7, 9), (64, 64), (256, 256)])
def test_allowance_accepts_the_kernel_arithmetic_and_pytorch_float32(hw):
    """On the GPU test's inputs (every pair of mean and std): the float32 emulation of the kernel's arithmetic and PyTorch's own float32
    instance norm on the CPU stay inside the allowance."""
    x = ER.plane_inputs(9, hw[0], hw[1], torch.float32, "cpu", seed=3)
    x64 = x.double()
    r_emul = _ratio(ER.emulate(x[0])[None], x64)
    r_torch = _ratio(F.instance_norm(x, eps=1e-5), x64)
    print(hw, "max |err| / allowance: emulation %.3f, F.instance_norm float32 %.3f" % (r_emul, r_torch))
    assert r_emul <= 1.0 and r_torch <= 1.0, (r_emul, r_torch)
    const = torch.full((1, 1, hw[0], hw[1]), 100.37, dtype=torch.float32)
    assert (ER.emulate(const[0]) == 0).all()                                                # a constant plane: exactly zero


def test_allowance_rejects_three_wrong_variants():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 64, 64, generator=g, dtype=torch.float64) + 1e3).float()            # mean 1e3, std 1: E[x^2] - mean^2 cancels
    r = {"right": _ratio(ER.emulate(x)[None], x.double()[None]), "one_pass": _ratio(ER.emulate(x, variant="one_pass")[None], x.double()[None])}
    y = torch.randn(2, 4, 4, generator=g, dtype=torch.float64).float()                     # 4 x 4: n - 1 instead of n is 3 % of rstd
    r["unbiased"] = _ratio(ER.emulate(y, variant="unbiased")[None], y.double()[None])
    assert _ratio(ER.emulate(y)[None], y.double()[None]) <= 1.0
    z = (torch.randn(2, 16, 16, generator=g, dtype=torch.float64) * 1e-3).float()           # std 1e-3: var = 1e-6 against eps = 1e-5
    r["no_eps"] = _ratio(ER.emulate(z, variant="no_eps")[None], z.double()[None])
    assert _ratio(ER.emulate(z)[None], z.double()[None]) <= 1.0
    print("max |err| / allowance:", r)
    assert r["right"] <= 1.0, r
    assert r["one_pass"] > 1.0 and r["unbiased"] > 1.0 and r["no_eps"] > 1.0, r


@pytest.mark.parametrize("n", [4097, 16384, 65536])
def test_allowance_rejects_the_wrong_variants_at_the_larger_resident_planes(n):
    """The same three variants on planes of the workgroup shapes that the GPU test reaches with 4097 .. 16385 and `max` elements: the
    comparison there is not vacuous either.  "unbiased" changes rstd by the factor sqrt(n / (n - 1)), 1 / (2 n) relative, so an element of
    |x_hat| = h moves by h / (2 n) against an allowance of 4 * 2^-24 * (2 h + 1) on a plane of mean 0: with h about 4 that is some 230 x the
    allowance at 4097, 57 x at 16384 and 14 x at 65536 (printed below), so all three variants stay separable up to the resident limit
    and all three are asserted; the ratio falls below 1 only near n = 10^6, on the streamed path."""
    g = torch.Generator().manual_seed(5 + n)
    x = (torch.randn(2, 1, n, generator=g, dtype=torch.float64) + 1e3).float()              # mean 1e3, std 1
    y = torch.randn(2, 1, n, generator=g, dtype=torch.float64).float()                      # mean 0, std 1
    z = (torch.randn(2, 1, n, generator=g, dtype=torch.float64) * 1e-3).float()             # std 1e-3
    r = {"right": max(_ratio(ER.emulate(t)[None], t.double()[None]) for t in (x, y, z))}
    for t, kind in ((x, "one_pass"), (y, "unbiased"), (z, "no_eps")):
        r[kind] = _ratio(ER.emulate(t, variant=kind)[None], t.double()[None])
    print(n, "max |err| / allowance:", r)
    assert r["right"] <= 1.0, r
    assert r["one_pass"] > 1.0 and r["unbiased"] > 1.0 and r["no_eps"] > 1.0, r


# ---------------------------------------------------------------- the Python layer
def test_python_refusals_on_the_cpu():
    from igs_amd import backbone as BB
    x = torch.randn(2, 4, 6, 8)
    for call in (lambda t: BB.instance_norm(t), lambda t: BB.instance_norm(t, relu=True, inplace=True), lambda t: BB.residual_tail(t, t.clone()),
                 lambda t: BB.residual_tail(t, t.clone(), norm_skip=True), lambda t: BB.feature_add_position(t, t.clone(), 2, 4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x)
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(NotImplementedError):
                call(x.to(dt))
        with pytest.raises(ValueError):
            call(x[0])
        with torch.enable_grad():
            with pytest.raises(NotImplementedError, match="frozen in IGS.*no backward is provided"):
                call(x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                               # ... which under no_grad is only on the wrong device
        with torch.no_grad():
            BB.instance_norm(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        BB.residual_tail(x, x.half())
    with pytest.raises(NotImplementedError):
        BB.feature_add_position(x, x.half(), 2, 4)
    with pytest.raises(ValueError):
        BB.residual_tail(x, x[:, :2])
    with pytest.raises(ValueError):
        BB.feature_add_position(x, x[:, :, :3], 2, 4)
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        BB.instance_norm(x[:, :, :1, :1])
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        BB.residual_tail(x[:, :, :1, :1], x[:, :, :1, :1])
    with pytest.raises(ValueError, match="multiple of 4"):
        BB.feature_add_position(x[:, :2], x[:, :2], 2, 2)
    with pytest.raises(ValueError, match="split"):
        BB.feature_add_position(x, x, 4, 4)
    with pytest.raises(ValueError, match="split"):
        BB.feature_add_position(x, x, 0, 4)
    with pytest.raises(ValueError, match="feature_channels"):
        BB.feature_add_position(x, x, 2, 8)


def test_use_native_encoder_norms_binds_fifteen_norms_and_keeps_the_state_dict():
    from igs_amd import backbone as BB
    enc = ER.make_encoder()
    keys = list(enc.state_dict().keys())
    ref_forward = type(enc).forward
    assert BB.use_native_encoder_norms(enc) == 15
    assert list(enc.state_dict().keys()) == keys
    blocks = [m for m in enc.modules() if isinstance(m, ER.Block)]
    assert len(blocks) == 6 and all("forward" in vars(b) for b in blocks) and "forward" in vars(enc)
    assert type(enc).forward is ref_forward                                                  # (the class is untouched: other instances keep theirs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                               # the bound forward runs the native path: no fallback
        enc(torch.randn(1, 3, 32, 32))


@pytest.mark.parametrize("norm", [nn.BatchNorm2d, lambda c: nn.InstanceNorm2d(c, affine=True), lambda c: nn.InstanceNorm2d(c, track_running_stats=True)])
def test_use_native_encoder_norms_refuses_other_norms_without_touching_them(norm):
    from igs_amd import backbone as BB
    enc = ER.make_encoder(norm=norm)
    with pytest.raises(NotImplementedError, match="InstanceNorm2d"):
        BB.use_native_encoder_norms(enc)
    assert "forward" not in vars(enc) and not any("forward" in vars(m) for m in enc.modules())
    with torch.no_grad():
        assert enc(torch.randn(1, 3, 32, 32))[0].shape == (1, 128, 4, 4)                     # still the PyTorch module it was
    # one wrong norm deep inside is enough, and is found before the first block is bound
    enc = ER.make_encoder()
    enc.layer3[1].norm2 = nn.BatchNorm2d(128)
    with pytest.raises(NotImplementedError):
        BB.use_native_encoder_norms(enc)
    assert not any("forward" in vars(m) for m in enc.modules())
    with pytest.raises(NotImplementedError, match="CNNEncoder attributes"):
        BB.use_native_encoder_norms(nn.Sequential(nn.Conv2d(3, 3, 1)))


def test_use_native_position_sets_exactly_one_name():
    from igs_amd import backbone as BB
    other = object()
    ns = types.SimpleNamespace(feature_add_position=ER.restate_position, split_feature=other, merge_splits=other)
    before = dict(vars(ns))
    assert BB.use_native_position(ns) == 1
    changed = [k for k in vars(ns) if vars(ns)[k] is not before[k]]
    assert changed == ["feature_add_position"] and ns.feature_add_position is BB.feature_add_position and set(vars(ns)) == set(before)
    empty = types.SimpleNamespace()
    assert BB.use_native_position(empty) == 0 and not vars(empty)
    import inspect
    assert list(inspect.signature(BB.feature_add_position).parameters) == ["feature0", "feature1", "attn_splits", "feature_channels"]
