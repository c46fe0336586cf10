"""IGS.condition3D's native parts without a GPU: the float64 restatements and their derived bounds (tests/condition3d_restatement.py)
against the outputs of the reference's own ray_to_plucker, rsh_cart_3, ModLN and condition3D (tests/golden/ref_condition3d.npz, made by
tests/golden/make_condition3d_golden.py), the non-vacuity of every bound, and the argument refusals of the C ABI, the compiled module
and the Python layer (igs_amd/csrc/cond.hip, igs_amd/motion.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import condition3d_restatement as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_ray_condition_fwd", "igs_modln_fwd", "igs_modln_bwd", "igs_modln_bwd_scratch_bytes")
EPS = 1e-6


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_condition3d.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


# ---------------------------------------------------------------- the restatements against the reference's outputs
def test_fixture_is_the_stated_case(fx):
    assert fx["x"].shape == (4, 8, 6, 10) and fx["rays"].shape == (2, 2, 6, 10, 6) and fx["depth"].shape == (2, 2, 15, 23)
    assert fx["cond"].shape == (4, 6, 10, 33) and fx["mod"].shape == (4, 6, 10, 16) and fx["out"].shape == (4, 8, 6, 10)
    assert fx["out_strides"].tolist() == [480, 1, 80, 8]                   # the reference returned a channels-last-strided view
    n = fx["rays"][..., 3:].norm(dim=-1)
    assert (n - 1).abs().min() > 1e-3                                      # no direction is a unit vector
    assert (fx["norm_weight"] - 1).abs().min() > 1e-3 and fx["norm_bias"].abs().min() > 1e-3
    assert fx["x"].mean(1).abs().min() > 1.0                               # a non-zero pixel mean


def test_ray_condition_restatement_matches_the_reference(fx):
    rays, depth = fx["rays"], fx["depth"]
    ref = fx["cond"].double()
    got = CR.ray_condition_restate(rays.double(), depth.double())
    bound = CR.ray_condition_bound(rays, depth)
    err = (got - ref).abs()
    print("cond: max |restatement - reference| %.3e, max err / bound %.3f, max |ref| %.3f" % (err.max().item(), (err / bound).max().item(), ref.abs().max().item()))
    assert (err <= bound).all()
    # the bound rejects each wrong variant
    for kw in (dict(align_corners=True), dict(normalise=False), dict(swap_cross=True)):
        wrong = CR.ray_condition_restate(rays.double(), depth.double(), **kw)
        assert not ((wrong - ref).abs() <= bound).all(), kw
    # the second statement of the resize: F.interpolate in float64
    d64 = depth.double().reshape(4, 1, 15, 23)
    assert ((F.interpolate(d64, size=(6, 10), mode="bilinear", align_corners=False)[:, 0] - got[..., 32]).abs() <= 1e-13 * 6).all()


def test_modln_restatement_matches_the_reference_forward(fx):
    x, mod, w, b = fx["x"], fx["mod"], fx["norm_weight"], fx["norm_bias"]
    ref = fx["out"].double()
    got = CR.modln_restate(x.double(), mod.double(), w.double(), b.double(), EPS)
    bound = CR.modln_forward_bound(x, mod, w, b, EPS)
    err = (got - ref).abs()
    print("out: max |restatement - reference| %.3e, max err / bound %.3f, max |ref| %.3f" % (err.max().item(), (err / bound).max().item(), ref.abs().max().item()))
    assert (err <= bound).all()
    for kw in (dict(swap_halves=True), dict(unbiased=True)):
        wrong = CR.modln_restate(x.double(), mod.double(), w.double(), b.double(), EPS, **kw)
        assert not ((wrong - ref).abs() <= bound).all(), kw
    # reference_composition (what the benchmark times) is the same function: in float64 it agrees with the restatements composed
    module = CR.AdaLNModule.from_arrays(fx).double()
    with torch.no_grad():
        comp = CR.reference_composition(x.double(), fx["rays"].double(), fx["depth"].double(), module)
        cond64 = CR.ray_condition_restate(fx["rays"].double(), fx["depth"].double())
        two = CR.modln_restate(x.double(), module.mlp(cond64), w.double(), b.double(), EPS)
    assert comp.stride() == tuple(fx["out_strides"].tolist()) and comp.shape == ref.shape
    assert ((comp - two).abs() <= 1e-11 * (1 + two.abs())).all()
    assert ((comp - ref).abs() <= 1e-3 * (1 + ref.abs())).all()           # (and it is the fixture's module: a gross check only)


def test_modln_restatement_backward_matches_the_reference_autograd(fx):
    x, mod, w, b, g = fx["x"], fx["mod"], fx["norm_weight"], fx["norm_bias"], fx["gout"]
    want = CR.modln_backward_restate(x.double(), mod.double(), w.double(), b.double(), EPS, g.double())
    bounds = CR.modln_backward_bounds(x, mod, w, b, EPS, g)
    for name, wv in zip(("dx", "dmod", "dweight", "dbias"), want):
        err = (wv - fx[name].double()).abs()
        print("%s: max |restatement - reference| %.3e, max err / bound %.3f" % (name, err.max().item(), (err / bounds[name]).max().item()))
        assert err.shape == bounds[name].shape and (err <= bounds[name]).all(), name
        assert (fx[name] != 0).any()
    assert torch.equal(fx["dmod"][..., :8], g.permute(0, 2, 3, 1))       # d shift is the upstream gradient itself
    # the backward bounds reject the gradients of the wrong variants
    for kw in (dict(swap_halves=True), dict(unbiased=True)):
        xs, ms, ws, bs = (t.double().clone().requires_grad_(True) for t in (x, mod, w, b))
        CR.modln_restate(xs, ms, ws, bs, EPS, **kw).backward(g.double())
        assert not ((xs.grad - fx["dx"].double()).abs() <= bounds["dx"]).all(), kw
        assert not ((ms.grad - fx["dmod"].double()).abs() <= bounds["dmod"]).all(), kw


@pytest.mark.parametrize("C", [8, 128, 1024])
def test_forward_bound_holds_torch_float32_and_rejects_wrong_variances(C):
    """PyTorch's own float32 layer_norm + modulation stays inside the bound on four kinds of input; at C = 8 and 128 the bound rejects a
    float32 E[x^2] - mu^2 variance on the offset input and the unbiased variance on the ordinary input.  (At C = 1024 the worst-case
    bound, which grows with C, is too loose to reject them: stated, not hidden.)"""
    g = torch.Generator().manual_seed(C)
    P = 4096 if C < 1024 else 512
    w, b = 1.0 + 0.5 * torch.randn(C, generator=g), 0.4 * torch.randn(C, generator=g)
    mod = 0.7 * torch.randn(1, 64, P // 64, 2 * C, generator=g)

    def f32(x, var_fn=None):
        xp = x.permute(0, 2, 3, 1)
        if var_fn is None:
            y = F.layer_norm(xp, (C,), w, b, EPS)
        else:
            mu = xp.mean(-1, keepdim=True)
            y = (xp - mu) * torch.rsqrt(var_fn(xp, mu) + EPS) * w + b
        return (y * (1 + mod[..., C:]) + mod[..., :C]).permute(0, 3, 1, 2)

    inputs = dict(ordinary=3 + 0.5 * torch.randn(1, C, 64, P // 64, generator=g), offset=4096 + 2 * torch.randn(1, C, 64, P // 64, generator=g),
                  constant=torch.full((1, C, 64, P // 64), 2.5), tiny=1e-4 * torch.randn(1, C, 64, P // 64, generator=g))
    for name, x in inputs.items():
        ref = CR.modln_restate(x.double(), mod.double(), w.double(), b.double(), EPS)
        bound = CR.modln_forward_bound(x, mod, w, b, EPS)
        ratio = ((f32(x).double() - ref).abs() / bound).max().item()
        print("C = %d, %s: torch float32 at %.3f of the bound" % (C, name, ratio))
        assert ratio <= 1.0, name
        if C <= 128 and name == "offset":
            naive = f32(x, lambda xp, mu: ((xp * xp).mean(-1, keepdim=True) - mu * mu).clamp_min(0))
            frac = ((naive.double() - ref).abs() > bound).double().mean().item()
            print("   E[x^2] - mu^2 violates the bound on %.0f %% of the elements" % (100 * frac))
            assert frac > 0.5
        if C <= 128 and name == "ordinary":
            unb = f32(x, lambda xp, mu: ((xp - mu) ** 2).sum(-1, keepdim=True) / (C - 1))
            frac = ((unb.double() - ref).abs() > bound).double().mean().item()
            print("   the unbiased variance violates the bound on %.0f %% of the elements" % (100 * frac))
            assert frac > 0.9


def test_restatements_by_hand():
    """Axis-aligned rays give known constants; a depth map resized to its own size is returned bit for bit; a pixel whose channels are
    all equal gives out = bias (1 + scale) + shift."""
    v = torch.tensor([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    s = CR.sh3(v)
    K0, K1, K2, K20, K30 = CR.K0, CR.K1, CR.K2, CR.K20, CR.K30
    assert s[0].tolist() == [K0, 0, K1, 0, 0, 0, 2 * K20, 0, 0, 0, 0, 0, 2 * K30, 0, 0, 0]
    assert s[1].tolist() == [K0, 0, 0, K1, 0, 0, -K20, 0, 0.5 * K2, 0, 0, 0, 0, -CR.K3C, 0, CR.K3A]
    assert s[2].tolist() == [K0, 0, 0, 0, 0, 0, -K20, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    rays = torch.zeros(1, 1, 1, 2, 6, dtype=torch.float64)
    rays[..., 0, 1], rays[..., 0, 3] = 1.0, -3.0                           # origin (0, 1, 0), direction -3 x: d = -x, m = +z
    rays[..., 1, 0] = 5.0                                                  # a zero direction stays zero (the 1e-12 floor), m = 0
    d, m = CR.plucker(rays)
    assert d[0, 0, 0].tolist() == [[-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]] and m[0, 0, 0].tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]
    depth = torch.rand(3, 5, 7, dtype=torch.float64)
    assert torch.equal(CR.resize_bilinear(depth, 5, 7), depth)
    assert torch.equal(CR.resize_bilinear(depth.float(), 5, 7), depth.float())
    two = torch.tensor([[[1.0, 3.0]]], dtype=torch.float64)                # 1 x 2 -> 1 x 4: 1, 1.5, 2.5, 3
    assert CR.resize_bilinear(two, 1, 4)[0, 0].tolist() == [1.0, 1.5, 2.5, 3.0]
    x = torch.full((1, 4, 1, 2), 7.0, dtype=torch.float64)
    mod = torch.arange(16, dtype=torch.float64).reshape(1, 1, 2, 8) / 8
    w, b = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), torch.tensor([0.5, -0.5, 0.25, 1.0], dtype=torch.float64)
    out = CR.modln_restate(x, mod, w, b, EPS)
    assert torch.equal(out, b.view(1, 4, 1, 1) * (1 + mod[..., 4:].permute(0, 3, 1, 2)) + mod[..., :4].permute(0, 3, 1, 2))


# ---------------------------------------------------------------- the C ABI
def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1) with a message, never IGS_RAST_E_HIP (-2): without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    for name in NAMES:
        assert name in _cabi.EXPORTS and hasattr(L, name)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = _cabi.last_error

    def ray(N=4, H=6, W=10, Hd=15, Wd=23, ptrs=None):
        ptrs = ptrs or [p] * 3
        return L.igs_ray_condition_fwd(None, N, H, W, Hd, Wd, *ptrs)

    for kw, what in ((dict(N=-1), "N out of range"), (dict(H=0), "H out of range"), (dict(H=8193), "H out of range"), (dict(W=0), "W out of range"),
                     (dict(W=8193), "W out of range"), (dict(Hd=0), "Hd out of range"), (dict(Hd=8193), "Hd out of range"),
                     (dict(Wd=0), "Wd out of range"), (dict(Wd=8193), "Wd out of range"), (dict(N=5, H=2048, W=2048), "N * H * W out of range")):
        assert ray(**kw) == -1 and what in err(), (kw, err())
    for i in range(3):
        ptrs = [p] * 3
        ptrs[i] = None
        assert ray(ptrs=ptrs) == -1 and "NULL" in err(), i
    assert ray(N=0, ptrs=[None] * 3) == 0

    def fwd(N=4, Cc=8, H=6, W=10, xdt=0, mdt=0, xs=None, eps=1e-6, ptrs=None):
        xs = xs or (Cc * H * W, H * W, W, 1)
        ptrs = ptrs or [p] * 7                                           # x, mod, weight, bias, out, mean, rstd
        return L.igs_modln_fwd(None, N, Cc, H, W, xdt, ptrs[0], *xs, mdt, ptrs[1], ptrs[2], ptrs[3], eps, ptrs[4], ptrs[5], ptrs[6])

    def bwd(N=4, Cc=8, H=6, W=10, xdt=0, mdt=0, xs=None, ptrs=None):
        xs = xs or (Cc * H * W, H * W, W, 1)
        ptrs = ptrs or [p] * 12                      # x, mod, weight, bias, mean, rstd, gout, dx, dmod, dweight, dbias, scratch
        return L.igs_modln_bwd(None, N, Cc, H, W, xdt, ptrs[0], *xs, mdt, *ptrs[1:])

    bad = ((dict(N=-1), "N out of range"), (dict(Cc=0), "C out of range"), (dict(Cc=1025), "C out of range"), (dict(H=0), "H out of range"),
           (dict(H=8193), "H out of range"), (dict(W=0), "W out of range"), (dict(W=8193), "W out of range"),
           (dict(N=5, H=2048, W=2048), "N * H * W out of range"), (dict(xdt=2), "dtype"), (dict(mdt=-1), "dtype"))
    for kw, what in bad:
        assert fwd(**kw) == -1 and what in err(), (kw, err())
        assert bwd(**kw) == -1 and what in err(), (kw, err())
        if "dt" not in "".join(kw):
            k = dict(N=4, Cc=8, H=6, W=10)
            k.update(kw)
            assert L.igs_modln_bwd_scratch_bytes(k["N"], k["Cc"], k["H"], k["W"]) == 0
    assert fwd(xs=(480, 1, 80, 8)) == -1 and "channels-last" in err()
    assert bwd(xs=(480, 1, 80, 8)) == -1 and "channels-last" in err()
    assert fwd(xs=(480, 60, 11, 1)) == -1 and "plane must be contiguous" in err()
    assert fwd(xs=(-1, 60, 10, 1)) == -1 and "negative" in err()
    assert fwd(eps=-1.0) == -1 and "eps" in err()
    assert fwd(ptrs=[p] * 5 + [p, None]) == -1 and "both or neither" in err()
    for i in range(5):
        ptrs = [p] * 7
        ptrs[i] = None
        assert fwd(ptrs=ptrs) == -1 and "NULL" in err(), i
    for i in list(range(7)) + [11]:
        ptrs = [p] * 12
        ptrs[i] = None
        assert bwd(ptrs=ptrs) == -1 and "NULL" in err(), i
    # nothing to do: 0 without a launch
    assert fwd(N=0, ptrs=[None] * 7) == 0 and bwd(N=0, ptrs=[None] * 12) == 0
    assert bwd(ptrs=[p] * 7 + [None] * 5) == 0                           # no gradient wanted
    # the limits themselves are accepted; the scratch is one row of 2 C floats per workgroup (32 pixels each at C = 128) and 64 rows
    # for the first round of the reduction
    assert L.igs_modln_bwd_scratch_bytes(1, 1024, 8192, 2048) > 0 and L.igs_modln_bwd_scratch_bytes(1 << 24, 1, 1, 1) > 0
    tiles = 20 * 128 * 128 // 32
    s = L.igs_modln_bwd_scratch_bytes(20, 128, 128, 128)
    assert (tiles + 64) * 2 * 128 * 4 <= s <= (tiles + 64) * 2 * 128 * 4 + 4096


def test_header_states_the_limits_and_version_is_unchanged():
    h = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    for s in ("#define IGS_COND_MAX_PIXELS (1 << 24)", "#define IGS_COND_MAX_HW 8192", "#define IGS_MODLN_MAX_C 1024"):
        assert s in h
    for name in NAMES:
        assert name + "(" in h
    from igs_amd import _cabi
    assert _cabi.lib().igs_rast_version() == 4
    assert "cond.hip" in open(os.path.join(ROOT, "igs_amd", "build.py")).read()


# ---------------------------------------------------------------- the compiled module and the Python layer
def test_compiled_module_refusals():
    from igs_amd import _cabi
    E = _cabi.ext()
    x, mod, w, b = torch.zeros(4, 8, 6, 10), torch.zeros(4, 6, 10, 16), torch.ones(8), torch.zeros(8)
    rays, depth = torch.zeros(4, 6, 10, 6), torch.zeros(4, 15, 23)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.cond_ray_fwd(rays, depth)
    with pytest.raises(NotImplementedError, match="rays must be"):
        E.cond_ray_fwd(rays.double(), depth)
    with pytest.raises(RuntimeError, match="shape"):
        E.cond_ray_fwd(rays[..., :5], depth)
    with pytest.raises(RuntimeError, match="shape"):
        E.cond_ray_fwd(rays, depth[:3])
    with pytest.raises(RuntimeError, match="out of range"):
        E.cond_ray_fwd(torch.zeros(1, 1, 8193, 6), depth[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.modln_fwd(x, mod, w, b, 1e-6, False)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.modln_fwd(x.double(), mod, w, b, 1e-6, False)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.modln_fwd(x, mod.bfloat16(), w, b, 1e-6, False)
    with pytest.raises(NotImplementedError, match="weight must be"):
        E.modln_fwd(x, mod, w.double(), b, 1e-6, False)
    with pytest.raises(RuntimeError, match="shape"):
        E.modln_fwd(x[0], mod, w, b, 1e-6, False)
    with pytest.raises(RuntimeError, match="shape"):
        E.modln_fwd(x, mod[..., :8], w, b, 1e-6, False)
    with pytest.raises(RuntimeError, match="shape"):
        E.modln_fwd(x, mod, w[:7], b, 1e-6, False)
    with pytest.raises(RuntimeError, match="out of range"):
        E.modln_fwd(torch.zeros(1, 1025, 1, 1), torch.zeros(1, 1, 1, 2050), torch.ones(1025), torch.ones(1025), 1e-6, False)
    st, g = torch.zeros(4, 6, 10), torch.zeros(4, 8, 6, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.modln_bwd(x, mod, w, b, st, st, g)
    with pytest.raises(RuntimeError, match="shape"):
        E.modln_bwd(x, mod, w, b, st[:3], st, g)
    with pytest.raises(RuntimeError, match="shape"):
        E.modln_bwd(x, mod, w, b, st, st, g[:, :7])


def test_python_layer_refusals():
    from igs_amd import motion
    x, mod, w, b = torch.zeros(4, 8, 6, 10), torch.zeros(4, 6, 10, 16), torch.ones(8), torch.zeros(8)
    rays, depth = torch.zeros(2, 2, 6, 10, 6), torch.zeros(2, 2, 15, 23)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.ray_condition(rays, depth, (6, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.modln(x, mod, w, b)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        motion.modln(x.bfloat16(), mod, w, b)
    with pytest.raises(NotImplementedError, match="weight and bias must be float32"):
        motion.modln(x, mod, w.half(), b)
    with pytest.raises(NotImplementedError, match="rays and depth must be float32"):
        motion.ray_condition(rays.half(), depth, (6, 10))
    with pytest.raises(NotImplementedError, match="gradients to rays and depth"):
        motion.ray_condition(rays, depth.clone().requires_grad_(True), (6, 10))
    with pytest.raises(ValueError, match="rays must be"):
        motion.ray_condition(rays[0], depth, (6, 10))
    with pytest.raises(ValueError, match="depth must be"):
        motion.ray_condition(rays, depth[:1], (6, 10))
    with pytest.raises(ValueError, match="feature resolution"):
        motion.ray_condition(rays, depth, (10, 6))
    with pytest.raises(ValueError, match="x must be"):
        motion.modln(x[0], mod, w, b)
    with pytest.raises(ValueError, match="mod must be"):
        motion.modln(x, mod[:, :5], w, b)
    with pytest.raises(ValueError, match="weight and bias must be"):
        motion.modln(x, mod, w[:7], b)
    module = CR.AdaLNModule(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.condition3d(x, rays, depth, module)
    with pytest.raises(ValueError, match="normalises"):
        motion.condition3d(x[:, :4], rays, depth, module)
    with pytest.raises(ValueError, match="do not match"):
        motion.condition3d(x[:3], rays, depth, module)
    with pytest.raises(ValueError, match="motion_feature must be"):
        motion.condition3d(x[0], rays, depth, module)
    module.norm = torch.nn.LayerNorm(8, elementwise_affine=False)
    with pytest.raises(NotImplementedError, match="without affine"):
        motion.condition3d(x, rays, depth, module)
