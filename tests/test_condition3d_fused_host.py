"""The fused condition3D forward without a GPU (igs_amd/csrc/cond_fused.hip, igs_amd/motion.py): the float64 restatement and its derived
bound (tests/condition3d_fused_restatement.py) against the reference's stored outputs (tests/golden/ref_condition3d.npz), the exports and
their declared signatures, every refusal of the C ABI before any HIP call, the pack's element counts and layout, the Python layer's
exceptions and the binder's dispatch (with a stand-in for the compiled module)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import condition3d_fused_restatement as FR
import condition3d_restatement as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_condition3d_pack_elems", "igs_condition3d_fwd")


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_condition3d.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


# ---------------------------------------------------------------- the restatement against the reference's outputs
def test_restatement_reproduces_the_reference_fixture(fx):
    """The reference evaluated cond, the MLP and the modulated LayerNorm in float32 with PyTorch's kernels: fma chains of the same lengths
    in some order, so its mod is within the MLP bound E of mod64 and its out within the whole bound of out64."""
    module = CR.AdaLNModule.from_arrays(fx)
    r = FR.restate(fx["x"], fx["rays"], fx["depth"], module)
    assert r["mod64"].shape == fx["mod"].shape and r["out64"].shape == fx["out"].shape
    rm, ro = FR.worst(fx["mod"], r["mod64"], r["E"]), FR.worst(fx["out"], r["out64"], r["bound"])
    print("fixture: max |mod - mod64| / E %.3f, max |out - out64| / bound %.3f" % (rm, ro))
    assert rm <= 1.0 and ro <= 1.0
    # not vacuous: the bound rejects the swapped halves, the unbiased variance and a module without the depth channel's weight
    for kw in (dict(swap_halves=True), dict(unbiased=True)):
        wrong = CR.modln_restate(fx["x"].double(), r["mod64"], fx["norm_weight"].double(), fx["norm_bias"].double(), float(fx["eps"]), **kw)
        assert FR.worst(fx["out"], wrong, r["bound"]) > 1.0, kw
    W1, b1, W2, b2 = FR.module_arrays(module)
    W1z = W1.copy()
    W1z[:, 32] = 0
    modz, _ = FR.mlp_with_bound(r["cond64"].reshape(-1, 33).numpy(), r["bcond"].reshape(-1, 33).numpy(), W1z, b1, W2, b2)
    assert FR.worst(fx["mod"], torch.from_numpy(modz).reshape(fx["mod"].shape), r["E"]) > 1.0
    # the float16 instance's bound is the wider one, and the restatement is the composition of the two existing ones
    rh = FR.restate(fx["x"], fx["rays"], fx["depth"], module, half=True)
    assert (rh["E"] > r["E"]).all()
    with torch.no_grad():
        two = CR.modln_restate(fx["x"].double(), module.double().mlp(r["cond64"]), fx["norm_weight"].double(), fx["norm_bias"].double(), float(fx["eps"]))
    assert ((two - r["out64"]).abs() <= 1e-11 * (1 + two.abs())).all()


# ---------------------------------------------------------------- the C ABI
def _aligned_buffer(nbytes=4096):
    raw = C.create_string_buffer(nbytes + 64)
    return raw, (C.addressof(raw) + 63) & ~63


def test_exports_and_declared_signatures():
    from igs_amd import _cabi
    L = _cabi.lib()
    h = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    for name in NAMES:
        assert name in _cabi.EXPORTS and hasattr(L, name)
        m = re.search(r"\b%s\(([^;]*)\);" % name, h)
        assert m, name
        assert len(m.group(1).split(",")) == len(_cabi.SIGNATURES[name][1]), name
    assert len(_cabi.SIGNATURES["igs_condition3d_fwd"][1]) == 23 and len(_cabi.SIGNATURES["igs_condition3d_pack_elems"][1]) == 3
    assert "#define IGS_COND_MLP_MAX_WIDTH 128" in h and "#define IGS_COND_FUSED_MAX_STRIDE (1LL << 27)" in h
    assert "cond_fused.hip" in open(os.path.join(ROOT, "igs_amd", "build.py")).read()
    assert L.igs_rast_version() == 4


def test_pack_elems():
    from igs_amd import _cabi
    L = _cabi.lib()
    for Cc, hid in ((128, 128), (8, 128), (7, 5), (33, 65), (96, 32), (128, 1), (1, 1), (32, 33)):
        ct, ht = -(-Cc // 32), -(-hid // 32)
        for dt in (0, 1):
            assert L.igs_condition3d_pack_elems(Cc, hid, dt) == (2 * ht + 2 * ct * ht) * 1024, (Cc, hid, dt)
    assert L.igs_condition3d_pack_elems(128, 128, 0) == 40 * 1024
    for Cc, hid, dt in ((129, 128, 0), (0, 128, 0), (128, 0, 0), (128, 129, 1), (128, 128, 2), (128, 128, -1)):
        assert L.igs_condition3d_pack_elems(Cc, hid, dt) == -1, (Cc, hid, dt)


def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1) with a message, never IGS_RAST_E_HIP (-2): without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    raw, p = _aligned_buffer()
    err = _cabi.last_error
    PTRS = ("x", "rays", "depth", "wpack", "bpack", "weight", "bias", "out")

    def fwd(N=4, Cc=8, hid=128, H=6, W=10, Hd=15, Wd=23, xdt=0, mdt=0, xs=None, eps=1e-6, **ptrs):
        xs = xs or (Cc * H * W, H * W, W, 1)
        q = {k: p for k in PTRS}
        q.update(ptrs)
        return L.igs_condition3d_fwd(None, N, Cc, hid, H, W, Hd, Wd, xdt, q["x"], *xs, q["rays"], q["depth"], mdt, q["wpack"], q["bpack"],
                                     q["weight"], q["bias"], eps, q["out"])

    bad = ((dict(N=-1), "N out of range"), (dict(Cc=0), "C out of range"), (dict(Cc=129), "C out of range"), (dict(hid=0), "hidden out of range"),
           (dict(hid=129), "hidden out of range"), (dict(H=0), "H out of range"), (dict(H=8193), "H out of range"), (dict(W=0), "W out of range"),
           (dict(W=8193), "W out of range"), (dict(Hd=0), "Hd out of range"), (dict(Hd=8193), "Hd out of range"), (dict(Wd=0), "Wd out of range"),
           (dict(Wd=8193), "Wd out of range"), (dict(N=5, H=2048, W=2048), "N * H * W out of range"), (dict(xdt=2), "dtype"), (dict(xdt=-1), "dtype"),
           (dict(mdt=2), "dtype"), (dict(mdt=-1), "dtype"), (dict(xs=(480, 1, 80, 8)), "channels-last"),
           (dict(xs=(480, 60, 11, 1)), "plane must be contiguous"), (dict(xs=(-1, 60, 10, 1)), "negative"), (dict(xs=(480, -60, 10, 1)), "negative"),
           (dict(xs=(480, (1 << 27) + 1, 10, 1)), "IGS_COND_FUSED_MAX_STRIDE"), (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"))
    for kw, what in bad:
        assert fwd(**kw) == -1 and what in err() and "igs_condition3d_fwd" in err(), (kw, err())
    for name in PTRS:
        assert fwd(**{name: None}) == -1 and "NULL" in err(), name
        if name != "x":
            assert fwd(**{name: p + (4 if name == "wpack" else 2)}) == -1 and "aligned" in err(), (name, err())
    assert fwd(x=p + 2) == -1 and "aligned" in err()                     # a float32 x on a 2-byte boundary
    assert fwd(x=p + 1, xdt=1) == -1 and "aligned" in err()              # a float16 x on an odd address
    assert fwd(wpack=p + 8, mdt=1) == -1 and "16 bytes" in err()
    # N == 0: nothing to do, 0 without a launch, whatever the pointers
    assert fwd(N=0, **{k: None for k in PTRS}) == 0
    del raw


# ---------------------------------------------------------------- the pack
@pytest.mark.parametrize("Cc,hid", [(8, 128), (7, 5), (33, 65), (128, 1), (96, 32)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_pack_puts_every_weight_where_the_header_says(Cc, hid, dtype):
    from igs_amd import _cabi, motion
    torch.manual_seed(Cc + hid)
    m = CR.AdaLNModule(Cc, hidden=hid)
    wpack, bpack = motion.pack_condition_mlp(m.mlp, dtype)
    half = dtype == torch.float16
    assert wpack.dtype == dtype and wpack.is_contiguous() and wpack.numel() == _cabi.lib().igs_condition3d_pack_elems(Cc, hid, int(half))
    W1, W2 = m.mlp[0].weight.detach().to(dtype).numpy(), m.mlp[2].weight.detach().to(dtype).numpy()
    want = FR.pack_restate(W1, W2, Cc, half)                             # zeros wherever the definition puts no weight
    assert np.array_equal(wpack.numpy(), want)
    assert (W1 != 0).all() and np.count_nonzero(want) == W1.size + W2.size
    # what the float32 kernel reads as the depth column: element 0 of lane (r, 0), chunk 0 of tile (ot, 1)
    if not half:
        for o in range(hid):
            assert wpack[(2 * (o // 32) + 1) * 1024 + 4 * (o % 32)] == m.mlp[0].weight[o, 32]
    assert bpack.dtype == torch.float32 and bpack.shape == (3, 128)
    b1, b2 = m.mlp[0].bias.detach(), m.mlp[2].bias.detach()
    want_b = torch.zeros(3, 128)
    want_b[0, :hid], want_b[1, :Cc], want_b[2, :Cc] = b1, b2[:Cc], b2[Cc:]
    assert torch.equal(bpack, want_b)
    nb = CR.AdaLNModule(Cc, hidden=hid)
    nb.mlp[2].bias = None
    assert (motion.pack_condition_mlp(nb.mlp)[1][1:] == 0).all()


# ---------------------------------------------------------------- the compiled module and the Python layer
def _case(N=4, Cc=8, H=6, W=10, hid=128):
    torch.manual_seed(3)
    return (torch.zeros(N, Cc, H, W), torch.zeros(N // 2, 2, H, W, 6), torch.zeros(N // 2, 2, 15, 23), CR.AdaLNModule(Cc, hidden=hid))


def test_compiled_module_refusals():
    from igs_amd import _cabi, motion
    E = _cabi.ext()._cond
    x, rays, depth, m = _case()
    rays, depth = rays.reshape(4, 6, 10, 6), depth.reshape(4, 15, 23)
    wpack, bpack = motion.pack_condition_mlp(m.mlp)
    w, b = m.norm.weight.detach(), m.norm.bias.detach()
    assert E.pack_elems(8, 128, False) == wpack.numel() and E.pack_elems(129, 128, False) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.condition3d_fwd(x, rays, depth, wpack, bpack, 128, w, b, 1e-6)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.condition3d_fwd(x.double(), rays, depth, wpack, bpack, 128, w, b, 1e-6)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.condition3d_fwd(x, rays, depth, wpack.bfloat16(), bpack, 128, w, b, 1e-6)
    with pytest.raises(NotImplementedError, match="rays must be"):
        E.condition3d_fwd(x, rays.half(), depth, wpack, bpack, 128, w, b, 1e-6)
    for bad in (dict(x=x[0]), dict(rays=rays[..., :5]), dict(rays=rays[:3]), dict(depth=depth[:3]), dict(wpack=wpack[:-1]), dict(bpack=bpack[:2]),
                dict(w=w[:7]), dict(b=b[:7]), dict(hidden=64)):
        k = dict(x=x, rays=rays, depth=depth, wpack=wpack, bpack=bpack, hidden=128, w=w, b=b)
        k.update(bad)
        with pytest.raises(RuntimeError, match="shape"):
            E.condition3d_fwd(k["x"], k["rays"], k["depth"], k["wpack"], k["bpack"], k["hidden"], k["w"], k["b"], 1e-6)
    with pytest.raises(RuntimeError, match="1..128"):
        E.condition3d_fwd(torch.zeros(1, 129, 1, 1), torch.zeros(1, 1, 1, 6), torch.zeros(1, 1, 1), wpack, bpack, 128, torch.ones(129), torch.ones(129), 1e-6)
    with pytest.raises(RuntimeError, match="out of range"):
        E.condition3d_fwd(torch.zeros(1, 8, 1, 8193), torch.zeros(1, 1, 8193, 6), torch.zeros(1, 1, 1), wpack, bpack, 128, w, b, 1e-6)


def test_python_layer_exceptions():
    from igs_amd import motion
    x, rays, depth, m = _case()
    f = motion.condition3d_fused
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, rays, depth, m)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, rays, depth, m, mlp_dtype=torch.float16)
        with pytest.raises(ValueError, match="motion_feature must be"):
            f(x[0], rays, depth, m)
        with pytest.raises(ValueError, match="rays must be"):
            f(x, rays[0], depth, m)
        with pytest.raises(ValueError, match="rays must be"):
            f(x, rays[..., :5], depth, m)
        with pytest.raises(ValueError, match="do not match"):
            f(x, rays[:1], depth[:1], m)
        with pytest.raises(ValueError, match="depth must be"):
            f(x, rays, depth[0], m)
        with pytest.raises(ValueError, match="feature resolution"):
            f(x.transpose(2, 3), rays, depth, m)
        with pytest.raises(ValueError, match="normalises"):
            f(x[:, :7], rays, depth, m)
        with pytest.raises(NotImplementedError, match="rays and depth must be float32"):
            f(x, rays.half(), depth, m)
        with pytest.raises(NotImplementedError, match="float32 or float16"):
            f(x.bfloat16(), rays, depth, m)
        with pytest.raises(NotImplementedError, match="mlp_dtype"):
            f(_OnGpu.of(x), _OnGpu.of(rays), _OnGpu.of(depth), m, mlp_dtype=torch.bfloat16)
        # an .mlp of another structure
        nn = torch.nn
        for mlp in (nn.Sequential(nn.Linear(33, 128), nn.ReLU(), nn.Linear(128, 16)), nn.Sequential(nn.Linear(33, 128), nn.SiLU(), nn.Linear(128, 16), nn.SiLU()),
                    nn.Sequential(nn.Linear(33, 16)), nn.Sequential(nn.Linear(32, 128), nn.SiLU(), nn.Linear(128, 16)),
                    nn.Sequential(nn.Linear(33, 128), nn.SiLU(), nn.Linear(128, 8)), nn.Sequential(nn.Linear(33, 129), nn.SiLU(), nn.Linear(129, 16)),
                    lambda c: c):
            other = types.SimpleNamespace(norm=m.norm, mlp=mlp)
            with pytest.raises(NotImplementedError, match="mlp must|1..128"):
                f(x, rays, depth, other)
        big = CR.AdaLNModule(129)
        with pytest.raises(NotImplementedError, match="1..128"):
            f(torch.zeros(4, 129, 6, 10), rays, depth, big)
        noaffine = types.SimpleNamespace(norm=nn.LayerNorm(8, elementwise_affine=False), mlp=m.mlp)
        with pytest.raises(NotImplementedError, match="affine"):
            f(x, rays, depth, noaffine)
    # forward only: anything that requires grad under enabled grad
    with pytest.raises(NotImplementedError, match="forward only"):
        f(x, rays, depth, m)                                             # the module's parameters
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="forward only"):
        f(x.clone().requires_grad_(True), rays, depth, m)
    with pytest.raises(NotImplementedError, match="forward only"):
        f(x, rays, depth.clone().requires_grad_(True), m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, rays, depth, m)                                             # nothing requires grad: the same as under no_grad


# ---------------------------------------------------------------- the binder
class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on a GPU: lets the Python layer run up to its call into the compiled module."""
    is_cuda = property(lambda self: True)

    @staticmethod
    def of(t):
        return t.as_subclass(_OnGpu)


class _StandIn:
    """The compiled module's fused entry (_C._cond.condition3d_fwd): records its arguments and returns zeros."""

    def __init__(self):
        self.fused = []
        self._cond = self

    def condition3d_fwd(self, x, rays, depth, wpack, bpack, hidden, weight, bias, eps):
        self.fused.append(dict(x=x, rays=rays, depth=depth, wpack=wpack, bpack=bpack, hidden=hidden, weight=weight, bias=bias, eps=eps))
        return torch.zeros(x.shape)


def _model(Cc=8, local_ray=False, use_condition3d=True):
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = types.SimpleNamespace(local_ray=local_ray, use_condition3d=use_condition3d)
            self.ModLN = CR.AdaLNModule(Cc)

        def condition3D(self, motion_feature, rays, depth):
            raise AssertionError("the class's method must not be reached once bound")
    return Model()


def test_binder_dispatch(monkeypatch):
    from igs_amd import motion
    ext, three_step = _StandIn(), []
    monkeypatch.setattr(motion, "_ext", lambda: ext)
    monkeypatch.setattr(motion, "condition3d", lambda *a: three_step.append(a) or "three-step")
    for kw in (dict(local_ray=True), dict(use_condition3d=False)):
        model = _model(**kw)
        with pytest.raises(NotImplementedError, match="local_ray|use_condition3d"):
            motion.use_native_condition3d(model)
        assert "condition3D" not in model.__dict__                       # nothing was changed
    model = _model()
    keys = list(model.state_dict())
    assert motion.use_native_condition3d(model) is model and list(model.state_dict()) == keys
    x, rays, depth, _ = _case()
    x, rays, depth = _OnGpu.of(x), _OnGpu.of(rays), _OnGpu.of(depth)
    # a call that needs a gradient (the module's parameters require grad) reaches condition3d with the caller's arguments
    assert model.condition3D(x, rays, depth) == "three-step" and not ext.fused
    assert three_step[-1][0] is x and three_step[-1][3] is model.ModLN
    with torch.no_grad():
        out = model.condition3D(x, rays, depth)
    assert len(three_step) == 1 and len(ext.fused) == 1 and out.shape == x.shape
    call = ext.fused[0]
    assert call["hidden"] == 128 and call["wpack"].dtype == torch.float32 and call["rays"].shape == (4, 6, 10, 6) and call["depth"].shape == (4, 15, 23)
    want = motion.pack_condition_mlp(model.ModLN.mlp)
    assert torch.equal(call["wpack"], want[0]) and torch.equal(call["bpack"], want[1]) and call["eps"] == model.ModLN.norm.eps
    with torch.no_grad():
        model.condition3D(x, rays, depth)
        assert ext.fused[1]["wpack"] is call["wpack"]                    # kept on the module, not packed again
        model.ModLN.mlp[2].weight.mul_(2)                                # an in-place update: the version changes, the pointer does not
        model.condition3D(x, rays, depth)
    assert ext.fused[2]["wpack"] is not call["wpack"]
    assert torch.equal(ext.fused[2]["wpack"], motion.pack_condition_mlp(model.ModLN.mlp)[0]) and not torch.equal(ext.fused[2]["wpack"], call["wpack"])
    # an input that requires grad, with the parameters frozen: still the three-step path; with nothing requiring grad: fused
    for p in model.parameters():
        p.requires_grad_(False)
    model.condition3D(_OnGpu.of(torch.zeros(4, 8, 6, 10).requires_grad_(True)), rays, depth)
    assert len(three_step) == 2 and len(ext.fused) == 3
    model.condition3D(x, rays, depth)
    assert len(three_step) == 2 and len(ext.fused) == 4
    # a module that does not qualify keeps the three-step path
    model.ModLN.mlp = torch.nn.Sequential(torch.nn.Linear(33, 128), torch.nn.ReLU(), torch.nn.Linear(128, 16))
    with torch.no_grad():
        model.condition3D(x, rays, depth)
    assert len(three_step) == 3 and len(ext.fused) == 4
