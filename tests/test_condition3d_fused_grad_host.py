"""The fused condition3D backward without a GPU (igs_amd/csrc/cond_fused_bwd.hip, igs_amd/motion.py): the float64 restatement of the
gradients (tests/condition3d_fused_grad_restatement.py) against torch.autograd and against the reference's recorded gradients
(tests/golden/ref_condition3d.npz), the transposed pack, the exports with their declared signatures, every refusal of igs_condition3d_bwd
before any HIP call, the scratch size, the Python layer's exceptions, the training binder's dispatch (with a stand-in for the compiled
module) and the resources of the built gfx950 kernels."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import condition3d_fused_grad_restatement as GR
import condition3d_fused_restatement as FR
import condition3d_restatement as CR
import decoder_restatement as DR
from test_condition3d_fused_host import _OnGpu, _aligned_buffer, _case, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_condition3d_bwd_scratch_bytes", "igs_condition3d_bwd")
CHUNK = GR.CHUNK_ROWS                                                    # IGS_COND_BWD_CHUNK_ROWS


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_condition3d.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _inputs(N, Cc, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cc, H, W, generator=g)
    rays = torch.randn(1, N, H, W, 6, generator=g)
    depth = torch.rand(1, N, 2 * H + 1, W + 3, generator=g) * 3 + 0.5
    gout = torch.randn(N, Cc, H, W, generator=g)
    return x, rays, depth, gout


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("Cc,hid,N,H,W", [(7, 5, 2, 3, 5), (8, 128, 3, 4, 3), (33, 65, 1, 2, 7)])
def test_restatement_equals_float64_autograd(Cc, hid, N, H, W):
    torch.manual_seed(Cc * hid)
    m = CR.AdaLNModule(Cc, hidden=hid)
    with torch.no_grad():
        m.norm.weight.uniform_(0.5, 1.5)
        m.norm.bias.uniform_(-0.5, 0.5)
    x, rays, depth, gout = _inputs(N, Cc, H, W, Cc + hid)
    grads, _ = GR.restate(x, rays, depth, m, gout)
    md = CR.AdaLNModule(Cc, hidden=hid).double()
    md.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    xd = x.double().requires_grad_(True)
    CR.reference_composition(xd, rays.double(), depth.double(), md).backward(gout.double())
    got = GR.module_grads(xd, md)
    for k in GR.NAMES:
        d = (got[k] - grads[k]).abs().max()
        assert d <= 1e-10 * (1 + grads[k].abs().max()), (k, float(d))


def test_restatement_reproduces_the_reference_fixture(fx):
    """The fixture's dx, dweight, dbias and dmod are the reference's float32 gradients of the modulated LayerNorm at its own float32 mod.
    The restated ones differ by modln_backward_bounds on the fixture's mod plus what the MLP error E (which also bounds
    |fixture mod - mod64|) moves them."""
    module = CR.AdaLNModule.from_arrays(fx)
    grads, bounds = GR.restate(fx["x"], fx["rays"], fx["depth"], module, fx["gout"])
    lb = CR.modln_backward_bounds(fx["x"], fx["mod"], fx["norm_weight"], fx["norm_bias"], float(fx["eps"]), fx["gout"])
    ratios = dict(dx=FR.worst(fx["dx"], grads["dx"], lb["dx"] + bounds["moved"]["dx"]),
                  dweight=FR.worst(fx["dweight"], grads["dnw"], lb["dweight"] + bounds["moved"]["dnw"]),
                  dbias=FR.worst(fx["dbias"], grads["dnb"], lb["dbias"] + bounds["moved"]["dnb"]),
                  dmod=FR.worst(fx["dmod"], grads["dmod"], lb["dmod"]))
    print("fixture: max |reference - restated| / bound", {k: round(v, 3) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert grads["dmod"].shape == fx["dmod"].shape
    # not vacuous on this fixture either
    for mut, key, ref in (("unbiased_dx", "dx", "dx"), ("dscale_without_n", "dmod", "dmod")):
        wrong, _ = GR.restate(fx["x"], fx["rays"], fx["depth"], module, fx["gout"], mutate=mut)
        assert FR.worst(fx[ref], wrong[key], lb[ref] + (bounds["moved"]["dx"] if key == "dx" else 0)) > 1.0, mut


# ---------------------------------------------------------------- the transposed pack
@pytest.mark.parametrize("Cc,hid", [(8, 128), (7, 5), (33, 65), (128, 1), (96, 32)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_transposed_pack_puts_every_weight_where_the_header_says(Cc, hid, dtype):
    from igs_amd import motion
    torch.manual_seed(Cc + hid)
    m = CR.AdaLNModule(Cc, hidden=hid)
    half = dtype == torch.float16
    wpack, bpack, wpack_t = motion.pack_condition_mlp(m.mlp, dtype, transposed=True)
    two = motion.pack_condition_mlp(m.mlp, dtype)
    assert len(two) == 2 and torch.equal(wpack, two[0]) and torch.equal(bpack, two[1])
    ct, ht = -(-Cc // 32), -(-hid // 32)
    assert wpack_t.dtype == dtype and wpack_t.is_contiguous() and wpack_t.numel() == 2 * ct * ht * 1024
    W2 = m.mlp[2].weight.detach().to(dtype).numpy()
    M = np.zeros((hid, 64 * ct), W2.dtype)                               # M[j][32 ct s + c] = W2[s C + c][j]
    M[:, :Cc] = W2[:Cc].T
    M[:, 32 * ct:32 * ct + Cc] = W2[Cc:].T
    want = DR.pack_tile_order(M, half)
    assert np.array_equal(wpack_t.numpy(), want) and np.count_nonzero(want) == W2.size
    # element by element from the header's sentence: tile (ot, kt) of ht x 2 ct, element e = chunk E + j of lane (r, h)
    E = 8 if half else 4
    flat = wpack_t.numpy()
    rng = np.random.RandomState(0)
    for _ in range(64):
        j, s, c = rng.randint(hid), rng.randint(2), rng.randint(Cc)
        i = 32 * ct * s + c
        ot, r, kt, col = j // 32, j % 32, i // 32, i % 32
        h, e = (col >> 2) & 1, (col & 3) + 4 * (col >> 3)
        assert flat[(ot * 2 * ct + kt) * 1024 + ((e // E) * 64 + 32 * h + r) * E + e % E] == W2[s * Cc + c, j]


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
    assert len(_cabi.SIGNATURES["igs_condition3d_bwd"][1]) == 33 and len(_cabi.SIGNATURES["igs_condition3d_bwd_scratch_bytes"][1]) == 5
    assert "#define IGS_COND_BWD_CHUNK_ROWS %d" % CHUNK in h
    assert "cond_fused_bwd.hip" in open(os.path.join(ROOT, "igs_amd", "build.py")).read()
    assert L.igs_rast_version() == 4


def _pstride(Cc, hid):
    return (hid * 33 + 2 * Cc * hid + hid + 2 * Cc + 2 * Cc + 3) & ~3


def test_scratch_bytes():
    """7 float32 [rows][128] slots of one chunk plus one partial per started slice of 256 rows, rows = 32 per started group of 32 pixels
    of an image, capped at the chunk: monotone in the pixel count, constant above one chunk."""
    from igs_amd import _cabi
    L = _cabi.lib()
    f = L.igs_condition3d_bwd_scratch_bytes

    def want(N, Cc, hid, H, W):
        rows = min(GR.padded_rows(N, H, W), CHUNK)
        return 4 * (7 * rows * 128 + -(-rows // GR.SLICE_ROWS) * _pstride(Cc, hid))
    for N, Cc, hid, H, W in ((1, 128, 128, 1, 1), (4, 8, 128, 6, 10), (3, 7, 5, 33, 2), (2, 33, 65, 100, 100), (16, 128, 128, 128, 128)):
        assert f(N, Cc, hid, H, W) == want(N, Cc, hid, H, W), (N, Cc, hid, H, W)
    # below, at and above the chunk: two images of CHUNK - 64, CHUNK and CHUNK + 32 pixels in all, then many
    sizes = [f(2, 32, 32, 1, CHUNK // 2 - 32), f(2, 32, 32, 1, CHUNK // 2),
             f(2, 32, 32, 2, CHUNK // 4 + 8), f(64, 32, 32, 2, CHUNK // 4 + 8), f(4, 32, 32, 2048, 2048)]
    assert sizes[0] < sizes[1] == sizes[2] == sizes[3] == sizes[4], sizes
    assert sizes[1] == 4 * (7 * CHUNK * 128 + GR.SLICES * _pstride(32, 32))
    prev = 0
    for px in (1, 31, 32, 33, 255, 256, 257, 4096, CHUNK // 2 - 1, CHUNK // 2):
        cur = f(2, 128, 128, 1, px)
        assert cur >= prev, px
        prev = cur
    assert f(0, 8, 8, 4, 4) == 0
    for bad in ((-1, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 129, 8, 4, 4), (1, 8, 0, 4, 4), (1, 8, 129, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 8193),
                (5, 8, 8, 2048, 2048)):
        assert f(*bad) == -1, bad


def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1) with a message, never IGS_RAST_E_HIP (-2): without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    raw, p = _aligned_buffer()
    err = _cabi.last_error
    IN = ("x", "rays", "depth", "wpack", "wpack_t", "bpack", "weight", "bias", "gout", "scratch")
    OUT = ("dx", "dW1", "db1", "dW2", "db2", "dweight", "dbias")

    def bwd(N=4, Cc=8, hid=128, H=6, W=10, Hd=15, Wd=23, xdt=0, mdt=0, xs=None, eps=1e-6, sb=1 << 40, **ptrs):
        xs = xs or (Cc * H * W, H * W, W, 1)
        q = {k: p for k in IN + OUT}
        q.update(ptrs)
        return L.igs_condition3d_bwd(None, N, Cc, hid, H, W, Hd, Wd, xdt, q["x"], *xs, q["rays"], q["depth"], mdt, q["wpack"], q["wpack_t"],
                                     q["bpack"], q["weight"], q["bias"], eps, q["gout"], q["scratch"], sb, *[q[k] for k in OUT])

    bad = ((dict(N=-1), "N out of range"), (dict(Cc=0), "C out of range"), (dict(Cc=129), "C out of range"), (dict(hid=0), "hidden out of range"),
           (dict(hid=129), "hidden out of range"), (dict(H=0), "H out of range"), (dict(H=8193), "H out of range"), (dict(W=0), "W out of range"),
           (dict(W=8193), "W out of range"), (dict(Hd=0), "Hd out of range"), (dict(Hd=8193), "Hd out of range"), (dict(Wd=0), "Wd out of range"),
           (dict(Wd=8193), "Wd out of range"), (dict(N=5, H=2048, W=2048), "N * H * W out of range"), (dict(xdt=2), "dtype"), (dict(xdt=-1), "dtype"),
           (dict(mdt=2), "dtype"), (dict(mdt=-1), "dtype"), (dict(xs=(480, 1, 80, 8)), "channels-last"),
           (dict(xs=(480, 60, 11, 1)), "plane must be contiguous"), (dict(xs=(-1, 60, 10, 1)), "negative"), (dict(xs=(480, -60, 10, 1)), "negative"),
           (dict(xs=(480, (1 << 27) + 1, 10, 1)), "IGS_COND_FUSED_MAX_STRIDE"), (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"),
           (dict(sb=L.igs_condition3d_bwd_scratch_bytes(4, 8, 128, 6, 10) - 1), "scratch is smaller"), (dict(sb=0), "scratch is smaller"))
    for kw, what in bad:
        assert bwd(**kw) == -1 and what in err() and "igs_condition3d_bwd" in err(), (kw, err())
    for name in IN:
        assert bwd(**{name: None}) == -1 and "NULL" in err(), name
        if name != "x":
            assert bwd(**{name: p + (4 if name in ("wpack", "wpack_t", "scratch") else 2)}) == -1 and "aligned" in err(), (name, err())
    for name in OUT:
        assert bwd(**{name: p + (1 if name == "dx" else 2)}) == -1 and "aligned" in err(), (name, err())
    assert bwd(x=p + 2) == -1 and "aligned" in err()
    assert bwd(x=p + 1, xdt=1) == -1 and "aligned" in err()
    assert bwd(dx=p + 2) == -1 and "aligned" in err()                    # a float32 d x on a 2-byte boundary
    assert bwd(wpack_t=p + 8, mdt=1) == -1 and "16 bytes" in err()
    # N == 0 and no output wanted: 0 without a launch
    assert bwd(N=0, **{k: None for k in IN + OUT}) == 0
    assert bwd(sb=L.igs_condition3d_bwd_scratch_bytes(4, 8, 128, 6, 10), **{k: None for k in OUT}) == 0
    del raw


# ---------------------------------------------------------------- the compiled module and the Python layer
def test_compiled_module_refusals():
    from igs_amd import _cabi, motion
    E = _cabi.ext()._cond
    x, rays, depth, m = _case()
    rays, depth = rays.reshape(4, 6, 10, 6), depth.reshape(4, 15, 23)
    wpack, bpack, wpack_t = motion.pack_condition_mlp(m.mlp, transposed=True)
    w, b, g = m.norm.weight.detach(), m.norm.bias.detach(), torch.zeros_like(x)
    assert E.bwd_scratch_bytes(4, 8, 128, 6, 10) == _cabi.lib().igs_condition3d_bwd_scratch_bytes(4, 8, 128, 6, 10)
    assert E.bwd_scratch_bytes(4, 129, 128, 6, 10) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.condition3d_bwd(x, rays, depth, wpack, wpack_t, bpack, 128, w, b, 1e-6, g)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.condition3d_bwd(x.double(), rays, depth, wpack, wpack_t, bpack, 128, w, b, 1e-6, g)
    for bad in (dict(x=x[0]), dict(rays=rays[:3]), dict(depth=depth[:3]), dict(wpack=wpack[:-1]), dict(wpack_t=wpack_t[:-1]), dict(wpack_t=wpack_t.half()),
                dict(bpack=bpack[:2]), dict(w=w[:7]), dict(g=g[:3]), dict(g=g.half()), dict(hidden=64)):
        k = dict(x=x, rays=rays, depth=depth, wpack=wpack, wpack_t=wpack_t, bpack=bpack, hidden=128, w=w, b=b, g=g)
        k.update(bad)
        with pytest.raises((RuntimeError, NotImplementedError), match="shape|must be"):
            E.condition3d_bwd(k["x"], k["rays"], k["depth"], k["wpack"], k["wpack_t"], k["bpack"], k["hidden"], k["w"], k["b"], 1e-6, k["g"])


def test_python_layer_exceptions():
    from igs_amd import motion
    x, rays, depth, m = _case()
    f = motion.condition3d_fused_autograd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x, rays, depth, m)                                             # the parameters require grad: the training path, on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(x.clone().requires_grad_(True), rays, depth, m, mlp_dtype=torch.float16)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, rays, depth, m)                                         # condition3d_fused itself
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        f(x.bfloat16(), rays, depth, m)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        f(x.double(), rays, depth, m)
    with pytest.raises(NotImplementedError, match="mlp_dtype"):
        f(x, rays, depth, m, mlp_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="motion_feature must be"):
        f(x[0], rays, depth, m)
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
    with pytest.raises(NotImplementedError, match="rays and depth"):
        f(x, rays.clone().requires_grad_(True), depth, m)
    with pytest.raises(NotImplementedError, match="rays and depth"):
        f(x, rays, depth.clone().requires_grad_(True), m)
    two, three = motion.pack_condition_mlp(m.mlp), motion.pack_condition_mlp(m.mlp, transposed=True)
    with pytest.raises(ValueError, match="transposed=True"):
        f(x, rays, depth, m, packed=two)
    with pytest.raises(ValueError, match="packed holds"):
        f(x, rays, depth, m, packed=three, mlp_dtype=torch.float16)
    with pytest.raises(ValueError, match="packed holds"):
        f(x, rays, depth, m, packed=(three[0], three[1], three[2].half()))
    other = torch.nn.Sequential(torch.nn.Linear(33, 128), torch.nn.ReLU(), torch.nn.Linear(128, 16))
    with pytest.raises(NotImplementedError, match="mlp must"):
        f(x, rays, depth, _Other(m.norm, other))


class _Other:
    def __init__(self, norm, mlp):
        self.norm, self.mlp = norm, mlp


# ---------------------------------------------------------------- the binder
class _StandIn:
    """The compiled module's fused entries: record their arguments; zeros forward, Nones-or-zeros backward."""

    def __init__(self):
        self.fused, self.bwd = [], []
        self._cond = self

    def condition3d_fwd(self, x, rays, depth, wpack, bpack, hidden, weight, bias, eps):
        self.fused.append(dict(x=x, wpack=wpack, bpack=bpack, hidden=hidden))
        return torch.zeros(x.shape)

    def condition3d_bwd(self, x, rays, depth, wpack, wpack_t, bpack, hidden, weight, bias, eps, g, *wants):
        self.bwd.append(dict(x=x, wpack_t=wpack_t, g=g, wants=wants))
        C = x.shape[1]
        shapes = (x.shape, (hidden, 33), (hidden,), (2 * C, hidden), (2 * C,), (C,), (C,))
        return tuple(torch.zeros(s) if w else None for s, w in zip(shapes, wants))


def test_training_binder_dispatch(monkeypatch):
    from igs_amd import motion
    ext, three_step = _StandIn(), []
    monkeypatch.setattr(motion, "_ext", lambda: ext)
    monkeypatch.setattr(motion, "condition3d", lambda *a: three_step.append(a) or "three-step")
    assert set(motion.COND_FUSED_BWD_NATIVE) == {torch.float32, torch.float16}
    assert all(isinstance(v, bool) for v in motion.COND_FUSED_BWD_NATIVE.values())
    for kw in (dict(local_ray=True), dict(use_condition3d=False)):
        model = _model(**kw)
        with pytest.raises(NotImplementedError, match="local_ray|use_condition3d"):
            motion.use_native_condition3d(model, training=True)
        assert "condition3D" not in model.__dict__
    x, rays, depth, _ = _case()
    x, rays, depth = _OnGpu.of(x), _OnGpu.of(rays), _OnGpu.of(depth)

    # the default binds today's method: a call that needs a gradient is the three-step path whatever the table says
    monkeypatch.setattr(motion, "COND_FUSED_BWD_NATIVE", {torch.float32: True, torch.float16: True})
    plain = motion.use_native_condition3d(_model())
    assert plain.condition3D(x, rays, depth) == "three-step" and len(three_step) == 1 and not ext.fused

    model = _model()
    keys, cls = list(model.state_dict()), type(model)
    assert motion.use_native_condition3d(model, training=True) is model and list(model.state_dict()) == keys and type(model) is cls
    # False: condition3d with the caller's arguments
    monkeypatch.setattr(motion, "COND_FUSED_BWD_NATIVE", {torch.float32: False, torch.float16: True})
    assert model.condition3D(x, rays, depth) == "three-step" and len(three_step) == 2 and not ext.fused
    assert three_step[-1][0] is x and three_step[-1][3] is model.ModLN
    # True: the fused Function, its packs kept under the training key
    monkeypatch.setattr(motion, "COND_FUSED_BWD_NATIVE", {torch.float32: True, torch.float16: False})
    out = model.condition3D(x, rays, depth)
    assert len(three_step) == 2 and len(ext.fused) == 1 and out.requires_grad and out.shape == x.shape
    cache = model.ModLN.__dict__[motion.COND_FUSED_TRAIN_CACHE]
    assert len(cache["pack"]) == 3 and ext.fused[0]["wpack"] is cache["pack"][0] and motion.COND_FUSED_CACHE not in model.ModLN.__dict__
    out.sum().backward()
    assert len(ext.bwd) == 1 and ext.bwd[0]["wpack_t"] is cache["pack"][2]
    assert ext.bwd[0]["wants"] == (False, True, True, True, True, True, True)       # x does not require grad
    assert all(p.grad is not None for p in model.ModLN.parameters())
    model.condition3D(x, rays, depth)
    assert model.ModLN.__dict__[motion.COND_FUSED_TRAIN_CACHE] is cache              # kept, not packed again
    with torch.no_grad():
        model.ModLN.mlp[2].weight.mul_(2)                                            # an optimiser step: the version changes
    model.condition3D(x, rays, depth)
    fresh = model.ModLN.__dict__[motion.COND_FUSED_TRAIN_CACHE]
    assert fresh is not cache and torch.equal(fresh["pack"][2], motion.pack_condition_mlp(model.ModLN.mlp, transposed=True)[2])
    # rays that require grad: condition3d (which refuses them), not the fused Function
    n = len(ext.fused)
    model.condition3D(x, _OnGpu.of(torch.zeros(2, 2, 6, 10, 6).requires_grad_(True)), depth)
    assert len(three_step) == 3 and len(ext.fused) == n
    # a call without a gradient still takes the fused forward and the forward's cache
    with torch.no_grad():
        model.condition3D(x, rays, depth)
    assert len(ext.fused) == n + 1 and len(three_step) == 3 and motion.COND_FUSED_CACHE in model.ModLN.__dict__
    # only x requires grad: the weight gradients are not asked for
    for p in model.parameters():
        p.requires_grad_(False)
    xg = _OnGpu.of(torch.zeros(4, 8, 6, 10).requires_grad_(True))
    model.condition3D(xg, rays, depth).sum().backward()
    assert ext.bwd[-1]["wants"] == (True, False, False, False, False, False, False)
    # a module that does not qualify keeps the three-step path
    model.ModLN.mlp = torch.nn.Sequential(torch.nn.Linear(33, 128), torch.nn.ReLU(), torch.nn.Linear(128, 16))
    model.condition3D(x, rays, depth)
    assert len(three_step) == 4


# ---------------------------------------------------------------- the built code objects
def test_backward_kernels_use_no_scratch_and_fit_the_lds():
    """the pixels kernel in four instances (MLP dtype x dtype of x), the hidden and the wgrad kernel in two, one
    reduce kernel; none with private memory or register spills, all within 256 registers and 160 KB of LDS.  The forward's four
    instances are still four."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = A.code_objects(build.LIB)
    try:
        found, fwd = {}, []
        for co in cos:
            for name, md in kernel_metadata(co).items():
                if re.match(r"^_ZL?\d+condition3d_bwd_(pixels|hidden|wgrad|reduce)_kernel", name):
                    found[name] = md
                if re.match(r"^_ZL?\d+condition3d_fused_kernel", name):
                    fwd.append(name)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(fwd) == 4, sorted(fwd)
    count = lambda kind: len([n for n in found if "condition3d_bwd_%s_kernel" % kind in n])
    assert (count("pixels"), count("hidden"), count("wgrad"), count("reduce")) == (4, 2, 2, 1), sorted(found)
    for name, md in found.items():
        print(name, "vgpr", md[".vgpr_count"], "agpr", md.get(".agpr_count", 0), "lds", md[".group_segment_fixed_size"],
              "scalars parked in vector lanes", md.get(".sgpr_spill_count", 0))
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0, (name, "register spills to memory")
        assert int(md[".vgpr_count"]) <= 256, name
        assert int(md[".group_segment_fixed_size"]) <= 160 * 1024, name
