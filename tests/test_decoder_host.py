"""The fused residual decoder (igs_amd/csrc/mlp.hip, igs_amd/motion.py) without a GPU: the float64 restatement against the reference-produced
golden file, exports and argument counts, the refusals of the C ABI before any HIP call and of the Python layer and the binder on CPU
stand-in modules, the packed weight layout against its restated definition, and the scratch and LDS of the built gfx950 kernels."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import decoder_restatement as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_mlp_heads_pack_elems", "igs_mlp_heads_fwd")
INVALID = -1
F32, F16 = 0, 1
SILU, RELU = 0, 1


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("i", [0, 1])
def test_restatement_equals_the_reference(i):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_decoder.npz"))
    tag = "case%d." % i
    idx = [int(j) for j in z[tag + "linear_index"]]
    ws = [z[tag + "mlp.layers.%d.weight" % j] for j in idx]
    bs = [z[tag + "mlp.layers.%d.bias" % j] for j in idx]
    nh = len([k for k in z.files if re.match(re.escape(tag) + r"heads\.\d+\.weight$", k)])
    hws, hbs = [z[tag + "heads.%d.weight" % k] for k in range(nh)], [z[tag + "heads.%d.bias" % k] for k in range(nh)]
    assert z[tag + "x"].dtype == np.float64 and z[tag + "x"].shape[0] == 40
    assert [w.shape for w in ws] == ([(24, 20), (24, 24), (24, 24)] if i == 0 else [(32, 16), (32, 32)])
    assert [w.shape[0] for w in hws] == ([3, 4] if i == 0 else [5]) and list(z[tag + "act_after"]) == ([1, 1, 0] if i == 0 else [1, 0])
    outs, bounds = DR.forward_with_bound(z[tag + "x"], ws, bs, hws, hbs, str(z[tag + "activation"]), list(z[tag + "act_after"]))
    for k, o in enumerate(outs):
        assert np.abs(o - z[tag + "out%d" % k]).max() <= 1e-12
        assert (bounds[k] > 0).all() and bounds[k].max() < 1e-4
    # ... and the stand-in module computes what the restatement does
    r = DR.make_renderer(dim_in=20, n_neurons=24, dim_out=24, n_hidden_layers=2, seed=i).double()
    x = torch.randn(9, 20, dtype=torch.float64)
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    assert aa == [1, 1, 0]
    with torch.no_grad():
        d = r.decode_residual_feature(x)
    for (k, v), o in zip(d.items(), DR.forward(x.numpy(), ws, bs, hws, hbs, "silu", aa)):
        assert np.abs(v.numpy() - o).max() <= 1e-12, k


def test_bound_rejects_a_wrong_decoder_and_accepts_float32_pytorch():
    """The bound is tight enough to matter: float32 eager PyTorch is inside it, a decoder with an activation behind the last hidden Linear,
    one with ReLU for SiLU and one with two columns of a weight swapped are far outside."""
    r = DR.make_renderer(dim_in=33, n_neurons=50, dim_out=40, n_hidden_layers=2, seed=5)
    x = torch.randn(200, 33, generator=torch.Generator().manual_seed(1))
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    want, bound = DR.forward_with_bound(x.double().numpy(), ws, bs, hws, hbs, "silu", aa)
    with torch.no_grad():
        eager = list(r.decode_residual_feature(x).values())
    ratio = max(DR.worst_ratio(e.double().numpy(), w, b) for e, w, b in zip(eager, want, bound))
    swapped = [w.copy() for w in ws]
    swapped[1][:, [0, 1]] = swapped[1][:, [1, 0]]
    wrong = {"act_after": DR.forward(x.double().numpy(), ws, bs, hws, hbs, "silu", [1, 1, 1]),
             "relu": DR.forward(x.double().numpy(), ws, bs, hws, hbs, "relu", aa),
             "swapped": DR.forward(x.double().numpy(), swapped, bs, hws, hbs, "silu", aa)}
    bad = {k: max(DR.worst_ratio(o, w, b) for o, w, b in zip(v, want, bound)) for k, v in wrong.items()}
    print("float32 eager PyTorch: worst |error| / bound %.4f; wrong variants %s" % (ratio, {k: "%.3g" % v for k, v in bad.items()}))
    assert ratio <= 1.0 and all(v > 100 for v in bad.values())
    # ... and the swapped columns are a different operand for the kernel too: the pack places every weight, so it cannot hide them
    from igs_amd.motion import pack_mlp
    t = lambda arrs: [None if a is None else torch.from_numpy(a).float() for a in arrs]
    right, wrong_pack = pack_mlp(t(ws), t(bs), t(hws), t(hbs)), pack_mlp(t(swapped), t(bs), t(hws), t(hbs))
    assert right[0].shape == wrong_pack[0].shape and torch.equal(right[1], wrong_pack[1])
    differ = (right[0] != wrong_pack[0]).nonzero().flatten()
    assert differ.numel() == 2 * 50 - 2 * int((ws[1][:, 0] == ws[1][:, 1]).sum()) and differ.min() >= 2 * 2 * 1024          # layer 1's tiles only


# ---------------------------------------------------------------- exports and ABI
def test_exports_and_argument_counts():
    from igs_amd import _cabi, build
    from igs_amd import motion as M
    L = _cabi.lib()
    hdr = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m, n
        assert len(_cabi.SIGNATURES[n][1]) == len(m.group(1).split(",")), n
    assert "mlp.hip" in build.SOURCES
    ext = _cabi.ext()
    for f in ("mlp_heads_fwd", "pack_elems"):
        assert hasattr(ext._mlp, f), f                                                           # (a private submodule of _C)
    for name, val in (("WIDTH", M.MLP_MAX_WIDTH), ("HIDDEN", M.MLP_MAX_HIDDEN), ("HEADS", M.MLP_MAX_HEADS)):
        assert re.search(r"#define IGS_MLP_MAX_%s %d\b" % (name, val), hdr), name
    assert (M.MLP_MAX_WIDTH, M.MLP_MAX_HIDDEN, M.MLP_MAX_HEADS) == (128, 3, 8)
    for name, code in M.MLP_ACTIVATIONS.items():
        assert re.search(r"#define IGS_MLP_ACT_%s %d\b" % (name.upper(), code), hdr), name
    for fn in ("mlp_heads", "decode_residual_feature", "use_native_decoder", "pack_mlp"):
        assert callable(getattr(M, fn)), fn


def _ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


X, WP, BP, O0, O1 = 0x10000000, 0x30000000, 0x50000000, 0x70000000, 0x90000000


def _fwd(L, N=1000, dtype=F32, act=SILU, widths=(128, 128, 128, 128), act_after=(1, 1, 0), heads=(3, 4), x=X, rs=None, wp=WP, bp=BP, outs=(O0, O1),
         n_hidden=None, n_heads=None):
    n_hidden = (len(widths) - 1 if widths is not None else 0) if n_hidden is None else n_hidden
    n_heads = (len(heads) if heads is not None else 0) if n_heads is None else n_heads
    o = None if outs is None else (ctypes.c_void_p * len(outs))(*outs)
    rs = (widths[0] if widths else 1) if rs is None else rs
    return L.igs_mlp_heads_fwd(None, N, dtype, act, n_hidden, _ints(widths), _ints(act_after), n_heads, _ints(heads), x, rs, wp, bp, o)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    L = _cabi.lib()
    cases = [(dict(N=-1), "N out of range"), (dict(N=(1 << 32) + 1), "N out of range"),
             (dict(widths=(0, 128, 128, 128)), "width"), (dict(widths=(128, 129, 128, 128)), "width"), (dict(widths=(128, 128, 128, -3)), "width"),
             (dict(widths=(256,), act_after=()), "width"),
             (dict(widths=(128,) * 5, act_after=(1,) * 4), "n_hidden"), (dict(n_hidden=-1), "n_hidden"),
             (dict(heads=(), outs=()), "n_heads"), (dict(heads=(1,) * 9, outs=(O0,) * 9), "n_heads"), (dict(n_heads=0), "n_heads"),
             (dict(heads=(3, 0)), "head width"), (dict(heads=(3, 129)), "head width"), (dict(heads=(64, 65)), "add up"), (dict(heads=(128, 1)), "add up"),
             (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(act=2), "activation"), (dict(act=-1), "activation"),
             (dict(x=None), "NULL"), (dict(wp=None), "NULL"), (dict(bp=None), "NULL"), (dict(outs=None), "NULL"), (dict(outs=(O0, None)), "NULL output"),
             (dict(widths=None, n_hidden=3), "NULL widths"), (dict(heads=None, n_heads=2), "NULL widths or head_widths"), (dict(act_after=None), "NULL act_after"),
             (dict(rs=127), "row stride"), (dict(rs=0), "row stride"), (dict(rs=-128), "row stride"), (dict(rs=(1 << 31) + 4), "row stride"),
             (dict(x=X + 2), "aligned to its element size"), (dict(dtype=F16, x=X + 1), "aligned"), (dict(outs=(O0 + 2, O1)), "aligned"),
             (dict(bp=BP + 2), "aligned"), (dict(wp=WP + 8), "16 bytes")]
    for kw, word in cases:
        assert _fwd(L, **kw) == INVALID, kw
        assert word in _cabi.last_error() and "igs_mlp_heads_fwd" in _cabi.last_error(), (kw, _cabi.last_error())
    assert _fwd(L, N=0) == 0 and _fwd(L, N=0, x=None, wp=None, bp=None, outs=None) == 0          # nothing to do
    assert _fwd(L, N=0, widths=(129, 128, 128, 128)) == INVALID and _fwd(L, N=0, act=5) == INVALID and _fwd(L, N=0, rs=64) == INVALID
    assert _fwd(L, N=0, widths=(1,), act_after=(), heads=(128,), outs=(O0,)) == 0                # the corners of the ranges are in
    pe = L.igs_mlp_heads_pack_elems
    assert pe(3, _ints((128, 128, 128, 128)), 2, _ints((3, 4))) == (3 * 16 + 4) * 1024           # the shipped decoder: 104 KB of half
    assert pe(0, _ints((33,)), 1, _ints((7,))) == 2 * 1024 and pe(2, _ints((20, 24, 64)), 1, _ints((128,))) == (1 + 2 + 8) * 1024
    for args in ((4, (128,) * 5, 1, (7,)), (1, (128, 129), 1, (7,)), (0, (0,), 1, (7,)), (0, (8,), 0, ()), (0, (8,), 2, (100, 29)), (0, (8,), 9, (1,) * 9)):
        assert pe(args[0], _ints(args[1]), args[2], _ints(args[3])) == -1, args
    assert pe(0, None, 1, _ints((7,))) == -1


# ---------------------------------------------------------------- the packed layout
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_pack_equals_the_restated_layout_on_asymmetric_integer_weights(half):
    from igs_amd import _cabi
    from igs_amd.motion import pack_mlp, pack_mlp_tile_order
    dt = torch.float16 if half else torch.float32
    for O, I in ((40, 70), (1, 1), (128, 128), (33, 32), (7, 128)):
        W = ((torch.arange(O * I).reshape(O, I) * 7 + 3) % 2039 - 1000).to(dt)                   # no two entries of a tile alike; |.| <= 1039: exact in half
        assert not half or torch.equal(W.double(), ((torch.arange(O * I).reshape(O, I) * 7 + 3) % 2039 - 1000).double())
        got = pack_mlp_tile_order(W)
        assert got.dtype == dt and np.array_equal(got.numpy(), DR.pack_tile_order(W.numpy(), half)), (O, I)
    g = torch.Generator().manual_seed(0)
    ws = [torch.randn(24, 20, generator=g).to(dt), torch.randn(64, 24, generator=g).to(dt)]
    bs = [torch.randn(24, generator=g).to(dt), None]
    hws, hbs = [torch.randn(3, 64, generator=g).to(dt), torch.randn(4, 64, generator=g).to(dt)], [None, torch.randn(4, generator=g).to(dt)]
    wpack, bpack = pack_mlp(ws, bs, hws, hbs)
    want = np.concatenate([DR.pack_tile_order(w.numpy(), half) for w in ws + [torch.cat(hws, 0)]])
    assert wpack.dtype == dt and wpack.is_contiguous() and np.array_equal(wpack.numpy(), want)
    assert wpack.numel() == _cabi.lib().igs_mlp_heads_pack_elems(2, _ints((20, 24, 64)), 2, _ints((3, 4)))
    assert bpack.dtype == torch.float32 and bpack.shape == (3, 128)
    assert torch.equal(bpack[0, :24], bs[0].float()) and not bpack[0, 24:].any() and not bpack[1].any()
    assert not bpack[2, :3].any() and torch.equal(bpack[2, 3:7], hbs[1].float()) and not bpack[2, 7:].any()


# ---------------------------------------------------------------- the built code objects
def test_kernels_use_no_scratch_and_fit_the_lds():
    """four instances (float16 / float32, four-element or scalar loads of x); none with scratch or register spills
    to memory; the register budget of the residency the design counts on (128 in half: one workgroup of 16 waves, 4 per SIMD; 256 in
    float: two workgroups of 4 waves, 2 per SIMD; the counts themselves are printed, they move with the compiler); LDS within the 160 KB
    of a gfx950 compute unit: every layer at once in half (128 KB + 3.5 KB), one layer in float (64 KB + 3.5 KB, twice per unit)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = A.code_objects(build.LIB)
    try:
        found = {}
        for co in cos:
            for name, md in kernel_metadata(co).items():
                if re.match(r"^_ZL?\d+mlp_heads_kernel", name):
                    found[name] = md
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(found) == 4, sorted(found)
    for name, md in found.items():
        half = "IDF16_" in name
        print(name, "vgpr", md[".vgpr_count"], "agpr", md.get(".agpr_count", 0), "lds", md[".group_segment_fixed_size"])
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0, (name, "register spills to memory")
        assert int(md[".vgpr_count"]) + int(md.get(".agpr_count", 0)) <= (128 if half else 256), name
        assert int(md[".max_flat_workgroup_size"]) == (1024 if half else 256), name
        assert int(md[".group_segment_fixed_size"]) <= 160 * 1024, name
        assert int(md[".group_segment_fixed_size"]) == (4 * 32768 if half else 65536) + 2048 + 1024 + 512, name


# ---------------------------------------------------------------- the Python layer
def _parts(r):
    mods = [m for m in r.mlp_net.layers if isinstance(m, nn.Linear)]
    return [m.weight for m in mods], [m.bias for m in mods], [m.weight for m in r.out_layers], [m.bias for m in r.out_layers]


def test_python_refusals_on_the_cpu():
    from igs_amd import motion as M
    r = DR.make_renderer()
    ws, bs, hws, hbs = _parts(r)
    x = torch.randn(5, 20)
    call = lambda t, **kw: M.mlp_heads(t, ws, bs, hws, hbs, **kw)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.decode_residual_feature(r, x)
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(NotImplementedError, match="float32 or float16"):
                call(x.to(dt))
        with pytest.raises(NotImplementedError, match="share a dtype"):
            call(x.half())
        with pytest.raises(NotImplementedError, match="share a dtype"):
            M.mlp_heads(x, ws, bs, [w.half() for w in hws], hbs)
        with pytest.raises(NotImplementedError, match="activation"):
            call(x, activation="gelu")
        with pytest.raises(NotImplementedError, match="hidden Linears"):
            M.mlp_heads(x, [ws[0], ws[1], ws[1], ws[1]], [None] * 4, hws, hbs)
        with pytest.raises(NotImplementedError, match="heads"):
            M.mlp_heads(x, ws, bs, [hws[0]] * 9, [None] * 9)
        with pytest.raises(NotImplementedError, match="1..128"):
            M.mlp_heads(torch.randn(5, 129), [torch.randn(24, 129)], [None], [torch.randn(3, 24)], [None])
        with pytest.raises(NotImplementedError, match="1..128"):
            M.mlp_heads(x, ws, bs, [torch.randn(100, 24), torch.randn(29, 24)], [None, None])
        for bad in (lambda: call(x[0]), lambda: call(x[None]), lambda: call(torch.randn(5, 21)), lambda: M.mlp_heads(x, ws, bs[:2], hws, hbs),
                    lambda: M.mlp_heads(x, ws, bs, hws, [hbs[0]]), lambda: M.mlp_heads(x, [ws[0], ws[0]], [None, None], hws, hbs),
                    lambda: M.mlp_heads(x, ws, bs, [torch.randn(3, 25)], [None]), lambda: M.mlp_heads(x, ws, [bs[0][:5], None, None], hws, hbs),
                    lambda: M.mlp_heads(x, ws, bs, [torch.randn(3)], [None]), lambda: call(x, act_after=[1, 1])):
            with pytest.raises(ValueError):
                bad()
    for t in (x.clone().requires_grad_(True), x):                                                # grad enabled: x, or only the parameters, require it
        with pytest.raises(NotImplementedError, match="forward only"):
            call(t)
    with pytest.raises(NotImplementedError, match="forward only"):
        M.decode_residual_feature(r, x)


def test_use_native_decoder_binds_the_instance_and_keeps_the_state_dict():
    from igs_amd import motion as M
    r = DR.make_renderer()
    keys, classes = list(r.state_dict().keys()), [type(m) for m in r.modules()]
    assert "decode_residual_feature" not in vars(r)
    assert M.use_native_decoder(r) == 5
    assert "decode_residual_feature" in vars(r) and type(r).decode_residual_feature is not vars(r)["decode_residual_feature"]
    assert list(r.state_dict().keys()) == keys and [type(m) for m in r.modules()] == classes
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):                  # the bound method runs the native path: no fallback
        r.decode_residual_feature(torch.randn(4, 20))
    assert M.use_native_decoder(DR.make_renderer(mlp=False)) == 2                                # cfg.mlp_network_config is None: the heads alone
    assert M.use_native_decoder(DR.make_renderer(n_hidden_layers=1, activation="relu", feature_channels={"a": 5}, bias=False)) == 3


def _break(r, what):
    L = r.mlp_net.layers
    if what == "gelu":
        L[1] = nn.GELU()
    elif what == "two linears":
        L[1] = nn.Linear(24, 24)
    elif what == "starts with an activation":
        r.mlp_net.layers = nn.Sequential(nn.SiLU(), *L)
    elif what == "layer norm":
        r.mlp_net.layers = nn.Sequential(*L, nn.SiLU(), nn.LayerNorm(24))
    elif what == "mixed":
        L[3] = nn.ReLU()
    elif what == "output_activation":
        r.mlp_net.output_activation = lambda x: torch.exp(x)
    elif what == "sigmoid module":
        r.mlp_net.output_activation = nn.Sigmoid()
    elif what == "wide":
        L[0], L[2] = nn.Linear(20, 136), nn.Linear(136, 24)
    elif what == "wide heads":
        r.out_layers = nn.ModuleList([nn.Linear(24, 100), nn.Linear(24, 29)])
    elif what == "four linears":
        r.mlp_net.layers = nn.Sequential(*L, nn.SiLU(), nn.Linear(24, 24))
    elif what == "head count":
        r.out_layers.append(nn.Linear(24, 2))
    elif what == "conv head":
        r.out_layers[1] = nn.Conv1d(24, 4, 1)
    elif what == "head input":
        r.out_layers[1] = nn.Linear(20, 4)
    return r


@pytest.mark.parametrize("what", ["gelu", "two linears", "starts with an activation", "layer norm", "mixed", "output_activation", "sigmoid module",
                                  "wide", "wide heads", "four linears", "head count", "conv head", "head input"])
def test_use_native_decoder_refuses_before_any_binding(what):
    from igs_amd import motion as M
    r = _break(DR.make_renderer(), what)
    before = dict(vars(r))
    with pytest.raises(NotImplementedError):
        M.use_native_decoder(r)
    assert vars(r) == before and "decode_residual_feature" not in vars(r) and M.DECODER_CACHE not in vars(r)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        M.decode_residual_feature(r, torch.randn(4, 20))
    if what not in ("conv head", "head input", "head count"):
        with torch.no_grad():
            assert r.decode_residual_feature(torch.randn(4, 20))["xyz"].shape[0] == 4            # still the PyTorch module it was
