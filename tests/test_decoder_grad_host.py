"""The residual decoder's backward (igs_amd/csrc/mlp.hip, igs_amd/motion.py) without a GPU: exports and argument counts, the refusals of
igs_mlp_heads_bwd before any HIP call, the scratch size, the transposed pack, the float64 restatement of the gradients against
torch.autograd, the exact case builder's premise, the Python layer and the training binder on CPU stand-in modules, and the resources of
the built gfx950 kernels."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import decoder_grad_restatement as GR
import decoder_restatement as DR
from test_decoder_host import _break, _ints, _parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_mlp_heads_bwd_scratch_bytes", "igs_mlp_heads_bwd")
INVALID = -1
F32, F16 = 0, 1
SILU, RELU = 0, 1
CHUNK = 16384                        # MLP_BWD_CHUNK_ROWS


def test_exports_and_argument_counts():
    from igs_amd import _cabi
    from igs_amd import motion as M
    L = _cabi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "igs_rast.h")).read(), flags=re.S)
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m, n
        assert len(_cabi.SIGNATURES[n][1]) == len(m.group(1).split(",")), n
    ext = _cabi.ext()
    for f in ("mlp_heads_bwd", "bwd_scratch_bytes"):
        assert hasattr(ext._mlp, f), f
    for fn in ("mlp_heads_autograd", "decode_residual_feature_train", "use_native_decoder", "pack_mlp"):
        assert callable(getattr(M, fn)), fn


X, WP, WT, BP, G0, G1, SC, DX, DW, DB = (0x10000000 * k for k in range(1, 11))
SHIPPED = dict(widths=(128, 128, 128, 128), heads=(3, 4))


def _scratch(L, N, dtype=F32, widths=SHIPPED["widths"], heads=SHIPPED["heads"]):
    return L.igs_mlp_heads_bwd_scratch_bytes(N, dtype, len(widths) - 1, _ints(widths), len(heads), _ints(heads))


def _bwd(L, N=1000, dtype=F32, act=SILU, widths=SHIPPED["widths"], act_after=(1, 1, 0), heads=SHIPPED["heads"], x=X, rs=None, wp=WP, wt=WT, bp=BP,
         douts=(G0, G1), sc=SC, sc_bytes=None, dx=DX, dw=DW, db=DB, n_hidden=None, n_heads=None):
    n_hidden = (len(widths) - 1 if widths is not None else 0) if n_hidden is None else n_hidden
    n_heads = (len(heads) if heads is not None else 0) if n_heads is None else n_heads
    g = None if douts is None else (ctypes.c_void_p * len(douts))(*douts)
    rs = (widths[0] if widths else 1) if rs is None else rs
    if sc_bytes is None:
        sc_bytes = max(_scratch(L, max(N, 0) if N <= (1 << 32) else 0), 0) if widths == SHIPPED["widths"] and heads == SHIPPED["heads"] else 1 << 40
    return L.igs_mlp_heads_bwd(None, N, dtype, act, n_hidden, _ints(widths), _ints(act_after), n_heads, _ints(heads), x, rs, wp, wt, bp, g, sc,
                               sc_bytes, dx, dw, db)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    L = _cabi.lib()
    cases = [(dict(N=-1), "N out of range"), (dict(N=(1 << 32) + 1), "N out of range"),
             (dict(widths=(0, 128, 128, 128)), "width"), (dict(widths=(128, 129, 128, 128)), "width"), (dict(widths=(256,), act_after=()), "width"),
             (dict(widths=(128,) * 5, act_after=(1,) * 4), "n_hidden"), (dict(n_hidden=-1), "n_hidden"),
             (dict(heads=(), douts=()), "n_heads"), (dict(heads=(1,) * 9, douts=(G0,) * 9), "n_heads"), (dict(n_heads=0), "n_heads"),
             (dict(heads=(3, 0)), "head width"), (dict(heads=(3, 129)), "head width"), (dict(heads=(64, 65)), "add up"),
             (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(act=2), "activation"), (dict(act=-1), "activation"),
             (dict(x=None), "NULL"), (dict(wp=None), "NULL"), (dict(wt=None), "NULL"), (dict(bp=None), "NULL"), (dict(douts=None), "NULL"),
             (dict(sc=None), "NULL"),
             (dict(widths=None, n_hidden=3), "NULL widths"), (dict(heads=None, n_heads=2), "NULL widths or head_widths"), (dict(act_after=None), "NULL act_after"),
             (dict(rs=127), "row stride"), (dict(rs=0), "row stride"), (dict(rs=-128), "row stride"), (dict(rs=(1 << 31) + 4), "row stride"),
             (dict(x=X + 2), "aligned to its element size"), (dict(dtype=F16, x=X + 1), "aligned"), (dict(douts=(G0 + 2, G1)), "aligned"),
             (dict(dtype=F16, douts=(G0, G1 + 1)), "aligned"), (dict(dx=DX + 2), "aligned"), (dict(dw=DW + 2), "aligned"), (dict(db=DB + 1), "aligned"),
             (dict(bp=BP + 2), "aligned"), (dict(wp=WP + 8), "16 bytes"), (dict(wt=WT + 8), "16 bytes"), (dict(sc=SC + 8), "16 bytes"),
             (dict(sc_bytes=0), "scratch is smaller"), (dict(sc_bytes=_scratch(L, 1000) - 1), "scratch is smaller"),
             (dict(N=5 * CHUNK, sc_bytes=_scratch(L, CHUNK) - 1), "scratch is smaller")]
    for kw, word in cases:
        assert _bwd(L, **kw) == INVALID, kw
        assert word in _cabi.last_error() and "igs_mlp_heads_bwd" in _cabi.last_error(), (kw, _cabi.last_error())
    # nothing wanted: every check still runs, nothing is launched
    assert _bwd(L, dx=None, dw=None, db=None) == 0 and _bwd(L, dx=None, dw=None, db=None, douts=(None, None)) == 0
    assert _bwd(L, dx=None, dw=None, db=None, sc_bytes=5) == INVALID
    # N = 0 with no gradient given: nothing to do at all
    assert _bwd(L, N=0, dx=None, dw=None, db=None) == 0 and _bwd(L, N=0, x=None, wp=None, wt=None, bp=None, douts=None, sc=None, dx=None, dw=None, db=None) == 0
    assert _bwd(L, N=0, widths=(129, 128, 128, 128), dw=None, db=None) == INVALID and _bwd(L, N=0, act=5, dw=None, db=None) == INVALID
    assert _bwd(L, N=0, dw=DW + 1, db=None) == INVALID


def test_scratch_bytes_stop_growing_above_the_chunk():
    from igs_amd import _cabi
    L = _cabi.lib()
    sizes = [_scratch(L, n) for n in (0, 1, 255, 256, 257, 1000, CHUNK - 1, CHUNK, CHUNK + 1, 70001, 200000, 1 << 32)]
    assert sizes[0] == 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0
    assert sizes[6] < sizes[7] == sizes[8] == sizes[9] == sizes[10] == sizes[11]
    tw, tb = 3 * 128 * 128 + 7 * 128, 3 * 128 + 7
    assert sizes[7] == 4 * (8 * CHUNK * 128 + 64 * ((tw + tb + 3) // 4 * 4))                  # 8 slots of the chunk and 64 slices' partials
    assert sizes[5] == 4 * (8 * 1000 * 128 + 4 * ((tw + tb + 3) // 4 * 4))
    assert _scratch(L, 1000, dtype=F16) == sizes[5]                                             # float32 scratch whatever the dtype
    small = _scratch(L, CHUNK, widths=(33,), heads=(7,))
    assert small == 4 * (2 * CHUNK * 128 + 64 * ((33 * 7 + 7 + 3) // 4 * 4))
    for bad in (dict(N=-1), dict(N=(1 << 32) + 1), dict(N=5, dtype=2), dict(N=5, widths=(128, 129)), dict(N=5, widths=(128,) * 5),
                dict(N=5, heads=(64, 65)), dict(N=5, heads=()), dict(N=5, heads=(0,))):
        assert _scratch(L, **bad) == -1, bad
    assert L.igs_mlp_heads_bwd_scratch_bytes(5, F32, 0, None, 1, _ints((7,))) == -1


# ---------------------------------------------------------------- the transposed pack
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_transposed_pack_equals_the_restated_layout_of_the_transpose(half):
    from igs_amd.motion import pack_mlp
    dt = torch.float16 if half else torch.float32
    mk = lambda O, I, k: ((torch.arange(O * I).reshape(O, I) * 7 + 3 + k) % 2039 - 1000).to(dt)          # asymmetric, exact in half
    ws, bs = [mk(40, 70, 0), mk(128, 40, 1)], [None, torch.arange(128).to(dt)]
    hws, hbs = [mk(3, 128, 2), mk(4, 128, 3)], [torch.arange(3).to(dt), None]
    two = pack_mlp(ws, bs, hws, hbs)
    three = pack_mlp(ws, bs, hws, hbs, transposed=True)
    assert len(two) == 2 and len(three) == 3
    assert torch.equal(two[0], three[0]) and torch.equal(two[1], three[1])                              # the default keeps the current tuple
    want = np.concatenate([DR.pack_tile_order(w.numpy().T, half) for w in ws + [torch.cat(hws, 0)]])
    assert three[2].dtype == dt and three[2].is_contiguous() and three[2].shape == three[0].shape
    assert np.array_equal(three[2].numpy(), want)
    assert not np.array_equal(three[2].numpy(), three[0].numpy())
    cast = pack_mlp([w.float() for w in ws], bs, [w.float() for w in hws], hbs, transposed=True, dtype=dt)
    assert all(torch.equal(a, b) for a, b in zip(cast, three))


# ---------------------------------------------------------------- the restatement
def _torch_grads(r, x, douts):
    x = x.clone().requires_grad_(True)
    outs = list(r.decode_residual_feature(x).values())
    loss = sum((o * g).sum() for o, g in zip(outs, douts) if g is not None)
    loss.backward()
    lin = [m for m in r.mlp_net.layers if isinstance(m, torch.nn.Linear)]
    return dict(dx=x.grad, dw=[m.weight.grad for m in lin], db=[m.bias.grad for m in lin], dhw=[m.weight.grad for m in r.out_layers],
                dhb=[m.bias.grad for m in r.out_layers])


@pytest.mark.parametrize("activation", ["silu", "relu"])
def test_restated_gradients_equal_float64_autograd(activation):
    r = DR.make_renderer(dim_in=20, n_neurons=24, dim_out=24, n_hidden_layers=2, activation=activation, seed=2).double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 20, dtype=torch.float64, generator=g)
    douts = [torch.randn(37, 3, dtype=torch.float64, generator=g), torch.randn(37, 4, dtype=torch.float64, generator=g)]
    want = _torch_grads(r, x, douts)
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    assert aa == [1, 1, 0]
    got, bound = GR.gradients_with_bound(x.numpy(), ws, bs, hws, hbs, [d.numpy() for d in douts], activation, aa)
    for (name, a), (_, b), (_, e) in zip(GR.flat(got), GR.flat(want), GR.flat(bound)):
        b = b.numpy()
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0), name
        assert e.shape == a.shape and (e >= 0).all() and e.max() < 1e-3, name
    # a head without an upstream gradient is a head with a zero one
    got0 = GR.gradients(x.numpy(), ws, bs, hws, hbs, [None, douts[1].numpy()], activation, aa)
    want0 = GR.gradients(x.numpy(), ws, bs, hws, hbs, [np.zeros((37, 3)), douts[1].numpy()], activation, aa)
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(GR.flat(got0), GR.flat(want0)))


def test_restated_silu_derivative_equals_autograd_at_large_values():
    from test_gpu_decoder import LARGE
    z = torch.tensor(LARGE + (0.0, -1.2784645, 1.0, -1.0, 20.0, -20.0), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.silu(z).sum().backward()
    got = GR.silu_grad(z.detach().numpy())
    assert np.isfinite(got).all() and np.abs(got - z.grad.numpy()).max() <= 1e-15
    assert np.abs(got).max() <= 1.1 and np.array_equal(GR.act_grad(np.array([-1.0, 0.0, 2.0]), "relu"), [0.0, 0.0, 1.0])


EXACT_HOST = [((128, [128], (3, 4), 129), 0.05), ((33, [24, 24], (3, 4, 48, 1, 3), 129), 0.05), ((33, [128, 128, 128], (128,), 129), 0.05),
              ((128, [128, 128, 128], (3, 4), 257), 0.05), ((100, [128, 24, 64], (7,), 65), 0.05), ((128, [], (3, 4), 97), 0.05)]


@pytest.mark.parametrize("cfg,density", EXACT_HOST, ids=lambda v: str(v).replace(" ", ""))
def test_exact_grad_case_holds_its_premise(cfg, density):
    C0, hidden, heads, N = cfg
    case = GR.exact_grad_case(C0, hidden, heads, N, density=density, seed=len(hidden) + C0)
    print("exact_grad_case %s: largest sum of |a| |b| %d" % (cfg, case["worst"]))
    assert case["worst"] < 2 ** 11 and all(set(np.unique(d)) <= {-1.0, 0.0, 1.0} for d in case["douts"])
    with pytest.raises(AssertionError, match="is zero"):
        GR.exact_grad_case(C0, hidden or [16], heads, N, density=0.0, seed=1)


# ---------------------------------------------------------------- the Python layer
def test_python_layer_on_the_cpu():
    from igs_amd import motion as M
    r = DR.make_renderer()
    ws, bs, hws, hbs = _parts(r)
    x = torch.randn(5, 20)
    call = lambda t, **kw: M.mlp_heads_autograd(t, ws, bs, hws, hbs, **kw)
    for t in (x.clone().requires_grad_(True), x):                                                # requiring grad is no refusal here
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(t)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        call(x)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError, match="float32 or float16"):
            call(x.to(dt))
    with pytest.raises(NotImplementedError, match="share a dtype"):
        call(x.half())
    with pytest.raises(NotImplementedError, match="activation"):
        call(x, activation="gelu")
    with pytest.raises(NotImplementedError, match="hidden Linears"):
        M.mlp_heads_autograd(x, [ws[0], ws[1], ws[1], ws[1]], [None] * 4, hws, hbs)
    with pytest.raises(NotImplementedError, match="heads"):
        M.mlp_heads_autograd(x, ws, bs, [hws[0]] * 9, [None] * 9)
    with pytest.raises(NotImplementedError, match="1..128"):
        M.mlp_heads_autograd(x, ws, bs, [torch.randn(100, 24), torch.randn(29, 24)], [None, None])
    for bad in (lambda: call(x[0]), lambda: call(torch.randn(5, 21)), lambda: M.mlp_heads_autograd(x, ws, bs[:2], hws, hbs),
                lambda: M.mlp_heads_autograd(x, ws, bs, [torch.randn(3, 25)], [None]), lambda: call(x, act_after=[1, 1])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.decode_residual_feature_train(r, x)
    with pytest.raises(NotImplementedError, match="forward only"):                               # the forward-only names are as they were
        M.mlp_heads(x, ws, bs, hws, hbs)
    with pytest.raises(NotImplementedError, match="forward only"):
        M.decode_residual_feature(r, x)


def test_training_binder_binds_the_instance_and_keeps_the_state_dict():
    from igs_amd import motion as M
    r = DR.make_renderer()
    keys, classes = list(r.state_dict().keys()), [type(m) for m in r.modules()]
    assert M.use_native_decoder(r, training=True) == 5
    assert vars(r)["decode_residual_feature"].__func__ is M.decode_residual_feature_train
    assert list(r.state_dict().keys()) == keys and [type(m) for m in r.modules()] == classes
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                   # grad enabled: the training path, no fallback
        r.decode_residual_feature(torch.randn(4, 20))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        r.decode_residual_feature(torch.randn(4, 20))
    assert list(r.state_dict().keys()) == keys
    r2 = DR.make_renderer()
    assert M.use_native_decoder(r2) == 5 and vars(r2)["decode_residual_feature"].__func__ is M.decode_residual_feature
    with pytest.raises(NotImplementedError, match="forward only"):                               # without the keyword: as before
        r2.decode_residual_feature(torch.randn(4, 20))
    assert M.use_native_decoder(DR.make_renderer(mlp=False), training=True) == 2


@pytest.mark.parametrize("what", ["gelu", "two linears", "mixed", "output_activation", "wide", "four linears", "head count", "conv head"])
def test_training_binder_refuses_before_any_binding(what):
    from igs_amd import motion as M
    r = _break(DR.make_renderer(), what)
    before = dict(vars(r))
    with pytest.raises(NotImplementedError):
        M.use_native_decoder(r, training=True)
    assert vars(r) == before and "decode_residual_feature" not in vars(r) and M.DECODER_TRAIN_CACHE not in vars(r)
    with pytest.raises(NotImplementedError):
        M.decode_residual_feature_train(r, torch.randn(4, 20))
    assert M.DECODER_TRAIN_CACHE not in vars(r)


# ---------------------------------------------------------------- the built code objects
def test_backward_kernels_use_no_scratch_and_fit_the_lds():
    """the rows kernel in four instances (dtype, four-element or scalar loads of x), the wgrad kernel in two, one
    reduce kernel; none with private memory or register spills; the rows kernel within the 256 registers of two waves per SIMD and one
    Linear's 64 KB (float) or 32 KB (half) of LDS.  The forward's four instances are still four."""
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
                if re.match(r"^_ZL?\d+mlp_bwd_(rows|wgrad|reduce)_kernel", name):
                    found[name] = md
                if re.match(r"^_ZL?\d+mlp_heads_kernel", name):
                    fwd.append(name)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(fwd) == 4, sorted(fwd)
    count = lambda kind: len([n for n in found if "mlp_bwd_%s_kernel" % kind in n])
    assert (count("rows"), count("wgrad"), count("reduce")) == (4, 2, 1), sorted(found)
    for name, md in found.items():
        print(name, "vgpr", md[".vgpr_count"], "agpr", md.get(".agpr_count", 0), "lds", md[".group_segment_fixed_size"],
              "sgpr", md.get(".sgpr_count"), "scalars parked in vector lanes", md.get(".sgpr_spill_count", 0))
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0, (name, "register spills to memory")
        assert int(md[".vgpr_count"]) <= 256, name                                               # (the unified file: the accumulator registers are counted in)
        assert int(md[".group_segment_fixed_size"]) <= 160 * 1024, name
        if "rows" in name:
            half = "IDF16_" in name
            assert int(md[".group_segment_fixed_size"]) == (32768 if half else 65536) + 2048 + 1024 + 512, name
        else:
            assert int(md[".group_segment_fixed_size"]) == 0, name
