"""The backward of the fused projections (igs_amd/csrc/proj_bwd.hip, igs_amd/tokens.py) without a GPU: the written-out gradients of
tests/layer_head_grad_restatement.py against float64 autograd of the forward's restatement, the transposed pack against its independent
restatement, the exports, the refusals of the C ABI (every one happens before any HIP call, so addresses that are never read stand in for
device memory), the scratch size, the built kernels' resources, the binders with training=True, and the teeth of the allowance."""
import os
import re
import shutil
import sys

import pytest
import torch
import torch.nn as nn

import layer_head_grad_restatement as GR
import layer_head_restatement as LH
import token_ops_restatement as TR

F32, F16 = torch.float32, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("igs_token_proj_bwd_scratch_bytes", "igs_token_proj_bwd")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _grads(T, n, seed, none=()):
    g = torch.Generator().manual_seed(seed)
    return [None if j in none else torch.randn(T, 128, dtype=torch.float64, generator=g) for j in range(n)]


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n,T,rot,none", [(1, 1, None, ()), (3, 33, (0, 1, 32), ()), (5, 40, (0, 0, 0, 20, 20), (1,)), (2, 7, (6, 3), (0,)),
                                          (2, 5, None, (0, 1))])
def test_the_written_out_gradients_equal_float64_autograd_of_the_forward(n, T, rot, none):
    x = LH.project_inputs(T, n + T, "cpu").requires_grad_(True)
    ws = [w.requires_grad_(True) for w in LH.make_weights(n, T)]
    grads = _grads(T, n, 3 * T + n, none)
    out = LH.project_restate(x, ws, rot)
    total = sum((out[:, 128 * j: 128 * (j + 1)] * g).sum() for j, g in enumerate(grads) if g is not None)
    auto = torch.autograd.grad(total, [x] + ws, allow_unused=True) if len(none) < n else [None] * (n + 1)
    dx, dws = GR.project_grad_restate(x.detach(), [w.detach() for w in ws], grads, rot)
    assert GR.rel(dx, torch.zeros_like(dx) if auto[0] is None else auto[0]) <= 1e-12
    for j in range(n):
        assert (dws[j] is None) == (j in none), j
        if dws[j] is None:                                                                       # (an output without a gradient: autograd gives none, or zeros)
            assert auto[1 + j] is None or not auto[1 + j].any(), j
        else:
            assert GR.rel(dws[j], auto[1 + j]) <= 1e-12, j


# ---------------------------------------------------------------- the transposed pack
@pytest.mark.parametrize("dtype", [F32, F16])
def test_the_library_packs_the_transposes_as_the_restatement_does_bit_for_bit(dtype):
    from igs_amd import tokens as TK
    import layer_tail_restatement as LR
    ws = LH.make_weights(5, 2, F32)
    pack, pack_t = TK.pack_projections(ws, dtype, transposed=True)
    assert torch.equal(_bits(pack), _bits(TK.pack_projections(ws, dtype))), "the default return changed"
    assert pack_t.dtype == dtype and pack_t.is_contiguous() and pack_t.numel() == 5 * LH.MATRIX
    assert torch.equal(_bits(pack_t), _bits(GR.pack_transposed([w.to(dtype) for w in ws])))
    for j, w in enumerate(ws):
        assert torch.equal(_bits(LR.unpack_matrix(pack_t[j * LH.MATRIX: (j + 1) * LH.MATRIX], 128, 128)), _bits(w.to(dtype).t())), j


# ---------------------------------------------------------------- exports
def test_entry_points_are_exported_declared_and_built():
    from igs_amd import _cabi, build
    from igs_amd import tokens as TK
    L = _cabi.lib()
    header = open(build.HERE + "/../include/igs_rast.h").read()
    for name in NAMES:
        assert name in _cabi.SIGNATURES and hasattr(L, name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == len(_cabi.SIGNATURES[name][1]), name
    assert "proj_bwd.hip" in build.SOURCES and "proj.hip" in build.SOURCES
    assert "#define IGS_TOKEN_PROJ_BWD_MAX_SLICES %d\n" % GR.MAX_SLICES in header
    ext = _cabi.ext()
    for f in ("token_proj_bwd", "bwd_scratch_bytes", "token_proj_fwd", "pack_elems"):
        assert hasattr(ext._proj, f), f
    for fn in ("project_tokens_autograd", "pack_projections", "use_native_layer_heads", "use_native_feature_transformer"):
        assert callable(getattr(TK, fn)), fn
    for const, kind in ((TK.LAYER_HEAD_BWD_NATIVE, bool), (TK.LAYER_HEAD_BWD_MIN_OUTPUTS, int)):
        assert const.keys() == {F32, F16} and all(type(v) is kind for v in const.values())


# ---------------------------------------------------------------- the scratch
def test_scratch_bytes_are_monotone_constant_above_the_slice_cap_and_refuse_sizes_out_of_range():
    from igs_amd import _cabi
    L, ext = _cabi.lib(), _cabi.ext()
    cap_rows = GR.MIN_SLICE_ROWS * GR.MAX_SLICES
    for n in (1, 3, 5):
        sizes = [L.igs_token_proj_bwd_scratch_bytes(T, n) for T in (0, 1, 512, 513, 1024, 1025, cap_rows - 1, cap_rows, cap_rows + 1, 4 * cap_rows, 1 << 24)]
        assert sizes == [GR.scratch_bytes(T, n) for T in (0, 1, 512, 513, 1024, 1025, cap_rows - 1, cap_rows, cap_rows + 1, 4 * cap_rows, 1 << 24)]
        assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] == n * GR.DW_BYTES == sizes[2] < sizes[3]
        assert sizes[7] == sizes[8] == sizes[9] == sizes[10] == GR.MAX_SLICES * n * GR.DW_BYTES
        assert ext._proj.bwd_scratch_bytes(513, n) == sizes[3]
    for T, n in ((-1, 3), ((1 << 24) + 1, 3), (5, 0), (5, 6), (5, -1)):
        assert L.igs_token_proj_bwd_scratch_bytes(T, n) == -1 == ext._proj.bwd_scratch_bytes(T, n), (T, n)
    # above the cap the slices get longer, in whole trips, and never outnumber the room
    for T in (cap_rows + 1, 163840, 1 << 24):
        rows, count, room = GR.slice_plan(T)
        assert rows % 128 == 0 and rows >= GR.MIN_SLICE_ROWS and count <= room == GR.MAX_SLICES and rows * count >= T


# ---------------------------------------------------------------- the C ABI's refusals
# Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes.
FAKE = (0x1000000, 0x3000000, 0x7000000, 0x10000000, 0xB000000, 0xE000000)
REFUSED = GR.refusals(*FAKE)


def _show(x):
    if isinstance(x, tuple):
        return "(" + ",".join(_show(v) for v in x) + ")"
    return str(x) if not isinstance(x, int) or abs(x) < 1 << 20 else hex(x)


@pytest.mark.parametrize("kw,word", REFUSED, ids=lambda v: v if isinstance(v, str) else "-".join("%s=%s" % (k, _show(x)) for k, x in v.items()))
def test_the_c_abi_refuses_each_argument_for_its_own_reason_before_any_hip_call(kw, word):
    from igs_amd import _cabi
    assert GR.call_abi(_cabi.lib(), None, dict(GR.good_call(*FAKE), **kw)) == E_INVALID, kw
    assert word in _cabi.last_error() and "igs_token_proj_bwd" in _cabi.last_error(), (kw, word, _cabi.last_error())


def test_nothing_wanted_and_t_zero_return_zero_after_the_size_checks():
    from igs_amd import _cabi
    call = lambda **kw: GR.call_abi(_cabi.lib(), None, dict(GR.good_call(*FAKE), **kw))
    none = (None, None, None)
    assert call(dx=None, dW=none) == 0 and call(dx=None, dW=None) == 0                          # nothing wanted: returns before any launch
    assert call(dx=None, dW=None, x=None, wt=None, scr=None, g=None, gstr=None, rot=None) == 0
    assert call(T=0, dW=None) == 0 and call(T=0, dW=none, x=None, g=None, gstr=None, wt=None, scr=None, dx=None) == 0
    for kw, word in ((dict(n=6), "n out of range"), (dict(dxstr=100), "row stride"), (dict(gdt=3), "dtype"), (dict(rot=(0, 5, 0)), "rot"),
                     (dict(dW=(FAKE[5] + 4, None, None)), "16 bytes")):
        assert call(T=0, **dict(dict(dW=None), **kw)) == E_INVALID and word in _cabi.last_error(), kw
        assert call(dx=None, **dict(dict(dW=None), **kw)) == E_INVALID and word in _cabi.last_error(), kw
    src = open(os.path.join(ROOT, "igs_amd", "csrc", "proj_bwd.hip")).read()
    zero = src[src.index("if (T == 0) {"):]
    assert "hipMemsetAsync(wp[j], 0" in zero[: zero.index("return 0;")]


# ---------------------------------------------------------------- the built code objects
def test_backward_kernels_use_no_private_memory_and_fit_the_lds_as_the_forward_does():
    """The d x kernel and the weight-gradient kernel in two instances each (compute dtype), one reduce kernel: none with private memory or
    register spills; the d x kernel with the forward's LDS (128 KB float32: one workgroup per compute unit; 64 KB float16: two) and within
    the registers those occupancies leave a wave (512 / 256)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as AB
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = AB.code_objects(build.LIB)
    try:
        found = {}
        for co in cos:
            for name, md in kernel_metadata(co).items():
                if re.match(r"^_ZL?\d+token_proj_bwd_(dx|wgrad|reduce)_kernel", name):
                    found[name] = md
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    count = lambda kind: len([n for n in found if "token_proj_bwd_%s_kernel" % kind in n])
    assert (count("dx"), count("wgrad"), count("reduce")) == (2, 2, 1), sorted(found)
    for name, md in found.items():
        regs, lds = int(md[".vgpr_count"]), int(md[".group_segment_fixed_size"])                 # (the unified file: accumulator registers counted in)
        print(name, "vgpr", regs, "agpr", md.get(".agpr_count", 0), "lds", lds, "scalars parked in vector lanes", md.get(".sgpr_spill_count", 0))
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "private bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0, (name, "register spills to memory")
        if "_dx_" in name:
            half = "DF16_" in name
            assert lds == (64 if half else 128) * 1024 and regs <= (256 if half else 512), (name, lds, regs)
        else:
            assert lds == 0 and regs <= 512, name


# ---------------------------------------------------------------- the Python layer
def test_project_tokens_is_still_forward_only_and_the_autograd_form_refuses_what_it_refuses():
    from igs_amd import tokens as TK
    x, ws = torch.zeros(3, 128), LH.make_weights(2, 0, F32)
    with pytest.raises(NotImplementedError, match="forward only"):
        TK.project_tokens(x.clone().requires_grad_(True), ws)
    with pytest.raises(NotImplementedError, match="forward only"):
        TK.project_tokens(x, [ws[0], ws[1].clone().requires_grad_(True)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TK.project_tokens_autograd(x.clone().requires_grad_(True), ws)                          # ... which this one serves, on a GPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TK.project_tokens_autograd(x, ws)
    for bad in (torch.zeros(3, 64), torch.zeros(())):
        with pytest.raises(ValueError):
            TK.project_tokens_autograd(bad, ws)
    for bad_ws in ([], ws * 3, [torch.zeros(128, 64)], [torch.zeros(128)]):
        with pytest.raises(ValueError):
            TK.project_tokens_autograd(x, bad_ws)
    for rot in ((0,), (0, 3), (-1, 0)):
        with pytest.raises(ValueError, match="rot"):
            TK.project_tokens_autograd(x, ws, rot=rot)
    with pytest.raises(NotImplementedError, match="bias"):
        TK.project_tokens_autograd(x, [nn.Linear(128, 128)])
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError):
            TK.project_tokens_autograd(x.to(dt), ws)
        with pytest.raises(NotImplementedError):
            TK.project_tokens_autograd(x, [w.to(dt) for w in ws])
        with pytest.raises(NotImplementedError):
            TK.project_tokens_autograd(x, ws, compute_dtype=dt)
    pack, pack_t = TK.pack_projections(ws, F32, transposed=True)
    half, half_t = TK.pack_projections(ws, F16, transposed=True)
    for kw in (dict(packed=half, packed_t=pack_t), dict(packed=pack, packed_t=half_t)):
        with pytest.raises(ValueError, match="packed holds"):
            TK.project_tokens_autograd(x, ws, compute_dtype=F32, **kw)
    for kw in (dict(packed=pack, packed_t=pack_t[:-1024]), dict(packed=TK.pack_projections(ws[:1], F32), packed_t=pack_t)):
        with pytest.raises(ValueError, match="packed holds"):
            TK.project_tokens_autograd(x, ws, compute_dtype=F32, **kw)


def test_the_training_binders_bind_and_refuse_before_anything_is_changed():
    from igs_amd import tokens as TK
    model = LH.make_transformer(True)
    before = [(m, m.__dict__.get("forward")) for m in model.modules()]
    model.layers[1].cross_attn_ffn.k_proj = nn.Linear(128, 128, bias=True)
    for bind in (lambda: TK.use_native_layer_heads(model, training=True), lambda: TK.use_native_feature_transformer(model, True, training=True)):
        with pytest.raises(NotImplementedError, match="bias"):
            bind()
    with pytest.raises(NotImplementedError, match="blocks"):
        TK.use_native_feature_transformer(model.layers[0], True, training=True)
    with pytest.raises(NotImplementedError):
        TK.use_native_layer_heads(TR.make_layer(d_model=64, no_ffn=True), training=True)
    assert all(m.__dict__.get("forward") is f for m, f in before), "a refused binder changed a forward"
    assert not any(TK.HEAD_CACHE in m.__dict__ or TK.FT_STATE in m.__dict__ for m in model.modules())
    for bidirectional in (True, False):
        good = LH.make_transformer(bidirectional)
        assert TK.use_native_feature_transformer(good, bidirectional, training=True) == 4
        assert good.forward.__func__ is TK._feature_forward and good.__dict__[TK.FT_STATE]["training"] is True
        assert all(m.forward.__func__ is TK._layer_head_forward_training for b in good.layers for m in b.children())
        assert set(good.state_dict()) == set(LH.make_transformer(bidirectional).state_dict())
        assert TK.use_native_feature_transformer(good, bidirectional) == 4 and good.__dict__[TK.FT_STATE]["training"] is False      # the default: today's
        assert all(m.forward.__func__ is TK._layer_head_forward for b in good.layers for m in b.children())


def test_the_cache_keeps_the_pack_and_the_transposed_pack_per_dtype_and_rebuilds_them_when_a_weight_changes():
    from igs_amd import tokens as TK
    layer = TR.make_layer(128, no_ffn=True, seed=1)
    ws = [layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight]
    pack = TK._head_pack(layer, "qkv", F32, ws)
    assert TK._head_pack(layer, "qkv", F32, ws) is pack and "pack_t" not in layer.__dict__[TK.HEAD_CACHE][("qkv", F32)]
    both = TK._head_pack(layer, "qkv", F32, ws, transposed=True)
    assert both[0] is pack and torch.equal(both[1], TK.pack_projections(ws, F32, transposed=True)[1])
    assert TK._head_pack(layer, "qkv", F32, ws, transposed=True)[1] is both[1]
    half = TK._head_pack(layer, "qkv", F16, ws, transposed=True)
    assert half[0].dtype == F16 and half[1].dtype == F16 and set(layer.__dict__[TK.HEAD_CACHE]) == {("qkv", F32), ("qkv", F16)}
    with torch.no_grad():
        layer.k_proj.weight.mul_(2.0)                                                            # an optimiser step: _version changes
    again = TK._head_pack(layer, "qkv", F32, ws, transposed=True)
    assert again[1] is not both[1] and torch.equal(again[1], TK.pack_projections(ws, F32, transposed=True)[1])
    assert torch.equal(again[0], TK.pack_projections(ws, F32))


# ---------------------------------------------------------------- the allowance
def test_the_allowance_has_teeth():
    """On the CPU: float32 F.linear under autograd passes the four-times rule against itself; the same gradients with one element moved by
    1e-3 of the largest, or with the roll left out, do not."""
    T, n, rot = 40, 3, (0, 1, 20)
    x, ws, grads = LH.project_inputs(T, 1, "cpu"), LH.make_weights(n, 1), _grads(T, n, 9)
    ref_dx, ref_dw = GR.project_grad_restate(x, ws, grads, rot)
    dx, dws = GR.linear_autograd(x, ws, grads, rot, F32, F32)
    GR.four_times("d x", dx, dx, ref_dx, F32)
    GR.four_times("d W_1", dws[1], dws[1], ref_dw[1], F32)
    bad = dx.clone()
    bad[17, 5] += 1e-3 * ref_dx.abs().max().float()
    with pytest.raises(AssertionError):
        GR.four_times("d x perturbed", bad, dx, ref_dx, F32)
    bad = dws[1].clone()
    bad[100, 3] += 1e-3 * ref_dw[1].abs().max().float()
    with pytest.raises(AssertionError):
        GR.four_times("d W_1 perturbed", bad, dws[1], ref_dw[1], F32)
    unrolled = GR.linear_autograd(x, ws, grads, None, F32, F32)
    with pytest.raises(AssertionError):
        GR.four_times("d x without the roll", unrolled[0], dx, ref_dx, F32)
    with pytest.raises(AssertionError):
        GR.four_times("an unwritten element", torch.full_like(dx, float("nan")), dx, ref_dx, F32)
