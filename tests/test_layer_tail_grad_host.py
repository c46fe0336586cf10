"""The backward of the fused layer tail (igs_amd/csrc/ffn_bwd.hip, igs_amd/tokens.py) without a GPU: the written-out gradients of
tests/layer_tail_grad_restatement.py against float64 autograd, the transposed pack against its independent restatement, the exports, the
refusals of the C ABI (every one happens before any HIP call, so addresses that are never read stand in for device memory), the scratch size,
the built kernels' resources, the binder with training=True, and the teeth of the allowance."""
import os
import re
import shutil
import sys

import pytest
import torch

import layer_tail_grad_restatement as GR
import layer_tail_restatement as LR

F32, F16 = torch.float32, torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _case(T, hidden, seed, zero_row=None):
    layer = LR.make_tail_layer(hidden or 64, no_ffn=not hidden, seed=seed)
    a, s = LR.tail_inputs(T, seed, "cpu")
    if zero_row is not None:
        a[zero_row] = 0.0                                                                        # a constant m: variance 0
    g = torch.randn(T, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 5))
    return a, s, g, LR.layer_weights(layer, torch.float64)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("T", [1, 33])
@pytest.mark.parametrize("hidden", [0, 32, 96])
def test_the_written_out_gradients_equal_float64_autograd(hidden, T):
    a, s, g, w = _case(T, hidden, seed=3 * T + hidden, zero_row=T - 1)
    mine, auto = GR.tail_grad_restate(a, s, g, *w), GR.tail_grad_autograd(a, s, g, *w)
    for name, x, y in zip(GR.NAMES, mine, auto):
        assert (x is None) == (y is None) == (not hidden and name in GR.NAMES[5:]), name
        if x is not None:
            assert x.shape == y.shape and GR.rel(x, y) <= 1e-12, (name, GR.rel(x, y))


def test_gelu_grad_is_finite_for_every_finite_z():
    z = torch.tensor([0.0, -0.0, 1e-30, 30.0, -30.0, 1e4, -1e4, 1e200, -1e200, 1.7e308, -1.7e308], dtype=torch.float64)
    d = GR.gelu_grad(z)
    assert torch.isfinite(d).all() and d[0] == 0.5 and d[5] == 1.0 and d[6] == 0.0


# ---------------------------------------------------------------- the transposed pack
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("hidden", [0, 32, 96, 1024])
def test_unpack_of_the_transposed_pack_is_the_transpose_and_the_library_packs_the_same(hidden, dtype):
    from igs_amd import tokens as TK
    layer = LR.make_tail_layer(hidden or 64, no_ffn=not hidden, seed=hidden + 1)
    Wm, _, W1, W2, _ = LR.layer_weights(layer, dtype)
    flat_t = GR.pack_tail_t(Wm, W1, W2)
    assert flat_t.numel() == LR.pack_elems(hidden, bool(hidden)) and flat_t.dtype == dtype
    for got, want in zip(GR.unpack_tail_t(flat_t, hidden), (Wm, W1, W2)):
        assert (got is None) == (want is None)
        if want is not None:
            assert torch.equal(_bits(got), _bits(want))
    pack, pack_t = TK.pack_layer_tail(layer, dtype, transposed=True)
    assert torch.equal(_bits(pack), _bits(TK.pack_layer_tail(layer, dtype))) and torch.equal(_bits(pack), _bits(LR.pack_tail(Wm, W1, W2)))
    assert pack_t.dtype == dtype and pack_t.is_contiguous() and torch.equal(_bits(pack_t), _bits(flat_t))
    if hidden:
        # the 12 tiles of hidden units 32 j .. 32 j + 31 are two contiguous pieces at the forward pack's offsets
        j = hidden // 32 - 1
        w1t = flat_t[16 * LR.TILE:][j * 8 * LR.TILE: (j + 1) * 8 * LR.TILE]
        w2t = flat_t[(16 + hidden // 32 * 8) * LR.TILE:][j * 4 * LR.TILE: (j + 1) * 4 * LR.TILE]
        assert torch.equal(LR.unpack_matrix(w1t, 256, 32, True), W1[32 * j:].t()) and torch.equal(LR.unpack_matrix(w2t, 32, 128), W2[:, 32 * j:].t())


# ---------------------------------------------------------------- exports
NAMES = ("igs_layer_tail_bwd_scratch_bytes", "igs_layer_tail_bwd")


def test_entry_points_are_exported_declared_and_built():
    from igs_amd import _cabi, build
    from igs_amd import tokens as TK
    L = _cabi.lib()
    header = open(build.HERE + "/../include/igs_rast.h").read()
    for n in NAMES:
        assert n in _cabi.SIGNATURES and hasattr(L, n), n
        decl = re.search(r"\b%s\(([^;]*)\);" % n, header)
        assert decl and len(decl.group(1).split(",")) == len(_cabi.SIGNATURES[n][1]), n
    assert "ffn_bwd.hip" in build.SOURCES and "ffn.hip" in build.SOURCES
    assert "#define IGS_LAYER_TAIL_BWD_CHUNK_ROWS %d\n" % GR.CHUNK_ROWS in header
    ext = _cabi.ext()
    for f in ("layer_tail_bwd", "bwd_scratch_bytes", "layer_tail_fwd", "pack_elems"):
        assert hasattr(ext._ffn, f), f
    for fn in ("layer_tail_autograd", "pack_layer_tail", "use_native_layer_tails"):
        assert callable(getattr(TK, fn)), fn
    assert TK.LAYER_TAIL_BWD_NATIVE.keys() == {F32, F16} and all(isinstance(v, bool) for v in TK.LAYER_TAIL_BWD_NATIVE.values())


# ---------------------------------------------------------------- the scratch
def test_scratch_bytes_do_not_grow_above_one_chunk_and_refuse_sizes_out_of_range():
    from igs_amd import _cabi
    L, R = _cabi.lib(), GR.CHUNK_ROWS
    for hidden in (0, 32, 1024, 2048):
        one = L.igs_layer_tail_bwd_scratch_bytes(R, 0, int(hidden > 0), hidden)
        assert one == L.igs_layer_tail_bwd_scratch_bytes(4 * R, 0, int(hidden > 0), hidden) == GR.scratch_bytes(R, hidden) > 0
        assert one == L.igs_layer_tail_bwd_scratch_bytes(R, 1, int(hidden > 0), hidden) == _cabi.ext()._ffn.bwd_scratch_bytes(R, True, hidden)
        assert L.igs_layer_tail_bwd_scratch_bytes(129, 0, int(hidden > 0), hidden) == GR.scratch_bytes(129, hidden) < one
    assert L.igs_layer_tail_bwd_scratch_bytes(0, 0, 1, 64) == 0
    # what this backward exists for: at [32768, 128], hidden 1024, below half of the 2560 float32 values per row the unfused tail keeps
    assert L.igs_layer_tail_bwd_scratch_bytes(32768, 0, 1, 1024) < 32768 * 2560 * 4 // 2
    for T, cdt, ffn, hidden in ((-1, 0, 1, 64), ((1 << 24) + 1, 0, 1, 64), (5, 2, 1, 64), (5, -1, 0, 0), (5, 0, 1, 48), (5, 0, 1, 0), (5, 0, 1, 2080)):
        assert L.igs_layer_tail_bwd_scratch_bytes(T, cdt, ffn, hidden) == -1, (T, cdt, ffn, hidden)
    assert L.igs_layer_tail_bwd_scratch_bytes(5, 0, 0, 48) == GR.scratch_bytes(5, 0)              # hidden is not read without FFN


# ---------------------------------------------------------------- the C ABI's refusals
# Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes.  Every
# operand has an address of its own with spans that do not meet, so GOOD passes every argument check and each case differs from it in the
# one thing that its reason word names.  (GOOD itself would launch, so it is never sent.)
A, S, G, WP, WT, SCR, DA, DS = 0x1000000, 0x3000000, 0x5000000, 0x7000000, 0x7800000, 0x10000000, 0xB000000, 0xD000000
L1W, L1B, L2W, L2B = 0x9000000, 0x9100000, 0x9200000, 0x9300000
PG = dict(dWm=0xE000000, dl1w=0xE100000, dl1b=0xE200000, dW1=0xE300000, dW2=0xE400000, dl2w=0xE500000, dl2b=0xE600000)
GOOD = dict(T=5, cdt=0, has_ffn=1, hidden=64, a=A, adt=0, astr=128, s=S, sdt=0, sstr=128, g=G, gdt=0, gstr=128, w=WP, wt=WT, l1w=L1W, l1b=L1B,
            eps1=1e-5, l2w=L2W, l2b=L2B, eps2=1e-5, scr=SCR, sbytes=1 << 30, da=DA, dadt=0, dastr=128, ds=DS, dsdt=0, dsstr=128, **PG)
ORDER = ("T", "cdt", "has_ffn", "hidden", "a", "adt", "astr", "s", "sdt", "sstr", "g", "gdt", "gstr", "w", "wt", "l1w", "l1b", "eps1", "l2w", "l2b",
         "eps2", "scr", "sbytes", "da", "dadt", "dastr", "ds", "dsdt", "dsstr", "dWm", "dl1w", "dl1b", "dW1", "dW2", "dl2w", "dl2b")


def _call(**kw):
    from igs_amd import _cabi
    k = dict(GOOD, **kw)
    return _cabi.lib().igs_layer_tail_bwd(None, *[k[n] for n in ORDER])


NEED = GR.scratch_bytes(5, 64)
REFUSED = ([(dict(hidden=h), "hidden") for h in (0, 48, 2080, -32)]
           + [(dict(T=-1), "T out of range"), (dict(T=(1 << 24) + 1), "T out of range")]
           + [(dict([(k, v)]), "row stride") for k in ("astr", "sstr", "gstr", "dastr", "dsstr") for v in (127, 0, -128, (1 << 31) + 4)]
           + [(dict([(k, None)]), "NULL") for k in ("a", "s", "g", "w", "wt", "l1w", "l1b", "l2w", "l2b", "scr")]
           + [(dict(has_ffn=0, a=None), "NULL"), (dict(has_ffn=0, g=None), "NULL"), (dict(has_ffn=0, wt=None), "NULL")]
           + [(dict([(k, v)]), "dtype") for k in ("cdt", "adt", "sdt", "gdt", "dadt", "dsdt") for v in (-1, 2)]
           + [(dict(eps1=-1.0), "eps"), (dict(eps1=float("inf")), "eps"), (dict(eps2=float("nan")), "eps")]
           + [(dict([(k, GOOD[k] + 2)]), "aligned to its element size") for k in ("a", "s", "g", "da", "ds", "l1w", "l2b")]
           + [(dict([(d, 1), (k, GOOD[k] + 1)]), "aligned to its element size") for d, k in (("gdt", "g"), ("dadt", "da"), ("dsdt", "ds"))]
           + [(dict(w=WP + 4), "16 bytes"), (dict(wt=WT + 8), "16 bytes"), (dict(cdt=1, wt=WT + 2), "16 bytes"), (dict(scr=SCR + 8), "scratch must be aligned")]
           + [(dict([(k, PG[k] + 2)]), "aligned to 4 bytes") for k in PG]
           + [(dict(sbytes=NEED - 1), "scratch is smaller"), (dict(sbytes=0), "scratch is smaller"), (dict(T=GR.CHUNK_ROWS, sbytes=NEED), "scratch is smaller")]
           # da / ds over an input: the same rows, the last element of the last row, rows between rows at a wider stride, another dtype
           + [(dict(da=A), "da overlaps"), (dict(da=G + (4 * 128 + 127) * 4), "da overlaps"), (dict(astr=256, da=A + 128 * 4, dastr=256), "da overlaps"),
              (dict(da=S), "da overlaps"), (dict(ds=G), "ds overlaps"), (dict(sdt=1, ds=S + 4 * 128 * 2), "ds overlaps"), (dict(a=DS + 16), "ds overlaps")])


@pytest.mark.parametrize("kw,word", REFUSED, ids=lambda v: v if isinstance(v, str) else "-".join(
    "%s=%s" % (k, x if x is None or isinstance(x, float) or abs(x) < 1 << 20 else hex(x)) for k, x in v.items()))
def test_the_c_abi_refuses_each_argument_for_its_own_reason_before_any_hip_call(kw, word):
    from igs_amd import _cabi
    assert _call(**kw) == E_INVALID, kw
    assert word in _cabi.last_error() and "igs_layer_tail_bwd" in _cabi.last_error(), (kw, word, _cabi.last_error())


def test_scratch_of_exactly_the_needed_size_and_all_outputs_null_pass_the_checks_and_launch_nothing():
    none = {k: None for k in PG}
    assert _call(sbytes=NEED, da=None, ds=None, **none) == 0                                     # nothing wanted: returns before any launch
    assert _call(has_ffn=0, s=None, sbytes=GR.scratch_bytes(5, 0), da=None, ds=None, **none) == 0    # s is not read without FFN


def test_t_zero_checks_the_sizes_and_zero_fills_the_parameter_gradients():
    """T == 0 with no parameter gradient makes no HIP call at all; with them it zero-fills (on the GPU: tests/test_gpu_layer_tail_grad.py)."""
    from igs_amd import _cabi
    none = {k: None for k in PG}
    assert _call(T=0, **none) == 0 and _call(T=0, a=None, g=None, w=None, scr=None, da=None, ds=None, **none) == 0
    for kw, word in ((dict(hidden=48), "hidden"), (dict(dsstr=100), "row stride"), (dict(gdt=3), "dtype"), (dict(eps1=-1.0), "eps"),
                     (dict(dW1=PG["dW1"] + 1), "aligned to 4 bytes")):
        assert _call(T=0, **dict(none, **kw)) == E_INVALID and word in _cabi.last_error(), kw
    src = open(os.path.join(ROOT, "igs_amd", "csrc", "ffn_bwd.hip")).read()
    zero = src[src.index("if (T == 0) {"):]
    assert "hipMemsetAsync(outs[i], 0" in zero[: zero.index("return 0;")]


# ---------------------------------------------------------------- the built code objects
def test_backward_kernels_use_no_private_memory_and_fit_the_lds():
    """The rows kernel in four instances (compute dtype x FFN), the wgrad kernel in two, one reduce kernel: none with private memory or
    register spills; the rows kernel within the 512 registers of one wave per SIMD and 160 KB of LDS.  The forward's four are still four."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from igs_amd import build
    build.build()
    import audit_barriers as AB
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = AB.code_objects(build.LIB)
    try:
        found, fwd = {}, []
        for co in cos:
            for name, md in kernel_metadata(co).items():
                if re.match(r"^_ZL?\d+layer_tail_bwd_(rows|wgrad|reduce)_kernel", name):
                    found[name] = md
                if re.match(r"^_ZL?\d+layer_tail_kernel", name):
                    fwd.append(name)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert len(fwd) == 4, sorted(fwd)
    count = lambda kind: len([n for n in found if "layer_tail_bwd_%s_kernel" % kind in n])
    assert (count("rows"), count("wgrad"), count("reduce")) == (4, 2, 1), sorted(found)
    for name, md in found.items():
        regs = int(md[".vgpr_count"])                                                            # (the unified file: the accumulator registers are counted in)
        print(name, "vgpr", md[".vgpr_count"], "agpr", md.get(".agpr_count", 0), "lds", md[".group_segment_fixed_size"],
              "scalars parked in vector lanes", md.get(".sgpr_spill_count", 0))
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "private bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0, (name, "register spills to memory")
        assert regs <= 512 and int(md[".group_segment_fixed_size"]) <= 160 * 1024, name


# ---------------------------------------------------------------- the Python layer
def test_layer_tail_is_still_forward_only_and_the_autograd_form_refuses_what_it_refuses():
    from igs_amd import tokens as TK
    layer = LR.make_tail_layer(64, seed=4)
    x = torch.zeros(3, 128)
    with pytest.raises(NotImplementedError, match="forward only"):
        TK.layer_tail(x.clone().requires_grad_(True), x, layer)
    with pytest.raises(NotImplementedError, match="forward only"):
        TK.layer_tail(x, x, layer)                                                               # the parameters require grad
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TK.layer_tail_autograd(x.clone().requires_grad_(True), x, layer)                          # ... which this one serves, on a GPU
    for a, s in ((x[:, :64], x[:, :64]), (x, x[:2])):
        with pytest.raises(ValueError):
            TK.layer_tail_autograd(a, s, layer)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError):
            TK.layer_tail_autograd(x.to(dt), x, layer)
        with pytest.raises(NotImplementedError):
            TK.layer_tail_autograd(x, x, layer, compute_dtype=dt)
    pack, pack_t = TK.pack_layer_tail(layer, F16, transposed=True)
    with pytest.raises(ValueError, match="packed holds"):
        TK.layer_tail_autograd(x, x, layer, packed=pack, packed_t=pack_t, compute_dtype=F32)
    with pytest.raises(ValueError, match="packed holds"):
        TK.layer_tail_autograd(x, x, layer, packed=TK.pack_layer_tail(layer, F32), packed_t=pack_t, compute_dtype=F32)
    import test_layer_tail_host as H
    for name in ("merge with a bias", "tanh gelu", "hidden 48", "d_model 64", "bfloat16"):
        with pytest.raises(NotImplementedError):
            TK.layer_tail_autograd(x, x, H.BAD_LAYERS[name]())


def test_the_training_binder_binds_refuses_before_anything_is_changed_and_caches_both_packs_per_dtype():
    from igs_amd import tokens as TK
    import test_layer_tail_host as H
    pair = H.Pair(LR.make_tail_layer(no_ffn=True, seed=2))
    keys = list(pair.state_dict().keys())
    assert TK.use_native_layer_tails(pair, training=True) == 2
    assert all(m.forward.__func__ is TK._layer_tail_forward_training and m.forward.__self__ is m for m in (pair.good, pair.other))
    assert list(pair.state_dict().keys()) == keys
    assert TK.use_native_layer_tails(pair) == 2 and TK.use_native_layer_tails(pair, training=False) == 2          # the parent's behaviour
    assert all(m.forward.__func__ is TK._layer_tail_forward for m in (pair.good, pair.other))
    bad = H.Pair(H.BAD_LAYERS["mlp[0] with a bias"]())
    before = [m.forward for m in bad.modules()]
    with pytest.raises(NotImplementedError):
        TK.use_native_layer_tails(bad, training=True)
    assert [m.forward for m in bad.modules()] == before and not any("forward" in m.__dict__ or TK.TAIL_CACHE in m.__dict__ for m in bad.modules())
    # the cache: one entry per compute dtype, the transposed pack added when a gradient is wanted, both rebuilt after a parameter changed
    layer = pair.good
    params = TK._tail_params(layer)
    for dt in (F32, F16):
        e = TK._tail_entry(layer, dt, params, False)
        assert "pack_t" not in e and torch.equal(_bits(e["pack"]), _bits(TK.pack_layer_tail(layer, dt)))
        e2 = TK._tail_entry(layer, dt, params, True)
        assert e2 is e and torch.equal(_bits(e["pack_t"]), _bits(TK.pack_layer_tail(layer, dt, transposed=True)[1]))
    assert set(layer.__dict__[TK.TAIL_CACHE]) == {F32, F16}
    with torch.no_grad():
        layer.mlp[0].weight.mul_(2.0)                                                            # what an optimiser step does: _version moves
    e3 = TK._tail_entry(layer, F32, params, True)
    assert e3 is not e and torch.equal(_bits(e3["pack_t"]), _bits(TK.pack_layer_tail(layer, F32, transposed=True)[1]))
    assert torch.equal(_bits(e3["pack"]), _bits(TK.pack_layer_tail(layer, F32)))


# ---------------------------------------------------------------- the allowance has teeth
def test_the_allowance_rejects_a_dropped_row_and_swapped_gelu_grad_channels():
    """Against the floors of the four-times rule (the least the allowance can be with a comparator as good as float32 / float16 allow, 4 x
    1e-4 taken as a generous comparator error in float16): a reference whose weight gradients miss the last of 129 rows, and one whose GELU'
    has two hidden channels swapped, lie outside."""
    a, s, g, w = _case(129, 96, seed=9)
    ref = GR.tail_grad_restate(a, s, g, *w)
    worst = max(GR.allowed(1e-4, F16), GR.allowed(1e-7, F32))
    dropped = GR.tail_grad_restate(a, s, g, *w, wgrad_rows=slice(0, 128))
    for i in (2, 3, 4, 5, 6, 7, 8):
        assert GR.rel(dropped[i], ref[i]) > worst, (GR.NAMES[i], GR.rel(dropped[i], ref[i]))
    for i in (0, 1):
        assert torch.equal(dropped[i], ref[i])

    def swapped(z):
        d = GR.gelu_grad(z)
        d[:, [5, 70]] = d[:, [70, 5]]
        return d
    wrong = GR.tail_grad_restate(a, s, g, *w, gelu_grad_fn=swapped)
    for i in (0, 1, 2, 3, 4, 5):                                                                 # everything behind dz
        assert GR.rel(wrong[i], ref[i]) > worst, (GR.NAMES[i], GR.rel(wrong[i], ref[i]))
