"""The fused layer tail (igs_amd/csrc/ffn.hip, igs_amd/tokens.py) without a GPU: the pack layout against its independent restatement, the
exports and argument counts, the refusals of the C ABI (every one of them happens before any HIP call, so host pointers that are never read
stand in for device memory) and the refusals of pack_layer_tail, layer_tail and use_native_layer_tails, which change nothing when they
refuse."""
import re

import pytest
import torch
import torch.nn as nn

import layer_tail_restatement as LR
import token_ops_restatement as TR

F32, F16 = torch.float32, torch.float16
NAMES = ("igs_layer_tail_pack_elems", "igs_layer_tail_fwd")
E_INVALID = -1


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ---------------------------------------------------------------- the pack
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("hidden", [32, 96, 1024])
def test_unpack_of_pack_is_the_matrix_bit_for_bit_and_the_library_packs_the_same(hidden, dtype):
    from igs_amd import tokens as TK
    layer = LR.make_tail_layer(hidden, seed=hidden)
    Wm, _, W1, W2, _ = LR.layer_weights(layer, dtype)
    flat = LR.pack_tail(Wm, W1, W2)
    assert flat.numel() == LR.pack_elems(hidden) and flat.dtype == dtype
    for got, want in zip(LR.unpack_tail(flat, hidden), (Wm, W1, W2)):
        assert torch.equal(_bits(got), _bits(want))
    mine = TK.pack_layer_tail(layer, dtype)
    assert mine.dtype == dtype and mine.is_contiguous() and torch.equal(_bits(mine), _bits(flat))
    # the 12 tiles of hidden units 32 j .. 32 j + 31 are two contiguous pieces: W1's rows and W2's columns of that range
    j = hidden // 32 - 1
    w1 = flat[16 * LR.TILE:][j * 8 * LR.TILE: (j + 1) * 8 * LR.TILE]
    w2 = flat[(16 + hidden // 32 * 8) * LR.TILE:][j * 4 * LR.TILE: (j + 1) * 4 * LR.TILE]
    assert torch.equal(LR.unpack_matrix(w1, 32, 256), W1[32 * j:]) and torch.equal(LR.unpack_matrix(w2, 128, 32, True), W2[:, 32 * j:])


@pytest.mark.parametrize("dtype", [F32, F16])
def test_pack_without_ffn_is_merge_alone(dtype):
    from igs_amd import tokens as TK
    layer = LR.make_tail_layer(no_ffn=True, seed=3)
    flat = TK.pack_layer_tail(layer, dtype)
    assert flat.numel() == LR.pack_elems(0, False) == 16 * 1024
    assert torch.equal(_bits(LR.unpack_tail(flat)[0]), _bits(layer.merge.weight.detach().to(dtype)))


# ---------------------------------------------------------------- exports
def test_entry_points_are_exported_declared_and_built():
    from igs_amd import _cabi, build
    L = _cabi.lib()
    header = open(build.HERE + "/../include/igs_rast.h").read()
    for n in NAMES:
        assert n in _cabi.SIGNATURES and hasattr(L, n), n
        decl = re.search(r"\b%s\(([^;]*)\);" % n, header)
        assert decl and len(decl.group(1).split(",")) == len(_cabi.SIGNATURES[n][1]), n
    assert "ffn.hip" in build.SOURCES
    ext = _cabi.ext()
    for f in ("layer_tail_fwd", "pack_elems"):
        assert hasattr(ext._ffn, f), f                                                           # (a private submodule of _C)
    from igs_amd import tokens as TK
    for fn in ("pack_layer_tail", "layer_tail", "use_native_layer_tails"):
        assert callable(getattr(TK, fn)), fn
    for hidden in (32, 96, 1024, 2048):
        assert L.igs_layer_tail_pack_elems(hidden, 1) == LR.pack_elems(hidden) == ext._ffn.pack_elems(hidden, True)
    assert L.igs_layer_tail_pack_elems(0, 0) == L.igs_layer_tail_pack_elems(48, 0) == 16 * 1024     # hidden is not read without FFN
    for hidden in (0, 16, 48, 2080, -32):
        assert L.igs_layer_tail_pack_elems(hidden, 1) == -1, hidden


# ---------------------------------------------------------------- the C ABI's refusals
# Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes.  Every
# operand has an address of its own with spans that do not meet, so GOOD passes every argument check and each case below differs from it
# in the one thing that its reason word names.  (GOOD itself would launch, so it is never sent.)
A, S, OUT, WP, L1W, L1B, L2W, L2B = 0x1000000, 0x3000000, 0x5000000, 0x7000000, 0x9000000, 0x9100000, 0x9200000, 0x9300000
GOOD = dict(T=5, cdt=0, has_ffn=1, hidden=64, a=A, adt=0, astr=128, s=S, sdt=0, sstr=128, w=WP, l1w=L1W, l1b=L1B, eps1=1e-5,
            l2w=L2W, l2b=L2B, eps2=1e-5, out=OUT, odt=0, ostr=128)


def _call(**kw):
    from igs_amd import _cabi
    k = dict(GOOD, **kw)
    return _cabi.lib().igs_layer_tail_fwd(None, k["T"], k["cdt"], k["has_ffn"], k["hidden"], k["a"], k["adt"], k["astr"], k["s"], k["sdt"], k["sstr"],
                                          k["w"], k["l1w"], k["l1b"], k["eps1"], k["l2w"], k["l2b"], k["eps2"], k["out"], k["odt"], k["ostr"])


REFUSED = ([(dict(hidden=h), "hidden") for h in (0, 48, 2080, -32)]
           + [(dict(T=-1), "T out of range"), (dict(T=(1 << 24) + 1), "T out of range")]
           + [(dict([(k, v)]), "row stride") for k in ("astr", "sstr", "ostr") for v in (127, 0, -128, (1 << 31) + 4)]
           + [(dict([(k, None)]), "NULL") for k in ("a", "s", "w", "l1w", "l1b", "l2w", "l2b", "out")]
           + [(dict(has_ffn=0, a=None), "NULL"), (dict(has_ffn=0, l1b=None), "NULL")]
           + [(dict([(k, v)]), "dtype") for k in ("cdt", "adt", "sdt", "odt") for v in (-1, 2)]
           + [(dict(eps1=-1.0), "eps"), (dict(eps1=float("inf")), "eps"), (dict(eps2=float("nan")), "eps")]
           + [(dict(a=A + 2), "aligned to its element size"), (dict(adt=1, a=A + 1), "aligned to its element size"),
              (dict(s=S + 1), "aligned to its element size"), (dict(out=OUT + 2), "aligned to its element size"),
              (dict(odt=1, out=OUT + 1), "aligned to its element size"), (dict(l1w=L1W + 2), "aligned to its element size"),
              (dict(l1b=L1B + 1), "aligned to its element size"), (dict(l2w=L2W + 2), "aligned to its element size"),
              (dict(l2b=L2B + 3), "aligned to its element size")]
           + [(dict(w=WP + 4), "16 bytes"), (dict(w=WP + 8), "16 bytes"), (dict(cdt=1, w=WP + 2), "16 bytes")]
           # out over an input: the same rows, the last element of a's last row, a's rows between out's at a wider stride, s in another dtype
           + [(dict(out=A), "out overlaps"), (dict(out=A + (4 * 128 + 127) * 4), "out overlaps"), (dict(astr=256, out=A + 128 * 4, ostr=256), "out overlaps"),
              (dict(out=S), "out overlaps"), (dict(sdt=1, out=S + 4 * 128 * 2), "out overlaps"), (dict(a=OUT + 16), "out overlaps")])


@pytest.mark.parametrize("kw,word", REFUSED, ids=lambda v: v if isinstance(v, str) else "-".join(
    "%s=%s" % (k, x if x is None or isinstance(x, float) or abs(x) < 1 << 20 else hex(x)) for k, x in v.items()))
def test_the_c_abi_refuses_each_argument_for_its_own_reason_before_any_hip_call(kw, word):
    from igs_amd import _cabi
    assert _call(**kw) == E_INVALID, kw
    assert word in _cabi.last_error() and "igs_layer_tail_fwd" in _cabi.last_error(), (kw, word, _cabi.last_error())


def test_nothing_to_do_returns_zero_after_the_size_checks():
    from igs_amd import _cabi
    assert _call(T=0) == 0 and _call(T=0, a=None, out=None, w=None) == 0                          # T = 0 launches nothing
    assert _call(T=0, out=A) == 0                                                                # ... and has no rows that could overlap
    for kw, word in ((dict(hidden=48), "hidden"), (dict(ostr=100), "row stride"), (dict(adt=3), "dtype"), (dict(eps1=-1.0), "eps")):
        assert _call(T=0, **kw) == E_INVALID and word in _cabi.last_error(), kw                  # the sizes and codes are still checked
    assert _call(T=0, has_ffn=0, hidden=48) == 0 and _call(T=0, has_ffn=0, eps2=-1.0) == 0       # hidden and eps2 are not read without FFN


# ---------------------------------------------------------------- the Python layer's refusals
class Pair(nn.Module):
    """A served layer beside the one under test: a binder that refuses must leave both alone."""

    def __init__(self, other):
        super().__init__()
        self.good, self.other = LR.make_tail_layer(64, seed=1), other


def _with(layer, **attrs):
    for k, v in attrs.items():
        setattr(layer, k, v)
    return layer


def _mlp(*mods):
    return nn.Sequential(*mods)


class Tanh(nn.GELU):
    pass


BAD_LAYERS = {
    "merge with a bias": lambda: _with(LR.make_tail_layer(64), merge=nn.Linear(128, 128)),
    "mlp[0] with a bias": lambda: _with(LR.make_tail_layer(64), mlp=_mlp(nn.Linear(256, 64), nn.GELU(), nn.Linear(64, 128, bias=False))),
    "mlp[2] with a bias": lambda: _with(LR.make_tail_layer(64), mlp=_mlp(nn.Linear(256, 64, bias=False), nn.GELU(), nn.Linear(64, 128))),
    "tanh gelu": lambda: _with(LR.make_tail_layer(64), mlp=_mlp(nn.Linear(256, 64, bias=False), nn.GELU(approximate="tanh"), nn.Linear(64, 128, bias=False))),
    "relu": lambda: _with(LR.make_tail_layer(64), mlp=_mlp(nn.Linear(256, 64, bias=False), nn.ReLU(), nn.Linear(64, 128, bias=False))),
    "four modules": lambda: _with(LR.make_tail_layer(64), mlp=_mlp(nn.Linear(256, 64, bias=False), nn.GELU(), nn.Linear(64, 128, bias=False), nn.Identity())),
    "not a Sequential": lambda: _with(LR.make_tail_layer(64), mlp=nn.Linear(256, 128, bias=False)),
    "hidden 48": lambda: LR.make_tail_layer(48),
    "hidden 2080": lambda: LR.make_tail_layer(2080),
    "hidden 16": lambda: LR.make_tail_layer(16),
    "mlp from 128": lambda: _with(LR.make_tail_layer(64), mlp=_mlp(nn.Linear(128, 64, bias=False), nn.GELU(), nn.Linear(64, 128, bias=False))),
    "d_model 64": lambda: TR.make_layer(d_model=64),
    "d_model 64 without ffn": lambda: TR.make_layer(d_model=64, no_ffn=True),
    "bfloat16": lambda: LR.make_tail_layer(64).to(torch.bfloat16),
    "float64": lambda: LR.make_tail_layer(64, no_ffn=True).double(),
    "norm1 without affine": lambda: _with(LR.make_tail_layer(64), norm1=nn.LayerNorm(128, elementwise_affine=False)),
    "norm2 is a GroupNorm": lambda: _with(LR.make_tail_layer(64), norm2=nn.GroupNorm(4, 128)),
    "nhead 2": lambda: _with(LR.make_tail_layer(64), nhead=2),
}


@pytest.mark.parametrize("name", list(BAD_LAYERS))
def test_the_binder_refuses_before_anything_is_changed(name):
    from igs_amd import tokens as TK
    pair = Pair(BAD_LAYERS[name]())
    before = [m.forward for m in pair.modules()]
    keys = list(pair.state_dict().keys())
    with pytest.raises(NotImplementedError):
        TK.use_native_layer_tails(pair)
    assert [m.forward for m in pair.modules()] == before and not any("forward" in m.__dict__ or TK.TAIL_CACHE in m.__dict__ for m in pair.modules())
    assert list(pair.state_dict().keys()) == keys
    if name != "nhead 2":
        with pytest.raises(NotImplementedError):
            TK.pack_layer_tail(pair.other)
        x = torch.zeros(3, 128)
        with pytest.raises(NotImplementedError), torch.no_grad():
            TK.layer_tail(x, x, pair.other)


def test_the_binder_binds_served_layers_and_leaves_the_other_binder_alone():
    from igs_amd import tokens as TK
    pair = Pair(LR.make_tail_layer(no_ffn=True, seed=2))
    keys = list(pair.state_dict().keys())
    assert TK.use_native_layer_tails(pair) == 2
    assert all(m.forward.__func__ is TK._layer_tail_forward and m.forward.__self__ is m for m in (pair.good, pair.other))
    assert list(pair.state_dict().keys()) == keys and type(pair.good) is TR.TransformerLayer
    assert TK.use_native_transformer_layers(pair) == 2 and pair.good.forward.__func__ is TK._layer_forward
    assert TK.LAYER_TAIL_FUSED.keys() == {F32, F16}


def test_layer_tail_refuses_gradients_shapes_dtypes_and_the_cpu():
    from igs_amd import tokens as TK
    layer = LR.make_tail_layer(64)
    x = torch.zeros(2, 3, 128)
    with pytest.raises(NotImplementedError, match="forward only"):                               # the parameters require grad
        TK.layer_tail(x, x, layer)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="one GPU"):
            TK.layer_tail(x, x, layer)
        for a, s in ((x[..., :64], x[..., :64]), (x, x[:1]), (torch.zeros(()), torch.zeros(()))):
            with pytest.raises(ValueError):
                TK.layer_tail(a, s, layer)
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(NotImplementedError, match="float32 or float16"):
                TK.layer_tail(x.to(dt), x, layer)
            with pytest.raises(NotImplementedError, match="float32 or float16"):
                TK.layer_tail(x, x, layer, compute_dtype=dt)
            with pytest.raises(NotImplementedError):
                TK.pack_layer_tail(layer, dt)
        with pytest.raises(ValueError, match="packed holds"):
            TK.layer_tail(x, x, layer, packed=TK.pack_layer_tail(layer, F16), compute_dtype=F32)
    for p in layer.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="forward only"):                               # an input requires grad
        TK.layer_tail(x.clone().requires_grad_(True), x, layer)
