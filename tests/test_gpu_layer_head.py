"""The fused q / k / v projections (igs_amd/csrc/proj.hip through the C ABI and through igs_amd.tokens) against the float64 restatement of
tests/layer_head_restatement.py on the same float32 / float16 inputs, and the two binders that use them.

Every output element is compared.  The allowance is the project's four-times rule on max |err| / max |ref|: the comparator is F.linear on the
same inputs in the same compute dtype (rounded to the output's dtype), and the fused result may be at most 4 x as far from float64 as that
comparator is, with the floors of test_gpu_token_ops.py (1e-5 in float32, 2e-3 in float16).  For the binders the comparator is the same
stand-in transformer bound with use_native_layer_tails alone.  Both errors are printed for every case.

The C ABI cases run on PyTorch's current stream so that the test chooses where the operands lie: rows at a stride above the minimum, bases
one element past the 16-byte grid (the scalar access path), mixed x / out dtypes, and the output pre-filled with NaN inside an allocation that
holds a sentinel everywhere else, the columns of a row beyond 128 n included, which is checked afterwards.

The tests that need no GPU (the pack, the exports, the refusals, which all happen before any HIP call) are not marked; the others are.
The binder tests set the routing constants they depend on (tokens.LAYER_HEAD_FUSED, LAYER_HEAD_MIN_OUTPUTS, LAYER_TAIL_FFN_MIN_FILL), so
that they pin the kernels' paths whatever the measurements of DESIGN.md section 28 decide; one test checks the routing by the constants.

Recorded on one MI355X, max |err| / max |ref| against float64: float32 compute 3.1e-7 to 7.0e-7 on both sides (2.5e-4
to 4.2e-4 where the result is float16); float16 compute 1.5e-4 to 5.6e-4 fused beside 2.5e-4 to 6.4e-4 for F.linear; the bound stand-in
transformers 8.9e-7 to 1.2e-6 beside 7.5e-7 to 1.1e-6 for use_native_layer_tails alone in float32, 1.1e-3 to 2.4e-3 beside 1.1e-3 to 1.9e-3
under float16 autocast."""
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import layer_head_restatement as LH
import token_ops_restatement as TR
import window_attention_restatement as WR

gpu = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
CODE = {F32: 0, F16: 1}
FLOOR = {F32: 1e-5, F16: 2e-3}
BAND = 64
SENTINEL = 12345.0
E_INVALID = -1
NAMES = ("igs_token_proj_pack_elems", "igs_token_proj_fwd")


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _ok(rc):
    from igs_amd import _cabi
    assert rc == 0, _cabi.last_error()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _four_times(label, fused, cmp_, ref, cdt):
    assert not torch.isnan(fused).any(), (label, "an element was not written")
    e_f, e_c = _rel(fused, ref), _rel(cmp_, ref)
    allowed = max(4 * e_c, FLOOR[cdt])
    print("%s: max |err| / max |ref| against float64: comparator %.3e, fused %.3e (allowed %.3e)" % (label, e_c, e_f, allowed))
    assert e_f <= allowed, (label, e_f, e_c)


class Rows:
    """[N, width] rows at `stride` elements, starting BAND + offset elements into an allocation that holds SENTINEL outside the rows."""

    def __init__(self, N, width, dtype, stride=None, offset=0, src=None):
        self.stride = stride = width if stride is None else stride
        self.big = torch.full((2 * BAND + offset + max(N, 1) * stride + 8,), SENTINEL, dtype=dtype, device=DEV)
        self.v = self.big[BAND + offset:].as_strided((N, width), (stride, 1))
        self.inside = torch.zeros_like(self.big, dtype=torch.bool)
        self.inside[BAND + offset:].as_strided((N, width), (stride, 1)).fill_(True)
        self.v.copy_(src if src is not None else torch.full((N, width), float("nan")))

    def check(self, label):
        assert (self.big[~self.inside] == SENTINEL).all(), (label, "an element outside the rows was written")


class Heads:
    """n weights as the C ABI takes them: float64 and float32 copies and the pack per compute dtype on the GPU."""

    def __init__(self, n, seed=0):
        self.n = n
        self.w32 = [w.to(DEV) for w in LH.make_weights(n, seed, F32)]
        self.w64 = [w.double() for w in self.w32]
        self.packs = {dt: LH.pack_projections([w.cpu().to(dt) for w in self.w32]).contiguous().to(DEV) for dt in (F32, F16)}

    def run(self, cdt, x, out, rot=None):
        import ctypes
        r = None if rot is None else (ctypes.c_longlong * self.n)(*rot)
        _ok(_lib().igs_token_proj_fwd(_stream(), x.v.shape[0], self.n, CODE[cdt], x.v.data_ptr(), CODE[x.v.dtype], x.stride, self.packs[cdt].data_ptr(), r,
                                      out.v.data_ptr(), CODE[out.v.dtype], out.stride))

    def dense(self, cdt, x, rot=None, odt=F32):
        """The fused result for a contiguous [T, 128] tensor."""
        rx, out = Rows(x.shape[0], 128, x.dtype, src=x), Rows(x.shape[0], 128 * self.n, odt)
        self.run(cdt, rx, out, rot)
        out.check("dense")
        return out.v.clone()

    def comparator(self, cdt, x, rot, odt):
        """F.linear on the same input in the same compute dtype, rounded to the output's dtype, rolled and laid side by side."""
        outs = [F.linear(x.to(cdt), w.to(cdt)).to(odt) for w in self.w32]
        return torch.cat([torch.roll(o, 0 if rot is None else rot[j], 0) for j, o in enumerate(outs)], 1)


_HEADS = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """The tests of other files that measure peak memory count a cached block handed out whole (PyTorch's allocator does not split a large
    block for a remainder below 1 MB), so this file returns what it allocated: its shared operands are dropped and the cache is emptied."""
    yield
    _HEADS.clear()
    _REFS.clear()
    if torch.cuda.is_available():
        import gc
        gc.collect()
        torch.cuda.empty_cache()


def _heads(n):
    if n not in _HEADS:
        _HEADS[n] = Heads(n, seed=n)
    return _HEADS[n]


def _rot_for(T, n, turn=0):
    """Offsets from {0, 1, T / 2, T - 1}, a different one for neighbouring outputs."""
    if T == 0:
        return None
    return [(0, 1 % T, T // 2, T - 1)[(j + turn) % 4] for j in range(n)]


# (x dtype, out dtype, extra stride of x / out, offset from the 16-byte grid)
VARIANTS = [(F32, F32, (0, 0), 0), (F32, F32, (4, 8), 0), (F32, F32, (3, 5), 1), (F16, F16, (0, 0), 0), (F32, F16, (128, 4), 0),
            (F16, F16, (2, 0), 1), (F16, F32, (8, 8), 0)]


def _abi_case(heads, cdt, T, variant, seed, turn=0):
    xdt, odt, extra, offset = variant
    n = heads.n
    x64 = LH.project_inputs(T, seed, DEV)
    x, out = Rows(T, 128, xdt, 128 + extra[0], offset, x64.to(xdt)), Rows(T, 128 * n, odt, 128 * n + extra[1], offset)
    rot = _rot_for(T, n, turn)
    label = "T %d n %d compute %s x %s out %s stride +%s offset %d rot %s" % (T, n, str(cdt)[6:], str(xdt)[6:], str(odt)[6:], extra, offset, rot)
    heads.run(cdt, x, out, rot)
    for r in (x, out):
        r.check(label)
    assert torch.equal(x.v.double(), x64.to(xdt).double()), (label, "the input was written")
    if T == 0:
        return
    _four_times(label, out.v, heads.comparator(cdt, x.v.contiguous(), rot, odt), LH.project_restate(x.v.double(), heads.w64, rot), cdt)


# ---------------------------------------------------------------- 1. through the C ABI against float64
# a trip is 128 rows, a wave's share 32: T at both boundaries, nothing at all, and one wave's share past two trips.  n = 1, 2: the
# matrices stay in LDS; n = 3, 5: they stream through the two buffers (an odd count, so a matrix meets both buffers over the trips).
TRIP_T = (0, 1, 31, 33, 127, 128, 129, 32 * 1 + 128 * 2)


@gpu
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_element_against_float64_at_the_wave_and_trip_boundaries(n, cdt):
    assert LH.TRIP_ROWS == 128
    heads = _heads(n)
    for i, T in enumerate(TRIP_T):
        _abi_case(heads, cdt, T, VARIANTS[(i + n) % len(VARIANTS)], seed=7 * T + n, turn=i)
    # the scalar access path (a base off the 16-byte grid, float32 and float16) and the widest strides just past a wave's share and a trip
    for T in (33, 129):
        for v in (2, 5, 4):
            _abi_case(heads, cdt, T, VARIANTS[v], seed=11 * T + n + v, turn=v)


@gpu
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [2, 3])
def test_a_workgroup_takes_a_second_trip(n, cdt):
    """The documented launch rule (include/igs_rast.h): min(trips, compute units x (float16 ? 2 : 1)) workgroups, so one row more than a
    full grid of trips sends workgroup 0 round its loop again.  No float64 reference at this size: rows from both ends and from the second
    trip must have the bits they have in a small call (a row's result depends on that row and the weights only)."""
    heads = _heads(n)
    groups = torch.cuda.get_device_properties(0).multi_processor_count * (2 if cdt == F16 else 1)
    T = groups * LH.TRIP_ROWS + 1
    x = torch.randn(T, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    rot = _rot_for(T, n, 1)
    rx, out = Rows(T, 128, F32, src=x), Rows(T, 128 * n, F32, 128 * n + 4)
    heads.run(cdt, rx, out, rot)
    out.check("second trip")
    assert not torch.isnan(out.v).any(), "an element was not written"
    pick = torch.cat([torch.arange(0, 200), torch.arange(T // 2 - 70, T // 2 + 70), torch.arange(T - 200, T)]).to(DEV)
    small = heads.dense(cdt, x[pick].contiguous())
    for j in range(n):
        got = out.v[(pick + rot[j]) % T, 128 * j: 128 * (j + 1)]
        assert torch.equal(_bits(got), _bits(small[:, 128 * j: 128 * (j + 1)])), (j, "rows of the large call differ from the small call's")


# ---------------------------------------------------------------- 2. rot
@gpu
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n,T", [(4, 200), (5, 130), (1, 64), (2, 2)])
def test_rot_is_torch_roll_of_the_unrotated_result_bit_for_bit(n, T, cdt):
    heads = _heads(n)
    x = LH.project_inputs(T, 21, DEV).to(F32)
    plain = heads.dense(cdt, x)
    assert torch.equal(_bits(plain), _bits(heads.dense(cdt, x, [0] * n))), "rot = NULL and rot = 0 differ"
    for turn in range(4):
        rot = _rot_for(T, n, turn)
        got = heads.dense(cdt, x, rot)
        for j in range(n):
            want = torch.roll(plain[:, 128 * j: 128 * (j + 1)], rot[j], 0)
            assert torch.equal(_bits(got[:, 128 * j: 128 * (j + 1)]), _bits(want)), (rot, j)


# ---------------------------------------------------------------- 3. bits
@gpu
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [2, 5])
def test_a_row_has_the_same_bits_alone_elsewhere_and_twice(n, cdt):
    heads = _heads(n)
    x = LH.project_inputs(300, 11, DEV).to(F32)
    whole = heads.dense(cdt, x)
    assert torch.equal(_bits(whole), _bits(heads.dense(cdt, x))), "two runs of the same call differ"
    other = LH.project_inputs(50, 12, DEV).to(F32)
    for i in (0, 31, 37, 127, 128, 255, 299):
        alone = heads.dense(cdt, x[i: i + 1])
        assert torch.equal(_bits(alone[0]), _bits(whole[i])), (i, "alone")
        other[13] = x[i]
        assert torch.equal(_bits(heads.dense(cdt, other)[13]), _bits(whole[i])), (i, "at another position")


@gpu
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 3])
def test_a_nan_stays_in_its_row(n, cdt):
    heads = _heads(n)
    T, bad = 140, 77
    x = LH.project_inputs(T, 5, DEV).to(F32)
    rot = _rot_for(T, n, 1)
    clean = heads.dense(cdt, x, rot)
    x[bad, 19] = float("nan")
    dirty = heads.dense(cdt, x, rot)
    hit = torch.zeros(T, 128 * n, dtype=torch.bool, device=DEV)
    for j in range(n):
        hit[(bad + rot[j]) % T, 128 * j: 128 * (j + 1)] = True
    assert torch.isnan(dirty[hit]).all(), "the row's outputs are not all NaN"
    assert torch.equal(_bits(dirty)[~hit], _bits(clean)[~hit]), "a NaN changed another row"


# ---------------------------------------------------------------- 4. the pack, the exports, the refusals (no GPU needed)
@pytest.mark.parametrize("dtype", [F32, F16])
def test_the_library_packs_each_matrix_as_the_layer_tail_packs_merge(dtype):
    from igs_amd import tokens as TK
    import layer_tail_restatement as LR
    ws = LH.make_weights(5, 1, F32)
    mine = TK.pack_projections(ws, dtype)
    assert mine.dtype == dtype and mine.is_contiguous() and mine.numel() == 5 * LH.MATRIX
    assert torch.equal(_bits(mine), _bits(LH.pack_projections([w.to(dtype) for w in ws])))
    for j, w in enumerate(ws):
        assert torch.equal(_bits(LR.unpack_matrix(mine[j * LH.MATRIX: (j + 1) * LH.MATRIX], 128, 128)), _bits(w.to(dtype))), j
    lin = nn.Linear(128, 128, bias=False)
    assert torch.equal(TK.pack_projections([lin], dtype), TK.pack_projections([lin.weight], dtype))


def test_entry_points_are_exported_declared_and_built():
    from igs_amd import _cabi, build
    L = _cabi.lib()
    header = open(build.HERE + "/../include/igs_rast.h").read()
    for name in NAMES:
        assert name in _cabi.SIGNATURES and hasattr(L, name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == len(_cabi.SIGNATURES[name][1]), name
    assert "proj.hip" in build.SOURCES
    ext = _cabi.ext()
    for f in ("token_proj_fwd", "pack_elems"):
        assert hasattr(ext._proj, f), f
    for n in range(1, LH.MAX_OUT + 1):
        assert L.igs_token_proj_pack_elems(n) == n * LH.MATRIX == ext._proj.pack_elems(n)
    for n in (0, -1, LH.MAX_OUT + 1):
        assert L.igs_token_proj_pack_elems(n) == -1 == ext._proj.pack_elems(n)


# Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes.
FAKE = (0x1000000, 0x3000000, 0x5000000)
REFUSED = LH.refusals(*FAKE)
_ID = lambda v: v if isinstance(v, str) else "-".join("%s=%s" % (k, x if not isinstance(x, int) or abs(x) < 1 << 20 else hex(x)) for k, x in v.items())


@pytest.mark.parametrize("kw,word", REFUSED, ids=_ID)
def test_the_c_abi_refuses_each_argument_for_its_own_reason_before_any_hip_call(kw, word):
    from igs_amd import _cabi
    assert LH.call_abi(_cabi.lib(), None, dict(LH.good_call(*FAKE), **kw)) == E_INVALID, kw
    assert word in _cabi.last_error() and "igs_token_proj_fwd" in _cabi.last_error(), (kw, word, _cabi.last_error())


def test_nothing_to_do_returns_zero_after_the_size_checks():
    from igs_amd import _cabi
    call = lambda **kw: LH.call_abi(_cabi.lib(), None, dict(LH.good_call(*FAKE), **kw))
    assert call(T=0) == 0 and call(T=0, x=None, out=None, w=None) == 0 and call(T=0, rot=None) == 0      # T = 0 launches nothing
    assert call(T=0, out=FAKE[0]) == 0                                                                   # ... and has no rows that could overlap
    for kw, word in ((dict(n=6), "n out of range"), (dict(ostr=100), "row stride"), (dict(xdt=3), "dtype"), (dict(rot=(0, 1, 0)), "rot")):
        assert call(T=0, **kw) == E_INVALID and word in _cabi.last_error(), kw                           # the sizes and codes are still checked


@gpu
def test_a_refused_call_launches_nothing():
    """The same list with device memory behind the addresses: every case is refused, and afterwards the output still holds its fill and the
    input its values."""
    from igs_amd import _cabi
    x = Rows(5, 128, F32, src=LH.project_inputs(5, 1, DEV).to(F32))
    out = Rows(5, 1024, F32)
    out.v.fill_(SENTINEL)
    w = _heads(5).packs[F32]
    kept = x.big.clone()
    base = (x.v.data_ptr(), w.data_ptr(), out.v.data_ptr())
    for kw, word in LH.refusals(*base):
        assert LH.call_abi(_cabi.lib(), _stream(), dict(LH.good_call(*base), **kw)) == E_INVALID, kw
        assert word in _cabi.last_error(), (kw, _cabi.last_error())
    torch.cuda.synchronize()
    assert (out.big == SENTINEL).all() and torch.equal(x.big, kept)


def test_project_tokens_refuses_gradients_shapes_dtypes_and_the_cpu():
    from igs_amd import tokens as TK
    x, ws = torch.zeros(3, 128), LH.make_weights(2, 0, F32)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TK.project_tokens(x, ws)
        for bad in (torch.zeros(3, 64), torch.zeros(())):
            with pytest.raises(ValueError):
                TK.project_tokens(bad, ws)
        for bad_ws in ([], ws * 3, [torch.zeros(128, 64)], [torch.zeros(128)]):
            with pytest.raises(ValueError):
                TK.project_tokens(x, bad_ws)
        for rot in ((0,), (0, 3), (-1, 0)):
            with pytest.raises(ValueError, match="rot"):
                TK.project_tokens(x, ws, rot=rot)
        with pytest.raises(NotImplementedError, match="128"):
            TK.project_tokens(torch.zeros(3, 64), [torch.zeros(64, 64)])
        with pytest.raises(NotImplementedError, match="bias"):
            TK.project_tokens(x, [nn.Linear(128, 128)])
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(NotImplementedError):
                TK.project_tokens(x.to(dt), ws)
            with pytest.raises(NotImplementedError):
                TK.project_tokens(x, [w.to(dt) for w in ws])
            with pytest.raises(NotImplementedError):
                TK.project_tokens(x, ws, compute_dtype=dt)
            with pytest.raises(NotImplementedError):
                TK.pack_projections(ws, dt)
        with pytest.raises(ValueError, match="packed"):
            TK.project_tokens(x, ws, packed=TK.pack_projections(ws, F16), compute_dtype=F32)
    with pytest.raises(NotImplementedError, match="forward only"):
        TK.project_tokens(x.clone().requires_grad_(True), ws)
    with pytest.raises(NotImplementedError, match="forward only"):
        TK.project_tokens(x, [ws[0], ws[1].clone().requires_grad_(True)])


def test_the_binders_refuse_before_they_change_anything():
    from igs_amd import tokens as TK
    model = LH.make_transformer(True)
    before = [(m, m.__dict__.get("forward")) for m in model.modules()]
    model.layers[1].cross_attn_ffn.k_proj = nn.Linear(128, 128, bias=True)
    for bind in (lambda: TK.use_native_layer_heads(model), lambda: TK.use_native_feature_transformer(model, True)):
        with pytest.raises(NotImplementedError, match="bias"):
            bind()
    with pytest.raises(NotImplementedError, match="blocks"):
        TK.use_native_feature_transformer(model.layers[0], True)
    with pytest.raises(NotImplementedError):
        TK.use_native_layer_heads(TR.make_layer(d_model=64, no_ffn=True))
    assert all(m.__dict__.get("forward") is f for m, f in before), "a refused binder changed a forward"
    good = LH.make_transformer(False)
    assert TK.use_native_feature_transformer(good, False) == 4
    assert good.forward.__func__ is TK._feature_forward and all(m.forward.__func__ is TK._layer_head_forward for b in good.layers for m in b.children())
    assert TK.use_native_layer_heads(good, training=True) == 4 and good.layers[0].self_attn.forward.__func__ is TK._layer_head_forward_training
    assert set(good.state_dict()) == set(LH.make_transformer(False).state_dict())


# ---------------------------------------------------------------- 5. the binders on stand-in transformers
H = W = 4
SPLITS = 2                                                           # 2 x 2-token windows: the smallest a shifted call allows; block 1 is shifted


@pytest.fixture
def routed(monkeypatch):
    """The routing constants the binder tests pin: every launch fused, the fused tail whatever the fill."""
    from igs_amd import tokens as TK
    monkeypatch.setattr(TK, "LAYER_HEAD_FUSED", {F32: True, F16: True})
    monkeypatch.setattr(TK, "LAYER_HEAD_MIN_OUTPUTS", {F32: 1, F16: 1})
    monkeypatch.setattr(TK, "LAYER_TAIL_FFN_MIN_FILL", {F32: 0.0, F16: 0.0})
    return TK


def _attention(monkeypatch, native):
    """The two names the layers look up in their module: the native window attention, or the restatement's."""
    from igs_amd import attention as AT
    monkeypatch.setattr(TR, "single_head_split_window_attention", AT.single_head_split_window_attention if native else WR.restated_split)
    monkeypatch.setattr(TR, "single_head_full_attention", AT.single_head_full_attention if native else WR.restated_full)


_REFS = {}


def _reference(monkeypatch, bidirectional, b):
    """The unbound stand-in in float64 with the restated attention, computed once per case and left unchanged."""
    key = (bidirectional, b)
    if key not in _REFS:
        _attention(monkeypatch, False)
        model = LH.make_transformer(bidirectional).double().to(DEV)
        f0, f1 = LH.feature_inputs(b, H, W, b, DEV)
        with torch.no_grad():
            out = model(f0.double(), f1.double(), attn_type="swin", attn_num_splits=SPLITS)
        _REFS[key] = torch.cat(list(out), 0) if bidirectional else out
    return _REFS[key]


def _run(model, b, half):
    f0, f1 = LH.feature_inputs(b, H, W, b, DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=F16, enabled=half):
        out = model(f0, f1, attn_type="swin", attn_num_splits=SPLITS)
    return torch.cat(list(out), 0) if isinstance(out, tuple) else out


class Counter:
    """Counts the calls of a function and keeps what `note` makes of each call's arguments."""

    def __init__(self, fn, note=lambda *a, **k: None):
        self.fn, self.note, self.seen = fn, note, []

    def __call__(self, *a, **k):
        self.seen.append(self.note(*a, **k))
        return self.fn(*a, **k)


def _count_launches(monkeypatch):
    from igs_amd import _cabi
    proj = _cabi.ext()._proj
    counter = Counter(proj.token_proj_fwd, lambda x, pack, n, *a, **k: n)
    monkeypatch.setattr(proj, "token_proj_fwd", counter)
    return counter


@gpu
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16-autocast"])
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("bidirectional", [True, False], ids=["two-way", "one-way"])
def test_bound_transformer_against_float64_with_pinned_launches_and_no_cat_in_the_loop(routed, monkeypatch, bidirectional, b, half):
    TK = routed
    ref = _reference(monkeypatch, bidirectional, b)
    _attention(monkeypatch, True)
    today, mine = (LH.make_transformer(bidirectional).to(DEV) for _ in range(2))
    assert TK.use_native_layer_tails(today) == 4 and TK.use_native_feature_transformer(mine, bidirectional) == 4
    cmp_ = _run(today, b, half)
    features = LH.feature_inputs(b, H, W, b, DEV)
    _run(mine, b, half)                                                # (the first call packs the weights, with torch.cat; the packs are kept)
    with monkeypatch.context() as m:
        launches = _count_launches(m)
        cats = Counter(torch.cat)
        m.setattr(torch, "cat", cats)
        with torch.no_grad(), torch.autocast("cuda", dtype=F16, enabled=half):
            out = mine(*features, attn_type="swin", attn_num_splits=SPLITS)
    # a two-way block: five projections of its input, then the cross layer's q; a one-way block: q, k, v of its input, k, v of feature1, q
    assert launches.seen == ([5, 1] if bidirectional else [3, 2, 1]) * 2, launches.seen
    assert len(cats.seen) == (1 if bidirectional else 0), "torch.cat was called inside the block loop"
    got = torch.cat(list(out), 0) if bidirectional else out
    assert got.dtype == cmp_.dtype and got.shape == ref.shape and got.is_contiguous()
    cdt = F16 if half else F32
    _four_times("%s b %d %s" % ("two-way" if bidirectional else "one-way", b, str(cdt)[6:]), got, cmp_, ref, cdt)


@gpu
@pytest.mark.parametrize("tails", ["before", "after", "none"])
@pytest.mark.parametrize("native_attention", [True, False], ids=["native-attention", "restated-attention"])
def test_it_composes_with_the_window_attention_and_the_tail_binder(routed, monkeypatch, native_attention, tails):
    TK = routed
    ref = _reference(monkeypatch, True, 1)
    _attention(monkeypatch, native_attention)
    today, mine = (LH.make_transformer(True).to(DEV) for _ in range(2))
    TK.use_native_layer_tails(today)
    if tails == "before":
        TK.use_native_layer_tails(mine)
    TK.use_native_feature_transformer(mine, True)
    if tails == "after":
        TK.use_native_layer_tails(mine)
    launches = _count_launches(monkeypatch)
    got = _run(mine, 1, False)
    assert launches.seen == [5, 1] * 2, launches.seen
    _four_times("attention %s, tails %s" % (native_attention, tails), got, _run(today, 1, False), ref, F32)


@gpu
@pytest.mark.parametrize("bidirectional", [True, False], ids=["two-way", "one-way"])
def test_a_call_that_needs_a_gradient_takes_todays_path(routed, monkeypatch, bidirectional):
    TK = routed
    _attention(monkeypatch, True)
    plain, today, mine = (LH.make_transformer(bidirectional).to(DEV) for _ in range(3))
    TK.use_native_layer_tails(today)
    TK.use_native_feature_transformer(mine, bidirectional)
    launches = _count_launches(monkeypatch)
    grads = []
    for model in (plain, today, mine):
        f0, f1 = (t.requires_grad_(True) for t in LH.feature_inputs(1, H, W, 3, DEV))
        out = model(f0, f1, attn_type="swin", attn_num_splits=SPLITS)
        out = torch.cat(list(out), 0) if bidirectional else out
        out.backward(torch.cos(torch.arange(out.numel(), device=DEV, dtype=F32)).view(out.shape))
        grads.append([out.detach(), f0.grad, f1.grad] + [p.grad for p in model.parameters()])
    assert launches.seen == [], "a call that needs a gradient reached the fused projections"
    for i, (p, t, m) in enumerate(zip(*grads)):
        assert torch.equal(_bits(m), _bits(t)), (i, "differs from the forward of use_native_layer_tails")
        # float32 throughout; DESIGN.md section 27 records 1e-6 for this route against the unbound module
        assert _rel(m, p.double()) <= 1e-4, (i, _rel(m, p.double()))
    # ... and under no_grad the same module, parameters still requiring grad, takes the launches
    _run(mine, 1, False)
    assert launches.seen == ([5, 1] if bidirectional else [3, 2, 1]) * 2


@gpu
def test_the_routing_constants_decide_and_another_attn_type_runs_the_original(monkeypatch):
    from igs_amd import tokens as TK
    monkeypatch.setattr(TK, "LAYER_TAIL_FFN_MIN_FILL", {F32: 0.0, F16: 0.0})
    _attention(monkeypatch, True)
    model = LH.make_transformer(True).to(DEV)
    TK.use_native_feature_transformer(model, True)
    launches = _count_launches(monkeypatch)
    base = _run(model, 1, False)
    want = ([5, 1] if TK.LAYER_HEAD_MIN_OUTPUTS[F32] <= 1 else [5]) * 2 if TK.LAYER_HEAD_FUSED[F32] else []
    assert launches.seen == want, (launches.seen, want)
    for fused, least, want in ((True, 2, [5, 5]), (True, 1, [5, 1, 5, 1]), (False, 1, [])):
        monkeypatch.setattr(TK, "LAYER_HEAD_FUSED", {F32: fused, F16: fused})
        monkeypatch.setattr(TK, "LAYER_HEAD_MIN_OUTPUTS", {F32: least, F16: least})
        del launches.seen[:]
        got = _run(model, 1, False)
        assert launches.seen == want, (fused, least, launches.seen)
        assert _rel(got, base.double()) <= 1e-5, (fused, least)
    # another attn_type: the forward that was bound over runs and reaches the first bound layer, which refuses it as it always did
    del launches.seen[:]
    with pytest.raises(NotImplementedError, match="attn_type"), torch.no_grad():
        model(*LH.feature_inputs(1, H, W, 1, DEV), attn_type="self_swin2d_cross_1d", attn_num_splits=SPLITS)
    assert launches.seen == []


@gpu
def test_a_bound_layer_fuses_three_or_one_and_two(routed, monkeypatch):
    TK = routed
    _attention(monkeypatch, True)
    layer, twin = (TR.make_layer(128, no_ffn=False, seed=5).to(DEV) for _ in range(2))
    assert TK.use_native_layer_heads(layer) == 1 and TK.use_native_layer_tails(twin) == 1
    launches = _count_launches(monkeypatch)
    g = torch.Generator().manual_seed(2)
    s, t = (torch.randn(2, H * W, 128, generator=g).to(DEV) for _ in range(2))
    kw = dict(height=H, width=W, attn_num_splits=SPLITS, with_shift=True, shifted_window_attn_mask=WR.paint_mask(H, W, SPLITS).float().to(DEV))
    for half in (False, True):
        with torch.no_grad(), torch.autocast("cuda", dtype=F16, enabled=half):
            del launches.seen[:]
            a, b = layer(s, s, **kw), twin(s, s, **kw)
            assert launches.seen == [3]
            c, d = layer(s, t, **kw), twin(s, t, **kw)
            assert launches.seen == [3, 1, 2]
        ref64 = TR.make_layer(128, no_ffn=False, seed=5).double().to(DEV)
        for got, cmp_, tgt in ((a, b, s), (c, d, t)):
            _attention(monkeypatch, False)
            with torch.no_grad():
                ref = ref64(s.double(), tgt.double(), **kw)
            _attention(monkeypatch, True)
            _four_times("layer half %s self %s" % (half, tgt is s), got, cmp_, ref, F16 if half else F32)
    # a weight changed in place: the pack is rebuilt
    with torch.no_grad():
        layer.q_proj.weight.mul_(2.0)
        twin.q_proj.weight.mul_(2.0)
        assert _rel(layer(s, s, **kw), twin(s, s, **kw).double()) <= 1e-5
