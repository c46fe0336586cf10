"""The fused layer tail on the MI355X (igs_amd/csrc/ffn.hip through the C ABI and through igs_amd.tokens) against the float64 restatement of
tests/layer_tail_restatement.py on the same float32 / float16 inputs.

Every output element is compared.  The allowance is the project's four-times rule on max |err| / max |ref|: the comparator is the unfused
native path (merge, layer_norm, cat, the two Linears around the GELU, layer_norm with the residual) on the same inputs in the same compute
dtype, and the fused result may be at most 4 x as far from float64 as that comparator is, with the floors of test_gpu_token_ops.py (1e-5 in
float32, 2e-3 in float16).  Both errors are printed for every case.

The C ABI cases run on PyTorch's current stream so that the test chooses where the operands lie: rows at a stride above 128, bases one
element past the 16-byte grid (the scalar access path), mixed a / s / out dtypes, and every output pre-filled with NaN inside an
allocation that holds a sentinel everywhere else, which is checked afterwards.

A NaN in `s` of a layer WITHOUT FFN reaches only its own element (out = s + n1, as in the reference); the all-NaN row is asserted where the
computation spreads it: a NaN in `a` in both variants, a NaN in `s` with the FFN.

The forward that use_native_layer_tails binds gives a layer with FFN to the fused kernel only when its rows fill a round of workgroups
(tokens.LAYER_TAIL_FFN_MIN_FILL; the kernel's time does not shrink with the rows), which no quick test does: the stand-in tests set that
constant to 0, and one test checks the default routing.

Recorded on one MI355X, max |err| / max |ref| against float64: float32 compute 5.7e-8 to 2.7e-7 fused beside 5.7e-8
to 1.4e-7 unfused (4.5e-4 on both sides where the result is float16); float16 compute 1.5e-5 to 2.1e-4 fused beside 2.2e-5 to 2.0e-4 unfused;
the bound stand-in layer 4.5e-7 to 9.1e-7 beside 3.5e-7 to 6.6e-7 unpatched in float32, 6.0e-4 to 7.9e-4 beside 6.8e-4 to 8.7e-4 under
float16 autocast; the gradient route equals use_native_transformer_layers' figures (9.5e-7 / 1.0e-6 float32, 1.2e-3 / 1.5e-3 autocast)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import layer_tail_restatement as LR
import token_ops_restatement as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
CODE = {F32: 0, F16: 1}
FLOOR = {F32: 1e-5, F16: 2e-3}
BAND = 64
SENTINEL = 12345.0


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


class Rows:
    """[N, 128] rows at `stride` elements, starting BAND + offset elements into an allocation that holds SENTINEL outside the rows."""

    def __init__(self, N, dtype, stride=128, offset=0, src=None):
        self.big = torch.full((2 * BAND + offset + max(N, 1) * stride + 8,), SENTINEL, dtype=dtype, device=DEV)
        self.v = self.big[BAND + offset:].as_strided((N, 128), (stride, 1))
        self.inside = torch.zeros_like(self.big, dtype=torch.bool)
        self.inside[BAND + offset:].as_strided((N, 128), (stride, 1)).fill_(True)
        self.v.copy_(src if src is not None else torch.full((N, 128), float("nan")))
        self.stride = stride

    def check(self, label):
        assert (self.big[~self.inside] == SENTINEL).all(), (label, "an element outside the rows was written")


# (a dtype, s dtype, out dtype, extra stride of a / s / out, offset from the 16-byte grid)
VARIANTS = [(F32, F32, F32, (0, 0, 0), 0), (F32, F32, F32, (4, 8, 12), 0), (F32, F32, F32, (3, 0, 5), 1), (F16, F32, F16, (0, 0, 0), 0),
            (F32, F16, F32, (128, 4, 0), 0), (F16, F16, F16, (0, 2, 0), 1), (F16, F16, F32, (8, 8, 8), 0)]


class Tail:
    """A stand-in layer's tail as the C ABI takes it: the pack per compute dtype and the float32 LayerNorm parameters on the GPU."""

    def __init__(self, hidden, seed=0):
        self.hidden, self.has_ffn = hidden, hidden > 0
        self.layer = LR.make_tail_layer(hidden, no_ffn=not self.has_ffn, seed=seed).to(DEV)
        self.w64 = LR.layer_weights(self.layer, torch.float64)
        w32 = LR.layer_weights(self.layer, F32)
        self.packs = {dt: LR.pack_tail(*(None if w is None else w.to(dt) for w in (w32[0], w32[2], w32[3]))).contiguous() for dt in (F32, F16)}
        self.ln1 = [t.contiguous() for t in w32[1][:2]] + [w32[1][2]]
        self.ln2 = ([t.contiguous() for t in w32[4][:2]] + [w32[4][2]]) if self.has_ffn else [None, None, 1e-5]

    def run(self, cdt, a, s, out):
        T = a.v.shape[0]
        ptr = lambda t: None if t is None else t.data_ptr()
        _ok(_lib().igs_layer_tail_fwd(_stream(), T, CODE[cdt], int(self.has_ffn), self.hidden, a.v.data_ptr(), CODE[a.v.dtype], a.stride,
                                      s.v.data_ptr(), CODE[s.v.dtype], s.stride, self.packs[cdt].data_ptr(), ptr(self.ln1[0]), ptr(self.ln1[1]), self.ln1[2],
                                      ptr(self.ln2[0]), ptr(self.ln2[1]), self.ln2[2], out.v.data_ptr(), CODE[out.v.dtype], out.stride))

    def dense(self, cdt, a, s, odt=F32):
        """The fused result for contiguous [T, 128] tensors."""
        ra, rs, out = Rows(a.shape[0], a.dtype, src=a), Rows(s.shape[0], s.dtype, src=s), Rows(a.shape[0], odt)
        self.run(cdt, ra, rs, out)
        out.check("dense")
        return out.v.clone()

    def reference(self, a, s):
        return LR.tail_restate(a.double(), s.double(), *self.w64)

    def comparator(self, cdt, a, s, odt):
        """Today's path on the same inputs in the same compute dtype: half operands and float32 norms under autocast, as the bound forward."""
        from igs_amd import tokens as TK
        L = self.layer
        with torch.no_grad(), torch.autocast("cuda", dtype=F16, enabled=cdt == F16):
            m = F.linear(a if cdt == F16 else a.float(), L.merge.weight)
            if not self.has_ffn:
                return TK.layer_norm(m, L.norm1.weight, L.norm1.bias, L.norm1.eps, residual=s, out_dtype=odt)
            n1 = TK.layer_norm(m, L.norm1.weight, L.norm1.bias, L.norm1.eps, out_dtype=F32)
            y = L.mlp(torch.cat([s.float(), n1], -1))
            return TK.layer_norm(y, L.norm2.weight, L.norm2.bias, L.norm2.eps, residual=s, out_dtype=odt)


_TAILS = {}


def _tail(hidden):
    if hidden not in _TAILS:
        _TAILS[hidden] = Tail(hidden, seed=hidden)
    return _TAILS[hidden]


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _four_times(label, fused, cmp_, ref, cdt):
    assert not torch.isnan(fused).any(), (label, "an element was not written")
    e_f, e_c = _rel(fused, ref), _rel(cmp_, ref)
    allowed = max(4 * e_c, FLOOR[cdt])
    print("%s: max |err| / max |ref| against float64: unfused %.3e, fused %.3e (allowed %.3e)" % (label, e_c, e_f, allowed))
    assert e_f <= allowed, (label, e_f, e_c)


def _abi_case(tail, cdt, T, variant, seed):
    adt, sdt, odt, extra, offset = variant
    a64, s64 = LR.tail_inputs(T, seed, DEV)
    a, s = Rows(T, adt, 128 + extra[0], offset, a64.to(adt)), Rows(T, sdt, 128 + extra[1], offset, s64.to(sdt))
    out = Rows(T, odt, 128 + extra[2], offset)
    label = "T %d hidden %d compute %s a %s s %s out %s stride +%s offset %d" % (T, tail.hidden, str(cdt)[6:], str(adt)[6:], str(sdt)[6:], str(odt)[6:], extra, offset)
    tail.run(cdt, a, s, out)
    for r in (a, s, out):
        r.check(label)
    assert torch.equal(a.v.double(), a64.to(adt).double()) and torch.equal(s.v.double(), s64.to(sdt).double()), (label, "an input was written")
    _four_times(label, out.v, tail.comparator(cdt, a.v.contiguous(), s.v.contiguous(), odt), tail.reference(a.v, s.v), cdt)


# ---------------------------------------------------------------- 1. through the C ABI against float64
# a trip is 128 rows, a wave's share 32: T at both boundaries.  hidden 32, 64, 96: one chunk, an even and an odd count for the two chunk
# buffers (a chunk is 32 units); 1024 is the shipped size; 0 stands for the layer without FFN.
TRIP_T = (1, 31, 32, 33, 127, 128, 129)


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 32, 64, 96, 1024])
def test_every_element_against_float64_at_the_wave_and_trip_boundaries(hidden, cdt):
    assert LR.TRIP_ROWS == 128
    tail = _tail(hidden)
    for i, T in enumerate(TRIP_T):
        _abi_case(tail, cdt, T, VARIANTS[(i + hidden // 32) % len(VARIANTS)], seed=7 * T + hidden)
    # the scalar access path (a base off the 16-byte grid, float32 and float16) and the widest strides just past a wave's share and a trip
    for T in (33, 129):
        for v in (2, 5, 4):
            _abi_case(tail, cdt, T, VARIANTS[v], seed=11 * T + hidden + v)


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 64])
def test_a_workgroup_takes_a_second_trip(hidden, cdt):
    """The documented launch rule (include/igs_rast.h): min(trips, compute units x (has_ffn ? 1 : 2)) workgroups, so one row more than a
    full grid of trips sends workgroup 0 round its loop again."""
    groups = torch.cuda.get_device_properties(0).multi_processor_count * (1 if hidden else 2)
    T = groups * LR.TRIP_ROWS + 1
    _abi_case(_tail(hidden), cdt, T, VARIANTS[3 if cdt == F16 else 1], seed=5)


# ---------------------------------------------------------------- 2. row independence
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 96])
def test_a_row_has_the_same_bits_alone_elsewhere_and_twice(hidden, cdt):
    tail = _tail(hidden)
    a, s = (t.to(F32) for t in LR.tail_inputs(200, 11, DEV))
    whole = tail.dense(cdt, a, s)
    assert torch.equal(_bits(whole), _bits(tail.dense(cdt, a, s))), "two runs of the same call differ"
    other_a, other_s = (t.to(F32) for t in LR.tail_inputs(50, 12, DEV))
    for i in (0, 31, 37, 127, 128, 199):
        alone = tail.dense(cdt, a[i: i + 1], s[i: i + 1])
        assert torch.equal(_bits(alone[0]), _bits(whole[i])), (i, "alone")
        other_a[13], other_s[13] = a[i], s[i]
        moved = tail.dense(cdt, other_a, other_s)
        assert torch.equal(_bits(moved[13]), _bits(whole[i])), (i, "at another position")


# ---------------------------------------------------------------- 3. non-finite rows
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 96])
@pytest.mark.parametrize("where", ["a", "s"])
def test_a_nan_stays_in_its_row(where, hidden, cdt):
    tail = _tail(hidden)
    a, s = (t.to(F32) for t in LR.tail_inputs(70, 21, DEV))
    clean = tail.dense(cdt, a, s)
    a2, s2 = a.clone(), s.clone()
    (a2 if where == "a" else s2)[37, 85] = float("nan")
    got = tail.dense(cdt, a2, s2)
    rest = torch.arange(70, device=DEV) != 37
    assert torch.equal(_bits(got[rest]), _bits(clean[rest])), "another row changed"
    if where == "a" or hidden:
        assert torch.isnan(got[37]).all()
    else:                                                                                        # out = s + n1: the NaN of s is one element's
        nan = torch.isnan(got[37])
        assert nan[85] and nan.sum() == 1 and torch.equal(_bits(got[37][~nan]), _bits(clean[37][~nan]))


# ---------------------------------------------------------------- 4. the stand-in layer, bound
def _layer_case(no_ffn, shift, seed=0):
    g = torch.Generator().manual_seed(40 + seed)
    source, target, gout = (torch.randn(2, 64, 128, generator=g).to(DEV) for _ in range(3))
    mask = torch.zeros(4, 16, 16, device=DEV)
    kw = dict(height=8, width=8, shifted_window_attn_mask=mask, with_shift=shift, attn_num_splits=2)
    return TR.make_layer(128, no_ffn=no_ffn, seed=seed).to(DEV), (source, target), gout, kw


def _count_fused_calls(monkeypatch, any_fill=True):
    """Counts the bound forward's calls of layer_tail; any_fill: a layer with FFN takes the fused tail however few rows it has (by default
    the binder wants a full round of workgroups, which no quick test has)."""
    from igs_amd import tokens as TK
    calls, real = [], TK.layer_tail
    if any_fill:
        monkeypatch.setattr(TK, "LAYER_TAIL_FFN_MIN_FILL", {F32: 0.0, F16: 0.0})

    def counted(*args, **kw):
        calls.append(kw.get("compute_dtype"))
        return real(*args, **kw)

    monkeypatch.setattr(TK, "layer_tail", counted)
    return calls


def _bound_under_no_grad(monkeypatch, no_ffn, shift, autocast, install):
    layer, inputs, _, kw = _layer_case(no_ffn, shift)
    want = copy.deepcopy(layer).double()(*[t.double() for t in inputs], **{k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()}).detach()
    keys = list(layer.state_dict().keys())
    calls = _count_fused_calls(monkeypatch)
    with torch.no_grad(), torch.autocast("cuda", dtype=F16, enabled=autocast):
        eager = layer(*inputs, **kw)
        install(layer)
        native = layer(*inputs, **kw)
    assert list(layer.state_dict().keys()) == keys
    assert calls == [F16 if autocast else F32], "the bound forward must take the fused tail once"
    assert native.dtype == eager.dtype and native.shape == eager.shape and torch.isfinite(native).all()
    e_eager, e_native = _rel(eager, want), _rel(native, want)
    allowed = max(4 * e_eager, 2e-3 if autocast else 1e-5)
    print("layer no_ffn %d shift %d autocast %d: unpatched %.3e, bound %.3e (allowed %.3e)" % (no_ffn, shift, autocast, e_eager, e_native, allowed))
    assert e_native <= allowed


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("no_ffn", [True, False])
def test_stand_in_layer_bound_against_its_float64_run(no_ffn, shift, autocast, monkeypatch):
    from igs_amd import tokens as TK
    _bound_under_no_grad(monkeypatch, no_ffn, shift, autocast, lambda m: TK.use_native_layer_tails(m) == 1 or pytest.fail("count"))


@pytest.mark.parametrize("no_ffn", [True, False])
def test_bound_layer_composes_with_the_native_window_attention(no_ffn, monkeypatch):
    from igs_amd import attention as AT, tokens as TK
    for name in (TK.ATTN_SPLIT, TK.ATTN_FULL):
        monkeypatch.setattr(TR, name, getattr(TR, name))                                         # (the stand-in module's names are restored afterwards)

    def install(m):
        assert TK.use_native_layer_tails(m) == 1 and AT.use_native_window_attention(TR) == 2

    _bound_under_no_grad(monkeypatch, no_ffn, True, False, install)
    assert TR.single_head_split_window_attention is AT.single_head_split_window_attention


def test_by_default_a_layer_with_ffn_takes_the_fused_tail_only_when_its_rows_fill_a_round(monkeypatch):
    from igs_amd import tokens as TK
    calls = _count_fused_calls(monkeypatch, any_fill=False)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert TK._tail_fill(torch.empty(cus * 128, 128, device=DEV)) == 1.0 and TK._tail_fill(torch.empty(cus * 64, 128, device=DEV)) == 0.5
    assert abs(TK._tail_fill(torch.empty(cus * 128 + 1, 128, device=DEV)) - 0.5) < 1e-3 and TK._tail_fill(torch.empty(0, 128, device=DEV)) == 0.0
    ffn, plain = _layer_case(False, False)[0], _layer_case(True, False)[0]
    assert TK.use_native_layer_tails(ffn) == 1 and TK.use_native_layer_tails(plain) == 1
    kw = dict(height=8, width=8, with_shift=False, attn_num_splits=2)
    with torch.no_grad():
        x = torch.randn(2, 64, 128, device=DEV)
        ffn(x, x, **kw)
        assert calls == [], "128 rows do not fill a round: the unfused tail"
        plain(x, x, **kw)
        assert calls == [F32], "a layer without FFN is not held to the fill"
        full = torch.randn(cus * 2, 64, 128, device=DEV)                                          # compute units x 128 rows
        out = ffn(full, full, **kw)
        assert calls == [F32, F32] and torch.isfinite(out).all()


# ---------------------------------------------------------------- 5. the gradient route
def _run(module, inputs, gout, **kw):
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = module(*leaves, **kw)
    grads = torch.autograd.grad(out, leaves + list(module.parameters()), gout.to(out.dtype))
    return [out.detach()] + [g.detach() for g in grads]


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("no_ffn", [True, False])
def test_with_gradients_the_bound_forward_keeps_the_unfused_tail(no_ffn, autocast, monkeypatch):
    from igs_amd import tokens as TK
    layer, inputs, gout, kw = _layer_case(no_ffn, True, seed=1)
    want = _run(copy.deepcopy(layer).double(), [t.double() for t in inputs], gout.double(), **{k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()})
    calls = _count_fused_calls(monkeypatch)
    with torch.autocast("cuda", dtype=F16, enabled=autocast):
        eager = _run(layer, inputs, gout, **kw)
        assert TK.use_native_layer_tails(layer) == 1
        native = _run(layer, inputs, gout, **kw)
    assert calls == [], "with gradients wanted the fused entry point must not be called"
    err = lambda got: max(_rel(a, b) for a, b in zip(got, want))
    e_eager, e_native = err(eager), err(native)
    allowed = max(4 * e_eager, 2e-3 if autocast else 1e-5)
    print("gradient route no_ffn %d autocast %d: unpatched %.3e, bound %.3e (allowed %.3e)" % (no_ffn, autocast, e_eager, e_native, allowed))
    assert [t.dtype for t in native] == [t.dtype for t in eager] and e_native <= allowed
    for p in layer.parameters():                                                                 # frozen parameters, an input that wants a gradient
        p.requires_grad_(False)
    leaf = inputs[0].clone().requires_grad_(True)
    assert layer(leaf, inputs[1], **kw).requires_grad and calls == []
    assert not layer(*inputs, **kw).requires_grad and len(calls) == 1                            # nothing wants one: fused, with grad mode on


# ---------------------------------------------------------------- 6. repacking
@pytest.mark.parametrize("no_ffn", [True, False])
def test_an_in_place_update_is_seen_by_the_next_call(no_ffn, monkeypatch):
    from igs_amd import tokens as TK
    monkeypatch.setattr(TK, "LAYER_TAIL_FFN_MIN_FILL", {F32: 0.0, F16: 0.0})                     # the fused tail however few the rows
    layer, inputs, _, kw = _layer_case(no_ffn, False, seed=2)
    assert TK.use_native_layer_tails(layer) == 1
    names = ["merge.weight", "norm1.bias"] + ([] if no_ffn else ["mlp.0.weight", "mlp.2.weight", "norm2.weight"])
    params = dict(layer.named_parameters())
    with torch.no_grad():
        before = layer(*inputs, **kw)
        pack = layer.__dict__[TK.TAIL_CACHE][F32]["pack"]
        with torch.autocast("cuda", dtype=F16):                                                   # the other compute dtype has a pack of its own
            layer(*inputs, **kw)
        again = layer(*inputs, **kw)
        assert layer.__dict__[TK.TAIL_CACHE][F32]["pack"] is pack and torch.equal(again, before)   # unchanged parameters: the same pack
        assert layer.__dict__[TK.TAIL_CACHE][F16]["pack"].dtype == F16
        for name in names:
            params[name].add_(0.05)
            after = layer(*inputs, **kw)
            fresh = copy.deepcopy(layer)
            fresh.__dict__.pop(TK.TAIL_CACHE, None)
            assert torch.equal(_bits(after), _bits(fresh(*inputs, **kw))), (name, "the next call must use the new weights")
            assert not torch.equal(after, before), name
            before = after
        assert torch.equal(layer.__dict__[TK.TAIL_CACHE][F32]["pack"], TK.pack_layer_tail(layer, F32))
        with torch.autocast("cuda", dtype=F16):                                                   # ... and the stale float16 pack is rebuilt too
            layer(*inputs, **kw)
        assert torch.equal(layer.__dict__[TK.TAIL_CACHE][F16]["pack"], TK.pack_layer_tail(layer, F16))


# ---------------------------------------------------------------- 7. refusals
def test_cpu_bfloat16_and_mixed_devices_are_refused():
    from igs_amd import tokens as TK
    layer = LR.make_tail_layer(64).to(DEV)
    x = torch.randn(3, 128, device=DEV)
    with torch.no_grad():
        assert TK.layer_tail(x, x, layer).shape == (3, 128)
        with pytest.raises(RuntimeError, match="one GPU"):
            TK.layer_tail(x.cpu(), x.cpu(), layer)
        with pytest.raises(RuntimeError, match="one GPU"):
            TK.layer_tail(x, x.cpu(), layer)
        with pytest.raises(RuntimeError, match="one GPU"):
            TK.layer_tail(x, x, copy.deepcopy(layer).cpu())
        with pytest.raises(NotImplementedError, match="float32 or float16"):
            TK.layer_tail(x.bfloat16(), x, layer)
        with pytest.raises(NotImplementedError, match="float32 or float16"):
            TK.layer_tail(x, x.double(), layer)
        with pytest.raises(ValueError):
            TK.layer_tail(x, x[:2], layer)
        assert TK.layer_tail(x[:0], x[:0], layer).shape == (0, 128)
