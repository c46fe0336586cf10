"""The backward of the fused layer tail on the MI355X (igs_amd/csrc/ffn_bwd.hip through the C ABI and through igs_amd.tokens) against the
float64 restatement of tests/layer_tail_grad_restatement.py on the same float32 / float16 inputs.

Every element of every gradient is compared.  The allowance is the four-times rule of test_gpu_layer_tail.py, per gradient tensor: the
comparator is the unfused native tail (merge, layer_norm, cat, the two Linears around the GELU, layer_norm with the residual) under
autograd on the same inputs in the same compute dtype, its da / ds rounded once to the dtype the fused call writes, and the fused
max |err| / max |ref| may be at most 4 x the comparator's, with the floors 1e-5 (float32) and 2e-3 (float16).  Both errors are printed.

The C ABI cases run on PyTorch's current stream; the operands lie where the forward's tests put them (rows at a stride above 128, bases one
element past the 16-byte grid, mixed a / s / g / da / ds dtypes), every output pre-filled with NaN inside a sentinel-guarded allocation.

Recorded on one MI355X ("The backward"), max |err| / max |ref| against float64 per gradient tensor: float32 compute
on float32 operands up to 1.8e-6 fused (median 4.2e-7) beside up to 3.3e-6 unfused (median 3.8e-7), 4.4e-4 on both sides where da / ds
are float16; float16 compute up to 5.6e-3 fused (median 4.8e-4) beside up to 5.5e-3 unfused (median 5.8e-4); the fused error at most
3.2 x (float32) and 2.8 x (float16) the comparator's in any tensor.  The bound stand-in layer 2.7e-7 to 4.3e-5 native beside 1.4e-7 to
4.3e-5 unfused in float32; chained behind the native window attention 2.0e-7 to 1.2e-6 beside 1.0e-7 to 1.0e-6.  Memory at T = 8832,
hidden 1024, float32: 4.5 MB held after the forward (95.0 MB unfused), backward peak 147.3 MB (131.1 MB scratch + 15.2 MB gradients)."""
import copy
import gc

import pytest
import torch

import layer_tail_grad_restatement as GR
import layer_tail_restatement as LR
import token_ops_restatement as TR
from test_gpu_layer_tail import BAND, CODE, DEV, F16, F32, Rows, _bits, _layer_case, _lib, _ok, _stream

pytestmark = pytest.mark.gpu
CHUNK = GR.CHUNK_ROWS
PARAMS = GR.NAMES[2:]


@pytest.fixture(autouse=True)
def _leave_the_allocator_as_found():
    """These tests free blocks of unusual sizes (the scratch, autograd graphs that only a collection releases).  Left in PyTorch's cache
    they would be handed out, unsplit, to later tests that assert exact allocation sizes; so every test here returns what it cached."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _param(shape):
    """A float32 parameter gradient pre-filled with NaN between two sentinel bands."""
    n = 1
    for d in shape:
        n *= d
    big = torch.full((2 * BAND + n,), 12345.0, dtype=F32, device=DEV)
    big[BAND: BAND + n] = float("nan")
    return big, big[BAND: BAND + n].view(shape)


class TailGrad:
    """A stand-in layer's tail as igs_layer_tail_bwd takes it: both packs per compute dtype and the float32 LayerNorm parameters."""

    def __init__(self, hidden, seed=0):
        self.hidden, self.has_ffn = hidden, hidden > 0
        self.layer = LR.make_tail_layer(hidden or 64, no_ffn=not self.has_ffn, seed=seed).to(DEV)
        self.w64 = LR.layer_weights(self.layer, torch.float64)
        w32 = LR.layer_weights(self.layer, F32)
        mats = lambda dt: [None if w is None else w.to(dt) for w in (w32[0], w32[2], w32[3])]
        self.packs = {dt: LR.pack_tail(*mats(dt)).contiguous() for dt in (F32, F16)}
        self.packs_t = {dt: GR.pack_tail_t(*mats(dt)).contiguous() for dt in (F32, F16)}
        self.ln1 = [t.contiguous() for t in w32[1][:2]] + [w32[1][2]]
        self.ln2 = ([t.contiguous() for t in w32[4][:2]] + [w32[4][2]]) if self.has_ffn else [None, None, 1e-5]
        H = hidden
        self.shapes = dict(dWm=(128, 128), dln1_w=(128,), dln1_b=(128,), dW1=(H, 256), dW2=(128, H), dln2_w=(128,), dln2_b=(128,))
        self.names = [n for n in GR.NAMES if self.has_ffn or n not in GR.NAMES[5:]]

    def scratch_bytes(self, T, cdt):
        return _lib().igs_layer_tail_bwd_scratch_bytes(T, CODE[cdt], int(self.has_ffn), self.hidden)

    def run(self, cdt, a, s, g, da=None, ds=None, want=PARAMS, label=""):
        """a, s, g, da, ds: Rows (da / ds None: not wanted).  Returns {name: tensor} of everything wanted."""
        T = a.v.shape[0]
        ptr = lambda t: None if t is None else t.data_ptr()
        pg = {n: _param(self.shapes[n]) for n in want if n in self.names}
        need = self.scratch_bytes(T, cdt)
        scratch = torch.full((need + 2 * BAND,), 0x5A, dtype=torch.uint8, device=DEV)           # (not initialised by the caller: any bytes)
        view = lambda r: (None, 0, 128) if r is None else (r.v.data_ptr(), CODE[r.v.dtype], r.stride)
        _ok(_lib().igs_layer_tail_bwd(_stream(), T, CODE[cdt], int(self.has_ffn), self.hidden, *view(a), *view(s), *view(g), self.packs[cdt].data_ptr(),
                                      self.packs_t[cdt].data_ptr(), ptr(self.ln1[0]), ptr(self.ln1[1]), self.ln1[2], ptr(self.ln2[0]), ptr(self.ln2[1]),
                                      self.ln2[2], scratch[BAND:].data_ptr(), need, *view(da), *view(ds), *[ptr(pg[n][1]) if n in pg else None for n in PARAMS]))
        torch.cuda.synchronize()
        assert (scratch[:BAND] == 0x5A).all() and (scratch[BAND + need:] == 0x5A).all(), (label, "written outside the scratch")
        out = {}
        for n, (big, v) in pg.items():
            assert (big[:BAND] == 12345.0).all() and (big[-BAND:] == 12345.0).all(), (label, n, "written outside the gradient")
            out[n] = v.clone()
        for n, r in (("da", da), ("ds", ds)):
            if r is not None:
                r.check(label)
                out[n] = r.v.clone()
        for r in (a, s, g):
            r.check(label)
        return out

    def dense(self, cdt, a, s, g, want=GR.NAMES):
        rows = lambda t: Rows(t.shape[0], t.dtype, src=t)
        T = a.shape[0]
        return self.run(cdt, rows(a), rows(s), rows(g), Rows(T, a.dtype) if "da" in want else None, Rows(T, s.dtype) if "ds" in want else None,
                        [n for n in want if n in PARAMS], "dense")

    def reference(self, a, s, g):
        return dict(zip(GR.NAMES, GR.tail_grad_restate(a.double(), s.double(), g.double(), *self.w64)))

    def comparator(self, cdt, a, s, g):
        """Today's training path on the same inputs in the same compute dtype: the unfused native tail under autograd."""
        from igs_amd import tokens as TK
        L = copy.deepcopy(self.layer)
        leaves = [a.detach().clone().requires_grad_(True), s.detach().clone().requires_grad_(True)]
        with torch.autocast("cuda", dtype=F16, enabled=cdt == F16):                              # (float32 compute: half operands are widened first)
            out = TK._layer_tail_unfused(L, *(leaves if cdt == F16 else [t.float() for t in leaves]))
        params = TK._tail_params(L)
        grads = torch.autograd.grad(out, leaves + params, g.to(out.dtype))
        return dict(zip(self.names, [t.detach() for t in grads]))


_TAILS = {}


def _tail(hidden):
    if hidden not in _TAILS:
        _TAILS[hidden] = TailGrad(hidden, seed=hidden + 3)
    return _TAILS[hidden]


def _four_times(label, fused, cmp_, ref, cdt, names):
    for n in names:
        assert n in fused and not torch.isnan(fused[n]).any(), (label, n, "an element was not written")
        e_f, e_c = GR.rel(fused[n], ref[n]), GR.rel(cmp_[n].to(fused[n].dtype), ref[n])
        allowed = GR.allowed(e_c, cdt)
        print("%s %s: max |err| / max |ref| against float64: unfused %.3e, fused %.3e (allowed %.3e)" % (label, n, e_c, e_f, allowed))
        assert e_f <= allowed, (label, n, e_f, e_c)


def _gout(T, seed):
    return torch.randn(T, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(DEV)


# (a dtype, s dtype, g dtype, da dtype, ds dtype, extra stride of a / s / g / da / ds, offset from the 16-byte grid)
VARIANTS = [(F32, F32, F32, F32, F32, (0, 0, 0, 0, 0), 0), (F32, F32, F32, F32, F32, (4, 8, 12, 16, 4), 0), (F32, F32, F32, F32, F32, (3, 0, 5, 1, 7), 1),
            (F16, F32, F16, F16, F32, (0, 0, 0, 0, 0), 0), (F32, F16, F32, F32, F16, (128, 4, 0, 8, 0), 0), (F16, F16, F16, F16, F16, (0, 2, 0, 6, 2), 1),
            (F16, F16, F32, F32, F16, (8, 8, 8, 8, 8), 0)]


def _abi_case(tail, cdt, T, variant, seed):
    adt, sdt, gdt, dadt, dsdt, extra, offset = variant
    a64, s64 = LR.tail_inputs(T, seed, DEV)
    g64 = _gout(T, seed + 2)
    a, s, g = (Rows(T, dt, 128 + e, offset, x.to(dt)) for dt, e, x in ((adt, extra[0], a64), (sdt, extra[1], s64), (gdt, extra[2], g64)))
    da, ds = Rows(T, dadt, 128 + extra[3], offset), Rows(T, dsdt, 128 + extra[4], offset)
    label = "T %d hidden %d compute %s a %s s %s g %s da %s ds %s stride +%s offset %d" % (
        T, tail.hidden, *(str(d)[6:] for d in (cdt, adt, sdt, gdt, dadt, dsdt)), extra, offset)
    fused = tail.run(cdt, a, s, g, da, ds, label=label)
    assert all(torch.equal(r.v.double(), x.to(r.v.dtype).double()) for r, x in ((a, a64), (s, s64), (g, g64))), (label, "an input was written")
    av, sv, gv = a.v.contiguous(), s.v.contiguous(), g.v.contiguous()
    _four_times(label, fused, tail.comparator(cdt, av, sv, gv), tail.reference(av, sv, gv), cdt, tail.names)


# ---------------------------------------------------------------- 1. through the C ABI against float64
# a trip is 128 rows, a wave's share 32, a weight-gradient step 16 rows: T at the boundaries.  hidden 32, 64, 96: one chunk, an even and an
# odd count for the two chunk buffers and less than one group of four output tiles; 1024 is the shipped size; 0: the layer without FFN.
TRIP_T = (1, 31, 32, 33, 127, 128, 129, 257)


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 32, 64, 96, 1024])
def test_every_gradient_element_against_float64_at_the_wave_and_trip_boundaries(hidden, cdt):
    tail = _tail(hidden)
    for i, T in enumerate(TRIP_T):
        _abi_case(tail, cdt, T, VARIANTS[(i + hidden // 32) % len(VARIANTS)], seed=7 * T + hidden)
    for v in (2, 5, 4):                                                                          # the scalar access path and the widest strides
        _abi_case(tail, cdt, 129, VARIANTS[v], seed=11 + hidden + v)


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
def test_three_chunks_with_a_partial_last_slice_and_trip(cdt):
    _abi_case(_tail(32), cdt, 2 * CHUNK + 33, VARIANTS[1 if cdt == F32 else 3], seed=5)


def test_t_zero_zero_fills_the_parameter_gradients():
    tail = _tail(64)
    empty = lambda: Rows(0, F32)
    got = tail.run(F32, empty(), empty(), empty(), empty(), empty(), label="T 0")
    assert all((got[n] == 0).all() for n in PARAMS)


# ---------------------------------------------------------------- 2. optional gradients
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 96])
def test_each_gradient_alone_has_the_bits_it_has_among_all(hidden, cdt):
    tail = _tail(hidden)
    a, s = (t.to(F32) for t in LR.tail_inputs(200, 31, DEV))
    g = _gout(200, 33).to(F32)
    everything = tail.dense(cdt, a, s, g)
    assert set(everything) == set(tail.names)
    for n in tail.names:
        alone = tail.dense(cdt, a, s, g, want=[n])
        assert list(alone) == [n] and torch.equal(_bits(alone[n]), _bits(everything[n])), n
    assert tail.dense(cdt, a, s, g, want=[]) == {}                                               # all NULL: nothing is written (the guards are checked)


# ---------------------------------------------------------------- 3. reproducibility and row isolation
@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 96])
def test_two_runs_agree_and_a_row_has_the_same_bits_alone_and_elsewhere(hidden, cdt):
    tail = _tail(hidden)
    a, s = (t.to(F32) for t in LR.tail_inputs(200, 11, DEV))
    g = _gout(200, 13).to(F32)
    whole, again = tail.dense(cdt, a, s, g), tail.dense(cdt, a, s, g)
    for n in tail.names:
        assert torch.equal(_bits(whole[n]), _bits(again[n])), (n, "two runs of the same call differ")
    oa, os_ = (t.to(F32) for t in LR.tail_inputs(50, 12, DEV))
    og = _gout(50, 14).to(F32)
    for i in (0, 31, 37, 127, 128, 199):
        alone = tail.dense(cdt, a[i: i + 1], s[i: i + 1], g[i: i + 1], want=["da", "ds"])
        oa[13], os_[13], og[13] = a[i], s[i], g[i]
        moved = tail.dense(cdt, oa, os_, og, want=["da", "ds"])
        for n in ("da", "ds"):
            assert torch.equal(_bits(alone[n][0]), _bits(whole[n][i])), (i, n, "alone")
            assert torch.equal(_bits(moved[n][13]), _bits(whole[n][i])), (i, n, "at another position")


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("hidden", [0, 96])
@pytest.mark.parametrize("where", ["g", "a"])
def test_a_nan_stays_in_its_row_and_reaches_the_parameter_gradients(where, hidden, cdt):
    tail = _tail(hidden)
    a, s = (t.to(F32) for t in LR.tail_inputs(70, 21, DEV))
    g = _gout(70, 23).to(F32)
    clean = tail.dense(cdt, a, s, g)
    a2, g2 = a.clone(), g.clone()
    (a2 if where == "a" else g2)[37, 85] = float("nan")
    got = tail.dense(cdt, a2, s, g2)
    rest = torch.arange(70, device=DEV) != 37
    for n in ("da", "ds"):
        assert torch.equal(_bits(got[n][rest]), _bits(clean[n][rest])), (n, "another row changed")
    assert torch.isnan(got["da"][37]).all()
    if hidden:
        assert torch.isnan(got["ds"][37]).all()
    elif where == "g":                                                                           # ds = g: the NaN of g is one element's
        assert torch.isnan(got["ds"][37]).sum() == 1 and torch.isnan(got["ds"][37, 85])
    assert torch.isnan(got["dWm"]).any() and torch.isnan(got["dln1_w"]).any()


@pytest.mark.parametrize("cdt", [F32, F16], ids=["f32", "f16"])
def test_large_pre_activations_give_finite_gradients(cdt):
    """z of +-30 .. +-1e4: s carries the magnitude into W1 [s ; n1] (float16 operands hold 1e4)."""
    tail = _tail(96)
    a, s = (t.to(F32) for t in LR.tail_inputs(64, 41, DEV))
    g = _gout(64, 43).to(F32)
    scale = torch.logspace(1.65, 4.15, 64, device=DEV).view(64, 1)                                # |s| = 45 .. 14000: z has a deviation of 0.7 |s|
    s = (torch.sign(s) * scale).to(F32)
    z = torch.cat([s.double(), torch.zeros_like(s).double()], -1) @ tail.w64[2].t()
    assert z.abs().max() >= 1e4 and (z.abs().amax(1) > 30).all()
    got = tail.dense(cdt, a, s, g)
    for n in tail.names:
        assert torch.isfinite(got[n]).all(), n


# ---------------------------------------------------------------- 4. the memory contract
def test_the_forward_keeps_its_output_only_and_the_backward_peaks_at_its_scratch():
    from igs_amd import tokens as TK
    T, hidden = CHUNK + 640, 1024
    tail = _tail(hidden)
    a, s = (t.to(F32) for t in LR.tail_inputs(T, 51, DEV))
    g = _gout(T, 53).to(F32)
    pack, pack_t = TK.pack_layer_tail(tail.layer, F32, transposed=True)
    slack = 8 << 20                                                                              # the allocator rounds a large block up to 2 MB: four such blocks

    def rise(fn, layer):
        leaves = [a.clone().requires_grad_(True), s.clone().requires_grad_(True)]
        for p in layer.parameters():
            p.grad = None
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        out = fn(*leaves)
        torch.cuda.synchronize()
        after_forward = torch.cuda.memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        out.backward(g)
        torch.cuda.synchronize()
        return after_forward, torch.cuda.max_memory_allocated() - base

    fwd, peak = rise(lambda x, y: TK.layer_tail_autograd(x, y, tail.layer, packed=pack, packed_t=pack_t, compute_dtype=F32), tail.layer)
    cmp_layer = copy.deepcopy(tail.layer)
    cmp_fwd, cmp_peak = rise(lambda x, y: TK._layer_tail_unfused(cmp_layer, x, y), cmp_layer)
    out_bytes = T * 128 * 4
    grads = 2 * out_bytes + 4 * sum(p.numel() for p in TK._tail_params(tail.layer)) + out_bytes      # da, ds, the parameters', and d out itself
    scratch = tail.scratch_bytes(T, F32)
    print("T %d hidden %d float32: after the forward +%.1f MB fused (output %.1f MB), +%.1f MB unfused; backward peak +%.1f MB fused "
          "(scratch %.1f MB + gradients %.1f MB), +%.1f MB unfused" % (T, hidden, fwd / 1e6, out_bytes / 1e6, cmp_fwd / 1e6, peak / 1e6, scratch / 1e6,
                                                                       grads / 1e6, cmp_peak / 1e6))
    assert out_bytes <= fwd <= out_bytes + (2 << 20)
    assert peak <= out_bytes + scratch + grads + slack
    assert scratch == tail.scratch_bytes(4 * T, F32)


# ---------------------------------------------------------------- 5. the bound module
def _force_native(monkeypatch, on=True):
    from igs_amd import tokens as TK
    monkeypatch.setattr(TK, "LAYER_TAIL_FFN_MIN_FILL", {F32: 0.0, F16: 0.0})
    monkeypatch.setattr(TK, "LAYER_TAIL_BWD_NATIVE", {F32: on, F16: on})
    calls, real = [], TK.layer_tail_autograd

    def counted(*args, **kw):
        calls.append(kw.get("compute_dtype"))
        return real(*args, **kw)

    monkeypatch.setattr(TK, "layer_tail_autograd", counted)
    return calls


def _step(module, inputs, gout, **kw):
    """out, the input gradients and every parameter's .grad after one forward + backward()."""
    for p in module.parameters():
        p.grad = None
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = module(*leaves, **kw)
    out.backward(gout.to(out.dtype))
    assert all(p.grad is not None for p in module.parameters()), "a .grad was not filled"
    return [out.detach()] + [t.grad.detach() for t in leaves] + [p.grad.detach().clone() for p in module.parameters()]


def _double(module, inputs, gout, kw):
    return _step(copy.deepcopy(module).double(), [t.double() for t in inputs], gout.double(), **{k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()})


def _within(label, native, cmp_, want, autocast):
    for i, (x, y, w) in enumerate(zip(native, cmp_, want)):
        e_n, e_c = GR.rel(x, w), GR.rel(y, w)
        allowed = GR.allowed(e_c, F16 if autocast else F32)
        print("%s tensor %d: unfused %.3e, native %.3e (allowed %.3e)" % (label, i, e_c, e_n, allowed))
        assert x.dtype == y.dtype and e_n <= allowed, (label, i, e_n, e_c)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("no_ffn", [True, False])
def test_bound_for_training_every_grad_is_within_the_rule_also_after_a_step(no_ffn, autocast, monkeypatch):
    from igs_amd import tokens as TK
    layer, inputs, gout, kw = _layer_case(no_ffn, True, seed=1)
    other, plain = copy.deepcopy(layer), copy.deepcopy(layer)                                    # plain stays unbound: the float64 run
    calls = _force_native(monkeypatch)
    assert TK.use_native_layer_tails(layer, training=True) == 1 and TK.use_native_transformer_layers(other) == 1
    for round_ in range(2):
        plain.load_state_dict(other.state_dict())
        want = _double(plain, inputs, gout, kw)
        with torch.autocast("cuda", dtype=F16, enabled=autocast):
            native, cmp_ = _step(layer, inputs, gout, **kw), _step(other, inputs, gout, **kw)
        assert calls == [F16 if autocast else F32] * (round_ + 1), "the bound forward must take the native training route once per step"
        _within("bound no_ffn %d autocast %d round %d" % (no_ffn, autocast, round_), native, cmp_, want, autocast)
        entry = layer.__dict__[TK.TAIL_CACHE][F16 if autocast else F32]
        with torch.no_grad():                                                                    # one SGD step on both, from the comparator's gradients
            for p, q in zip(layer.parameters(), other.parameters()):
                p.sub_(0.05 * q.grad)
                q.sub_(0.05 * q.grad)
    fresh = TK.pack_layer_tail(layer, F16 if autocast else F32, transposed=True)
    with torch.autocast("cuda", dtype=F16, enabled=autocast):
        _step(layer, inputs, gout, **kw)
    rebuilt = layer.__dict__[TK.TAIL_CACHE][F16 if autocast else F32]
    assert rebuilt is not entry and torch.equal(rebuilt["pack"], fresh[0]) and torch.equal(rebuilt["pack_t"], fresh[1])


@pytest.mark.parametrize("no_ffn", [True, False])
def test_chained_behind_the_native_window_attention(no_ffn, monkeypatch):
    """A 2 x 2-window stand-in layer with the native window attention in front: the gradient to the layer's inputs and parameters through the
    fused tail's backward against the same layer with the unfused tail."""
    from igs_amd import attention as AT, tokens as TK
    for name in (TK.ATTN_SPLIT, TK.ATTN_FULL):
        monkeypatch.setattr(TR, name, getattr(TR, name))                                         # (the stand-in module's names are restored afterwards)
    layer, inputs, gout, kw = _layer_case(no_ffn, True, seed=3)
    other = copy.deepcopy(layer)
    want = _double(other, inputs, gout, kw)
    calls = _force_native(monkeypatch)
    assert AT.use_native_window_attention(TR) == 2
    assert TK.use_native_layer_tails(layer, training=True) == 1 and TK.use_native_transformer_layers(other) == 1
    native, cmp_ = _step(layer, inputs, gout, **kw), _step(other, inputs, gout, **kw)
    assert calls == [F32]
    _within("chained no_ffn %d" % no_ffn, native, cmp_, want, False)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("no_ffn", [True, False])
def test_with_the_table_off_the_training_binder_routes_as_the_parent(no_ffn, autocast, monkeypatch):
    from igs_amd import tokens as TK
    layer, inputs, gout, kw = _layer_case(no_ffn, False, seed=2)
    other = copy.deepcopy(layer)
    calls = _force_native(monkeypatch, on=False)
    assert TK.LAYER_TAIL_BWD_NATIVE == {F32: False, F16: False}
    assert TK.use_native_layer_tails(layer, training=True) == 1 and TK.use_native_transformer_layers(other) == 1
    with torch.autocast("cuda", dtype=F16, enabled=autocast):
        mine, theirs = _step(layer, inputs, gout, **kw), _step(other, inputs, gout, **kw)
    assert calls == []
    for x, y in zip(mine, theirs):
        assert x.dtype == y.dtype and torch.equal(_bits(x.float()), _bits(y.float()))
