"""The two ends of Transformer1D on the MI355X (igs_amd/csrc/gnorm.hip through the C ABI and through igs_amd.tokens) against the float64
restatement of tests/transformer_ends_restatement.py on the same float32 / float16 inputs.

Every element is compared.  The allowances are derived, never measured (transformer_ends_restatement states the reasoning next to
group_norm_forward_bound and group_norm_backward_bounds).  The worst error-to-allowance ratio of every case is printed.

The C ABI cases run on PyTorch's current stream so that the test chooses where the operands lie: batch and channel strides above the
extent, row strides above C, bases one element past the 16-byte grid, and every output pre-filled with NaN inside an allocation that holds a
sentinel everywhere else (between the rows and channels too), which is checked afterwards.

The stand-in Transformer1D is compared with its float64 run: the patched float32 run may be at most 4 x as far off as the unpatched float32
PyTorch run of the same case (floor 1e-5), the rule of test_gpu_token_ops.py; errors are the largest |difference| / largest |reference|
over the output, the input gradient and every parameter gradient.

Recorded on one MI355X: worst |err| / allowance for the GroupNorm 0.35 forward, 0.25 statistics, 0.19 dx (the two-element
groups of the 600000-example case; 0.19, 0.15, 0.044 elsewhere), 0.068 dweight, 0.020 dbias in float32 and 0.989 / 0.980 for float16 results (the output's own rounding); 0.25 beside non-finite groups.  The
stand-in against its float64 run: unpatched 6.5e-7, patched 6.1e-7; under float16 autocast 2.6e-3 and 1.9e-3; at the shipped shape with
the block ops and the native attention 3.9e-6 and 4.6e-6."""
import copy

import pytest
import torch

import attention_restatement as AR
import token_ops_restatement as TR
import transformer_ends_restatement as ER

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
CODE = {F32: 0, F16: 1}
BAND = 64
SENTINEL = 12345.0
EPS = 1e-6


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _ok(rc):
    from igs_amd import _cabi
    assert rc == 0, _cabi.last_error()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Strided:
    """A view of `shape` at `strides` elements, starting BAND + offset elements into an allocation that holds SENTINEL outside the view;
    the view holds `src`, or NaN."""

    def __init__(self, shape, strides, dtype, offset=0, src=None):
        extent = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
        self.big = torch.full((2 * BAND + offset + extent + 8,), SENTINEL, dtype=dtype, device=DEV)
        self.v = self.big[BAND + offset:].as_strided(shape, strides)
        self.inside = torch.zeros_like(self.big, dtype=torch.bool)
        self.inside[BAND + offset:].as_strided(shape, strides).fill_(True)
        self.v.copy_(src if src is not None else torch.full(shape, float("nan")))

    def check(self, label):
        assert (self.big[~self.inside] == SENTINEL).all(), (label, "an element outside the operand was written")


class Cm(Strided):
    """[B, C, A] channel-major: channel stride A + channel_extra, batch stride C channel strides + batch_extra."""

    def __init__(self, B, C, A, dtype, batch_extra=0, channel_extra=0, offset=0, src=None):
        self.cs = A + channel_extra
        self.bs = C * self.cs + batch_extra
        super().__init__((B, C, A), (self.bs, self.cs, 1), dtype, offset, src)


class Tm(Strided):
    """[B, A, C] token-major rows at a stride of C + row_extra."""

    def __init__(self, B, A, C, dtype, row_extra=0, offset=0, src=None):
        self.rs = C + row_extra
        super().__init__((B, A, C), (A * self.rs, self.rs, 1), dtype, offset, src)


def _vector(n):
    return Strided((n,), (1,), F32)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _worst(got, ref, allow, label):
    assert not torch.isnan(got).any(), (label, "an element was not written")
    err = (got.double() - ref).abs()
    worst = (err / allow).max().item()
    print("%s: max |err| %.3e, max |err| / allowance %.3f" % (label, err.max().item(), worst))
    assert worst <= 1.0, (label, worst)


# ---------------------------------------------------------------- the GroupNorm through the C ABI
# B, C, G, A, x dtype, out dtype, batch extra, channel extra, row extra, offset from the 16-byte grid, affine
GN_CASES = [
    (1, 4, 1, 1, F32, F32, 0, 0, 0, 0, True), (1, 4, 2, 1, F16, F16, 0, 0, 0, 1, True),
    (2, 6, 3, 63, F32, F32, 5, 1, 2, 0, True), (2, 6, 3, 63, F16, F32, 0, 0, 0, 0, False),              # 2 channels per group
    (1, 8, 8, 33, F32, F16, 0, 3, 4, 1, True),                                                          # 1 channel per group
    (2, 12, 3, 7, F32, F32, 0, 0, 0, 0, True), (2, 12, 3, 7, F16, F16, 8, 4, 4, 0, True),
    (1, 128, 32, 64, F32, F32, 0, 0, 0, 0, True), (1, 128, 32, 64, F16, F16, 8, 4, 4, 0, True), (1, 128, 32, 64, F32, F32, 0, 0, 0, 1, True),
    (1, 128, 32, 65, F32, F32, 0, 0, 0, 0, True), (3, 128, 32, 257, F32, F16, 0, 0, 0, 0, True), (3, 128, 32, 257, F16, F32, 3, 1, 0, 0, False),
    (2, 132, 33, 67, F32, F32, 3, 1, 1, 0, True), (2, 132, 33, 68, F16, F32, 4, 4, 8, 0, True),         # C off the tile; four-element access on a part tile
    (1, 256, 32, 130, F16, F16, 0, 2, 0, 0, True),                                                      # 8 channels per group
    (1, 1024, 32, 5, F32, F32, 0, 0, 0, 0, True), (1, 1024, 32, 5, F32, F32, 0, 0, 0, 0, False),
    (1, 128, 32, 8192, F32, F32, 0, 0, 0, 0, True), (1, 128, 32, 8192, F16, F16, 0, 0, 0, 0, True),     # the shipped shape
    # more (example, group) pairs than the 2^20 workgroups of the statistics, more examples than one launch of the per-example reduction
    # takes (32768) and than one round of the d weight / d bias reduction (1024): 9.6 MB
    (600000, 4, 2, 1, F32, F32, 0, 0, 0, 0, True),
]


def _gn_fwd(x, G, w, b, out, stats, eps=EPS):
    B, C, A = x.v.shape
    _ok(_lib().igs_group_norm_tokens_fwd(_stream(), B, C, G, A, CODE[x.v.dtype], x.v.data_ptr(), x.bs, x.cs, w.data_ptr() if w is not None else None,
                                         b.data_ptr() if b is not None else None, eps, CODE[out.v.dtype], out.v.data_ptr(), out.rs, stats.v.data_ptr()))


def _gn_bwd(x, G, w, stats, g, dx, dw, db, scratch):
    B, C, A = x.v.shape
    _ok(_lib().igs_group_norm_tokens_bwd(_stream(), B, C, G, A, CODE[x.v.dtype], x.v.data_ptr(), x.bs, x.cs, w.data_ptr() if w is not None else None,
                                         stats.v.data_ptr(), CODE[g.v.dtype], g.v.data_ptr(), g.rs, CODE[dx.v.dtype] if dx else 0,
                                         dx.v.data_ptr() if dx else None, dx.bs if dx else C * A, dx.cs if dx else A, dw.v.data_ptr() if dw else None,
                                         db.v.data_ptr() if db else None, scratch.data_ptr() if scratch is not None else None))


def _scratch(B, C, G, A, extra=0):
    return torch.empty(_lib().igs_group_norm_tokens_bwd_scratch_bytes(B, C, G, A) + extra, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "B%d-C%d-G%d-A%d-%s-%s-b%d-c%d-r%d-o%d-a%d" % (c[0], c[1], c[2], c[3], str(c[4])[11:], str(c[5])[11:],
                                                                                                       c[6], c[7], c[8], c[9], int(c[10])))
def test_group_norm_forward_and_backward_against_float64(case):
    B, C, G, A, xdt, odt, bx, cx, rx, offset, affine = case
    seed = 3 * A + C
    label = "B %d C %d G %d A %d %s -> %s strides +%d +%d +%d offset %d affine %d" % (B, C, G, A, str(xdt)[6:], str(odt)[6:], bx, cx, rx, offset, affine)
    x = Cm(B, C, A, xdt, bx, cx, offset, ER.group_inputs(B, C, G, A, xdt, DEV, seed))
    w, b = TR.affine_inputs(C, DEV, seed) if affine else (None, None)
    w64, b64 = (w.double(), b.double()) if affine else (None, None)
    x64 = x.v.double()
    out, stats = Tm(B, A, C, odt, rx, offset), _vector(B * G * 2)
    _gn_fwd(x, G, w, b, out, stats)
    for t in (out, stats, x):
        t.check(label)
    _worst(out.v, ER.group_norm_tokens_restate(x64, G, w64, b64, EPS), ER.group_norm_forward_bound(x.v, G, w, b, EPS, odt), label + " forward")
    _worst(stats.v.view(B, G, 2), ER.group_norm_stats_restate(x64, G, EPS), ER.group_norm_stats_bound(x.v, G, EPS), label + " stats")
    # backward: dout in out's dtype at its own stride, dx in x's dtype at strides of its own; two runs bit for bit
    g = Tm(B, A, C, odt, rx, offset, torch.randn(B, A, C, generator=torch.Generator().manual_seed(seed + 1)).to(odt).to(DEV))
    want = ER.group_norm_tokens_backward_restate(x64, G, w64, EPS, g.v.double())
    bounds = ER.group_norm_backward_bounds(x.v, G, w, EPS, g.v, xdt)
    scratch = _scratch(B, C, G, A, 1)
    runs = []
    for _ in range(2):
        dx = Cm(B, C, A, xdt, 2 * bx, 3 * cx, offset)
        dw, db = _vector(C), _vector(C)
        _gn_bwd(x, G, w, stats, g, dx, dw, db, scratch[1:])
        for t in (dx, dw, db, g, stats):
            t.check(label)
        runs.append((dx.v.clone(), dw.v.clone(), db.v.clone()))
    for a, c in zip(*runs):
        assert torch.equal(_bits(a), _bits(c)), (label, "two backward runs differ")
    for got, r_, k in zip(runs[0], want, ("dx", "dweight", "dbias")):
        _worst(got, r_, bounds[k], label + " " + k)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("shape", [(2, 12, 3, 7), (2, 128, 32, 64), (1, 256, 32, 130)])
def test_a_nan_group_is_all_nan_and_a_constant_group_is_exactly_bias(shape, dtype):
    B, C, G, A = shape
    cpg = C // G
    src = ER.group_inputs(B, C, G, A, dtype, DEV, seed=C, constant_group=(0, 1))
    src[0, 2 * cpg + cpg // 2, (2 * A) // 3] = float("nan")                                      # group (0, 2)
    src[B - 1, 0, A // 2] = float("inf")                                                         # group (B - 1, 0)
    w, b = TR.affine_inputs(C, DEV, C)
    x, out, stats = Cm(B, C, A, dtype, src=src), Tm(B, A, C, F32), _vector(B * G * 2)
    _gn_fwd(x, G, w, b, out, stats)
    out.check("non-finite groups")
    y = out.v.permute(0, 2, 1).reshape(B, G, cpg * A)
    assert torch.isnan(y[0, 2]).all() and torch.isnan(y[B - 1, 0]).all()
    assert torch.equal(out.v[0, :, cpg:2 * cpg], b[cpg:2 * cpg].expand(A, cpg)), "a constant group must give exactly bias"
    finite = torch.ones(B, G, dtype=torch.bool, device=DEV)
    finite[0, 2] = finite[B - 1, 0] = False
    ref = ER.group_norm_tokens_restate(src.double(), G, w.double(), b.double(), EPS).permute(0, 2, 1).reshape(B, G, -1)
    allow = ER.group_norm_forward_bound(src, G, w, b, EPS).permute(0, 2, 1).reshape(B, G, -1)
    _worst(y[finite], ref[finite], allow[finite], "B %d C %d G %d A %d %s beside non-finite groups" % (B, C, G, A, str(dtype)[6:]))


@pytest.mark.parametrize("shape", [(2, 12, 3, 7), (1, 128, 32, 64)])
def test_every_optional_gradient_left_out_in_turn(shape):
    B, C, G, A = shape
    x = Cm(B, C, A, F32, src=ER.group_inputs(B, C, G, A, F32, DEV, seed=C))
    g = Tm(B, A, C, F32, src=torch.randn(B, A, C, device=DEV))
    w, b = TR.affine_inputs(C, DEV, C)
    out, stats = Tm(B, A, C, F32), _vector(B * G * 2)
    _gn_fwd(x, G, w, b, out, stats)
    scratch = _scratch(B, C, G, A)

    def run(want):
        outs = [Cm(B, C, A, F32) if want[0] else None, _vector(C) if want[1] else None, _vector(C) if want[2] else None]
        _gn_bwd(x, G, w, stats, g, outs[0], outs[1], outs[2], scratch)
        for o in outs:
            if o:
                o.check(want)
                assert not torch.isnan(o.v).any(), want
        return [o.v.clone() if o else None for o in outs]

    full = run((True, True, True))
    for want in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False), (False, False, True)):
        for a, c in zip(run(want), full):
            assert a is None or torch.equal(a, c), want


# ---------------------------------------------------------------- the residual add through the C ABI
# B, C, A, tok dtype, res dtype, out dtype, batch extra, channel extra, row extra, offset
ADD_CASES = [(1, 4, 1, F32, F32, F32, 0, 0, 0, 0), (2, 6, 63, F16, F32, F32, 5, 1, 2, 0), (1, 8, 33, F32, F16, F16, 0, 3, 4, 1), (2, 12, 7, F16, F16, F16, 0, 0, 0, 0),
             (1, 128, 64, F32, F32, F32, 0, 0, 0, 0), (1, 128, 64, F16, F16, F16, 8, 4, 4, 0), (1, 128, 65, F32, F32, F32, 0, 0, 0, 1),
             (3, 128, 257, F32, F16, F32, 0, 0, 0, 0), (2, 132, 67, F32, F32, F16, 3, 1, 1, 0), (2, 132, 68, F16, F32, F32, 4, 4, 8, 0),
             (1, 256, 130, F32, F32, F32, 0, 2, 0, 0), (1, 1024, 5, F32, F32, F32, 0, 0, 0, 0), (1, 128, 8192, F32, F32, F32, 0, 0, 0, 0),
             (1, 128, 8192, F16, F32, F32, 0, 0, 0, 0)]


@pytest.mark.parametrize("case", ADD_CASES, ids=lambda c: "B%d-C%d-A%d-%s-%s-%s-b%d-c%d-r%d-o%d" % (c[0], c[1], c[2], str(c[3])[11:], str(c[4])[11:], str(c[5])[11:],
                                                                                                   c[6], c[7], c[8], c[9]))
def test_tokens_add_residual_gives_the_bits_of_the_float32_sum_rounded_once(case):
    B, C, A, tdt, rdt, odt, bx, cx, rx, offset = case
    g = torch.Generator().manual_seed(A + C)
    tok = Tm(B, A, C, tdt, rx, offset, (3 * torch.randn(B, A, C, generator=g)).to(tdt).to(DEV))
    res = Cm(B, C, A, rdt, bx, cx, offset, (30 * torch.randn(B, C, A, generator=g) + 100).to(rdt).to(DEV))
    out = Tm(B, A, C, odt, 2 * rx, offset)
    _ok(_lib().igs_tokens_add_residual(_stream(), B, C, A, CODE[tdt], tok.v.data_ptr(), tok.rs, CODE[rdt], res.v.data_ptr(), res.bs, res.cs, CODE[odt],
                                       out.v.data_ptr(), out.rs))
    for t in (out, tok, res):
        t.check(case)
    want = (tok.v.float() + res.v.float().permute(0, 2, 1)).to(odt)
    assert torch.equal(_bits(out.v), _bits(want)), case


# ---------------------------------------------------------------- the Python layer: autograd, views, dtypes
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("sliced", [False, True])
def test_group_norm_tokens_autograd_against_float64(sliced, dtype):
    from igs_amd import tokens as TK
    B, C, G, A = 2, 32, 4, 70
    wide = ER.group_inputs(B, 3 * C, 3 * G, A + 6, dtype, DEV, seed=11)
    x = (wide[:, C: 2 * C, 2: A + 2] if sliced else wide[:, C: 2 * C, 2: A + 2].contiguous()).detach().requires_grad_(True)
    w, b = (t.requires_grad_(True) for t in TR.affine_inputs(C, DEV, 13))
    g = torch.randn(B, A, C, device=DEV).to(dtype)
    out = TK.group_norm_tokens(x, G, w, b, EPS)
    assert out.dtype == dtype and out.shape == (B, A, C) and out.is_contiguous()
    saved = out.grad_fn.saved_tensors
    assert saved[0].data_ptr() == x.data_ptr() and tuple(saved[2].shape) == (B, G, 2), "x is saved as it is, with the [B, G, 2] statistics"
    dx, dw, db = torch.autograd.grad(out, (x, w, b), g)
    xd, wd, bd = x.detach(), w.detach(), b.detach()
    label = "sliced %d %s " % (sliced, str(dtype)[6:])
    _worst(out.detach(), ER.group_norm_tokens_restate(xd.double(), G, wd.double(), bd.double(), EPS), ER.group_norm_forward_bound(xd, G, wd, bd, EPS, dtype),
           label + "forward")
    want = ER.group_norm_tokens_backward_restate(xd.double(), G, wd.double(), EPS, g.double())
    bounds = ER.group_norm_backward_bounds(xd, G, wd, EPS, g, dtype)
    for got, r, k in zip((dx, dw, db), want, ("dx", "dweight", "dbias")):
        _worst(got, r, bounds[k], label + k)
    assert dx.dtype == dtype and dx.shape == x.shape and dw.dtype == F32
    g2 = torch.randn(B, C, A, device=DEV).to(dtype).permute(0, 2, 1)                             # an upstream gradient that is not token-major: copied once
    (dx2,) = torch.autograd.grad(TK.group_norm_tokens(x, G, w, b, EPS), (x,), g2)
    _worst(dx2, ER.group_norm_tokens_backward_restate(xd.double(), G, wd.double(), EPS, g2.double())[0],
           ER.group_norm_backward_bounds(xd, G, wd, EPS, g2, dtype)["dx"], label + "dx from a permuted gradient")
    with torch.no_grad():                                                                        # nothing saved, another out dtype
        y = TK.group_norm_tokens(x, G, w, b, EPS, out_dtype=F32)
    assert y.dtype == F32 and y.grad_fn is None
    plain = TK.group_norm_tokens(xd, G)                                                          # no affine step, the default eps
    _worst(plain, ER.group_norm_tokens_restate(xd.double(), G, None, None, 1e-5), ER.group_norm_forward_bound(xd, G, None, None, 1e-5, dtype), label + "no affine")


def test_group_norm_tokens_reads_the_lift_layout_in_place_and_allocates_only_the_statistics():
    """x as GridEncoder hands it over: the [B, C, A] buffer behind the lift's permuted [B, A, C] view, permuted back."""
    from igs_amd import tokens as TK
    B, C, G, A = 1, 128, 32, 8192
    buf = ER.group_inputs(B, C, G, A, F32, DEV, seed=1)
    x = buf.permute(0, 2, 1).permute(0, 2, 1)
    assert TK._channel_major(x).data_ptr() == buf.data_ptr() and TK._channel_major(buf[:, 32:96]).data_ptr() == buf[:, 32:96].data_ptr()
    assert TK._channel_major(buf.permute(0, 2, 1)).data_ptr() != buf.data_ptr()                  # (token-major memory is copied)
    w, b = TR.affine_inputs(C, DEV, 2)
    with torch.no_grad():
        TK.group_norm_tokens(x, G, w, b, EPS)                                                    # (the library and the module are loaded)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = TK.group_norm_tokens(x, G, w, b, EPS)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    print("peak bytes above the operands: %d (the result: %d)" % (peak, out.numel() * 4))
    assert out.numel() * 4 <= peak <= out.numel() * 4 + 4096, "the result and the [B, G, 2] statistics, nothing else"


@pytest.mark.parametrize("tdt,rdt", [(F32, F32), (F16, F32), (F16, F16)])
def test_add_residual_tokens_view_contract_and_free_backward(tdt, rdt):
    from igs_amd import tokens as TK
    B, C, A = 2, 36, 70
    g = torch.Generator().manual_seed(5)
    tok = torch.randn(B, A, C, generator=g).to(tdt).to(DEV).requires_grad_(True)
    res = torch.randn(B, C, A, generator=g).to(rdt).to(DEV).requires_grad_(True)
    out = TK.add_residual_tokens(tok, res)
    odt = torch.promote_types(tdt, rdt)
    assert out.shape == (B, C, A) and out.dtype == odt and out.permute(0, 2, 1).is_contiguous() and out.stride() == (A * C, 1, C)
    want = (tok.detach().float().permute(0, 2, 1) + res.detach().float()).to(odt)
    assert torch.equal(_bits(out.detach().contiguous()), _bits(want))
    up = torch.randn(B, C, A, device=DEV).to(odt)
    dtok, dres = torch.autograd.grad(out, (tok, res), up)
    assert dtok.dtype == tdt and dres.dtype == rdt and torch.equal(dtok, up.permute(0, 2, 1).to(tdt)) and torch.equal(dres, up.to(rdt))
    if tdt == rdt:
        assert dres.data_ptr() == up.data_ptr() and dtok.data_ptr() == up.data_ptr(), "the backward hands the upstream gradient on: no launch, no copy"
    sliced = torch.randn(B, A, 2 * C, device=DEV).to(tdt)[..., C:]                               # rows of a wider buffer, read in place
    assert TK._token_major(sliced).data_ptr() == sliced.data_ptr()
    with torch.no_grad():
        y = TK.add_residual_tokens(sliced, res)
    assert torch.equal(y, (sliced.float().permute(0, 2, 1) + res.detach().float()).to(odt)) and y.grad_fn is None


def test_tensors_on_different_devices_are_refused():
    from igs_amd import tokens as TK
    x = torch.randn(2, 16, 5, device=DEV)
    w, b = TR.affine_inputs(16, DEV, 0)
    with pytest.raises(RuntimeError, match="one GPU"):
        TK.group_norm_tokens(x, 4, w.cpu(), b.cpu())
    with pytest.raises(RuntimeError, match="one GPU"):
        TK.add_residual_tokens(torch.randn(2, 5, 16, device=DEV), x.cpu())


# ---------------------------------------------------------------- the stand-in Transformer1D, patched against its float64 run
def _run(module, x, gout):
    """(output, input gradient, parameter gradients) as a flat list of detached tensors."""
    leaf = x.detach().clone().requires_grad_(True)
    out = module(leaf)
    grads = torch.autograd.grad(out, [leaf] + list(module.parameters()), gout.to(out.dtype))
    return [out.detach()] + [g.detach() for g in grads]


def _error(got, want):
    return max(((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(got, want))


def _four_times_rule(label, eager, native, want, floor=1e-5):
    e_eager, e_native = _error(eager, want), _error(native, want)
    print("%s: max relative |err| against float64: unpatched PyTorch %.3e, patched %.3e (allowed %.3e)" % (label, e_eager, e_native, max(4 * e_eager, floor)))
    assert all(torch.isfinite(t).all() for t in native), label
    assert [t.dtype for t in native] == [t.dtype for t in eager], (label, "dtypes differ from eager PyTorch")
    assert [t.shape for t in native] == [t.shape for t in eager], label
    assert e_native <= max(4 * e_eager, floor), (label, e_native, e_eager)


class BlockAttention(AR.AttentionStandIn):
    """The attention stand-in with an eager path of its own while no processor is set."""

    def __init__(self, channels, heads=2, seed=0):
        super().__init__(channels=channels, heads=heads, seed=seed)

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None):
        if self.processor is None:
            return self.restated(hidden_states)
        return super().forward(hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask)


def _case(C, G, A, inner, heads, seed):
    g = torch.Generator().manual_seed(80 + seed)
    x = (2.0 * torch.randn(1, C, A, generator=g) + 0.5).to(DEV)
    gout = torch.randn(1, C, A, generator=g).to(DEV)
    model = ER.make_transformer(C, G, inner, 1, seed=seed, make_attention=lambda dim: BlockAttention(dim, heads=heads, seed=seed)).to(DEV)
    return model, x, gout


def _three_runs(make, install, autocast=False):
    module, x, gout = make()
    want = _run(copy.deepcopy(module).double(), x.double(), gout.double())
    keys = list(module.state_dict().keys())
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        eager = _run(module, x, gout)
        install(module)
        native = _run(module, x, gout)
        with torch.no_grad():
            y = module(x)
    assert list(module.state_dict().keys()) == keys
    assert y.permute(0, 2, 1).is_contiguous() and y.shape == x.shape, "a [B, C, A]-shaped view of a token-major buffer"
    return eager, native, want


@pytest.mark.parametrize("autocast", [False, True])
def test_stand_in_transformer_patched_against_its_float64_run(autocast):
    """in 16, 4 groups, 70 anchors, one block of 2 heads x 8.  Under float16 autocast the norm answers in float32 and the output is float32,
    as eager PyTorch's are."""
    from igs_amd import tokens as TK
    eager, native, want = _three_runs(lambda: _case(16, 4, 70, 16, 2, 0), lambda m: TK.use_native_transformer_ends(m) == 1 or pytest.fail("count"), autocast)
    _four_times_rule("transformer ends autocast %d" % autocast, eager, native, want, floor=2e-3 if autocast else 1e-5)


def test_shipped_shape_composes_with_the_block_ops_and_the_native_attention():
    """in 128, 32 groups, 8192 anchors, one block of 8 heads x 64: GridEncoder.conv's sizes with every native binder on."""
    from igs_amd import attention as AT, tokens as TK

    def install(m):
        assert TK.use_native_transformer_ends(m) == 1 and TK.use_native_block_ops(m) == 3 and AT.use_native_attention(m) == 1

    eager, native, want = _three_runs(lambda: _case(128, 32, 8192, 512, 8, 2), install)
    _four_times_rule("shipped shape with every native binder", eager, native, want)
