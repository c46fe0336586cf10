"""The transformers' LayerNorm and GEGLU on the MI355X (igs_amd/csrc/tokens.hip through the C ABI and through igs_amd.tokens) against the
float64 restatement of tests/token_ops_restatement.py on the same float32 / float16 inputs.

Every element is compared.  The allowances are derived, never measured (token_ops_restatement states the reasoning next to
layer_norm_forward_bound, layer_norm_backward_bounds, geglu_forward_allowance and geglu_backward_allowance).  The worst error-to-allowance
ratio of every case is printed.

The C ABI cases run on PyTorch's current stream so that the test chooses where the operands lie: rows at a stride above their length (a
slice of a wider buffer), bases one element past the 16-byte grid, and every output pre-filled with NaN inside an allocation that holds a
sentinel everywhere else (between the rows too), which is checked afterwards.

The stand-in modules (TransformerLayer, BasicTransformerBlock of token_ops_restatement) are compared with their float64 runs: the patched
float32 run may be at most 4 x as far off as the unpatched float32 PyTorch run of the same case (floor 1e-5), the rule of
test_gpu_encoder_norms.py; errors are the largest |difference| / largest |reference| over the output, the input gradients and every
parameter gradient.

Recorded on one MI355X: worst |err| / allowance for LayerNorm 0.50 forward, 0.15 dx, 0.12 dweight, 0.19 dbias in
float32 and 0.994 / 0.987 in float16 (the output's own rounding); for GEGLU 0.18 forward, 0.23 backward in float32 and 0.997 / 0.996 in
float16.  Stand-ins, relative error against the float64 run: layer unpatched 6.8e-7 to 9.5e-7, patched 6.9e-7 to 1.07e-6; block (two heads) 1.70e-6 and
1.86e-6; under float16 autocast layer 1.06e-3 to 1.71e-3 on both sides, block 1.76e-3 unpatched and 1.29e-3 patched; with the native window
attention 8.1e-7 / 1.04e-6, with the native anchor attention (eight heads of 64) 1.30e-6.  The LayerNorm rows at the capacities of the
lane shapes, their neighbours and the widths off the grid of four: 0.50 forward, 0.11 dx, 0.11 dweight, 0.19 dbias
in float32 and 0.998 / 0.984 in float16."""
import copy

import pytest
import torch
import torch.nn.functional as F

import attention_restatement as AR
import token_ops_restatement as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
CODE = {F32: 0, F16: 1}
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


class Rows:
    """[N, C] rows at `stride` elements, starting BAND + offset elements into an allocation that holds SENTINEL outside the rows."""

    def __init__(self, N, C, dtype, stride=None, offset=0, src=None):
        stride = C if stride is None else stride
        self.big = torch.full((2 * BAND + offset + max(N, 1) * stride + 8,), SENTINEL, dtype=dtype, device=DEV)
        self.v = self.big[BAND + offset:].as_strided((N, C), (stride, 1))
        self.inside = torch.zeros_like(self.big, dtype=torch.bool)
        self.inside[BAND + offset:].as_strided((N, C), (stride, 1)).fill_(True)
        self.v.copy_(src if src is not None else torch.full((N, C), float("nan")))
        self.stride = stride

    def check(self, label):
        assert (self.big[~self.inside] == SENTINEL).all(), (label, "an element outside the rows was written")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _worst(got, ref, allow, label):
    assert not torch.isnan(got).any(), (label, "an element was not written")
    err = (got.double() - ref).abs()
    worst = (err / allow).max().item()
    print("%s: max |err| %.3e, max |err| / allowance %.3f" % (label, err.max().item(), worst))
    assert worst <= 1.0, (label, worst)


# ---------------------------------------------------------------- LayerNorm through the C ABI
# N, C, x dtype, out dtype, residual ("none" | "own" | "alias"), residual dtype, extra row stride, offset from the 16-byte grid, affine
LN_CASES = [
    (1, 4, F32, F32, "none", F32, 0, 0, True), (3, 4, F16, F16, "own", F16, 0, 0, True), (67, 4, F32, F32, "alias", F32, 4, 1, True),
    (1, 12, F16, F32, "own", F32, 0, 1, True), (257, 12, F32, F32, "none", F32, 3, 0, False), (3, 12, F32, F32, "own", F16, 0, 0, True),
    (3, 128, F32, F32, "own", F32, 0, 0, True), (67, 128, F16, F16, "none", F16, 128, 0, True), (257, 128, F32, F32, "alias", F32, 0, 0, True),
    (67, 128, F16, F32, "own", F32, 4, 1, False), (1, 128, F32, F32, "none", F32, 0, 1, True),
    (3, 132, F32, F32, "none", F32, 0, 0, True), (67, 132, F16, F16, "alias", F16, 8, 0, True), (257, 132, F32, F32, "own", F16, 1, 0, True),
    (1, 512, F16, F16, "none", F16, 0, 0, True), (67, 512, F32, F32, "own", F32, 0, 0, True), (257, 512, F32, F32, "none", F32, 512, 0, True),
    (257, 512, F16, F32, "alias", F32, 0, 1, True), (3, 512, F32, F32, "none", F32, 0, 0, False),
    (3, 1024, F32, F32, "alias", F32, 0, 0, True), (67, 1024, F16, F16, "own", F16, 16, 0, True), (257, 1024, F32, F32, "none", F32, 0, 1, True),
    (4200, 132, F32, F32, "own", F32, 0, 0, True),                                              # more row groups than workgroups in the backward
    # the capacity of each (lanes per row, groups per lane) shape of LN_LAUNCH in igs_amd/csrc/tokens.hip and the first width of the next
    # one, each in the four-element form and (a stride extra off the grid of four, or offset 1) in the scalar form of the same shape:
    # 64 fills (16, 1), 68 opens (16, 2); 256 fills (64, 1), 260 opens (64, 2); 516 opens (64, 4)   (128 | 132, 512 and 1024 are above)
    (3, 64, F32, F32, "own", F32, 0, 0, True), (67, 64, F16, F16, "alias", F16, 4, 1, True), (257, 64, F16, F32, "none", F32, 0, 0, False),
    (67, 68, F32, F32, "alias", F32, 0, 0, True), (3, 68, F16, F16, "own", F16, 1, 0, True),
    (3, 256, F16, F16, "own", F16, 0, 0, True), (67, 256, F32, F32, "alias", F32, 0, 1, True), (257, 256, F32, F32, "none", F32, 256, 0, True),
    (67, 260, F32, F32, "own", F32, 0, 0, True), (3, 260, F16, F32, "alias", F32, 2, 0, True),
    (3, 516, F32, F32, "alias", F32, 0, 0, True), (67, 516, F16, F16, "own", F16, 4, 1, True), (257, 516, F16, F32, "none", F32, 0, 0, True),
    # widths that are no multiple of four take the scalar form whatever the addresses, with a last group that is partly outside the row: the
    # first width of each scalar shape (1, 65, 129, 257, 513) and the last widths of the smallest and the largest one (63, 1023)
    (3, 1, F32, F32, "own", F32, 0, 0, True), (67, 63, F16, F16, "none", F16, 0, 0, True), (67, 65, F32, F32, "none", F32, 0, 0, True),
    (3, 129, F16, F16, "own", F16, 0, 0, True), (67, 257, F32, F32, "alias", F32, 0, 0, True), (3, 513, F32, F32, "own", F32, 3, 0, False),
    (67, 1023, F16, F32, "none", F32, 0, 1, True),
]


def _ln_operands(case, seed):
    N, C, xdt, odt, res, rdt, extra, offset, affine = case
    x = Rows(N, C, xdt, C + extra, offset, TR.row_inputs(N, C, xdt, DEV, seed))
    r = Rows(N, C, odt if res == "alias" else rdt, C + extra, offset, TR.row_inputs(N, C, rdt, DEV, seed + 5)) if res != "none" else None
    w, b = TR.affine_inputs(C, DEV, seed) if affine else (None, None)
    return x, r, w, b


def _ln_fwd(x, r, w, b, out, eps=1e-5):
    N, C = x.v.shape
    _ok(_lib().igs_layer_norm_fwd(_stream(), N, C, CODE[x.v.dtype], x.v.data_ptr(), x.stride, CODE[r.v.dtype] if r else 0, r.v.data_ptr() if r else None,
                                  r.stride if r else C, w.data_ptr() if w is not None else None, b.data_ptr() if b is not None else None, eps,
                                  CODE[out.v.dtype], out.v.data_ptr(), out.stride))


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "N%d-C%d-%s-%s-%s-%s-s%d-o%d-a%d" % (c[0], c[1], str(c[2])[11:], str(c[3])[11:], c[4], str(c[5])[11:],
                                                                                             c[6], c[7], int(c[8])))
def test_layer_norm_forward_and_backward_against_float64(case):
    N, C, xdt, odt, res, rdt, extra, offset, affine = case
    seed = 3 * N + C
    x, r, w, b = _ln_operands(case, seed)
    label = "N %d C %d %s -> %s res %s stride +%d offset %d affine %d" % (N, C, str(xdt)[6:], str(odt)[6:], res, extra, offset, affine)
    x64 = x.v.double()
    r64 = r.v.double() if r else None
    ref = TR.layer_norm_restate(x64, w.double() if affine else None, b.double() if affine else None, 1e-5, r64)
    allow = TR.layer_norm_forward_bound(x.v, w, b, 1e-5, r.v if r else None, odt)
    out = r if res == "alias" else Rows(N, C, odt, C + 2 * extra, offset)
    _ln_fwd(x, r, w, b, out)
    out.check(label)
    x.check(label)
    _worst(out.v, ref, allow, label + " forward")
    if res == "alias":                                                                           # the bits of a separate out
        r2 = Rows(N, C, odt, C + extra, offset, r64.to(odt))
        sep = Rows(N, C, odt, C + extra, offset)
        _ln_fwd(x, r2, w, b, sep)
        assert torch.equal(_bits(sep.v), _bits(out.v)), label
    # backward: dout in out's dtype at its own stride, dx in x's dtype at its own stride; two runs bit for bit
    g = Rows(N, C, odt, C + extra, offset, torch.randn(N, C, generator=torch.Generator().manual_seed(seed + 1)).to(odt).to(DEV))
    want = TR.layer_norm_backward_restate(x64, w.double() if affine else None, 1e-5, g.v.double())
    bounds = TR.layer_norm_backward_bounds(x.v, w, 1e-5, g.v, xdt)
    scratch = torch.empty(_lib().igs_layer_norm_bwd_scratch_bytes(N, C) + 1, dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        dx = Rows(N, C, xdt, C + 3 * extra, offset)
        dw, db = Rows(1, C, F32), Rows(1, C, F32)
        _ok(_lib().igs_layer_norm_bwd(_stream(), N, C, CODE[xdt], x.v.data_ptr(), x.stride, w.data_ptr() if affine else None, 1e-5, CODE[odt],
                                      g.v.data_ptr(), g.stride, CODE[xdt], dx.v.data_ptr(), dx.stride, dw.v.data_ptr(), db.v.data_ptr(),
                                      scratch[1:].data_ptr()))
        for t in (dx, dw, db):
            t.check(label)
        runs.append((dx.v.clone(), dw.v[0].clone(), db.v[0].clone()))
    for a, c in zip(*runs):
        assert torch.equal(_bits(a), _bits(c)), (label, "two backward runs differ")
    for got, r_, k in zip(runs[0], want, ("dx", "dweight", "dbias")):
        _worst(got, r_, bounds[k], label + " " + k)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("C", [12, 128, 512])
def test_a_nan_row_is_all_nan_and_a_constant_row_is_exactly_bias(C, dtype):
    x = TR.row_inputs(4, C, dtype, DEV, seed=C, constant_row=2)
    x[1, (2 * C) // 3] = float("nan")
    x[3, C // 2] = float("inf")
    w, b = TR.affine_inputs(C, DEV, C)
    res = TR.row_inputs(4, C, dtype, DEV, seed=C + 1)
    xr, rr = Rows(4, C, dtype, src=x), Rows(4, C, dtype, src=res)
    for r in (None, rr):
        out = Rows(4, C, F32)
        _ln_fwd(xr, r, w, b, out)
        out.check("non-finite rows")
        assert torch.isnan(out.v[1]).all() and torch.isnan(out.v[3]).all()
        assert torch.equal(out.v[2], b if r is None else res[2].float() + b), "a constant row must give exactly bias (+ res)"
        ref = TR.layer_norm_restate(x[:1].double(), w.double(), b.double(), 1e-5, res[:1].double() if r else None)
        _worst(out.v[:1], ref, TR.layer_norm_forward_bound(x[:1], w, b, 1e-5, res[:1] if r else None), "C %d beside non-finite rows" % C)


@pytest.mark.parametrize("C", [12, 512])
def test_every_optional_gradient_left_out_in_turn(C):
    N = 67
    x = TR.row_inputs(N, C, F32, DEV, seed=C)
    g = torch.randn(N, C, device=DEV)
    w, _ = TR.affine_inputs(C, DEV, C)
    scratch = torch.empty(_lib().igs_layer_norm_bwd_scratch_bytes(N, C), dtype=torch.uint8, device=DEV)

    def run(want):
        outs = [Rows(N, C, F32) if want[0] else None, Rows(1, C, F32) if want[1] else None, Rows(1, C, F32) if want[2] else None]
        dx, dw, db = (o.v.data_ptr() if o else None for o in outs)
        _ok(_lib().igs_layer_norm_bwd(_stream(), N, C, 0, x.data_ptr(), C, w.data_ptr(), 1e-5, 0, g.data_ptr(), C, 0, dx, C, dw, db,
                                      scratch.data_ptr() if (want[1] or want[2]) else None))
        for o in outs:
            if o:
                o.check(want)
                assert not torch.isnan(o.v).any(), want
        return [o.v.clone() if o else None for o in outs]

    full = run((True, True, True))
    for want in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False), (False, False, True)):
        for a, c in zip(run(want), full):
            assert a is None or torch.equal(a, c), want


@pytest.mark.parametrize("N,C", [(67, 132), (4200, 132), (3, 12)])
def test_parameter_gradients_are_the_partial_rows_added_in_the_documented_order(N, C):
    """d weight / d bias bit for bit from the [T][2][C] partial rows that the backward leaves in its scratch (from the scratch pointer
    rounded up to 256 bytes; T = min(ceil(N / rows per workgroup), 1024) with 16 rows per workgroup for C <= 128 and 4 above): 16 contiguous
    shares of ceil(T / 16) rows, each added row by row, then the 16 sums added in order.  (67, 132): T = 17, shares of 2, waves 9 to 15
    empty; (4200, 132): T = 1024, shares of 64, the eight-at-a-time loop; (3, 12): T = 1."""
    x = TR.row_inputs(N, C, F32, DEV, seed=N + C)
    g = torch.randn(N, C, generator=torch.Generator().manual_seed(N), dtype=F32).to(DEV)
    w, _ = TR.affine_inputs(C, DEV, C)
    rpg = 16 if C <= 128 else 4
    T = min(-(-N // rpg), 1024)
    nbytes = _lib().igs_layer_norm_bwd_scratch_bytes(N, C)
    assert nbytes == -(-T * 2 * C * 4 // 256) * 256 + 256
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    dw, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    _ok(_lib().igs_layer_norm_bwd(_stream(), N, C, 0, x.data_ptr(), C, w.data_ptr(), 1e-5, 0, g.data_ptr(), C, 0, None, C, dw.data_ptr(), db.data_ptr(),
                                  scratch.data_ptr()))
    torch.cuda.synchronize()
    at = -scratch.data_ptr() % 256
    part = scratch[at:at + T * 2 * C * 4].view(F32).view(T, 2 * C)
    want = TR.param_rows_sum(part)
    print("N %d C %d: T %d, max |dweight| %.3e" % (N, C, T, dw.abs().max().item()))
    assert torch.equal(_bits(dw.cpu()), _bits(want[:C])) and torch.equal(_bits(db.cpu()), _bits(want[C:]))


# ---------------------------------------------------------------- GEGLU through the C ABI
# N, D, dtype, extra row stride, offset, scale
GEGLU_CASES = [(1, 1, F32, 0, 0, 1.0), (5, 6, F32, 0, 0, 4.0), (67, 6, F16, 2, 1, 1.0), (5, 8, F32, 8, 0, 1.0), (67, 8, F16, 0, 0, 4.0), (67, 8, F32, 0, 1, 1.0),
               (5, 2048, F32, 0, 0, 4.0), (67, 2048, F16, 64, 0, 1.0), (1, 8192, F16, 0, 0, 4.0), (5, 8192, F32, 4, 0, 1.0), (67, 1, F16, 1, 0, 1.0)]
HALF_MAX = 65504.0


def _geglu_compare(got, ref, allow, label):
    """Where the float64 result leaves float16's range the kernel must overflow the same way; everything else inside the allowance."""
    assert not torch.isnan(got).any(), (label, "an element was not written")
    if got.dtype == F16:
        over = ref.abs() > HALF_MAX * (1 - 2.0 ** -11)
        assert ((got.double().abs() >= HALF_MAX * (1 - 2.0 ** -10)) & (torch.sign(got.double()) == torch.sign(ref)))[over].all(), (label, "overflow")
        got, ref, allow = got[~over], ref[~over], allow[~over]
    err = (got.double() - ref).abs()
    worst = (err / allow).max().item() if err.numel() else 0.0
    print("%s: max |err| / allowance %.3f" % (label, worst))
    assert worst <= 1.0, (label, worst)


@pytest.mark.parametrize("case", GEGLU_CASES, ids=lambda c: "N%d-D%d-%s-s%d-o%d-x%g" % (c[0], c[1], str(c[2])[11:], c[3], c[4], c[5]))
def test_geglu_forward_and_backward_against_float64(case):
    N, D, dtype, extra, offset, scale = case
    label = "N %d D %d %s stride +%d offset %d scale %g" % (N, D, str(dtype)[6:], extra, offset, scale)
    p = Rows(N, 2 * D, dtype, 2 * D + extra, offset, TR.geglu_inputs(N, D, dtype, DEV, seed=N + D, scale=scale))
    out = Rows(N, D, dtype, offset=offset)
    _ok(_lib().igs_geglu_fwd(_stream(), N, D, CODE[dtype], p.v.data_ptr(), p.stride, out.v.data_ptr()))
    out.check(label)
    p.check(label)
    p64 = p.v.double()
    _geglu_compare(out.v, TR.geglu_restate(p64), TR.geglu_forward_allowance(p.v, dtype), label + " forward")
    dout = Rows(N, D, dtype, offset=offset, src=torch.randn(N, D, generator=torch.Generator().manual_seed(D)).to(dtype).to(DEV))
    runs = []
    for _ in range(2):
        dp = Rows(N, 2 * D, dtype, offset=offset)
        _ok(_lib().igs_geglu_bwd(_stream(), N, D, CODE[dtype], p.v.data_ptr(), p.stride, dout.v.data_ptr(), dp.v.data_ptr()))
        dp.check(label)
        runs.append(dp.v.clone())
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), (label, "two backward runs differ")
    _geglu_compare(runs[0], TR.geglu_backward_restate(p64, dout.v.double()), TR.geglu_backward_allowance(p.v, dout.v, dtype), label + " backward")


# ---------------------------------------------------------------- the Python layer: autograd
@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("sliced", [False, True])
def test_layer_norm_autograd_against_float64(sliced, dtype):
    from igs_amd import tokens as TK
    B, L, C = 2, 33, 128
    wide = TR.row_inputs(B * L, 3 * C, dtype, DEV, seed=11).view(B, L, 3 * C)
    x = (wide[..., C: 2 * C] if sliced else wide[..., C: 2 * C].contiguous()).detach().requires_grad_(True)
    res = TR.row_inputs(B * L, C, dtype, DEV, seed=12).view(B, L, C).requires_grad_(True)
    w, b = (t.requires_grad_(True) for t in TR.affine_inputs(C, DEV, 13))
    g = torch.randn(B, L, C, device=DEV).to(dtype)
    out = TK.layer_norm(x, w, b, 1e-5, residual=res)
    assert out.dtype == dtype and out.shape == x.shape
    dx, dw, db, dres = torch.autograd.grad(out, (x, w, b, res), g)
    x2, g2 = x.detach().reshape(-1, C), g.reshape(-1, C)
    ref = TR.layer_norm_restate(x2.double(), w.detach().double(), b.detach().double(), 1e-5, res.detach().reshape(-1, C).double())
    _worst(out.detach().reshape(-1, C), ref, TR.layer_norm_forward_bound(x2, w.detach(), b.detach(), 1e-5, res.detach().reshape(-1, C), dtype), "forward")
    want = TR.layer_norm_backward_restate(x2.double(), w.detach().double(), 1e-5, g2.double())
    bounds = TR.layer_norm_backward_bounds(x2, w.detach(), 1e-5, g2, dtype)
    for got, r, k in zip((dx.reshape(-1, C), dw, db), want, ("dx", "dweight", "dbias")):
        _worst(got, r, bounds[k], "sliced %d %s %s" % (sliced, str(dtype)[6:], k))
    assert torch.equal(dres, g) and dx.dtype == dtype and dw.dtype == F32
    with torch.no_grad():                                                                        # nothing saved, another out dtype
        y = TK.layer_norm(x, w, b, 1e-5, out_dtype=F32)
    assert y.dtype == F32 and y.grad_fn is None
    plain = TK.layer_norm(x.detach(), None, None)                                                # no affine step
    _worst(plain.reshape(-1, C), TR.layer_norm_restate(x2.double(), None, None, 1e-5), TR.layer_norm_forward_bound(x2, None, None, 1e-5, None, dtype), "no affine")


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("sliced", [False, True])
def test_geglu_autograd_against_float64(sliced, dtype):
    from igs_amd import tokens as TK
    N, D = 37, 96
    p = TR.geglu_inputs(N, D, dtype, DEV, seed=5, row_stride=2 * D + 8 if sliced else None)
    p = p.view(1, N, 2 * D) if not sliced else p.unsqueeze(0)
    p = p.detach().requires_grad_(True)
    g = torch.randn(1, N, D, device=DEV).to(dtype)
    out = TK.geglu(p)
    assert out.shape == (1, N, D) and out.dtype == dtype
    (dp,) = torch.autograd.grad(out, p, g)
    p2 = p.detach().reshape(N, 2 * D)
    _geglu_compare(out.detach().reshape(N, D), TR.geglu_restate(p2.double()), TR.geglu_forward_allowance(p2, dtype), "geglu forward")
    _geglu_compare(dp.reshape(N, 2 * D), TR.geglu_backward_restate(p2.double(), g.reshape(N, D).double()),
                   TR.geglu_backward_allowance(p2, g.reshape(N, D), dtype), "geglu backward sliced %d %s" % (sliced, str(dtype)[6:]))


def test_tensors_on_different_devices_are_refused():
    from igs_amd import tokens as TK
    x = torch.randn(3, 16, device=DEV)
    w, b = TR.affine_inputs(16, DEV, 0)
    with pytest.raises(RuntimeError, match="one GPU"):
        TK.layer_norm(x, None, None, residual=x.cpu())
    with pytest.raises(RuntimeError, match="one GPU"):
        TK.layer_norm(x, w.cpu(), b.cpu())


# ---------------------------------------------------------------- the stand-in modules, patched against their float64 runs
def _run(module, inputs, gout, **kw):
    """(output, input gradients, parameter gradients) as a flat list of detached tensors."""
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = module(*leaves, **kw)
    params = [p for p in module.parameters()]
    grads = torch.autograd.grad(out, leaves + params, gout.to(out.dtype))
    return [out.detach()] + [g.detach() for g in grads]


def _error(got, want):
    return max(((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(got, want))


def _four_times_rule(label, eager, native, want, floor=1e-5):
    e_eager, e_native = _error(eager, want), _error(native, want)
    print("%s: max relative |err| against float64: unpatched PyTorch %.3e, patched %.3e (allowed %.3e)" % (label, e_eager, e_native, max(4 * e_eager, floor)))
    assert all(torch.isfinite(t).all() for t in native), label
    assert [t.dtype for t in native] == [t.dtype for t in eager], (label, "dtypes differ from eager PyTorch")
    assert e_native <= max(4 * e_eager, floor), (label, e_native, e_eager)


class BlockAttention(AR.AttentionStandIn):
    """The attention stand-in with an eager path of its own while no processor is set."""

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None):
        if self.processor is None:
            return self.restated(hidden_states)
        return super().forward(hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask)


def _layer_case(no_ffn, shift, seed=0):
    g = torch.Generator().manual_seed(40 + seed)
    source, target, gout = (torch.randn(2, 64, 128, generator=g).to(DEV) for _ in range(3))
    mask = torch.zeros(4, 16, 16, device=DEV)
    kw = dict(height=8, width=8, shifted_window_attn_mask=mask, with_shift=shift, attn_num_splits=2)
    layer = TR.make_layer(128, no_ffn=no_ffn, seed=seed).to(DEV)
    return layer, (source, target), gout, kw


def _block_case(seed=0, heads=2):
    """dim 512, 64 tokens, two heads of a simple (explicit softmax) attention; the composition with use_native_attention takes eight, since
    attn.hip's head size is 64."""
    g = torch.Generator().manual_seed(60 + seed)
    x, gout = (torch.randn(1, 64, 512, generator=g).to(DEV) for _ in range(2))
    return TR.make_block(512, BlockAttention(channels=512, heads=heads, seed=seed), seed=seed).to(DEV), (x,), gout, {}


def _three_runs(make, install, autocast=False):
    module, inputs, gout, kw = make()
    want = _run(copy.deepcopy(module).double(), [t.double() for t in inputs], gout.double(), **{k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()})
    keys = list(module.state_dict().keys())
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        eager = _run(module, inputs, gout, **kw)
        install(module)
        native = _run(module, inputs, gout, **kw)
    assert list(module.state_dict().keys()) == keys
    return eager, native, want


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("no_ffn", [True, False])
def test_stand_in_layer_patched_against_its_float64_run(no_ffn, shift, autocast):
    from igs_amd import tokens as TK
    eager, native, want = _three_runs(lambda: _layer_case(no_ffn, shift), lambda m: TK.use_native_transformer_layers(m) == 1 or pytest.fail("count"), autocast)
    _four_times_rule("layer no_ffn %d shift %d autocast %d" % (no_ffn, shift, autocast), eager, native, want, floor=2e-3 if autocast else 1e-5)


@pytest.mark.parametrize("autocast", [False, True])
def test_stand_in_block_patched_against_its_float64_run(autocast):
    from igs_amd import tokens as TK
    eager, native, want = _three_runs(_block_case, lambda m: TK.use_native_block_ops(m) == 3 or pytest.fail("count"), autocast)
    _four_times_rule("block autocast %d" % autocast, eager, native, want, floor=2e-3 if autocast else 1e-5)


@pytest.mark.parametrize("no_ffn", [True, False])
def test_layer_composes_with_the_native_window_attention(no_ffn, monkeypatch):
    from igs_amd import attention as AT, tokens as TK
    for name in (TK.ATTN_SPLIT, TK.ATTN_FULL):
        monkeypatch.setattr(TR, name, getattr(TR, name))                                         # (the stand-in module's names are restored afterwards)

    def install(m):
        assert TK.use_native_transformer_layers(m) == 1 and AT.use_native_window_attention(TR) == 2

    eager, native, want = _three_runs(lambda: _layer_case(no_ffn, True, seed=3), install)
    assert TR.single_head_split_window_attention is AT.single_head_split_window_attention
    _four_times_rule("layer no_ffn %d with window_attention" % no_ffn, eager, native, want)


def test_block_composes_with_the_native_attention():
    from igs_amd import attention as AT, tokens as TK

    def install(m):
        assert TK.use_native_block_ops(m) == 3 and AT.use_native_attention(m) == 1

    eager, native, want = _three_runs(lambda: _block_case(seed=2, heads=8), install)
    _four_times_rule("block with use_native_attention", eager, native, want)
