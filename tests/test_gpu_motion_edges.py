"""Anchor feature interpolation and the Gaussian deform (motion.hip) at the launch branches tests/test_gpu_motion.py does not reach:
interp_fwd_kernel / interp_chunk_kernel <8> and <16> (D in 257..1024), the backward's chunk lengths 128, 256 and 512 with in-degrees
either side of every chunk boundary, the inverse index at its radix pass-count boundaries (A_total = 255 / 256, 65 535 / 65 536), odd K,
rows without a valid slot, gradient subsets, the backward at the shipped size (1.6 M edges: chunk 128, a sort of 196 blocks of four
tiles), and the deform below its autograd Function (NULL upstream gradients, output subsets, M = 0, M = P, P = 1, mask indices outside
[0, P), the in-place C ABI).

Exact-input cases (tests/motion_restatement.py exact_interp_case: integer features and gradients, weights in {1, 1/2, 1/4}; the builder
asserts that every partial sum is exact in float32) are compared bit for bit with the float64 restatement.  Float cases use the derived
bounds test_gpu_motion.py holds the same kernels to (MR.interp_forward_bound, MR.interp_backward_bounds, MR.deform_*_ratio); each
prints its worst error-to-bound ratio before asserting it is at most 1.  tests/test_motion_host.py asserts without a GPU that every
size below lands in the branch its test names.
"""
import pytest
import torch

import motion_restatement as MR
from test_gpu_motion import _backward_pair, _case, _deform_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 64


def _report(what, **ratios):
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)


# ---------------------------------------------------------------- interpolation: float cases
def _float_case_ratios(F, w, col, seed=0):
    from igs_amd.motion import interpolate_anchor_features
    D = F.shape[-1]
    half = F.dtype == torch.float16
    out = interpolate_anchor_features(F, w, col)
    dF, dw, dout = _backward_pair(F, w, col, seed=seed)
    t = MR.interp_truth_blocked(F, w, col, dout)
    assert out.dtype == torch.float32 and dF.dtype == F.dtype and dF.shape == F.shape and dw.shape == w.shape
    tol_F, tol_w = MR.interp_backward_bounds(t, w.shape[1], D, half)
    return dict(out=MR.worst_ratio(out, t["out"], w.shape[1] * MR.U * t["out_abs"] + 1e-30),
                dF=MR.worst_ratio(dF.reshape(-1, D), t["dF"], tol_F), dw=MR.worst_ratio(dw.reshape(w.shape[0], -1), t["dw"], tol_w))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("D", [257, 512, 513, 1024])
def test_wide_rows_against_float64(D, dtype):
    """interp_fwd_kernel / interp_chunk_kernel <8> (D = 257, 512) and <16> (D = 513, 1024), 5 % of the slots padding."""
    F, w, col = _case(300, 8, 100, D, seed=D, dtype=dtype, pad=0.05)
    _report(f"wide rows D = {D} {dtype}", **_float_case_ratios(F, w, col))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_shipped_size_backward_against_float64(dtype):
    """N = 200 000 in-box Gaussians x K = 8 over A = 8192 anchors, D = 128: chunk length 128 and a radix sort of 196 blocks, each
    over four sort tiles.  The float64 truth is built in row blocks."""
    F, w, col = _case(200000, 8, 8192, 128, seed=21, dtype=dtype)
    _report(f"shipped backward {dtype}", **_float_case_ratios(F, w, col, seed=2))


# ---------------------------------------------------------------- interpolation: exact inputs, bit for bit
def _native(F, w, col, dout, want_F=True, want_w=True):
    from igs_amd.motion import interpolate_anchor_features
    Fn = F.detach().to(DEV).clone().requires_grad_(want_F)
    wn = w.detach().to(DEV).clone().requires_grad_(want_w)
    out = interpolate_anchor_features(Fn, wn, col.to(DEV))
    out.backward(dout.to(DEV))
    return out.detach(), Fn.grad, wn.grad


def _truth(F, w, col, dout):
    F64, w64 = F.detach().to(DEV).double().clone().requires_grad_(True), w.detach().to(DEV).double().clone().requires_grad_(True)
    ref = MR.interp_restate(F64, w64, col.to(DEV))
    ref.backward(dout.to(DEV).double())
    return ref.detach(), F64.grad, w64.grad


def _assert_bit_equal(F, w, col, dout, runs=1):
    got = _native(F, w, col, dout)
    ref = _truth(F, w, col, dout)
    for g, r, name in zip(got, ref, ("out", "dF", "dw")):
        assert g.dtype == torch.float32 and torch.equal(g.double(), r), name
    for _ in range(runs - 1):
        again = _native(F, w, col, dout)
        for g, a, name in zip(got, again, ("out", "dF", "dw")):
            assert torch.equal(g, a), f"{name} differs between two runs"
    return got


@pytest.mark.parametrize("chunk", sorted(MR.CHUNK_SHAPES))
def test_chunk_lengths_bit_equal(chunk):
    """Chunk lengths 128, 256 and 512; the first anchors' in-degrees sit either side of every chunk length (MR.CHUNK_DEGREES), one list
    has 150 000 edges; 2 % of the slots are -1.  out, dF and dw equal float64 bit for bit, and two runs agree."""
    N, K, D = MR.CHUNK_SHAPES[chunk]
    F, w, col, dout = MR.exact_interp_case(N, K, 300, D, degrees=MR.CHUNK_DEGREES, pad=0.02, seed=chunk)
    _, dF, _ = _assert_bit_equal(F, w, col, dout, runs=2)
    assert (dF[0] == 0).all()                          # the anchor without an edge


@pytest.mark.parametrize("A", MR.INDEX_PASS_ANCHORS)
def test_index_pass_boundaries_bit_equal(A):
    """The padding key A needs 8 bits at A = 255 and 9 at 256 (one radix pass, then two), 16 at 65 535 and 17 at 65 536 (two, then
    three): 5 % of the slots are -1, a few A + 7, and the first and last anchors have edges."""
    F, w, col, dout = MR.exact_interp_case(3000, 8, A, 3, pad=0.05, oob=9, seed=A)
    col[0, 0], col[1, 0], col[2, 0], col[2999, 7] = A - 1, 0, A - 1, A - 1
    _assert_bit_equal(F, w, col, dout)


@pytest.mark.parametrize("K", [3, 5, 7])
def test_odd_k_bit_equal(K):
    F, w, col, dout = MR.exact_interp_case(1000, K, 64, 64, pad=0.05, seed=K)
    _assert_bit_equal(F, w, col, dout)


def test_all_slots_invalid_gives_exact_zeros():
    F, w, col, dout = MR.exact_interp_case(500, 8, 32, 40, seed=1)
    col[:, ::2] = -1
    col[:, 1::2] = 32 + 3
    w[:, 0] = float("nan")                             # never read
    out, dF, dw = _native(F, w, col, dout)
    for t in (out, dF, dw):
        assert (t.view(torch.int32) == 0).all()        # +0.0 everywhere


def test_gradient_subsets_carry_the_bits_of_the_full_run():
    """dF only and dw only (N = 4000, K = 8, A = 16: every list has many chunks)."""
    F, w, col, dout = MR.exact_interp_case(4000, 8, 16, 40, pad=0.02, seed=4)
    out, dF, dw = _assert_bit_equal(F, w, col, dout)
    o1, dF1, none1 = _native(F, w, col, dout, want_w=False)
    o2, none2, dw2 = _native(F, w, col, dout, want_F=False)
    assert none1 is None and none2 is None
    assert torch.equal(o1, out) and torch.equal(o2, out) and torch.equal(dF1, dF) and torch.equal(dw2, dw)
    # and on float inputs, where the order of every sum shows in the bits
    Ff, wf, cf = _case(4000, 8, 16, 40, seed=5, pad=0.02)
    doutf = torch.randn(4000, 40, generator=torch.Generator().manual_seed(6))
    _, a, b = _native(Ff.reshape(-1, 40), wf.squeeze(-1), cf, doutf)
    _, a1, _ = _native(Ff.reshape(-1, 40), wf.squeeze(-1), cf, doutf, want_w=False)
    _, _, b2 = _native(Ff.reshape(-1, 40), wf.squeeze(-1), cf, doutf, want_F=False)
    assert torch.equal(a, a1) and torch.equal(b, b2)


# ---------------------------------------------------------------- deform
def _deform_check(xyz, rot, mask, dx, dr, what):
    """Forward and backward through igs_amd.motion.deform_xyz_rotation against float64, test_gpu_motion.py's rules.  Mask entries
    outside [0, P) are skipped: the truth drops them, their residuals' gradients are zero."""
    from igs_amd.motion import deform_xyz_rotation
    P = xyz.shape[0]
    valid = (mask >= 0) & (mask < P)
    half = dx.dtype == torch.float16
    leaves = [t.clone().requires_grad_(True) for t in (xyz, rot, dx, dr)]
    xo, ro = deform_xyz_rotation(leaves[0], leaves[1], mask, leaves[2], leaves[3])
    l64 = [t.detach().double().requires_grad_(True) for t in (xyz, rot, dx, dr)]
    xr, rr = MR.deform_xyz_rotation_restate(l64[0], l64[1], mask[valid], l64[2][valid], l64[3][valid])
    rx, rq = MR.deform_forward_ratios(xo.detach(), ro.detach(), xyz, mask[valid], dx[valid], xr.detach(), rr.detach())
    unm = torch.ones(P, dtype=torch.bool, device=DEV)
    unm[mask[valid]] = False
    assert torch.equal(xo[unm], xyz[unm]) and torch.equal(ro[unm], rot[unm])
    g = torch.Generator().manual_seed(P)
    gx, gr = torch.randn(P, 3, generator=g).to(DEV), torch.randn(P, 4, generator=g).to(DEV)
    torch.autograd.backward((xo, ro), (gx, gr))
    torch.autograd.backward((xr, rr), (gx.double(), gr.double()))
    ratios = dict(xyz=rx, rotation=rq)
    for a, b, name in zip(leaves, l64, ("d_xyz", "d_rotation", "d_res_xyz", "d_res_rotation")):
        assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
        gb = b.grad if b.grad is not None else torch.zeros_like(b)
        ratios[name] = MR.deform_grad_ratio(a.grad, gb, a.dtype == torch.float16)
    if (~valid).any():
        assert (leaves[2].grad[~valid] == 0).all() and (leaves[3].grad[~valid] == 0).all()
    _report(f"deform {what} {'f16' if half else 'f32'}", **ratios)
    return leaves


def test_deform_empty_mask_is_the_identity():
    from igs_amd.motion import deform_xyz_rotation
    xyz, rot, mask, dx, dr = _deform_case(777, 0, seed=2)
    assert mask.numel() == 0 and dx.shape == (0, 3)
    x, r = xyz.clone().requires_grad_(True), rot.clone().requires_grad_(True)
    xo, ro = deform_xyz_rotation(x, r, mask, dx, dr)
    assert torch.equal(xo.view(torch.int32), xyz.view(torch.int32)) and torch.equal(ro.view(torch.int32), rot.view(torch.int32))
    gx, gr = torch.randn_like(xo), torch.randn_like(ro)
    torch.autograd.backward((xo, ro), (gx, gr))
    assert torch.equal(x.grad, gx) and torch.equal(r.grad, gr)
    with torch.no_grad():
        xo, ro = deform_xyz_rotation(xyz, rot, mask, dx, dr)
    assert torch.equal(xo, xyz) and torch.equal(ro, rot) and xo.data_ptr() != xyz.data_ptr()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("P,M", [(1, 1), (1000, 1000), (1000, 777), (257, 3)], ids=["P1", "M=P", "off-grid", "three-of-257"])
def test_deform_sizes_against_float64(P, M, dtype):
    xyz, rot, mask, dx, dr = _deform_case(P, M, seed=P + M, dtype=dtype)
    if (P, M) == (1000, 777):
        assert not torch.equal(mask, mask.sort().values)                 # P off the 256 grid, an unsorted mask
    _deform_check(xyz, rot, mask, dx, dr, f"P = {P}, M = {M}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_deform_mask_indices_outside_are_skipped(dtype):
    xyz, rot, mask, dx, dr = _deform_case(1000, 600, seed=8, dtype=dtype)
    mask[3], mask[77], mask[300], mask[599] = -1, 1000, 1000 + 5, -(2 ** 40)
    _deform_check(xyz, rot, mask, dx, dr, "mask with -1 and P")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_deform_bwd_null_upstream_and_output_subsets(dtype):
    """Below the autograd Function: a missing upstream gradient (the zero-fill path) and every single output give the bits of the call
    that passes explicit zeros and wants everything, and that call meets the float64 bounds."""
    from igs_amd._cabi import ext
    E = ext()
    P, M = 1000, 600
    xyz, rot, mask, dx, dr = _deform_case(P, M, seed=12, dtype=dtype)
    g = torch.Generator().manual_seed(13)
    gx, gr = torch.randn(P, 3, generator=g).to(DEV), torch.randn(P, 4, generator=g).to(DEV)
    zx, zr = torch.zeros_like(gx), torch.zeros_like(gr)
    names = ("d_xyz", "d_rotation", "d_res_xyz", "d_res_rotation")
    for ux, ur, what in ((gx, gr, "both"), (None, gr, "grad_xyz None"), (gx, None, "grad_rotation None"), (None, None, "both None")):
        full = E.motion_deform_bwd(rot, mask, dx, dr, zx if ux is None else ux, zr if ur is None else ur, True, True, True, True)
        got = E.motion_deform_bwd(rot, mask, dx, dr, ux, ur, True, True, True, True)
        for a, b, name in zip(got, full, names):
            assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), (what, name)
        for i, name in enumerate(names):
            want = [j == i for j in range(4)]
            one = E.motion_deform_bwd(rot, mask, dx, dr, ux, ur, *want)
            assert all((o is None) != want[j] for j, o in enumerate(one)), (what, name)
            assert torch.equal(_bits(one[i]), _bits(full[i])), (what, name)
        l64 = [t.double().requires_grad_(True) for t in (xyz, rot, dx, dr)]
        xr, rr = MR.deform_xyz_rotation_restate(l64[0], l64[1], mask, l64[2], l64[3])
        torch.autograd.backward((xr, rr), ((zx if ux is None else ux).double(), (zr if ur is None else ur).double()))
        ratios = {name: MR.deform_grad_ratio(a, b.grad, a.dtype == torch.float16) for a, b, name in zip(full, l64, names)}
        _report(f"deform backward, {what}, {'f16' if dtype == torch.float16 else 'f32'}", **ratios)


def test_deform_cabi_in_place_gives_the_out_of_place_bits():
    from igs_amd import _cabi
    L = _cabi.lib()
    P, M = 1000, 400
    xyz, rot, mask, dx, dr = _deform_case(P, M, seed=14)
    stream = torch.cuda.current_stream().cuda_stream

    def banded(n):
        big = torch.full((n + 2 * BAND,), -777.0, device=DEV)
        return big, big[BAND:BAND + n]

    xb, xo = banded(3 * P)
    rb, ro = banded(4 * P)
    rc = L.igs_gaussian_deform_fwd(stream, P, M, 0, xyz.data_ptr(), rot.data_ptr(), mask.data_ptr(), dx.data_ptr(), dr.data_ptr(),
                                   xo.data_ptr(), ro.data_ptr())
    assert rc == 0, _cabi.last_error()
    xib, xi = banded(3 * P)
    rib, ri = banded(4 * P)
    xi.copy_(xyz.reshape(-1))
    ri.copy_(rot.reshape(-1))
    rc = L.igs_gaussian_deform_fwd(stream, P, M, 0, xi.data_ptr(), ri.data_ptr(), mask.data_ptr(), dx.data_ptr(), dr.data_ptr(),
                                   xi.data_ptr(), ri.data_ptr())
    assert rc == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert torch.equal(xi.view(torch.int32), xo.view(torch.int32)) and torch.equal(ri.view(torch.int32), ro.view(torch.int32))
    assert not torch.equal(xo.reshape(P, 3), xyz) and not torch.equal(ro.reshape(P, 4), rot)
    for big, n in ((xb, 3 * P), (rb, 4 * P), (xib, 3 * P), (rib, 4 * P)):
        assert (big[:BAND] == -777.0).all() and (big[BAND + n:] == -777.0).all(), "a guard band was written"
    xr, rr = MR.deform_xyz_rotation_restate(xyz.double(), rot.double(), mask, dx.double(), dr.double())
    rx, rq = MR.deform_forward_ratios(xo.reshape(P, 3), ro.reshape(P, 4), xyz, mask, dx, xr, rr)
    _report("deform C ABI", xyz=rx, rotation=rq)
