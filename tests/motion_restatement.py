"""Float64 PyTorch restatement of the two anchor-graph consumers of IGS's AGM-Net, in this repository's words (no reference program text).

  interp_restate     -- GS3DRenderer.query_ir_grid's tail (igs/models/gs.py:812-822): gather the K neighbour rows of the flattened
                        anchor features, weight them, sum over K; split the result by example counts.
  qmul_restate       -- quaternion_multiply (igs/utils/general_utils.py:177-200): F.normalize both inputs (eps 1e-12), then the Hamilton
                        product with w first.
  deform_restate     -- GaussianModel.deform (gs.py:347-375) for the shipped residual keys xyz and rotation: clone the fields, add the
                        xyz residual on the masked rows, rotate the masked rows by the residual quaternion.

Every function is differentiable (torch.autograd), so the GPU tests take their gradient truths from here.  A -1 (or out-of-range)
column contributes nothing, as the native path documents.
"""
import torch


def interp_restate(feats_flat, weights, col):
    """out[n] = sum_k w[n, k] * F[col[n, k]] (gs.py:816-820), with slots outside [0, A) dropped.  F [A, D], weights [N, K] or
    [N, K, 1], col [N*K] or [N, K]; computed in F's dtype."""
    A, D = feats_flat.shape
    w = weights.reshape(weights.shape[0], -1)
    N, K = w.shape
    c = col.reshape(N, K)
    ok = (c >= 0) & (c < A)
    rows = feats_flat[c.clamp(0, A - 1).reshape(-1)].reshape(N, K, D)          # gs.py:818 features[col] viewed [N, K, D]
    prod = rows * w.to(feats_flat.dtype).unsqueeze(-1)                           # gs.py:820 features * weights
    prod = torch.where(ok.unsqueeze(-1), prod, torch.zeros((), dtype=prod.dtype))
    return prod.sum(dim=1)                                                       # ... sum over dim 1


def split_by_batch(out, batch_y):
    """gs.py:821-822: torch.unique(batch_y, return_counts=True), then torch.split by the counts."""
    _, counts = torch.unique(batch_y, return_counts=True)
    return torch.split(out, counts.tolist())


def normalize(q, eps=1e-12):
    """F.normalize along dim 1: q / max(|q|, eps)."""
    return q / q.norm(dim=1, keepdim=True).clamp_min(eps)


def qmul_restate(a, b):
    """general_utils.py:189-200: normalise both, then (w, x, y, z) of the Hamilton product a * b."""
    a, b = normalize(a), normalize(b)
    w1, x1, y1, z1 = a.unbind(1)
    w2, x2, y2, z2 = b.unbind(1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2,
                        w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                        w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2], dim=1)


def deform_xyz_rotation_restate(xyz, rotation, mask, res_xyz, res_rotation):
    """gs.py:356-370 for the xyz and rotation keys: clone, then masked rows get xyz + residual and qmul(rotation, residual)."""
    xo = xyz.clone()
    ro = rotation.clone()
    xo[mask] = res_xyz.to(xyz.dtype) + xo[mask]
    ro[mask] = qmul_restate(ro[mask], res_rotation.to(rotation.dtype))
    return xo, ro


def deform_restate(gs, res_feat, mask):
    """gs.py:347-375 as a dict of the GaussianModel fields it builds."""
    xo, ro = deform_xyz_rotation_restate(gs.xyz, gs.rotation, mask, res_feat["xyz"], res_feat["rotation"])
    return {"xyz": xo, "opacity": gs.opacity.clone(), "rotation": ro, "scaling": gs.scaling.clone(), "shs": gs.shs.clone(),
            "resi_rotation": res_feat["rotation"].clone(), "mask": mask, "resi_xyz": res_feat["xyz"].clone()}


# ---------------------------------------------------------------- launch geometry, restated from motion.hip / radix_sort.hip / radix_sort.h (lines cited)
INTERP_MAX_D = 1024            # IGS_INTERP_MAX_D (include/igs_rast.h)
SORT_TILE = 2048               # radix_sort.h:15
SORT_MAX_BLOCKS = 256          # radix_sort.h:17


def interp_chunk(E):
    """motion.hip:24-29 interp_chunk: the backward's chunk length for E = N * K edges."""
    c = 64
    while c < 512 and c * 4 * 16 * 256 < E:
        c *= 2
    return c


def interp_index_bits(A):
    """motion.hip:41-42: bits of the inverse index's sort keys 0..A (A = an empty or out-of-range slot); ceil(bits / 8) radix passes."""
    bits = 1
    while (1 << bits) <= A:
        bits += 1
    return bits


def interp_index_passes(A):
    return (interp_index_bits(A) + 7) // 8


def radix_lands_in_b(bits):
    """radix_sort.h:25 radix_lands_in_b: a radix sort over `bits` key bits, 8 per pass, swaps its buffer pairs once per pass, so it ends
    in the second pair (kb, vb) after an odd number of passes and in the first (ka, va) after an even number (none included)."""
    return ((bits + 7) // 8) % 2 == 1


def interp_dv(D):
    """motion.hip:99 interp_dv: floats per lane of the row / chunk kernel instantiation that serves D."""
    return 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 8 if D <= 512 else 16


def sort_geometry(n):
    """radix_sort.hip:8-16 sort_per_block and the block count radix_sort_pairs takes from it: (blocks, elements per block) of one radix
    sort of n pairs."""
    nb = min((n + SORT_TILE - 1) // SORT_TILE, SORT_MAX_BLOCKS) or 1
    per = (n + nb - 1) // nb
    per = (per + SORT_TILE - 1) // SORT_TILE * SORT_TILE or SORT_TILE
    return (n + per - 1) // per or 1, per


# ---------------------------------------------------------------- exact-input cases of tests/test_gpu_motion_edges.py
# the in-degrees of the first anchors in the chunk-length cases: empty, one edge, and one either side of every chunk length and of two
# chunks, one list of many chunks (the rest of the anchors get random edges)
CHUNK_DEGREES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 150000)
CHUNK_SHAPES = {128: (132000, 8, 4), 256: (21100, 100, 5), 512: (42000, 100, 3)}      # chunk length: (N, K, D), A = 300
INDEX_PASS_ANCHORS = (255, 256, 65535, 65536)


def exact_margin(F, w, col, dout):
    """4 * the largest sum of |term| in any float32 accumulation of the forward and the backward on these inputs.  With integer F and
    dout and weights in {1, 1/2, 1/4} every term and every partial sum, in any order, is a multiple of 1/4 below that figure / 4, so
    all of them are exact in float32 while the figure stays below 2^24."""
    A, D = F.shape
    N, K = w.shape
    c = col.reshape(-1)
    ok = (c >= 0) & (c < A)
    fwd = interp_restate(F.double().abs(), w.double().abs(), col).max()
    per_anchor = torch.zeros(A, D, dtype=torch.float64)
    per_anchor.index_add_(0, c[ok], (w.double().abs().reshape(-1, 1) * dout.double().abs().repeat_interleave(K, 0))[ok])
    dwm = (dout.double().abs().max() * F.double().abs().max()) * D
    return 4.0 * max(float(fwd), float(per_anchor.max()), float(dwm))


def exact_interp_case(N, K, A, D, degrees=(), pad=0.02, oob=0, seed=0):
    """(F [A, D], w [N, K], col [N, K], dout [N, D]) on the CPU: integer F in [-50, 50) and dout in [-4, 4), weights in {1, 1/2, 1/4}.
    Anchor a < len(degrees) has exactly degrees[a] incoming edges; the other slots go to random anchors >= len(degrees), a fraction
    `pad` of them to -1 and `oob` of them to A + 7.  Asserts the exactness condition (exact_margin < 2^24)."""
    g = torch.Generator().manual_seed(seed)
    E, nd, fixed = N * K, len(degrees), int(sum(degrees))
    assert fixed + oob <= E and nd < A
    rest = torch.randint(nd, A, (E - fixed,), generator=g)
    rest[torch.rand(E - fixed, generator=g) < pad] = -1
    rest[:oob] = A + 7
    slots = torch.cat([torch.repeat_interleave(torch.arange(nd), torch.tensor(degrees, dtype=torch.long)), rest])
    col = slots[torch.randperm(E, generator=g)].reshape(N, K)
    F = torch.randint(-50, 50, (A, D), generator=g).float()
    w = 2.0 ** -torch.randint(0, 3, (N, K), generator=g).float()
    dout = torch.randint(-4, 4, (N, D), generator=g).float()
    assert exact_margin(F, w, col, dout) < 2 ** 24
    return F, w, col, dout


def in_degrees(col, A):
    c = col.reshape(-1)
    return torch.bincount(c[(c >= 0) & (c < A)], minlength=A)


# ---------------------------------------------------------------- derived bounds shared by the GPU tests
U = 2.0 ** -23                 # one float32 rounding per accumulated term, relative to the sum of the terms' magnitudes
U16 = 2.0 ** -11               # the one rounding of a float16 output


def interp_forward_bound(F, w, col):
    """K * 2^-23 * sum_k |w| |F|: K fmaf roundings, each below 2^-24 of a partial sum that the sum of magnitudes bounds."""
    return w.shape[1] * U * interp_restate(F.reshape(-1, F.shape[-1]).double().abs(), w.double().abs(), col) + 1e-30


def interp_truth_blocked(F, w, col, dout, block=16384):
    """Float64 forward and backward of interp_restate for the upstream gradient dout, in row blocks (no [N, K, D] temporary), with
    the sums of magnitudes the bounds need.  Returns a dict: out, out_abs [N, D]; dF, dF_abs [A, D]; dw, dw_abs [N, K]; deg (the
    largest in-degree)."""
    F64 = F.reshape(-1, F.shape[-1]).double()
    A, D = F64.shape
    w64 = w.reshape(w.shape[0], -1).double()
    N, K = w64.shape
    c = col.reshape(N, K)
    r = {"out": torch.empty(N, D, dtype=torch.float64, device=F.device), "dF": torch.zeros_like(F64), "dF_abs": torch.zeros_like(F64),
         "dw": torch.empty_like(w64)}
    r["out_abs"], r["dw_abs"] = torch.empty_like(r["out"]), torch.empty_like(w64)
    for a in range(0, N, block):
        cb, wb, gb = c[a:a + block], w64[a:a + block], dout[a:a + block].double()
        ok = ((cb >= 0) & (cb < A)).unsqueeze(-1)
        rows = torch.where(ok, F64[cb.clamp(0, A - 1)], torch.zeros((), dtype=torch.float64, device=F.device))      # [n, K, D]
        r["out"][a:a + block] = (rows * wb.unsqueeze(-1)).sum(1)
        r["out_abs"][a:a + block] = (rows.abs() * wb.abs().unsqueeze(-1)).sum(1)
        r["dw"][a:a + block] = (rows * gb.unsqueeze(1)).sum(-1)
        r["dw_abs"][a:a + block] = (rows.abs() * gb.abs().unsqueeze(1)).sum(-1)
        contrib = torch.where(ok, wb.unsqueeze(-1) * gb.unsqueeze(1), torch.zeros((), dtype=torch.float64, device=F.device)).reshape(-1, D)
        idx = cb.clamp(0, A - 1).reshape(-1)
        r["dF"].index_add_(0, idx, contrib)
        r["dF_abs"].index_add_(0, idx, contrib.abs())
    d = in_degrees(c, A)
    r["deg"] = int(d.max()) if d.numel() else 0
    return r


def interp_backward_bounds(truth, K, D, half):
    """(tol_dF [A, D], tol_dw [N, K]) from interp_truth_blocked's sums: deg * 2^-23 * sum |w| |g| for dF (plus the one float16 rounding
    of a half output, 2^-11 |dF|), D * 2^-23 * sum |g| |F| for dw (0 for a -1 or out-of-range slot, whose dw is exactly 0)."""
    tol_F = truth["deg"] * U * truth["dF_abs"] + (U16 * truth["dF"].abs() if half else 0) + 1e-30
    tol_w = D * U * truth["dw_abs"] + 1e-30
    return tol_F, tol_w


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over all elements (what the float tests print before they assert it is <= 1)."""
    if ref.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())      # (a zero bound admits a zero error only)


def deform_forward_ratios(xo, ro, xyz, mask, dx, xr, rr):
    """test_deform_forward_backward_against_float64's forward rules as error-to-bound ratios: xyz within one float32 rounding of
    |xyz| + |dxyz| (mask: the rows that took part), the quaternion within 1e-6."""
    bound = U * (xyz.double().abs() + torch.zeros_like(xr).index_put_((mask,), dx.double().abs(), accumulate=True))
    return worst_ratio(xo, xr, bound), worst_ratio(ro, rr, torch.full_like(rr, 1e-6))


def deform_grad_ratio(ga, gb, half):
    """The same test's gradient rule as a ratio: per row 1e-5 of the row's largest float64 gradient, plus 2^-10 |g| for a float16
    gradient; a float16 row whose true gradient exceeds 65504 (a residual below eps: g / 1e-12) must hold an inf and is left out."""
    ga = ga.double()
    if half:
        big = gb.abs().amax(1) > 65504
        assert torch.isinf(ga[big]).any(1).all()
        ga, gb = ga[~big], gb[~big]
    if gb.numel() == 0:
        return 0.0
    rowmax = gb.abs().amax(1, keepdim=True)
    tol = 1e-5 * rowmax + (2.0 ** -10 * gb.abs() if half else 0) + 1e-30
    return float(((ga - gb).abs() / tol).max())
