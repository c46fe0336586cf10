"""The fused condition3D backward (igs_amd/csrc/cond_fused_bwd.hip, igs_condition3d_bwd) restated in float64, and its derived bound.
Nothing here is fitted to a run: the module composes what the repository already has.

Per pixel, g = d out[:, p], n = xh w + b the normalised, affine value, shift / scale = the halves of mod = W2 silu(W1 cond + b1) + b2:

    d shift = g        d scale = g n        d n = g (1 + scale)        d w = sum_px d n xh        d b = sum_px d n
    d xh = d n w       d x = r (d xh - mean_C(d xh) - xh mean_C(d xh xh))
    d h = W2^T [d shift ; d scale]          d z1 = d h silu'(z1)
    d W2 = sum_px [d shift ; d scale] (x) h     d b2 = sum_px [d shift ; d scale]     d W1 = sum_px d z1 (x) cond     d b1 = sum_px d z1

The bound, u = 2^-24, a hat marks the kernel's value and e_v >= |v^ - v|:

  cond, z1, h, mod   condition3d_fused_restatement.mlp_with_bound's recurrence from e0 = ray_condition_bound gives e_cond, e_z1, e_h and
                     E = (E_shift, E_scale); the kernel recomputes these with the forward's statements.
  LayerNorm part     condition3d_restatement.modln_backward_bounds at the exact mod64 bounds d scale, d w, d b and d x for the float32
                     evaluation at the kernel's own scale.  What E_scale adds, first order times HO:
                         e(d n) = |g| E_scale                     d b: sum_px |g| E_scale          d w: sum_px |g| E_scale |xh|
                         e(d xh) = |g| E_scale |w| =: q           d x: r (q + mean_C q + |xh| mean_C(q |xh|))
                     d shift = g is a copy, d scale = g n does not see the scale.
  MLP part           decoder_grad_restatement's recurrence, started from the upstream error (0 for d shift, the d scale bound above):
                         d W2, d b2: P' terms, operands [d shift ; d scale] and h;    d h: an fma chain of 2C terms through W2;
                         silu': e_a = 0.5 e_z1 + u (SILUP_C (|a| + 0.5 e_z1) + SILUP_ABS), d z1 = d h a rounded once;
                         d W1, d b1: P' terms, operands d z1 and cond.
                     P' is the number of terms of a sum over pixels: the rows the kernel walks (32 per started group of 32 pixels of an
                     image; a masked lane adds +0) plus the slice partials of the final reduce (at most SLICES).
                     half: cond and h are rounded to half as in the forward, g, g n and d z1 once each as matrix operands
                     (2^-11 |v^| + 2^-25); the bias sums take the unrounded float32 values; d x is rounded once to a half x's dtype.
"""
import numpy as np
import torch

import condition3d_restatement as CR
import condition3d_fused_restatement as FR
import decoder_restatement as DR
import decoder_grad_restatement as DGR

U, UH, SUBH = DR.U, DR.UH, DR.SUBH
CHUNK_ROWS = 16384                # IGS_COND_BWD_CHUNK_ROWS
SLICE_ROWS = 256                  # CB_SLICE_ROWS
SLICES = CHUNK_ROWS // SLICE_ROWS
MUTATIONS = ("swap_dw2_halves", "silu_grad_one", "unbiased_dx", "drop_depth_column", "dscale_without_n")


def padded_rows(N, H, W):
    return N * 32 * ((H * W + 31) // 32)


def _operand(v, ev, half):
    """(|v^| bound, error) of v^ as a matrix operand: rounded to half on the half path."""
    if half:
        ev = ev + UH * (np.abs(v) + ev) + SUBH
    return np.abs(v) + ev, ev


def restate(x, rays, depth, module, g, half=False, mutate=None):
    """(grads, bounds): dicts of float64 CPU tensors dx [N, C, H, W], dW1 [hidden, 33], db1, dW2 [2C, hidden], db2, dnw [C], dnb [C] and
    dmod [N, H, W, 2C] (= [d shift, d scale], which the kernel keeps to itself).  x [N, C, H, W] float32 / float16, rays [B, V, H, W, 6],
    depth [B, V, Hd, Wd], g [N, C, H, W] float32.  half: the float16 MLP instance (its weights are the half roundings of the module's).
    mutate: one of MUTATIONS, for the tests of the bound itself -- the gradients of a wrong backward."""
    assert mutate is None or mutate in MUTATIONS, mutate
    x, rays, depth, g = x.detach().cpu(), rays.detach().cpu(), depth.detach().cpu(), g.detach().cpu().double()
    N, C, H, W = x.shape
    P = N * H * W
    terms = padded_rows(N, H, W) + SLICES
    f = FR.restate(x, rays, depth, module, half)
    W1, b1, W2, b2 = FR.module_arrays(module, half)
    hidden = W1.shape[0]
    b1 = np.zeros(hidden) if b1 is None else b1
    cond = f["cond64"].reshape(P, 33).numpy()
    e0 = f["bcond"].reshape(P, 33).numpy().astype(np.float64)
    mod64, E = f["mod64"], f["E"]
    nw, nb, eps = module.norm.weight.detach().cpu().double(), module.norm.bias.detach().cpu().double(), module.norm.eps
    xf = x.float().double()

    # ---- the LayerNorm part ----
    w4, b4 = nw.view(1, C, 1, 1), nb.view(1, C, 1, 1)
    mu, var, r, xh = CR.layer_norm_parts(xf, eps)
    n = xh * w4 + b4
    scale = mod64[..., C:].permute(0, 3, 1, 2)
    dshift, dscale = g, g * (1.0 if mutate == "dscale_without_n" else n)
    dn = g * (1 + scale)
    dnw, dnb = (dn * xh).sum((0, 2, 3)), dn.sum((0, 2, 3))
    dxh = dn * w4
    if mutate == "unbiased_dx":
        r_dx, xh_dx = CR.layer_norm_parts(xf, eps, unbiased=True)[2:]
        dx = r_dx * (dxh - dxh.mean(1, keepdim=True) - xh_dx * (dxh * xh_dx).sum(1, keepdim=True) / max(C - 1, 1))
    else:
        dx = r * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    lb = CR.modln_backward_bounds(x.float(), mod64, nw.float(), nb.float(), eps, g.float(), half_x=x.dtype == torch.float16)
    e_scale = E[..., C:].permute(0, 3, 1, 2)
    q = g.abs() * e_scale * w4.abs()
    moved = dict(dx=CR.HO * r * (q + q.mean(1, keepdim=True) + xh.abs() * (q * xh.abs()).mean(1, keepdim=True)),
                 dnw=CR.HO * (g.abs() * e_scale * xh.abs()).sum((0, 2, 3)), dnb=CR.HO * (g.abs() * e_scale).sum((0, 2, 3)))
    if x.dtype == torch.float16:
        moved["dx"] = moved["dx"] * (1 + 2.0 ** -11)                     # the rounding of d x also takes the moved value
    b_dx, b_dnw, b_dnb = lb["dx"] + moved["dx"], lb["dweight"] + moved["dnw"], lb["dbias"] + moved["dnb"]
    dmod = torch.cat([dshift, dscale], 1).permute(0, 2, 3, 1)            # [N, H, W, 2C]
    b_dmod = lb["dmod"]

    # ---- the MLP part ----
    h0, e_h0 = cond, e0
    if half:
        e_h0 = e_h0 + UH * (np.abs(h0) + e_h0) + SUBH
    z1 = h0 @ W1.T + b1
    hh0 = np.abs(h0) + e_h0
    ez1 = e_h0 @ np.abs(W1).T + DR.gamma(34) * (hh0 @ np.abs(W1).T + np.abs(b1))
    h1 = DR.silu(z1)
    e_h1 = 1.1 * ez1 + DR.SILU_A * U * (np.abs(h1) + 1.1 * ez1) + 2.0 ** -125 * (np.abs(z1) + ez1)
    h1o, e_h1o = _operand(h1, e_h1, half)

    gm, egm = dmod.reshape(P, 2 * C).numpy(), b_dmod.reshape(P, 2 * C).numpy()
    gmo, egmo = _operand(gm, egm, half)
    dW2 = gm.T @ h1
    if mutate == "swap_dw2_halves":
        dW2 = np.concatenate([dW2[C:], dW2[:C]], 0)
    b_dW2 = egmo.T @ h1o + np.abs(gm).T @ e_h1o + DR.gamma(terms + 1) * (gmo.T @ h1o)
    db2 = gm.sum(0)
    b_db2 = egm.sum(0) + DR.gamma(terms) * (np.abs(gm) + egm).sum(0)
    dh = gm @ W2
    e_dh = egmo @ np.abs(W2) + DR.gamma(2 * C + 1) * (gmo @ np.abs(W2))
    a = np.ones_like(z1) if mutate == "silu_grad_one" else DGR.silu_grad(z1)
    ea = 0.5 * ez1 + U * (DGR.SILUP_C * (np.abs(a) + 0.5 * ez1) + DGR.SILUP_ABS)
    dz1 = dh * a
    e_dz1 = np.abs(a) * e_dh + (np.abs(dh) + e_dh) * ea + U * (np.abs(dh) + e_dh) * (np.abs(a) + ea)
    dz1o, e_dz1o = _operand(dz1, e_dz1, half)
    dW1 = dz1.T @ h0
    if mutate == "drop_depth_column":
        dW1 = dW1.copy()
        dW1[:, 32] = 0.0
    b_dW1 = e_dz1o.T @ hh0 + np.abs(dz1).T @ e_h0 + DR.gamma(terms + 1) * (dz1o.T @ hh0)
    db1 = dz1.sum(0)
    b_db1 = e_dz1.sum(0) + DR.gamma(terms) * (np.abs(dz1) + e_dz1).sum(0)

    t = torch.from_numpy
    grads = dict(dx=dx, dW1=t(dW1), db1=t(db1), dW2=t(dW2), db2=t(db2), dnw=dnw, dnb=dnb, dmod=dmod)
    bounds = dict(dx=b_dx, dW1=t(b_dW1) + 1e-300, db1=t(b_db1) + 1e-300, dW2=t(b_dW2) + 1e-300, db2=t(b_db2) + 1e-300, dnw=b_dnw, dnb=b_dnb,
                  dmod=b_dmod, moved=moved)                              # moved: what E_scale alone adds to dx, dnw, dnb
    return grads, bounds


NAMES = ("dx", "dW1", "db1", "dW2", "db2", "dnw", "dnb")


def module_grads(x, module):
    """The seven gradients as autograd left them: x.grad and the module's parameters' .grad, in NAMES' order (a missing one: None)."""
    m = module.mlp
    return dict(zip(NAMES, (x.grad, m[0].weight.grad, m[0].bias.grad, m[2].weight.grad, m[2].bias.grad, module.norm.weight.grad,
                            module.norm.bias.grad)))


def worst_ratios(got, grads, bounds, names=NAMES):
    """{name: max |got - restated| / bound} (condition3d_fused_restatement.worst per tensor)."""
    return {k: FR.worst(got[k], grads[k], bounds[k]) for k in names}
