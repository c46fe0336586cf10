"""The fused condition3D forward (igs_amd/csrc/cond_fused.hip, igs_condition3d_fwd) restated in float64, and its derived bound.  Nothing
here is fitted to a run: the module composes what the repository already has.

  cond64, bcond   condition3d_restatement.ray_condition_restate / ray_condition_bound: the 33 channels and |float32 kernel - cond64|.
  mod64, E        ModLN's MLP, Linear(33, hidden) . SiLU . Linear(hidden, 2C), with decoder_restatement.forward_with_bound's recurrence
                  started from the input error e0 = bcond instead of zero:
                      a Linear of K inputs as an fma chain of K + 1 terms from the bias in any order (float32: 32 terms on the matrix
                      cores and one fma for the depth channel; float16: the matrix cores' float32 accumulators):
                          |z^ - z| <= |W| e + gamma(K + 1) (|W| |h^| + |b|),   |h^| <= |h| + e
                      SiLU: e <- 1.1 ez + SILU_A u (|s| + 1.1 ez) + 2^-125 (|z| + ez)
                  The float16 instance rounds cond to half once (e0 += 2^-11 |cond^| + 2^-25) and h once, as the operand of layer 2
                  (ez += |W2| (2^-11 |h^| + 2^-25)); its weights are the half roundings of the module's, which is what the restatement
                  then multiplies by; mod itself is NOT rounded (it goes from the accumulators into the modulation), so there is no final
                  store term.  E[..., :C] = E_shift, E[..., C:] = E_scale.
  out64, bound    out64 = modln_restate(x, mod64); with y the normalised, affine value
                      |out - out64| <= modln_forward_bound(x, mod64, ...) + (|y| E_scale + E_shift) HO
                  (the float32 evaluation of y (1 + s) + t at the kernel's own s, t, plus what the error of s and t moves the result;
                  HO covers the products of the two).  A float16 x is compared on its widened values.
"""
import numpy as np
import torch

import condition3d_restatement as CR
import decoder_restatement as DR


def mlp_with_bound(cond, e0, W1, b1, W2, b2, half=False):
    """(mod64, E) float64 [P, 2C] from cond [P, 33] and its error bound e0 [P, 33] (numpy float64).  half: the float16 instance; W1, W2 are
    then expected to hold half values already."""
    h, e = np.asarray(cond, np.float64), np.asarray(e0, np.float64)
    if half:
        e = e + DR.UH * (np.abs(h) + e) + DR.SUBH                       # cond rounded to half as layer 1's operand
    for l, (W, b, on) in enumerate(((W1, b1, True), (W2, b2, False))):
        W = np.asarray(W, np.float64)
        b = np.zeros(W.shape[0]) if b is None else np.asarray(b, np.float64)
        K = W.shape[1]
        z = h @ W.T + b
        hh = np.abs(h) + e                                               # >= |h^|
        ez = e @ np.abs(W).T + DR.gamma(K + 1) * (hh @ np.abs(W).T + np.abs(b))
        if half and l > 0:
            ez = ez + (DR.UH * hh + DR.SUBH) @ np.abs(W).T               # h rounded to half as layer 2's operand
        if on:
            s = DR.silu(z)
            h, e = s, 1.1 * ez + DR.SILU_A * DR.U * (np.abs(s) + 1.1 * ez) + 2.0 ** -125 * (np.abs(z) + ez)
        else:
            h, e = z, ez
    return h, e


def module_arrays(module, half=False):
    """(W1, b1, W2, b2) float64 numpy of a ModLN-shaped module's MLP; half: the weights rounded to half first, as the kernel holds them."""
    l0, l2 = module.mlp[0], module.mlp[2]
    wt = (lambda t: t.detach().cpu().half().double().numpy()) if half else (lambda t: t.detach().cpu().double().numpy())
    bt = lambda t: None if t is None else t.detach().cpu().double().numpy()          # noqa: E731
    return wt(l0.weight), bt(l0.bias), wt(l2.weight), bt(l2.bias)


def restate(x, rays, depth, module, half=False):
    """dict(cond64, bcond, mod64 [N, H, W, 2C], E, out64 [N, C, H, W], bound) as float64 CPU tensors.  x [N, C, H, W] float32 / float16,
    rays [B, V, H, W, 6], depth [B, V, Hd, Wd] float32 (any device); module: .norm (LayerNorm(C)) and .mlp."""
    x, rays, depth = x.detach().cpu(), rays.detach().cpu(), depth.detach().cpu()
    N, C, H, W = x.shape
    cond64 = CR.ray_condition_restate(rays.double(), depth.double())
    bcond = CR.ray_condition_bound(rays, depth)
    W1, b1, W2, b2 = module_arrays(module, half)
    mod, E = mlp_with_bound(cond64.reshape(-1, 33).numpy(), bcond.reshape(-1, 33).numpy(), W1, b1, W2, b2, half)
    mod64, E = torch.from_numpy(mod).reshape(N, H, W, 2 * C), torch.from_numpy(E).reshape(N, H, W, 2 * C)
    w, b, eps = module.norm.weight.detach().cpu(), module.norm.bias.detach().cpu(), module.norm.eps
    xf = x.float()                                                       # a float16 x: its widened values (exact)
    out64 = CR.modln_restate(xf.double(), mod64, w.double(), b.double(), eps)
    y = CR.layer_norm_parts(xf.double(), eps)[3] * w.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1)
    e_shift, e_scale = E[..., :C].permute(0, 3, 1, 2), E[..., C:].permute(0, 3, 1, 2)
    bound = CR.modln_forward_bound(xf, mod64, w, b, eps) + (y.abs() * e_scale + e_shift) * CR.HO
    return dict(cond64=cond64, bcond=bcond, mod64=mod64, E=E, out64=out64, bound=bound)


def worst(got, want, bound):
    """max |got - want| / bound over every element (0 / 0 = 0; a NaN or an inf in got counts as inf)."""
    d = (got.detach().cpu().double() - want).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    r = torch.where(torch.isfinite(d), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def pack_restate(W1, W2, C, half):
    """The packed weights from the header's definition: W1 [hidden, 33], W2[:C], W2[C:], each in decoder_restatement.pack_tile_order."""
    W1, W2 = np.asarray(W1), np.asarray(W2)
    return np.concatenate([DR.pack_tile_order(W1, half), DR.pack_tile_order(W2[:C], half), DR.pack_tile_order(W2[C:], half)])
