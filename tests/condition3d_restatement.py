"""PyTorch restatements of IGS.condition3D (igs/IGS.py:185-210 with ray_to_plucker :286-295, rsh_cart_3 :297-344, ModLN :259-284;
local_ray False) in this repository's words, and the error bounds the tests use.

  sh3                   -- the 16 real spherical harmonics of degree <= 3 as polynomials, index n (n + 1) + m.
  resize_bilinear       -- explicit corners of the half-pixel bilinear resize (include/igs_rast.h); F.interpolate is the second statement.
  ray_condition_restate -- cond [B*V, H, W, 33] in the inputs' dtype (use float64); keyword switches build the wrong variants.
  modln_restate         -- out [N, C, H, W] = LayerNorm_C(x) (1 + scale) + shift, biased variance from centred values.
  reference_composition -- the reference's sequence of torch calls (normalize, cross, two 16-way stacks, interpolate, LayerNorm on the
                           permuted view, the permute back) in the inputs' dtype: what tools/bench_condition3d.py times in float32.
  ray_condition_bound / modln_forward_bound / modln_backward_bounds -- per-element bounds on |float32 evaluation - float64 restatement|,
                           derived below from operation counts, not measured.
"""
import torch
import torch.nn.functional as F

u = 2.0 ** -24            # the unit roundoff of float32: one rounded operation has relative error <= u
HO = 1.0 + 2.0 ** -10     # covers the second-order terms of every product of (1 + k u) factors below (k <= 2100: (1 + u)^k - 1 <= k u HO)

# 1 / (2 sqrt(pi)), sqrt(3 / 4 pi), sqrt(15 / 4 pi), sqrt(5 / 16 pi), sqrt(35 / 32 pi), sqrt(105 / 4 pi), sqrt(21 / 32 pi), sqrt(7 / 16 pi)
K0, K1, K2, K20 = 0.282094791773878, 0.48860251190292, 1.09254843059208, 0.31539156525252
K3A, K3B, K3C, K30 = 0.590043589926644, 2.89061144264055, 0.457045799464466, 0.373176332590115


def sh3(v):
    """[..., 3] -> [..., 16]: Y_n^m at index n (n + 1) + m, odd orders with the Condon-Shortley sign, as polynomials (no normalisation)."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    x2, y2, z2 = x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, K0),
        -K1 * y, K1 * z, -K1 * x,
        K2 * (x * y), -K2 * (y * z), K20 * (3 * z2 - 1), -K2 * (x * z), 0.5 * K2 * (x2 - y2),
        -K3A * y * (3 * x2 - y2), K3B * (x * y) * z, -K3C * y * (5 * z2 - 1), K30 * z * (5 * z2 - 3), -K3C * x * (5 * z2 - 1),
        0.5 * K3B * z * (x2 - y2), -K3A * x * (x2 - 3 * y2)], -1)


def sh3_abs(v):
    """The same polynomials with every coefficient and every input replaced by its absolute value: an upper bound of every intermediate
    of any evaluation order of the expanded or factored forms."""
    x, y, z = v[..., 0].abs(), v[..., 1].abs(), v[..., 2].abs()
    x2, y2, z2 = x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, K0),
        K1 * y, K1 * z, K1 * x,
        K2 * x * y, K2 * y * z, K20 * (3 * z2 + 1), K2 * x * z, 0.5 * K2 * (x2 + y2),
        K3A * y * (3 * x2 + y2), K3B * x * y * z, K3C * y * (5 * z2 + 1), K30 * z * (5 * z2 + 3), K3C * x * (5 * z2 + 1),
        0.5 * K3B * z * (x2 + y2), K3A * x * (x2 + 3 * y2)], -1)


def plucker(rays, normalise=True, swap_cross=False):
    """(d, m): the unit direction d = dir / max(|dir|, 1e-12) and the moment m = origin x d."""
    o, d = rays[..., :3], rays[..., 3:6]
    if normalise:
        d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    m = torch.cross(d, o, dim=-1) if swap_cross else torch.cross(o, d, dim=-1)
    return d, m


def source_index(n_out, n_in, dtype, device, align_corners=False):
    i = torch.arange(n_out, dtype=dtype, device=device)
    if align_corners:
        return i * ((n_in - 1) / (n_out - 1)) if n_out > 1 else i * 0
    return ((i + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)


def resize_bilinear(depth, H, W, align_corners=False):
    """depth [N, Hd, Wd] -> [N, H, W]: four corners, the upper neighbour clamped to the last row / column."""
    N, Hd, Wd = depth.shape
    sy, sx = source_index(H, Hd, depth.dtype, depth.device, align_corners), source_index(W, Wd, depth.dtype, depth.device, align_corners)
    y0, x0 = sy.floor().clamp_max(Hd - 1).long(), sx.floor().clamp_max(Wd - 1).long()
    y1, x1 = (y0 + 1).clamp_max(Hd - 1), (x0 + 1).clamp_max(Wd - 1)
    ly, lx = (sy - y0).view(1, H, 1), (sx - x0).view(1, 1, W)
    top = depth[:, y0][:, :, x0] * (1 - lx) + depth[:, y0][:, :, x1] * lx
    bot = depth[:, y1][:, :, x0] * (1 - lx) + depth[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def ray_condition_restate(rays, depth, normalise=True, swap_cross=False, align_corners=False):
    """rays [B, V, H, W, 6], depth [B, V, Hd, Wd] -> cond [B*V, H, W, 33]."""
    B, V, H, W, _ = rays.shape
    d, m = plucker(rays, normalise, swap_cross)
    dep = resize_bilinear(depth.reshape(B * V, *depth.shape[2:]), H, W, align_corners)
    return torch.cat([sh3(d), sh3(m), dep.reshape(B, V, H, W, 1)], -1).reshape(B * V, H, W, 33)


def layer_norm_parts(x, eps, unbiased=False):
    """x [N, C, H, W] -> (mu, var, r, xhat) over the channel axis; the variance from centred values."""
    C = x.shape[1]
    mu = x.mean(1, keepdim=True)
    a = x - mu
    var = (a * a).sum(1, keepdim=True) / (C - 1 if unbiased else C)
    r = 1 / (var + eps).sqrt()
    return mu, var, r, a * r


def modln_restate(x, mod, weight, bias, eps, unbiased=False, swap_halves=False):
    """out [N, C, H, W] from x [N, C, H, W], mod [N, H, W, 2C] (shift first, scale second), weight / bias [C]."""
    C = x.shape[1]
    shift, scale = mod[..., :C].permute(0, 3, 1, 2), mod[..., C:].permute(0, 3, 1, 2)
    if swap_halves:
        shift, scale = scale, shift
    xh = layer_norm_parts(x, eps, unbiased)[3]
    return (xh * weight.view(1, C, 1, 1) + bias.view(1, C, 1, 1)) * (1 + scale) + shift


class AdaLNModule(torch.nn.Module):
    """LayerNorm over C channels plus the small MLP that maps the 33 condition channels to (shift, scale): the two attributes
    condition3d uses (`norm`, `mlp`), with the reference module's sizes (hidden width 128)."""

    def __init__(self, C, cond_dim=33, eps=1e-6, hidden=128):
        super().__init__()
        self.norm = torch.nn.LayerNorm(C, eps=eps)
        self.mlp = torch.nn.Sequential(torch.nn.Linear(cond_dim, hidden), torch.nn.SiLU(), torch.nn.Linear(hidden, 2 * C))

    @classmethod
    def from_arrays(cls, z):
        """From a fixture's stored parameters (norm_weight, norm_bias, mlp0_weight, mlp0_bias, mlp2_weight, mlp2_bias, eps)."""
        m = cls(z["norm_weight"].numel(), z["mlp0_weight"].shape[1], float(z["eps"]), z["mlp0_weight"].shape[0])
        with torch.no_grad():
            m.norm.weight.copy_(z["norm_weight"]); m.norm.bias.copy_(z["norm_bias"])
            m.mlp[0].weight.copy_(z["mlp0_weight"]); m.mlp[0].bias.copy_(z["mlp0_bias"])
            m.mlp[2].weight.copy_(z["mlp2_weight"]); m.mlp[2].bias.copy_(z["mlp2_bias"])
        return m


def reference_composition(motion_feature, rays, depth, module):
    """The reference's composition call for call, in the inputs' dtype: F.normalize, cross, cat, two 16-way stacks, cat, F.interpolate,
    cat, LayerNorm over a permuted (non-contiguous) view, the MLP, chunk, multiply, two adds, the permute back (a strided view)."""
    B, V = depth.shape[:2]
    dep = depth.reshape(B * V, 1, *depth.shape[2:])
    size = motion_feature.shape[-2:]
    o, d = rays[..., :3], rays[..., 3:6]
    d = F.normalize(d, p=2.0, dim=-1)
    ray = torch.cat((d, torch.cross(o, d, dim=-1)), dim=-1)
    ray = torch.cat((sh3(ray[..., :3]), sh3(ray[..., 3:6])), dim=-1)
    ray = ray.reshape(B * V, *ray.shape[2:])
    dep = F.interpolate(dep, size=size, mode="bilinear", align_corners=False).squeeze(dim=1)
    cond = torch.cat([ray, dep.unsqueeze(-1)], dim=-1)
    xp = motion_feature.permute(0, 2, 3, 1)
    shift, scale = module.mlp(cond).chunk(2, dim=-1)
    out = module.norm(xp) * (1 + scale) + shift
    return out.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------------------------
# Bounds.  Everything is evaluated in float64 on the float32 inputs; u = 2^-24, HO covers the second-order terms.
#
# Direction.  |dir|^2 is three products and two sums of non-negative terms (relative error <= 3 u), the square root halves that and rounds
#   (<= 2.5 u), the division rounds once more: every component of d has relative error <= 4 u.
# Moment.  A component of origin x d is two products and a difference (or a product and an fma) of inputs with relative error <= 4 u:
#   |d m_i| <= (4 + 2) u M_i,  M = |origin| x_abs |d| (the cross product with every term added: M_i >= |m_i|, and |M| <= 2 |origin|).
# Harmonics.  P is a polynomial of degree <= 3 with P_abs the same polynomial on absolute coefficients and inputs (sh3_abs).  A relative
#   perturbation e of every input of a monomial of degree k changes it by <= k e |monomial|, so
#       |P(d (1 + 4u)) - P(d)| <= 3 * 4 u P_abs(|d|),       |P(m + dm) - P(m)| <= 3 * 6 u P_abs(M)       (first order; HO)
#   and the evaluation itself is at most 10 rounded operations on partial results bounded by P_abs (the longest form: two squares, two
#   scalings, an offset, two products, a difference, and the roundings of two float32 coefficients):
#       |d Y(d)| <= (12 + 10) u P_abs(|d|) HO,      |d Y(m)| <= (18 + 10) u P_abs(M) HO.
# Depth.  The source coordinate fl(fl(s (i + 0.5)) - 0.5) with s = fl(Hd / H): the quotient, the product and the difference round
#   once each on values <= s (i + 0.5) + 0.5, so |d src_y| <= 3 u (Hd / H (i + 0.5) + 0.5) <= 3 u (Hd + 0.5).  The resize is continuous and
#   piecewise linear in the source coordinate, so a coordinate that lands in a neighbouring cell needs no special case:
#       |d depth| <= d src_y Ly + d src_x Lx + 10 u A
#   with Ly (Lx) the largest vertical (horizontal) difference of neighbouring pixels of the edge-replicated map over rows y0 - 1 .. y0 + 2
#   and columns x0 - 1 .. x0 + 2, and A the largest |depth| there (two weight differences, their complements, four products, three sums
#   <= 10 roundings of convex combinations).
# ------------------------------------------------------------------------------------------------------------------------------------
def ray_condition_bound(rays, depth):
    """[B*V, H, W, 33] float64."""
    B, V, H, W, _ = rays.shape
    r = rays.double()
    d, _ = plucker(r)
    o = r[..., :3].abs()
    da = d.abs()
    M = torch.stack([o[..., 1] * da[..., 2] + o[..., 2] * da[..., 1], o[..., 2] * da[..., 0] + o[..., 0] * da[..., 2],
                     o[..., 0] * da[..., 1] + o[..., 1] * da[..., 0]], -1)
    bd = 22 * u * HO * sh3_abs(da)
    bm = 28 * u * HO * sh3_abs(M)
    dep = depth.double().reshape(B * V, 1, *depth.shape[2:])
    Hd, Wd = dep.shape[-2:]
    sy = source_index(H, Hd, torch.float64, dep.device)
    sx = source_index(W, Wd, torch.float64, dep.device)
    y0, x0 = sy.floor().clamp_max(Hd - 1).long(), sx.floor().clamp_max(Wd - 1).long()
    pad = F.pad(dep, (2, 2, 2, 2), mode="replicate")                               # pixel (y, x) at [y + 2, x + 2]
    Ly = F.max_pool2d((pad[..., 1:, :] - pad[..., :-1, :]).abs(), kernel_size=(3, 4), stride=1)[:, 0]       # [N, Hd + 1, Wd + 1]
    Lx = F.max_pool2d((pad[..., :, 1:] - pad[..., :, :-1]).abs(), kernel_size=(4, 3), stride=1)[:, 0]
    A = F.max_pool2d(pad.abs(), kernel_size=(4, 4), stride=1)[:, 0]
    pick = lambda t: t[:, y0 + 1][:, :, x0 + 1]                                     # noqa: E731  (the 4 x 4 block around cell (y0, x0))
    ey = (3 * u * (sy + 1.0)).view(1, H, 1)
    ex = (3 * u * (sx + 1.0)).view(1, 1, W)
    bdep = (ey * pick(Ly) + ex * pick(Lx) + 10 * u * pick(A)) * HO + 1e-300
    return torch.cat([bd, bm, bdep.reshape(B, V, H, W, 1)], -1).reshape(B * V, H, W, 33)


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm + modulation, per pixel over its C channels (mean = the mean over the channels), first order, then doubled:
#   d mu   = (C + 1) u mean|x|                         C - 1 sums and the division, any summation order
#   a = x - mu:      d a = d mu + u |a|
#   d var  = 2 mean|a| d mu + d mu^2 + (C + 6) u var   the squares of perturbed a, then C + 1 roundings of the sum and a few of the squares
#   r = (var + eps)^-1/2:   d r = r (d var / (2 (var + eps)) + 4 u)          the sum with eps, the root, the reciprocal
#   xh = a r:        d xh = d a r + |a| d r + u |xh|
#   y = xh w + b:    d y = |w| d xh + 2 u |xh w| + u |y|
#   out = y (1 + s) + t:    bound = 2 (d y |1 + s| + 3 u (|y (1 + s)| + |t|) + u |out|)
# A variance formed as E[x^2] - mu^2 in float32 violates this when |mu| >> sd, the unbiased variance when C is small: the tests check both.
# ------------------------------------------------------------------------------------------------------------------------------------
def _forward_terms(x, mod, weight, bias, eps):
    x, mod, weight, bias = x.double(), mod.double(), weight.double(), bias.double()
    C = x.shape[1]
    w, b = weight.view(1, C, 1, 1), bias.view(1, C, 1, 1)
    t, s = mod[..., :C].permute(0, 3, 1, 2), mod[..., C:].permute(0, 3, 1, 2)
    mu, var, r, xh = layer_norm_parts(x, eps)
    a = x - mu
    dmu = (C + 1) * u * x.abs().mean(1, keepdim=True)
    da = dmu + u * a.abs()
    dvar = 2 * a.abs().mean(1, keepdim=True) * dmu + dmu * dmu + (C + 6) * u * var
    dr = r * (dvar / (2 * (var + eps)) + 4 * u)
    dxh = da * r + a.abs() * dr + u * xh.abs()
    y = xh * w + b
    dy = w.abs() * dxh + 2 * u * (xh * w).abs() + u * y.abs()
    return dict(C=C, w=w, b=b, t=t, s=s, r=r, dr=dr, xh=xh, dxh=dxh, y=y, dy=dy)


def modln_forward_bound(x, mod, weight, bias, eps):
    """[N, C, H, W] float64."""
    k = _forward_terms(x, mod, weight, bias, eps)
    y, s, t = k["y"], k["s"], k["t"]
    out = y * (1 + s) + t
    return 2 * (k["dy"] * (1 + s).abs() + 3 * u * ((y * (1 + s)).abs() + t.abs()) + u * out.abs()) + 1e-300


def half_rounding(ref):
    """One rounding to the nearest float16: 2^-11 relative, never finer than half the subnormal spacing 2^-24."""
    return torch.clamp(2.0 ** -11 * ref.abs(), min=2.0 ** -25)


# ------------------------------------------------------------------------------------------------------------------------------------
# Backward, for the upstream gradient g, M pixels in all; gh = g (1 + s) (two roundings), gw = gh w (a third); first order, doubled at the end:
#   d shift = g                                         a copy: exact
#   d scale = g y:          |g| d y + u |g y|
#   d bias  = sum_px gh:    (M + 1) u sum|gh|                                    two roundings per term, M - 1 of the sum in any order
#   d weight = sum_px gh xh:   sum |gh| d xh + (M + 2) u sum|gh xh|
#   m1 = mean_c gw:         d m1 = (C + 3) u mean|gw|
#   m2 = mean_c gw xh:      d m2 = mean(|gw| d xh) + (C + 4) u mean|gw xh|
#   t = gw - m1 - xh m2:    d t = 3 u |gw| + d m1 + d xh |m2| + |xh| d m2 + u |xh m2| + 4 u (|gw| + |m1| + |xh m2|)
#                           (the last term: the differences, and the scalings by C and 1 / C of the equivalent form that sums before it divides)
#   d x = r t:              d r |t| + r d t + u |d x|
# A float16 x or mod adds one rounding of the corresponding output to half (half_rounding).
# ------------------------------------------------------------------------------------------------------------------------------------
def modln_backward_restate(x, mod, weight, bias, eps, g):
    """(dx, dmod, dweight, dbias) by autograd through modln_restate, in the inputs' dtype (use float64)."""
    x, mod, weight, bias = (t.detach().clone().requires_grad_(True) for t in (x, mod, weight, bias))
    modln_restate(x, mod, weight, bias, eps).backward(g)
    return x.grad, mod.grad, weight.grad, bias.grad


def modln_backward_bounds(x, mod, weight, bias, eps, g, half_x=False, half_mod=False):
    """dict(dx [N, C, H, W], dmod [N, H, W, 2C], dweight [C], dbias [C]) float64."""
    k = _forward_terms(x, mod, weight, bias, eps)
    C, w, s, r, dr, xh, dxh, y, dy = k["C"], k["w"], k["s"], k["r"], k["dr"], k["xh"], k["dxh"], k["y"], k["dy"]
    g = g.double()
    M = x.shape[0] * x.shape[2] * x.shape[3]
    gh = g * (1 + s)
    gw = gh * w
    dscale = 2 * (g.abs() * dy + u * (g * y).abs())
    dmod = torch.cat([torch.zeros_like(dscale), dscale], 1).permute(0, 2, 3, 1) + 1e-300
    dbias = 2 * (M + 1) * u * gh.abs().sum((0, 2, 3)) + 1e-300
    dweight = 2 * ((gh.abs() * dxh).sum((0, 2, 3)) + (M + 2) * u * (gh * xh).abs().sum((0, 2, 3))) + 1e-300
    m1, m2 = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
    dm1 = (C + 3) * u * gw.abs().mean(1, keepdim=True)
    dm2 = (gw.abs() * dxh).mean(1, keepdim=True) + (C + 4) * u * (gw * xh).abs().mean(1, keepdim=True)
    t = gw - m1 - xh * m2
    dt = 3 * u * gw.abs() + dm1 + dxh * m2.abs() + xh.abs() * dm2 + u * (xh * m2).abs() + 4 * u * (gw.abs() + m1.abs() + (xh * m2).abs())
    dx = 2 * (dr * t.abs() + r * dt + u * (r * t).abs()) + 1e-300
    if half_x:
        dx = dx + half_rounding(r * t)
    if half_mod:
        dmod = dmod + half_rounding(torch.cat([g, g * y], 1).permute(0, 2, 3, 1))
    return dict(dx=dx, dmod=dmod, dweight=dweight, dbias=dbias)
