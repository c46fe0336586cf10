"""Float64 restatement of the N > 1 colour exchange (igs_amd/csrc/sh_exchange.hip: sh_grad_views_kernel<ADAM>, behind
igs_sh_grad_from_view_colors, igs_adam_sh_from_view_colors and igs_adam_exchange_step), the bounds a float32 evaluation is held to,
the launch geometry restated, and the seeded cases of tests/test_exchange_host.py (CPU) and tests/test_gpu_exchange_edges.py (MI355X).

    dL/dSH[p][k][c] = sum over the views v that see p of  clamp(b_k(dir_v(p)) * g_v[p][c]),      dir_v(p) = (mean_p - campos_v) / |...|

with b_k the real SH basis of oracle/torch_oracle.py (`sh_basis`), k < min((D + 1)^2, M); rows beyond the active degree are +0.0; a
view whose three colour gradients of p are all zero (either sign) does not see p.

The bound (`rebuild_allowance`).  u = 2^-24 is the unit roundoff of float32.  Every float32 operation below is rounded to nearest
(the library is built without fast-math: division and sqrtf are correctly rounded), a contraction to fma only removes roundings.
Count of roundings, each relative to the quantity named:

  normalisation, per component x of the direction                                                                   5.5 u |x|
      the subtraction mean - campos: 1 on the component; the same subtractions seen through the length: 1;
      x x + y y + z z: one product and two additions of non-negative terms = 3 on the sum, 1.5 after the root; sqrtf 1; the division 1
  a monomial of degree d <= 3 in x, y, z inherits d * 5.5                                                          16.5 u |monomial|
  the polynomial's own arithmetic, worst form C z (2 zz - 3 xx - 3 yy)                                              7   u B_k
      the squares 1, the scaling 3 xx 1 (2 zz and 4 zz are exact), two additions 2 -- each relative to the sum of the |terms|,
      which is what B_k (below) holds --, C z 1, the constant's own float32 rounding 1, the outer product 1
  the product b_k g                                                                                                  1   u |b_k g|
  V - 1 additions into the accumulator (the first one, into +0, is exact), each relative to a partial sum
      that is at most sum_v |b_k g_v|                                                                             V - 1

  K(V) = 25 + (V - 1):  16.5 + 7 + 1 = 24.5 per term, rounded up to 25 for the second-order terms (25 u)^2 / 2 and below.
  The clamp is monotone and 1-Lipschitz: it passes an error on unchanged or smaller.

  |float32 - float64|  <=  K(V) * u * sum_v B_k(|dir_v|) * |g_v|

B_k is basis polynomial k with every monomial and every constant in absolute value, at (|x|, |y|, |z|): the cancelling forms
2 zz - xx - yy, xx - 3 yy, ... count at their full size, which is what the additions' errors are relative to.
tests/test_exchange_host.py checks on the CPU that a float32 evaluation in the kernel's order stays inside the bound on every GPU
case, and that three wrong variants do not.
"""
import math
from collections import namedtuple

import torch

from oracle import torch_oracle as TO

U32 = 2.0 ** -24
K_TERM = 25.0          # per-term roundings (see above); K(V) = K_TERM + (V - 1)
MAX_VIEWS = 64
WG = 128               # Gaussians per workgroup of sh_grad_views_kernel


def K_of(V):
    return K_TERM + max(V - 1, 0)


def _dirs(means, campos_v):
    d = means.double() - campos_v.double()
    return d / d.norm(dim=1, keepdim=True)


def _seen(g):
    return (g != 0).any(dim=1)          # (-0.0 != 0 is False; a NaN is "seen")


def rebuild_sh(D, M, means, campos, gc, clamp):
    """float64 [P, M, 3].  means [P, 3], campos [V, 3], gc [V, P, 3] (float32 values), clamp 0 = off."""
    P = means.shape[0]
    used = min((D + 1) ** 2, M)
    out = torch.zeros((P, M, 3), dtype=torch.float64)
    for v in range(gc.shape[0]):
        g = gc[v].double()
        b = TO.sh_basis(D, _dirs(means, campos[v]))[:, :used]
        t = b[:, :, None] * g[:, None, :]
        if clamp > 0:
            t = t.clamp(-clamp, clamp)
        t = torch.where(_seen(gc[v])[:, None, None], t, torch.zeros_like(t))
        out[:, :used] += t
    return out


def abs_basis(D, a):
    """B_k at a = (|x|, |y|, |z|) [P, 3]: sh_basis with every monomial and constant in absolute value.  [P, (D + 1)^2]"""
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    C1, C2, C3 = abs(TO.C1), [abs(c) for c in TO.C2], [abs(c) for c in TO.C3]
    B = [torch.full_like(x, abs(TO.C0))]
    if D > 0:
        B += [C1 * y, C1 * z, C1 * x]
    if D > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz + xx + yy), C2[3] * xz, C2[4] * (xx + yy)]
    if D > 2:
        B += [C3[0] * y * (3 * xx + yy), C3[1] * xy * z, C3[2] * y * (4 * zz + xx + yy), C3[3] * z * (2 * zz + 3 * xx + 3 * yy),
              C3[4] * x * (4 * zz + xx + yy), C3[5] * z * (xx + yy), C3[6] * x * (xx + 3 * yy)]
    return torch.stack(B, 1)


def rebuild_allowance(D, M, means, campos, gc):
    """float64 [P, M, 3]: K(V) u sum_v B_k(|dir_v|) |g_v| (module docstring); exactly 0 where the result is an exact zero."""
    P, V = means.shape[0], gc.shape[0]
    used = min((D + 1) ** 2, M)
    s = torch.zeros((P, M, 3), dtype=torch.float64)
    for v in range(V):
        b = abs_basis(D, _dirs(means, campos[v]).abs())[:, :used]
        s[:, :used] += b[:, :, None] * gc[v].double().abs()[:, None, :]
    return K_of(V) * U32 * s


def rebuild_f32(D, M, means, campos, gc, clamp, variant=None):
    """The same sum evaluated in float32 in the kernel's order of operations (CPU).  `variant` names a WRONG evaluation the bound has
    to reject: "flip_c3" (the sign of the last degree-3 constant), "unnormalised" (direction not divided by its length),
    "clamp_after_sum" (the clamp applied to the sum instead of per view)."""
    f = torch.float32
    P = means.shape[0]
    used = min((D + 1) ** 2, M)
    C0, C1 = torch.tensor(TO.C0, dtype=f), torch.tensor(TO.C1, dtype=f)
    C2, C3 = [torch.tensor(c, dtype=f) for c in TO.C2], [torch.tensor(c, dtype=f) for c in TO.C3]
    if variant == "flip_c3":
        C3[6] = -C3[6]
    acc = torch.zeros((P, M, 3), dtype=f)
    for v in range(gc.shape[0]):
        d = means.to(f) - campos[v].to(f)
        ln = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt()
        if variant == "unnormalised":
            ln = torch.ones_like(ln)
        x, y, z = d[:, 0] / ln, d[:, 1] / ln, d[:, 2] / ln
        B = [C0.expand(P)]
        if D > 0:
            B += [-C1 * y, C1 * z, -C1 * x]
        if D > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            B += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
        if D > 2:
            B += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                  C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)]
        b = torch.stack(B, 1)[:, :used]
        t = b[:, :, None] * gc[v].to(f)[:, None, :]
        if clamp > 0 and variant != "clamp_after_sum":
            t = t.clamp(-clamp, clamp)
        t = torch.where(_seen(gc[v])[:, None, None], t, torch.zeros_like(t))
        acc[:, :used] += t
    if clamp > 0 and variant == "clamp_after_sum":
        acc = acc.clamp(-clamp, clamp)
    return acc


# ---------------------------------------------------------------- Adam
def _bars():
    from test_gpu_loss_optim_edges import ADAM_BARS, BETAS, EPS      # the project's own bars and Adam constants (not copied)
    return ADAM_BARS, BETAS, EPS


def adam_constants():
    _, betas, eps = _bars()
    return betas, eps


def adam_formula(p, m, v, g, lr, t, betas, eps):
    """One step of torch.optim.Adam written out in differentiable torch operations (float64); t = the 1-based number of the step."""
    b1, b2 = betas
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def adam_reference(p0, m0, v0, t0, grads, lr):
    """torch.optim.Adam in float64 on float64 gradients, started after t0 completed steps from the moments (m0, v0).
    Returns (param, dict(exp_avg, exp_avg_sq)) after len(grads) steps."""
    _, betas, eps = _bars()
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    opt.state[p] = dict(step=torch.tensor(float(t0)), exp_avg=m0.double().clone(), exp_avg_sq=v0.double().clone())
    for g in grads:
        p.grad = g.double().clone()
        opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t0 + len(grads)
    return p.detach(), dict(exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"])


def adam_allowance(p0, m0, v0, t0, grads, grad_allow, lr):
    """Allowances for (param, exp_avg, exp_avg_sq) after len(grads) steps: check_adam's bars (rtol |ref| + atol) plus the gradient
    allowances carried through the update to first order, sum_s |d out / d g_s| * grad_allow_s, the derivative by autograd on
    `adam_formula` (elementwise, so the gradient of out.sum() is the per-element derivative).  An element whose views nearly cancel
    has a large RELATIVE gradient error by construction; exp_avg_sq >= ~1e-8 (the builders' starting moments) bounds the derivative.
    Returns (allow_p, allow_m, allow_v, (p, m, v) of the formula)."""
    bars, betas, eps = _bars()
    gs = [g.double().clone().requires_grad_(True) for g in grads]
    p, m, v = p0.double(), m0.double(), v0.double()
    for s, g in enumerate(gs):
        p, m, v = adam_formula(p, m, v, g, lr, t0 + 1 + s, betas, eps)
    out = []
    for name, t, scale in (("param", p, lr), ("exp_avg", m, float(m.detach().abs().max()) if m.numel() else 0.0),
                           ("exp_avg_sq", v, float(v.detach().abs().max()) if v.numel() else 0.0)):
        rtol, atol = bars[name]
        a = rtol * t.detach().abs() + atol * scale
        if gs and t.numel():
            ds = torch.autograd.grad(t.sum(), gs, retain_graph=True, allow_unused=True)
            for d, ga in zip(ds, grad_allow):
                if d is not None:
                    a = a + d.abs() * ga
        out.append(a)
    return out[0], out[1], out[2], (p.detach(), m.detach(), v.detach())


# ---------------------------------------------------------------- launch geometry
Branches = namedtuple("Branches", "workgroups ng_last sweep store second_half")


def branches(P, M, sh_span_offset_floats, dsh_offset_bytes):
    """What sh_grad_views_kernel does for P Gaussians of M coefficients: `sh_span_offset_floats` = where the SH spans of param /
    exp_avg / exp_avg_sq start, in floats from a 16-byte aligned base (the three buffers share the offset); `dsh_offset_bytes` =
    dL_dsh's distance from a 16-byte boundary.
      sweep        <true>:  "vector" (F = 3M a multiple of 4 and the span bases 16-byte aligned), "scalar", "none" (M = 0)
      store        <false>: "float4" (M == 16 and dL_dsh aligned) or "scalar"
      second_half  of the LAST workgroup's float4 sweep: "none" (total4 <= 128), "partial" (128 < total4 < 256), "more"; "-" off the vector sweep"""
    F = 3 * M
    wgs = (P + WG - 1) // WG
    ng = P - WG * (wgs - 1) if P else 0
    aligned = (4 * sh_span_offset_floats) % 16 == 0        # (workgroup g0 starts g0 * F floats on: a multiple of 16 bytes when F % 4 == 0)
    sweep = "none" if M == 0 else ("vector" if F % 4 == 0 and aligned else "scalar")
    store = "float4" if M == 16 and dsh_offset_bytes % 16 == 0 else "scalar"
    second = "-"
    if sweep == "vector":
        total4 = ng * F // 4
        second = "none" if total4 <= 128 else ("partial" if total4 < 256 else "more")
    return Branches(wgs, ng, sweep, store, second)


def store_offsets(P):
    """Float offsets of the five groups in the flat store of igs_amd.refine.GaussianParams (GROUPS order)."""
    from igs_amd.refine import GROUPS
    off, o = {}, 0
    for name, k in GROUPS:
        off[name] = o
        o += k * P
    return off, o


def gap_offsets(P, M):
    """A second layout: the groups in another order with gaps of 5 to 8 floats between them, the SH span 16-byte aligned."""
    off, o = {}, 3
    for name, k in (("scaling", 3), ("shs", 3 * M), ("xyz", 3), ("opacity", 1), ("rotation", 4)):
        o += 5
        if name == "shs":
            o = (o + 3) & ~3
        off[name] = o
        o += k * P
    return off, o + 6


# ---------------------------------------------------------------- cases
# off = how many floats the outputs (dL_dsh, or the three SH spans) start past a 16-byte boundary
Case = namedtuple("Case", "id P V D M clamp off")

GRAD_CASES = [
    # P x (D, M): a covering subset -- every P and every (D, M) of the issue's lists occurs
    Case("P1-D0M1-scalar_store", 1, 3, 0, 1, 0.0, 0),
    Case("P127-D0M16-M_above-float4_store", 127, 3, 0, 16, 0.0, 0),
    Case("P128-D1M4-scalar_store", 128, 3, 1, 4, 0.0, 0),
    Case("P129-D1M16-M_above-float4_store", 129, 3, 1, 16, 0.0, 0),
    Case("P143-D2M9-scalar_store", 143, 3, 2, 9, 0.0, 0),
    Case("P1031-D3M4-M_below-scalar_store", 1031, 3, 3, 4, 0.0, 0),
    Case("P129-D3M12-M_below-scalar_store", 129, 3, 3, 12, 0.0, 0),
    Case("P1-D3M16-float4_store", 1, 3, 3, 16, 0.0, 0),
    Case("P1031-D3M16-float4_store", 1031, 3, 3, 16, 0.0, 0),
    # view counts
    Case("V0-P143-D3M16-float4_store", 143, 0, 3, 16, 0.0, 0),
    Case("V1-P143-D3M16-float4_store", 143, 1, 3, 16, 0.0, 0),
    Case("V64-P143-D3M16-float4_store", 143, 64, 3, 16, 0.0, 0),
    # clamp
    Case("clamp15-P1031-D3M16-float4_store", 1031, 3, 3, 16, 15.0, 0),
    Case("clamp15-P143-D2M9-scalar_store", 143, 3, 2, 9, 15.0, 0),
    # store path: dL_dsh 4 bytes off the 16-byte grid at M = 16
    Case("off4-P127-D3M16-scalar_store", 127, 3, 3, 16, 0.0, 1),
    Case("off4-clamp15-P1031-D3M16-scalar_store", 1031, 3, 3, 16, 15.0, 1),
]

ADAM_CASES = [
    Case("M16-P1031-vector-no_second_half", 1031, 3, 3, 16, 0.0, 0),         # last workgroup: 7 Gaussians, 84 float4
    Case("M16-P1031-off4-scalar", 1031, 3, 3, 16, 0.0, 1),
    Case("M16-P129-vector-no_second_half", 129, 3, 3, 16, 0.0, 0),           # last workgroup: one Gaussian, 12 float4
    Case("M16-P143-vector-partial_second_half", 143, 3, 3, 16, 0.0, 0),      # last workgroup: 15 Gaussians, 180 float4
    Case("M16-P150-vector-more", 150, 3, 3, 16, 15.0, 0),                    # last workgroup: 22 Gaussians, 264 float4; clamp on
    Case("M4-P143-vector-no_second_half", 143, 3, 1, 4, 0.0, 0),             # F = 12
    Case("M1-P129-F_not_multiple_of_4-scalar", 129, 3, 0, 1, 0.0, 0),        # F = 3
    Case("M9-P143-F_not_multiple_of_4-scalar", 143, 3, 2, 9, 0.0, 0),        # F = 27
    Case("M12-P129-M_below-vector-no_second_half", 129, 3, 3, 12, 0.0, 0),   # F = 36
    Case("V0-M16-P143-vector-partial_second_half", 143, 0, 3, 16, 0.0, 0),
    Case("V64-M16-P129-off4-scalar", 129, 64, 3, 16, 0.0, 1),
]

# igs_adam_exchange_step: layout "store" = GaussianParams' own offsets (SH span at 11 P floats), "gaps" = gap_offsets
XCase = namedtuple("XCase", "id P V D M clamp layout")
EXCHANGE_CASES = [
    XCase("store-P128-vector", 128, 3, 3, 16, 0.0, "store"),
    XCase("store-P129-scalar", 129, 3, 3, 16, 0.0, "store"),
    XCase("store-P143-scalar", 143, 3, 3, 16, 15.0, "store"),
    XCase("store-P1031-scalar", 1031, 3, 3, 16, 0.0, "store"),
    XCase("gaps-P143-vector-partial_second_half", 143, 3, 3, 16, 0.0, "gaps"),
    XCase("gaps-P129-M9-scalar", 129, 3, 2, 9, 0.0, "gaps"),
    XCase("store-P143-V0-scalar", 143, 0, 3, 16, 0.0, "store"),
    XCase("store-P143-M0-none", 143, 3, 3, 0, 0.0, "store"),
]

STEPS = 3
T0 = 4                                        # completed steps before the first one of a test (bias corrections of steps 5, 6, 7)
LR_SH = 2.5e-3
LRS = dict(xyz=1.0, rotation=1e-3, opacity=5e-2, scaling=5e-3, shs=LR_SH)       # lr_xyz = 1.0: a direction taken from an already-moved
SMALL = (("xyz", 3), ("rotation", 4), ("opacity", 1), ("scaling", 3))         # position would miss the bound by orders of magnitude


def _seed(c, step):
    return 1000003 * c.P + 10007 * c.V + 101 * c.D + 7 * c.M + (3 if c.clamp else 0) + 1000 * step


def build_inputs(c, step=0):
    """Seeded float32 inputs of a case: means [P, 3] in [-1.5, 1.5]^3, campos [V, 3] at distance 4..6, gc [V, P, 3].  Every third
    Gaussian is unseen in every view, every fifth is unseen in view 1; with a clamp the gradients are scaled until it bites."""
    gen = torch.Generator().manual_seed(_seed(c, 0))
    means = torch.rand(c.P, 3, generator=gen) * 3.0 - 1.5
    cd = torch.randn(max(c.V, 1), 3, generator=gen)
    campos = (cd / cd.norm(dim=1, keepdim=True) * (4.0 + 2.0 * torch.rand(max(c.V, 1), 1, generator=gen)))[:c.V]
    return means, campos, view_gradients(c, step)


def view_gradients(c, step):
    gen = torch.Generator().manual_seed(_seed(c, step) + 17)
    gc = torch.randn(c.V, c.P, 3, generator=gen) * (60.0 if c.clamp else 0.1)
    idx = torch.arange(c.P)
    if c.V:
        gc[:, idx % 3 == 2] = 0.0
    if c.V > 1:
        gc[1, idx % 5 == 4] = 0.0
    return gc


def build_state(c, n_floats, seed_add=0):
    """Starting parameters and non-zero moments for n_floats elements: exp_avg_sq >= 1e-8."""
    gen = torch.Generator().manual_seed(_seed(c, 0) + 29 + seed_add)
    p0 = torch.randn(n_floats, generator=gen) * 0.5
    m0 = torch.randn(n_floats, generator=gen) * 1e-2
    v0 = torch.rand(n_floats, generator=gen) * 1e-3 + 1e-8
    return p0, m0, v0


def small_gradients(c, n_floats, step):
    gen = torch.Generator().manual_seed(_seed(c, step) + 43)
    g = torch.randn(n_floats, generator=gen) * 0.1
    g[::97] = 0.0
    return g


def sh_reference(c, means, campos, grads_per_step, p0, m0, v0):
    """Three steps of the SH update in float64 with their allowances.  p0 / m0 / v0: [P * M * 3] float32.  `means`: [P, 3], or one
    per step (igs_adam_exchange_step moves the positions; a step's directions use the positions it was launched with).
    Returns dict(p, m, v, allow_p, allow_m, allow_v)."""
    ms = means if isinstance(means, (list, tuple)) else [means] * len(grads_per_step)
    g64 = [rebuild_sh(c.D, c.M, mn, campos, gc, c.clamp).reshape(-1) for mn, gc in zip(ms, grads_per_step)]
    ga = [rebuild_allowance(c.D, c.M, mn, campos, gc).reshape(-1) for mn, gc in zip(ms, grads_per_step)]
    rp, st = adam_reference(p0, m0, v0, T0, g64, LR_SH)
    ap, am, av, (fp, fm, fv) = adam_allowance(p0, m0, v0, T0, g64, ga, LR_SH)
    if rp.numel():          # the differentiable formula IS torch.optim.Adam
        assert float((fp - rp).abs().max()) <= 1e-12 * max(float(rp.abs().max()), 1.0)
        assert float((fv - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(st["exp_avg_sq"].abs().max())
    return dict(p=rp, m=st["exp_avg"], v=st["exp_avg_sq"], allow_p=ap, allow_m=am, allow_v=av)


# ---------------------------------------------------------------- the colour-gradient scene
COLOR_SCENE = dict(P=3000, size=96, seed=0)
NEAR_CLAMP = 1e-5          # a channel whose float64 colour before the clamp is this close to zero may clamp either way in float32
NEAR_CLAMP_CAP = 0.005     # at most this fraction of the channels of seen Gaussians may be excluded for it


def color_scene():
    """cfg1_scene (whose camera sees every Gaussian) with every 7th Gaussian moved far to the side of the frustum and every 11th
    behind the camera: rows the view does not see."""
    from igs_amd.scenes import cfg1_scene
    raw, cams, bg = cfg1_scene(P=COLOR_SCENE["P"], seed=COLOR_SCENE["seed"], size=COLOR_SCENE["size"])
    raw["xyz"][::7, 0] += 9.0
    raw["xyz"][3::11, 2] = -6.5
    return raw, cams, bg


def preclamp_colors(raw, cam):
    """float64 [P, 3]: the SH colour before max(0, .) (forward.cu:20-74: sum_k b_k sh_k + 0.5), degree 3."""
    d = _dirs(raw["xyz"], cam.camera_center.detach().cpu().reshape(3))
    return (TO.sh_basis(3, d)[:, :, None] * raw["shs"].double()).sum(1) + 0.5
