"""Float64 PyTorch restatement of what igs_amd/csrc/tokens.hip computes: LayerNorm over rows with an optional residual, the exact-GELU
GEGLU, and their gradients; stand-ins for the unimatch TransformerLayer and for BasicTransformerBlock in this repository's own wording (the
attribute names of the reference's modules, which are not available where the GPU tests run); the test inputs; a float32 emulation of the
kernels' arithmetic with deliberately wrong variants; and the per-element allowances of the tests, derived, never measured.

u = 2^-24 is the relative error of one float32 rounding.  Every bound is first order and doubled at the end (LayerNorm) or carries its
margin in the constants (GEGLU), as tests/condition3d_restatement.py and tests/encoder_norms_restatement.py do.
"""
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

import window_attention_restatement as WR

u = 2.0 ** -24
# the longest chain of float32 additions an element of a row sum goes through in tokens.hip: at most 4 steps of a lane's running sum, 2 to
# join its four sums, 6 butterfly steps
SUM_DEPTH = 12


def half_rounding(ref):
    """One rounding to the nearest float16: 2^-11 relative, never finer than half the subnormal spacing 2^-24."""
    return torch.clamp(2.0 ** -11 * ref.abs(), min=2.0 ** -25)


# ---------------------------------------------------------------- LayerNorm
def layer_norm_parts(x, eps, unbiased=False):
    """(mu, var, r, xh) of [N, C] rows, biased variance from centred values."""
    C = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).sum(-1, keepdim=True) / (C - 1 if unbiased else C)
    r = 1.0 / torch.sqrt(var + eps)
    return mu, var, r, (x - mu) * r


def layer_norm_restate(x, weight, bias, eps, res=None):
    """(res +) LN(x) * weight + bias in the dtype of x (pass float64); weight = bias = None: no affine step."""
    y = layer_norm_parts(x, eps)[3]
    if weight is not None:
        y = y * weight + bias
    return y if res is None else res + y


def layer_norm_backward_restate(x, weight, eps, g):
    """(dx, dweight, dbias) in closed form for the upstream gradient g; weight = None: ones."""
    mu, var, r, xh = layer_norm_parts(x, eps)
    gw = g if weight is None else g * weight
    m1, m2 = gw.mean(-1, keepdim=True), (gw * xh).mean(-1, keepdim=True)
    return r * (gw - m1 - xh * m2), (g * xh).sum(0), g.sum(0)


# Forward, per row of C elements, a = x - mu, S = SUM_DEPTH (first order, doubled at the end):
#   m = sum x / C, then d = x - m, s1 = sum d, mu = m + s1 / C: the second pass removes the error of m to first order; what is left is
#                    the rounding of the d (u |a| each), of their sum (S u mean|a|), of the division and of the last add:
#                    d mu = 2 u |mu| + (S + 2) u mean|a|
#   a = x - mu:      d a  = d mu + u |a|
#   var = s2 / C - (s1 / C)^2:   d var = 2 mean|a| d mu + d mu^2 + (S + 6) u var      (the squares of perturbed a, S + 1 roundings of the
#                    sum and a few of the squares, the division and the subtracted correction)
#   r = (var + eps)^-1/2:        d r = r (d var / (2 (var + eps)) + 4 u)             (the sum with eps, the root, the reciprocal)
#   xh = a r:        d xh = d a r + |a| d r + u |xh|
#   y = fma(xh, w, b):           d y = |w| d xh + u |y|                              (none when there is no affine step)
#   out = res + y:               + u |out|;    a float16 out: + one rounding to half
# A variance formed as E[x^2] - mu^2 in float32 violates this when |mu| >> sd, the unbiased variance when C is small, a dropped eps when
# var is of its order: the host tests check all three.
def _forward_terms(x, weight, eps):
    x = x.double()
    mu, var, r, xh = layer_norm_parts(x, eps)
    a = x - mu
    ma = a.abs().mean(-1, keepdim=True)
    dmu = 2 * u * mu.abs() + (SUM_DEPTH + 2) * u * ma
    da = dmu + u * a.abs()
    dvar = 2 * ma * dmu + dmu * dmu + (SUM_DEPTH + 6) * u * var
    dr = r * (dvar / (2 * (var + eps)) + 4 * u)
    dxh = da * r + a.abs() * dr + u * xh.abs()
    w = torch.ones_like(x[:1]) if weight is None else weight.double().view(1, -1)
    return dict(C=x.shape[-1], w=w, r=r, dr=dr, xh=xh, dxh=dxh)


def layer_norm_forward_bound(x, weight, bias, eps, res=None, out_dtype=torch.float32):
    """Per element, for the float32 / float16 inputs as given; float64."""
    k = _forward_terms(x, weight, eps)
    y = k["xh"] * k["w"] + (0.0 if bias is None else bias.double().view(1, -1))
    d = k["w"].abs() * k["dxh"] + (u * y.abs() if weight is not None else 0.0)
    out = y
    if res is not None:
        out = y + res.double()
        d = d + u * out.abs()
    d = 2 * d + 1e-300
    return d + half_rounding(out) if out_dtype == torch.float16 else d


# Backward for the upstream gradient g over N rows, gw = g w (one rounding):
#   d bias   = sum_n g:       (N + 1) u sum|g|                               N - 1 roundings of the sum in any order
#   d weight = sum_n g xh:    sum |g| d xh + (N + 2) u sum|g xh|
#   m1 = mean_c gw:           d m1 = (S + 3) u mean|gw|
#   m2 = mean_c gw xh:        d m2 = mean(|gw| d xh) + (S + 4) u mean|gw xh|
#   t = gw - m1 - xh m2:      d t = 3 u |gw| + d m1 + d xh |m2| + |xh| d m2 + u |xh m2| + 4 u (|gw| + |m1| + |xh m2|)
#   d x = r t:                d r |t| + r d t + u |d x|;   a float16 d x: + one rounding to half
def layer_norm_backward_bounds(x, weight, eps, g, dx_dtype=torch.float32):
    """dict(dx [N, C], dweight [C], dbias [C]) float64."""
    k = _forward_terms(x, weight, eps)
    w, r, dr, xh, dxh = k["w"], k["r"], k["dr"], k["xh"], k["dxh"]
    g = g.double()
    N = x.shape[0]
    gw = g * w
    dbias = 2 * (N + 1) * u * g.abs().sum(0) + 1e-300
    dweight = 2 * ((g.abs() * dxh).sum(0) + (N + 2) * u * (g * xh).abs().sum(0)) + 1e-300
    m1, m2 = gw.mean(-1, keepdim=True), (gw * xh).mean(-1, keepdim=True)
    dm1 = (SUM_DEPTH + 3) * u * gw.abs().mean(-1, keepdim=True)
    dm2 = (gw.abs() * dxh).mean(-1, keepdim=True) + (SUM_DEPTH + 4) * u * (gw * xh).abs().mean(-1, keepdim=True)
    t = gw - m1 - xh * m2
    dt = 3 * u * gw.abs() + dm1 + dxh * m2.abs() + xh.abs() * dm2 + u * (xh * m2).abs() + 4 * u * (gw.abs() + m1.abs() + (xh * m2).abs())
    dx = 2 * (dr * t.abs() + r * dt + u * (r * t).abs()) + 1e-300
    if dx_dtype == torch.float16:
        dx = dx + half_rounding(r * t)
    return dict(dx=dx, dweight=dweight, dbias=dbias)


def _tree_sum(t):
    """Pairwise float32 sum over the last dimension, kept as a column (the kernel: running sums per lane, then a butterfly)."""
    n = t.shape[-1]
    p = 1 << max(n - 1, 0).bit_length()
    t = torch.cat([t, t.new_zeros(t.shape[:-1] + (p - n,))], -1)
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t


def layer_norm_emulate(x, eps=1e-5, variant="right"):
    """LN(x) of [N, C] float32 rows in float32 arithmetic.  variant: "right" (tree mean, centred sums, the corrected two-pass form),
    "one_pass" (E[x^2] - mean^2), "unbiased" (C - 1), "no_eps"."""
    assert x.dtype == torch.float32
    n = torch.tensor(float(x.shape[-1]), dtype=torch.float32)
    m = _tree_sum(x) / n
    if variant == "one_pass":
        var, mean = _tree_sum(x * x) / n - m * m, m
    else:
        d = x - m
        dm = _tree_sum(d) / n
        var = _tree_sum(d * d) / (n - 1 if variant == "unbiased" else n) - dm * dm
        mean = m + dm
    var = torch.where(var < 0, torch.zeros_like(var), var)
    rstd = 1.0 / torch.sqrt(var + (0.0 if variant == "no_eps" else torch.tensor(eps, dtype=torch.float32)))
    return (x - mean) * rstd


ROW_MEANS = (0.0, 100.0, -1e3)
ROW_STDS = (1.0, 1e-3, 30.0)


def param_rows_sum(rows, waves=16):
    """The float32 sum of [T, K] partial parameter rows in the documented order of the backward's reduction (igs_amd/csrc/param_reduce.h):
    `waves` contiguous shares of ceil(T / waves) rows, each added row by row from 0.0f, then the share sums added in share order from
    0.0f.  On the CPU, one float32 rounding per addition."""
    rows = rows.detach().cpu().float()
    T, K = rows.shape
    share = -(-T // waves)
    total = torch.zeros(K)
    for k in range(waves):
        s = torch.zeros(K)
        for t in range(min(k * share, T), min(k * share + share, T)):
            s = s + rows[t]
        total = total + s
    return total


def row_inputs(N, C, dtype, device, seed, constant_row=None):
    """[N, C]: row n has the pair number q = (seed + 4 n) mod 9 of (mean, std) = (ROW_MEANS[q % 3], ROW_STDS[q // 3]), so three rows take
    three means and three stds and nine take every pair.  Row `constant_row` holds one value (one that no power-of-two count sums exactly)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g, dtype=torch.float64)
    q = (seed + 4 * torch.arange(N)) % 9
    x = x * torch.tensor(ROW_STDS, dtype=torch.float64)[q // 3, None] + torch.tensor(ROW_MEANS, dtype=torch.float64)[q % 3, None]
    if constant_row is not None:
        x[constant_row] = 100.37
    return x.to(dtype).to(device)


def affine_inputs(C, device, seed):
    """(weight, bias) [C] float32, away from 1 / 0."""
    g = torch.Generator().manual_seed(1000 + seed)
    return (1.0 + 0.5 * torch.randn(C, generator=g)).to(device), (0.4 * torch.randn(C, generator=g)).to(device)


# ---------------------------------------------------------------- GEGLU
SQRT_HALF, INV_SQRT_2PI = 0.7071067811865476, 0.3989422804014327
TINY = 2.0 ** -148                                                  # a few roundings to float32's subnormal grid (spacing 2^-149): 1e-30 * 1e-30 underflows


def cdf(g):
    return 0.5 * (1.0 + torch.erf(g * SQRT_HALF))


def pdf(g):
    return INV_SQRT_2PI * torch.exp(-0.5 * g * g)


def geglu_restate(p):
    """[..., 2 D] -> [..., D]: h * gelu(g), the exact GELU, in the dtype of p (pass float64)."""
    h, g = p.chunk(2, dim=-1)
    return h * (g * cdf(g))


def geglu_backward_restate(p, dout):
    """d p [..., 2 D] in closed form."""
    h, g = p.chunk(2, dim=-1)
    return torch.cat([dout * (g * cdf(g)), dout * h * (cdf(g) + g * pdf(g))], -1)


# Phi(g) = 0.5 (1 + erf(g c)), c = fl(1 / sqrt 2).  The argument g c carries two roundings, which erf' (at most 0.49 / |g c| of erf's own
# size, at most 1.13 in all) turns into less than u; erf itself is good to 16 ulp (the OpenCL / OCML specification), an ulp of a value below
# 1 being at most u: 16 u.  Both are errors of 1 + erf, whatever is left of it after the cancellation at negative g, so they are absolute
# in h g: 0.5 (16 + 1) u |h g| -> 9.  The roundings of 1 + erf, of g Phi and of the product with h are relative to the result: 3 u -> 4.
def geglu_forward_allowance(p, out_dtype=torch.float32):
    """u (4 |h gelu(g)| + 9 |h g|) per element, for the float32 / float16 input as given (+ one rounding to half for a float16 result)."""
    h, g = p.double().chunk(2, dim=-1)
    ref = h * (g * cdf(g))
    a = u * (4 * ref.abs() + 9 * (h * g).abs()) + TINY
    return a + half_rounding(ref) if out_dtype == torch.float16 else a


# d h = dout (g Phi): the forward's bound with dout in the place of h.
# d g = (dout h) (Phi + g phi), phi(g) = k exp(-g^2 / 2): the error of Phi is absolute again (8.5 u |dout h| -> 9); the roundings of dout h,
# of the fma and of the last product are relative to |dout h| (Phi + |g| phi), the sum WITHOUT its cancellation at negative g (3 u -> 4);
# phi carries the rounding of k and of the product (2 u), exp's 3 ulp (6 u) and the two roundings of its argument g^2 / 2, which the
# exponential turns into a relative u g^2: u (8 + g^2) |dout h g phi|.
def geglu_backward_allowance(p, dout, out_dtype=torch.float32):
    """[..., 2 D] per element of d p."""
    h, g = p.double().chunk(2, dim=-1)
    d = dout.double()
    c, f = cdf(g), pdf(g)
    dh = u * (4 * (d * g * c).abs() + 9 * (d * g).abs())
    dg = u * (4 * (d * h).abs() * (c + g.abs() * f) + 9 * (d * h).abs() + (8 + g * g) * (d * h * g * f).abs())
    a = torch.cat([dh, dg], -1) + TINY
    return a + half_rounding(geglu_backward_restate(p.double(), d)) if out_dtype == torch.float16 else a


def geglu_emulate(p, variant="right"):
    """h * gelu(g) in float32 arithmetic.  variant: "right", "tanh" (the tanh approximation), "sigmoid" (g sigmoid(1.702 g)), "swapped"
    (the halves exchanged)."""
    assert p.dtype == torch.float32
    h, g = p.chunk(2, dim=-1)
    if variant == "swapped":
        h, g = g, h
    if variant == "tanh":
        return h * F.gelu(g, approximate="tanh")
    if variant == "sigmoid":
        return h * (g * torch.sigmoid(1.702 * g))
    return h * (g * (0.5 * (1.0 + torch.erf(g * torch.tensor(SQRT_HALF, dtype=torch.float32)))))


H_EXTREMES = (0.0, -0.0, 1e-30, -1e-30, 50.0, -50.0, 3e4, -3e4)
G_EXTREMES = (6.0, -6.0, -12.0, 40.0, -40.0, 0.0, -0.0, 1e-30)


def geglu_inputs(N, D, dtype, device, seed, scale=1.0, row_stride=None):
    """[N, 2 D] = scale * randn with the extremes planted: every H_EXTREMES value meets every G_EXTREMES value once where N * D allows, the
    rest meet random partners.  row_stride > 2 D gives a slice of a wider buffer.  (1e-30 is zero in float16.)"""
    g = torch.Generator().manual_seed(seed)
    p = scale * torch.randn(N, 2 * D, generator=g, dtype=torch.float64)
    flat_h, flat_g = p[:, :D].reshape(-1).clone(), p[:, D:].reshape(-1).clone()
    n = flat_h.numel()
    k = 0
    for hv in H_EXTREMES:
        for gv in G_EXTREMES:
            at = (7 * k + 3) % n
            if k < n:
                flat_h[at], flat_g[at] = hv, gv
            k += 1
    for i, hv in enumerate(H_EXTREMES):                            # ... and random partners, where there is room
        if n > 200:
            flat_h[(11 * i + 150) % n] = hv
            flat_g[(13 * i + 170) % n] = G_EXTREMES[i]
    p = torch.cat([flat_h.view(N, D), flat_g.view(N, D)], 1).to(dtype)
    if row_stride is None or row_stride == 2 * D:
        return p.to(device)
    buf = torch.full((N, row_stride), 777.0, dtype=dtype, device=device)
    buf[:, : 2 * D] = p.to(device)
    return buf[:, : 2 * D]


# ---------------------------------------------------------------- stand-ins for the two modules
# the names the layer's forward looks up in its own module (the reference binds them at import); tests patch them
single_head_split_window_attention = WR.restated_split
single_head_full_attention = WR.restated_full


class TransformerLayer(nn.Module):
    """One attention step of the unimatch transformers: bias-free projections of source (query) and target (key, value), single-head swin
    or full attention, a merge projection and a LayerNorm; with an FFN the message is concatenated behind the source, goes through a
    bias-free two-layer GELU MLP of expansion 4 on the doubled width and a second LayerNorm.  The result is source + message."""

    def __init__(self, d_model=128, nhead=1, no_ffn=False, ffn_dim_expansion=4):
        super().__init__()
        self.dim, self.nhead, self.no_ffn = d_model, nhead, no_ffn
        self.q_proj = nn.Linear(d_model, d_model, bias=False)
        self.k_proj = nn.Linear(d_model, d_model, bias=False)
        self.v_proj = nn.Linear(d_model, d_model, bias=False)
        self.merge = nn.Linear(d_model, d_model, bias=False)
        self.norm1 = nn.LayerNorm(d_model)
        if not no_ffn:
            wide = 2 * d_model
            self.mlp = nn.Sequential(nn.Linear(wide, wide * ffn_dim_expansion, bias=False), nn.GELU(),
                                     nn.Linear(wide * ffn_dim_expansion, d_model, bias=False))
            self.norm2 = nn.LayerNorm(d_model)

    def forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, shifted_window_attn_mask_1d=None,
                attn_type="swin", with_shift=False, attn_num_splits=None):
        assert attn_type == "swin" and self.nhead == 1
        same = (source - target).abs().max() < 1e-6                 # the reference's self-attention test: three launches, unused under 'swin'
        ns = sys.modules[type(self).__module__]
        q, k, v = self.q_proj(source), self.k_proj(target), self.v_proj(target)
        if attn_num_splits > 1:
            message = ns.single_head_split_window_attention(q, k, v, num_splits=attn_num_splits, with_shift=with_shift, h=height, w=width,
                                                            attn_mask=shifted_window_attn_mask)
        else:
            message = ns.single_head_full_attention(q, k, v)
        message = self.norm1(self.merge(message))
        if not self.no_ffn:
            message = self.norm2(self.mlp(torch.cat([source, message], dim=-1)))
        return source + message


class LinearAttention(nn.Module):
    """The simplest module that can stand where the block's attention stands: one Linear over the channels."""

    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Linear(dim, dim)

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kwargs):
        return self.proj(hidden_states)


class Geglu(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, 2 * dim_out)

    def forward(self, hidden_states, scale=1.0):
        hidden_states, gate = self.proj(hidden_states).chunk(2, dim=-1)
        return hidden_states * F.gelu(gate)


class Gelu(nn.Module):
    """The activation the installer must refuse."""

    def __init__(self, dim_in, dim_out, approximate="none"):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out)
        self.approximate = approximate

    def forward(self, hidden_states):
        return F.gelu(self.proj(hidden_states), approximate=self.approximate)


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4, activation_fn="geglu"):
        super().__init__()
        inner = dim * mult
        act = Geglu(dim, inner) if activation_fn == "geglu" else Gelu(dim, inner, "tanh" if activation_fn == "gelu-approximate" else "none")
        self.net = nn.ModuleList([act, nn.Dropout(0.0), nn.Linear(inner, dim)])

    def forward(self, hidden_states, scale=1.0):
        for m in self.net:
            hidden_states = m(hidden_states)
        return hidden_states


class BasicTransformerBlock(nn.Module):
    """Pre-norm self-attention and a pre-norm GEGLU feed-forward, each added to its input; no cross-attention (norm2 = attn2 = None), plain
    LayerNorms.  `attn1` is any module over [B, A, dim]."""

    def __init__(self, dim, attn1, activation_fn="geglu", norm_elementwise_affine=True):
        super().__init__()
        self.only_cross_attention = False
        self.use_ada_layer_norm = self.use_ada_layer_norm_zero = self.use_ada_layer_norm_continuous = False
        self.norm1 = nn.LayerNorm(dim, elementwise_affine=norm_elementwise_affine)
        self.attn1 = attn1
        self.norm2 = None
        self.attn2 = None
        self.norm3 = nn.LayerNorm(dim, elementwise_affine=norm_elementwise_affine)
        self.ff = FeedForward(dim, activation_fn=activation_fn)

    def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None):
        hidden_states = self.attn1(self.norm1(hidden_states), encoder_hidden_states=None, attention_mask=attention_mask) + hidden_states
        return self.ff(self.norm3(hidden_states)) + hidden_states


def randomise(module, seed):
    """Every parameter redrawn from a seeded generator: matrices at 1 / sqrt(fan-in), LayerNorm weights around 1, every bias around 0."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * m.in_features ** -0.5)
                if m.bias is not None:
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, nn.LayerNorm) and m.weight is not None:
                m.weight.copy_(1.0 + 0.5 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.4 * torch.randn(m.bias.shape, generator=g))
    return module


def make_layer(d_model=128, no_ffn=False, seed=0):
    return randomise(TransformerLayer(d_model=d_model, no_ffn=no_ffn), seed)


def make_block(dim, attn1, seed=0, **kw):
    return randomise(BasicTransformerBlock(dim, attn1, **kw), seed)
