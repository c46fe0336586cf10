"""Float64 PyTorch restatement of what igs_amd/csrc/gnorm.hip computes: the GroupNorm over channel-major [B, C, A] written token-major
[B, A, C], its gradients, and the token-major + channel-major add; a stand-in for Transformer1D in this repository's own wording (the
attribute names of the reference's module, which is not available where the GPU tests run); the test inputs; a float32 emulation of the
kernels' arithmetic with deliberately wrong variants; and the per-element allowances of the tests, derived, never measured.

u = 2^-24 is the relative error of one float32 rounding.  A float32 sum whose every element goes through at most D additions is off by at
most D u sum|terms| to first order, whatever the order.  Every bound is first order and doubled at the end, as
tests/token_ops_restatement.py does for the LayerNorm, whose chain of reasoning the forward follows with the group in the place of the row.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import token_ops_restatement as TR
from token_ops_restatement import half_rounding, u

STATS_LANES, TILE, REDUCE_WAVES = 1024, 64, 16                      # gn_stats_kernel's workgroup, the token tile, param_reduce.h's waves


# ---------------------------------------------------------------- the depths of the kernels' sums (additions an element goes through)
def stats_depth(cpg, A):
    """gn_stats_kernel: a lane's running sum over its elements (at most ceil(cpg A / 1024) steps, one element at a time on the scalar
    path; the four-element path has a quarter of them and 2 to join a quad), 6 butterfly steps, 16 waves in order."""
    return -(-cpg * A // STATS_LANES) + 2 + 6 + 16


def tile_depth(A):
    """The sum over the tokens of one (example, channel) in the backward: 2 to join a lane's four tokens, 4 butterfly steps over the 16
    lanes of the channel, then param_reduce.h over the ceil(A / 64) tile rows: a wave's share in order, 16 waves in order."""
    tiles = -(-A // TILE)
    return 2 + 4 + -(-tiles // REDUCE_WAVES) + REDUCE_WAVES


def batch_depth(B):
    """d weight, d bias: param_reduce.h over the B rows of per-example sums (two rounds above 1024 rows: 64 shares, then their sums)."""
    if B > 1024:
        return -(-(-(-B // 64)) // REDUCE_WAVES) + REDUCE_WAVES + -(-64 // REDUCE_WAVES) + REDUCE_WAVES
    return -(-B // REDUCE_WAVES) + REDUCE_WAVES


def group_depth(cpg):
    """gn_bwd_group_kernel: a lane's fma chain over ceil(cpg / 64) channels, 6 butterfly steps."""
    return -(-cpg // 64) + 6


# ---------------------------------------------------------------- the three operations, float64
def group_norm_parts(x, G, eps, unbiased=False):
    """(mu, var, r, xh) of x [B, C, A]: mu, var, r are [B, G, 1], xh [B, C, A]; biased variance from centred values."""
    B, C, A = x.shape
    xg = x.reshape(B, G, -1)
    n = xg.shape[-1]
    mu = xg.mean(-1, keepdim=True)
    var = ((xg - mu) ** 2).sum(-1, keepdim=True) / (n - 1 if unbiased else n)
    r = 1.0 / torch.sqrt(var + eps)
    return mu, var, r, ((xg - mu) * r).reshape(B, C, A)


def group_norm_tokens_restate(x, G, weight, bias, eps):
    """F.group_norm(x, G, weight, bias, eps).permute(0, 2, 1) in the dtype of x (pass float64): [B, C, A] -> [B, A, C]."""
    y = group_norm_parts(x, G, eps)[3]
    if weight is not None:
        y = y * weight.view(1, -1, 1) + bias.view(1, -1, 1)
    return y.permute(0, 2, 1).contiguous()


def group_norm_stats_restate(x, G, eps):
    """[B, G, 2] = (mean, 1 / sqrt(var + eps))."""
    mu, var, r, _ = group_norm_parts(x, G, eps)
    return torch.cat([mu, r], -1)


def group_norm_tokens_backward_restate(x, G, weight, eps, g):
    """(dx [B, C, A], dweight [C], dbias [C]) in closed form for the upstream gradient g [B, A, C]; weight = None: ones."""
    B, C, A = x.shape
    mu, var, r, xh = group_norm_parts(x, G, eps)
    dy = g.permute(0, 2, 1)
    gw = dy if weight is None else dy * weight.view(1, -1, 1)
    n = (C // G) * A
    s1 = gw.reshape(B, G, -1).sum(-1, keepdim=True)
    s2 = (gw * xh).reshape(B, G, -1).sum(-1, keepdim=True)
    dx = r * (gw.reshape(B, G, -1) - (s1 + xh.reshape(B, G, -1) * s2) / n)
    return dx.reshape(B, C, A), (dy * xh).sum((0, 2)), dy.sum((0, 2))


def add_residual_restate(tokens, residual):
    """tokens [B, A, C] + residual [B, C, A] -> [B, A, C]."""
    return tokens + residual.permute(0, 2, 1)


# ---------------------------------------------------------------- allowances
# Forward, per group of n = cpg A elements, a = x - mu, S = stats_depth (first order, doubled at the end); the chain of
# token_ops_restatement.layer_norm_forward_bound with the group in the place of the row:
#   m = sum x / n, then d = x - m, s1 = sum d, mu = m + s1 / n:   d mu = 2 u |mu| + (S + 2) u mean|a|
#   a = x - mu:                   d a  = d mu + u |a|
#   var = s2 / n - (s1 / n)^2:    d var = 2 mean|a| d mu + d mu^2 + (S + 6) u var
#   r = (var + eps)^-1/2:         d r = r (d var / (2 (var + eps)) + 4 u)
#   xh = a r:                     d xh = d a r + |a| d r + u |xh|
#   y = fma(xh, w, b):            d y = |w| d xh + u |y|      (none when there is no affine step);  a float16 out: + one rounding to half
# The unbiased variance violates this when n is small, a group boundary one channel off or gamma taken per group whenever neighbouring
# groups or channels differ: the host tests check all three.
def _forward_terms(x, G, weight, eps):
    x = x.double()
    B, C, A = x.shape
    cpg = C // G
    S = stats_depth(cpg, A)
    mu, var, r, xh = group_norm_parts(x, G, eps)
    a = x.reshape(B, G, -1) - mu
    ma = a.abs().mean(-1, keepdim=True)
    dmu = 2 * u * mu.abs() + (S + 2) * u * ma
    da = dmu + u * a.abs()
    dvar = 2 * ma * dmu + dmu * dmu + (S + 6) * u * var
    dr = r * (dvar / (2 * (var + eps)) + 4 * u)
    dxh = (da * r + a.abs() * dr).reshape(B, C, A) + u * xh.abs()
    w = torch.ones(1, C, 1, dtype=torch.float64, device=x.device) if weight is None else weight.double().view(1, -1, 1)
    return dict(w=w, mu=mu, r=r, dmu=dmu, dr=dr, xh=xh, dxh=dxh, cpg=cpg)


def group_norm_forward_bound(x, G, weight, bias, eps, out_dtype=torch.float32):
    """Per element of the [B, A, C] result, for the float32 / float16 input as given; float64."""
    k = _forward_terms(x, G, weight, eps)
    y = k["xh"] * k["w"] + (0.0 if bias is None else bias.double().view(1, -1, 1))
    d = k["w"].abs() * k["dxh"] + (u * y.abs() if weight is not None else 0.0)
    d = (2 * d + 1e-300).permute(0, 2, 1)
    return d + half_rounding(y.permute(0, 2, 1)) if out_dtype == torch.float16 else d


def group_norm_stats_bound(x, G, eps):
    """[B, G, 2]: the allowances of mean and rstd."""
    k = _forward_terms(x, G, None, eps)
    return 2 * torch.cat([k["dmu"], k["dr"]], -1) + 1e-300


# Backward for the upstream gradient dy (g permuted to [B, C, A]), gw = gamma dy, T = tile_depth(A), E = batch_depth(B), K = group_depth(cpg):
#   pb[b, c] = sum_a dy:             d pb = T u sum_a |dy|
#   pw[b, c] = sum_a dy xh:          d pw = sum_a |dy| d xh + (T + 2) u sum_a |dy xh|         (the product and the fma)
#   d bias = sum_b pb:               sum_b d pb + E u sum_b |pb|   <=  (T + E) u sum_{b, a} |dy|
#   d weight = sum_b pw:             sum_{b, a} |dy| d xh + (T + E + 2) u sum_{b, a} |dy xh|
#   s1[b, g] = sum_c gamma_c pb:     d s1 = (T + K + 1) u sum_{c, a} |gw|                      (K fma steps, one rounding each)
#   s2[b, g] = sum_c gamma_c pw:     d s2 = sum_{c, a} |gw| d xh + (T + K + 3) u sum_{c, a} |gw xh|
#   q = fma(xh, s2, s1) / n:         d q = (d s1 + d xh |s2| + |xh| d s2 + u (|s1| + |xh s2|)) / n + u |q|
#   t = gw - q:                      d t = u |gw| + d q + u |t|
#   d x = r t:                       d r |t| + r d t + u |d x|;   a float16 d x: + one rounding to half
def group_norm_backward_bounds(x, G, weight, eps, g, dx_dtype=torch.float32):
    """dict(dx [B, C, A], dweight [C], dbias [C]) float64."""
    k = _forward_terms(x, G, weight, eps)
    w, r, dr, xh, dxh, cpg = k["w"], k["r"], k["dr"], k["xh"], k["dxh"], k["cpg"]
    B, C, A = xh.shape
    n = cpg * A
    T, E, K = tile_depth(A), batch_depth(B), group_depth(cpg)
    dy = g.double().permute(0, 2, 1)
    gw = dy * w
    dbias = 2 * (T + E) * u * dy.abs().sum((0, 2)) + 1e-300
    dweight = 2 * ((dy.abs() * dxh).sum((0, 2)) + (T + E + 2) * u * (dy * xh).abs().sum((0, 2))) + 1e-300
    grp = lambda t: t.reshape(B, G, -1)                             # noqa: E731
    s1, s2 = grp(gw).sum(-1, keepdim=True), grp(gw * xh).sum(-1, keepdim=True)
    ds1 = (T + K + 1) * u * grp(gw).abs().sum(-1, keepdim=True)
    ds2 = grp(gw.abs() * dxh).sum(-1, keepdim=True) + (T + K + 3) * u * grp(gw * xh).abs().sum(-1, keepdim=True)
    xg, dxg = grp(xh), grp(dxh)
    q = (s1 + xg * s2) / n
    dq = (ds1 + dxg * s2.abs() + xg.abs() * ds2 + u * (s1.abs() + (xg * s2).abs())) / n + u * q.abs()
    t = grp(gw) - q
    dt = u * grp(gw).abs() + dq + u * t.abs()
    dx = 2 * (dr * t.abs() + r * dt + u * (r * t).abs()) + 1e-300
    if dx_dtype == torch.float16:
        dx = dx + half_rounding(r * t)
    return dict(dx=dx.reshape(B, C, A), dweight=dweight, dbias=dbias)


# ---------------------------------------------------------------- float32 emulation with wrong variants
def group_norm_emulate(x, G, weight=None, bias=None, eps=1e-6, variant="right"):
    """The [B, A, C] result for x [B, C, A] float32 in float32 arithmetic (tree mean, centred sums, the corrected two-pass form).
    variant: "right", "unbiased" (n - 1), "shifted" (every group boundary one channel late: the channels are rolled by one before the
    grouping), "gamma_by_group" (weight and bias of the group's first channel for the whole group)."""
    assert x.dtype == torch.float32
    B, C, A = x.shape
    xs = torch.roll(x, 1, dims=1) if variant == "shifted" else x
    xg = xs.reshape(B, G, -1)
    n = torch.tensor(float(xg.shape[-1]), dtype=torch.float32)
    m = TR._tree_sum(xg) / n
    d = xg - m
    dm = TR._tree_sum(d) / n
    var = TR._tree_sum(d * d) / (n - 1 if variant == "unbiased" else n) - dm * dm
    var = torch.where(var < 0, torch.zeros_like(var), var)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    y = ((xg - (m + dm)) * rstd).reshape(B, C, A)
    if variant == "shifted":
        y = torch.roll(y, -1, dims=1)
    if weight is not None:
        if variant == "gamma_by_group":
            cpg = C // G
            weight, bias = weight[::cpg].repeat_interleave(cpg), bias[::cpg].repeat_interleave(cpg)
        y = y * weight.view(1, -1, 1) + bias.view(1, -1, 1)
    return y.permute(0, 2, 1).contiguous()


def group_norm_backward_emulate(x, G, weight, eps, g, variant="right"):
    """(dx, dweight, dbias) in float32 arithmetic from float32 statistics.  variant: "right", "no_s1" (the mean of gamma dy not
    subtracted in dx)."""
    assert x.dtype == torch.float32 and g.dtype == torch.float32
    B, C, A = x.shape
    n = torch.tensor(float((C // G) * A), dtype=torch.float32)
    xh = group_norm_emulate(x, G, None, None, eps).permute(0, 2, 1).reshape(B, G, -1)
    xg = x.reshape(B, G, -1)
    m = TR._tree_sum(xg) / n
    d = xg - m
    dm = TR._tree_sum(d) / n
    var = TR._tree_sum(d * d) / n - dm * dm
    rstd = 1.0 / torch.sqrt(torch.clamp(var, min=0.0) + torch.tensor(eps, dtype=torch.float32))
    dy = g.permute(0, 2, 1)
    gw = (dy if weight is None else dy * weight.view(1, -1, 1)).reshape(B, G, -1)
    s1, s2 = TR._tree_sum(gw), TR._tree_sum(gw * xh)
    if variant == "no_s1":
        s1 = torch.zeros_like(s1)
    dx = rstd * (gw - (xh * s2 + s1) / n)
    dyx = (dy * xh.reshape(B, C, A)).permute(1, 0, 2).reshape(C, -1)
    return dx.reshape(B, C, A), TR._tree_sum(dyx)[:, 0], TR._tree_sum(dy.permute(1, 0, 2).reshape(C, -1))[:, 0]


# ---------------------------------------------------------------- inputs
GROUP_STDS = (1.0, 1e-3, 1e3)
GROUP_MEAN_RATIOS = (0.0, 100.0, -10.0)                            # the mean of a group in units of its standard deviation
HALF_MEAN_MAX = 3e4                                                # float16 inputs: |mean| is held below this, so that no element overflows


def group_inputs(B, C, G, A, dtype, device, seed, constant_group=None):
    """[B, C, A]: group (b, g) has the pair number q = (seed + 4 (b G + g)) mod 9 of (std, mean / std) = (GROUP_STDS[q // 3],
    GROUP_MEAN_RATIOS[q % 3]), so three groups take three stds and three ratios and nine take every pair.  Group `constant_group` = (b, g)
    holds one value (one that no power-of-two count sums exactly)."""
    gen = torch.Generator().manual_seed(seed)
    cpg = C // G
    x = torch.randn(B, G, cpg * A, generator=gen, dtype=torch.float64)
    q = (seed + 4 * torch.arange(B * G)).view(B, G, 1) % 9
    std = torch.tensor(GROUP_STDS, dtype=torch.float64)[q // 3]
    mean = torch.tensor(GROUP_MEAN_RATIOS, dtype=torch.float64)[q % 3] * std
    if dtype == torch.float16:
        mean = mean.clamp(-HALF_MEAN_MAX, HALF_MEAN_MAX)
    x = x * std + mean
    if constant_group is not None:
        x[constant_group[0], constant_group[1]] = 100.37
    return x.view(B, C, A).to(dtype).to(device)


# ---------------------------------------------------------------- the stand-in for Transformer1D
class Block(TR.BasicTransformerBlock):
    """The block with the argument list that Transformer1D calls it with."""

    def forward(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, timestep=None,
                modulation_cond=None, cross_attention_kwargs=None, class_labels=None):
        return super().forward(hidden_states, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states)


class Transformer1D(nn.Module):
    """Channel-major [B, C, A] in and out: an affine GroupNorm (eps 1e-6), the tokens projected to the inner width, the blocks, the
    projection back, and the input added."""

    def __init__(self, in_channels, norm_num_groups, inner_dim, num_layers, make_attention=TR.LinearAttention):
        super().__init__()
        self.norm = nn.GroupNorm(norm_num_groups, in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Linear(in_channels, inner_dim)
        self.transformer_blocks = nn.ModuleList([Block(inner_dim, make_attention(inner_dim)) for _ in range(num_layers)])
        self.proj_out = nn.Linear(inner_dim, in_channels)
        self.gradient_checkpointing = False

    def forward(self, hidden_states, encoder_hidden_states=None, timestep=None, modulation_cond=None, class_labels=None,
                cross_attention_kwargs=None, attention_mask=None, encoder_attention_mask=None):
        tokens = self.proj_in(self.norm(hidden_states).permute(0, 2, 1))
        for block in self.transformer_blocks:
            tokens = block(tokens, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                           encoder_attention_mask=encoder_attention_mask, timestep=timestep, modulation_cond=modulation_cond,
                           cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels)
        return self.proj_out(tokens).permute(0, 2, 1).contiguous() + hidden_states


def randomise(module, seed):
    """TR.randomise, and the GroupNorm's weight around 1 and bias around 0."""
    TR.randomise(module, seed)
    g = torch.Generator().manual_seed(seed + 500)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.GroupNorm) and m.weight is not None:
                m.weight.copy_(1.0 + 0.5 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.4 * torch.randn(m.bias.shape, generator=g))
    return module


def make_transformer(in_channels, norm_num_groups, inner_dim, num_layers, seed=0, make_attention=TR.LinearAttention):
    return randomise(Transformer1D(in_channels, norm_num_groups, inner_dim, num_layers, make_attention), seed)
