"""Float64 PyTorch restatement of what igs_amd/csrc/inorm.hip computes: the four instance-norm modes and the closed form of
feature_add_position; the per-element allowances of the GPU tests with the reasoning behind them; a float32 emulation of the kernel's
arithmetic with three deliberately wrong variants; the test inputs; and a stand-in for the unimatch CNN encoder in this repository's own
wording (the attribute names and layer sizes of the reference's module, which is not available where the GPU tests run).

Modes (include/igs_rast.h): 0 IN(x); 1 relu(IN(x)); 2 relu(skip + relu(IN(x))); 3 relu(IN(skip) + relu(IN(x))), with
IN(t) = (t - mean) / sqrt(var + eps) per H x W plane and the biased variance.
"""
import math

import torch
import torch.nn as nn

PLAIN, RELU, RELU_ADD_RELU, RELU_ADDNORM_RELU = 0, 1, 2, 3
MODES = (PLAIN, RELU, RELU_ADD_RELU, RELU_ADDNORM_RELU)
HAS_SKIP = (RELU_ADD_RELU, RELU_ADDNORM_RELU)
U24, U23, U11 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -11


# ---------------------------------------------------------------- the norm modes
def stats(t, eps):
    """(mean, rstd) per plane of a [..., H, W] float64 tensor, biased variance from centred values."""
    mu = t.mean(dim=(-2, -1), keepdim=True)
    var = ((t - mu) ** 2).mean(dim=(-2, -1), keepdim=True)
    return mu, 1.0 / torch.sqrt(var + eps)


def restate(x, skip, mode, eps=1e-5):
    """The mode's result in the dtype of x (pass float64), [N, C, H, W]."""
    mu, rstd = stats(x, eps)
    y = (x - mu) * rstd
    if mode == PLAIN:
        return y
    y = torch.relu(y)
    if mode == RELU:
        return y
    if mode == RELU_ADDNORM_RELU:
        km, kr = stats(skip, eps)
        skip = (skip - km) * kr
    return torch.relu(skip + y)


def norm_term(t, eps):
    """4 * 2^-24 * ((|t| + |mean|) * rstd + |t_hat| + 1): the rounding of t - mean (both operands carry half an ulp of their own size once
    the mean is a rounded float32), of the mean and of rstd (relative, so scaled by |t_hat|), and one ulp-of-one term for the final
    multiply and the representation of a result of order one; the constant 4 is the margin over that arithmetic."""
    mu, rstd = stats(t, eps)
    return 4.0 * U24 * ((t.abs() + mu.abs()) * rstd + ((t - mu) * rstd).abs() + 1.0)


def allowance(x, skip, mode, eps, out_dtype, ref):
    """Per element, for float64 copies x / skip of the float32 or float16 inputs and the float64 restatement `ref`."""
    a = norm_term(x, eps)
    if mode == RELU_ADDNORM_RELU:
        a = a + norm_term(skip, eps)
    if mode in HAS_SKIP:
        a = a + U23 * ref.abs()
    if out_dtype == torch.float16:
        a = a + U11 * ref.abs()
    return a


def position_allowance(ref, out_dtype):
    """2e-6 + 2^-23 |out| (+ 2^-11 |out| for float16): three float32 roundings of an argument of at most 2 pi give about 1.1e-6, the
    sine's own error comes on top; the add rounds once."""
    a = 2e-6 + U23 * ref.abs()
    if out_dtype == torch.float16:
        a = a + U11 * ref.abs()
    return a


# ---------------------------------------------------------------- float32 emulation of the kernel's arithmetic, and wrong variants
def _tree_sum(t):
    """Pairwise float32 sum over the last dimension (the kernel: four running sums per thread, a butterfly, the waves in order)."""
    t = t.reshape(t.shape[0], -1)
    n = t.shape[1]
    p = 1 << max(n - 1, 0).bit_length()
    t = torch.cat([t, t.new_zeros(t.shape[0], p - n)], 1)
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def emulate(x, eps=1e-5, variant="right"):
    """IN(x) of a [P, H, W] float32 tensor in float32 arithmetic.  variant: "right" (tree mean, centred sums, the corrected two-pass
    form), "one_pass" (E[x^2] - mean^2), "unbiased" (n - 1), "no_eps"."""
    assert x.dtype == torch.float32
    P, n = x.shape[0], x.shape[1] * x.shape[2]
    nf = torch.tensor(float(n), dtype=torch.float32)
    m = (_tree_sum(x) / nf).view(P, 1, 1)
    if variant == "one_pass":
        var = (_tree_sum(x * x) / nf).view(P, 1, 1) - m * m
        mean = m
    else:
        d = x - m
        dm = (_tree_sum(d) / nf).view(P, 1, 1)
        s2 = _tree_sum(d * d).view(P, 1, 1)
        var = s2 / (nf - 1 if variant == "unbiased" else nf) - dm * dm
        mean = m + dm
    var = torch.where(var < 0, torch.zeros_like(var), var)
    rstd = 1.0 / torch.sqrt(var + (0.0 if variant == "no_eps" else torch.tensor(eps, dtype=torch.float32)))
    return (x - mean) * rstd


# ---------------------------------------------------------------- inputs
PLANE_MEANS = (0.0, 100.0, -1e3)
PLANE_STDS = (1.0, 1e-3, 30.0)


def plane_inputs(planes, H, W, dtype, device, seed, constant_plane=None):
    """[1, planes, H, W]: plane p has the pair number q = (seed + 4 p) mod 9 of (mean, std) = (PLANE_MEANS[q % 3], PLANE_STDS[q // 3]): three
    planes take three different means and three different stds, nine or more take every pair, and the seeds of the cases walk through
    the pairs.  Plane `constant_plane` holds one value (one that no power-of-two count sums exactly)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, planes, H, W, generator=g, dtype=torch.float64)
    for p in range(planes):
        q = (seed + 4 * p) % 9
        x[0, p] = x[0, p] * PLANE_STDS[q // 3] + PLANE_MEANS[q % 3]
    if constant_plane is not None:
        x[0, constant_plane] = 100.37
    return x.to(dtype).to(device)


# ---------------------------------------------------------------- feature_add_position, closed form
def position_table(C, wh, ww, dtype=torch.float64):
    """[C, wh, ww]: channel c < C / 2 holds s(c, y + 1, wh), channel c >= C / 2 holds s(c - C / 2, x + 1, ww)."""
    n = C // 2
    i = torch.arange(n, dtype=dtype)
    dim = 10000.0 ** (2.0 * torch.div(i, 2, rounding_mode="floor") / n)
    even = (torch.arange(n) % 2 == 0)

    def s(L):
        p = torch.arange(1, L + 1, dtype=dtype)
        a = (p / (L + 1e-6) * (2.0 * math.pi))[None, :] / dim[:, None]          # [n, L]
        return torch.where(even[:, None], a.sin(), a.cos())

    ty = s(wh)[:, :, None].expand(n, wh, ww)
    tx = s(ww)[:, None, :].expand(n, wh, ww)
    return torch.cat([ty, tx], 0)


def restate_position(f0, f1, splits):
    """feature_add_position for [B, C, H, W] float64 features."""
    B, C, H, W = f0.shape
    wh, ww = H // splits, W // splits
    pos = position_table(C, wh, ww, f0.dtype).to(f0.device).repeat(1, splits, splits)
    return f0 + pos, f1 + pos


# ---------------------------------------------------------------- a stand-in for the unimatch CNN encoder
class Block(nn.Module):
    """Two 3 x 3 convolutions, each followed by a norm and an in-place ReLU, plus the input (through a strided 1 x 1 convolution and a norm
    when the shape changes), then a ReLU."""

    def __init__(self, cin, cout, norm=nn.InstanceNorm2d, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = norm(cout)
        self.norm2 = norm(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.norm3 = norm(cout)
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class Encoder(nn.Module):
    """7 x 7 stride-2 stem to 64 channels, three stages of two blocks (64, 96 at stride 2, 128 at stride 2), a 1 x 1 output convolution:
    12 convolutions in blocks, 15 norms."""

    def __init__(self, out_dim=128, norm=nn.InstanceNorm2d, dims=(64, 96, 128)):
        super().__init__()
        self.num_branch = 1
        self.conv1 = nn.Conv2d(3, dims[0], 7, stride=2, padding=3, bias=False)
        self.norm1 = norm(dims[0])
        self.relu1 = nn.ReLU(inplace=True)
        self.layer1 = nn.Sequential(Block(dims[0], dims[0], norm), Block(dims[0], dims[0], norm))
        self.layer2 = nn.Sequential(Block(dims[0], dims[1], norm, 2), Block(dims[1], dims[1], norm))
        self.layer3 = nn.Sequential(Block(dims[1], dims[2], norm, 2), Block(dims[2], dims[2], norm))
        self.conv2 = nn.Conv2d(dims[2], out_dim, 1)

    def forward(self, x):
        x = self.relu1(self.norm1(self.conv1(x)))
        x = self.layer3(self.layer2(self.layer1(x)))
        return [self.conv2(x)]


def make_encoder(seed=0, norm=nn.InstanceNorm2d, **kw):
    torch.manual_seed(seed)
    return Encoder(norm=norm, **kw).eval().requires_grad_(False)
