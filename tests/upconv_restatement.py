"""The fused 2x bilinear upsample + 3x3 convolution (igs_amd/csrc/upconv.hip, igs_amd.motion.upsample_conv) restated in float64, with
the per-element error bound derived for it, the packing restated element by element, the wrong variants the bound must reject and the
cases the host and the GPU tests share.  No test here: tests/test_upconv_host.py and tests/test_gpu_upconv.py import it.

Reference: F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) and F.conv2d(padding=1) in double on the CPU.

Bound.  Write u24 = 2^-24, u11 = 2^-11, gamma_m(u) = m u / (1 - m u), and S = |bias| + conv(|weight|, up(|x|)) in float64: the sum of
the magnitudes of everything an output adds up (the interpolation weights are non-negative, so up(|x|) bounds |up(x)| term by term).
  float32: every output is ONE fma chain from the bias over the 9 Cin products (m = 9 Cin roundings), and an upsampled value is two
    lerps of two roundings each (the weights 0.25 / 0.75 are exact): 4 more.  bound = gamma_{9 Cin + 4}(u24) S.
  float16: the upsampled value (float32, 4 roundings) is rounded to half and so is the weight: each product carries (1 + u11)^2 - 1 =
    2 u11 + u11^2 beside the float32 chain's gamma; the result is rounded once to half: (...) S (1 + u11) + u11 |out64|.  A half operand
    below 2^-14 is subnormal and its rounding error is absolute, up to 2^-25, times the other factor: 9 Cin 2^-25 (max |weight| +
    max up(|x|)) covers every product.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U24, U11 = 2.0 ** -24, 2.0 ** -11
SHIPPED = (128, 128, 2, 5, 7)                                    # Cin, Cout, N, H, W
# (Cin, Cout).  igs_upconv_fwd picks the kernel by ceil(Cout / 32) output tiles: 1, 3, 1, 1, 4, then the two-tile kernel at the bottom, the
# top and the inside of its range 33 .. 64, under one, four and three input tiles, then the last Cout of three tiles and the first of four
WIDTHS = ((7, 5), (33, 65), (96, 32), (128, 1), (1, 128), (7, 33), (128, 64), (65, 48), (5, 96), (40, 97))
MAPS = ((1, 1), (1, 9), (9, 1), (17, 3), (33, 18))
CASES = [SHIPPED] + [(ci, co, 2, h, w) for ci, co in WIDTHS for h, w in MAPS]
VARIANTS = ("align_corners", "nearest", "flipped_taps", "transposed_taps", "replicate_padding", "low_resolution_zero_padding")
UPSAMPLING_VARIANTS = ("align_corners", "nearest")              # at H W = 1 these are the reference itself


def gamma(m, u):
    return m * u / (1.0 - m * u)


def make_case(Cin, Cout, N, H, W, seed=0):
    """(x float32 [N, Cin, H, W] = 3 + 0.5 randn, conv = nn.Conv2d(Cin, Cout, 3, padding=1) with its default weights and a bias drawn from
    0.4 randn: with Conv2d's default bias the float16 bound would not tell a missing bias)."""
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + 7 * H + W + seed)
    x = 3.0 + 0.5 * torch.randn(N, Cin, H, W, generator=g)
    torch.manual_seed(Cin * 131 + Cout + seed)
    conv = torch.nn.Conv2d(Cin, Cout, 3, stride=1, padding=1)
    with torch.no_grad():
        conv.bias.copy_(0.4 * torch.randn(Cout, generator=g))
    conv.requires_grad_(False)
    return x, conv


def upsample64(x):
    return F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)


def restate(x, weight, bias, half=False):
    """dict(out64, S, bound) for x [N, Cin, H, W], weight [Cout, Cin, 3, 3], bias [Cout] or None, each taken as the exact value it holds."""
    x64, w64 = x.detach().double(), weight.detach().double()
    b64 = torch.zeros(w64.shape[0], dtype=torch.float64) if bias is None else bias.detach().double()
    Cin = w64.shape[1]
    out64 = F.conv2d(upsample64(x64), w64, b64, padding=1)
    upabs = upsample64(x64.abs())
    S = F.conv2d(upabs, w64.abs(), b64.abs(), padding=1)
    g = gamma(9 * Cin + 4, U24)
    if half:
        bound = (2 * U11 + U11 * U11 + g) * S * (1 + U11) + U11 * out64.abs() + 9 * Cin * 2.0 ** -25 * (w64.abs().max() + upabs.max())
    else:
        bound = g * S
    return dict(out64=out64, S=S, bound=bound)


def variant(kind, x, weight, bias):
    """A plausible wrong implementation, in float64."""
    x64, w64 = x.detach().double(), weight.detach().double()
    b64 = None if bias is None else bias.detach().double()
    if kind == "align_corners":
        return F.conv2d(F.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=True), w64, b64, padding=1)
    if kind == "nearest":
        return F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), w64, b64, padding=1)
    if kind == "flipped_taps":
        return F.conv2d(upsample64(x64), w64.flip(2, 3), b64, padding=1)
    if kind == "transposed_taps":
        return F.conv2d(upsample64(x64), w64.transpose(2, 3), b64, padding=1)
    if kind == "replicate_padding":
        return F.conv2d(F.pad(upsample64(x64), (1, 1, 1, 1), mode="replicate"), w64, b64)
    if kind == "low_resolution_zero_padding":                   # the zero ring put round x, then upsampled: the halo is an interpolation towards 0
        return F.conv2d(upsample64(F.pad(x64, (1, 1, 1, 1)))[:, :, 1:-1, 1:-1], w64, b64)
    raise KeyError(kind)


def emulate_half(x, weight, bias):
    """The float16 instance's roundings on the CPU: float32 interpolation rounded to half, half weights, an exact (float64) sum, the
    float32 bias, one rounding to half."""
    up = F.interpolate(x.detach().float(), scale_factor=2, mode="bilinear", align_corners=False).half().double()
    b = None if bias is None else bias.detach().float().double()
    return F.conv2d(up, weight.detach().half().double(), b, padding=1).half()


def worst(got, out64, bound):
    """max |got - out64| / bound over every element (nan where got is not finite)."""
    d = (got.detach().double().cpu() - out64).abs() / bound
    return float("nan") if not torch.isfinite(d).all() else float(d.max())


@functools.lru_cache(maxsize=None)
def reference(case, half=False, x_half=False):
    """(x, conv, restate(...)) of a case, computed once and shared; x_half: x rounded to float16 first (the kernel then reads exactly that)."""
    x, conv = make_case(*case)
    if x_half:
        x = x.half()
    return x, conv, restate(x, conv.weight, conv.bias, half=half)


def pack_restate(weight, half):
    """wpack as include/igs_rast.h defines it, written out element by element from weight [Cout, Cin, 3, 3] (numpy)."""
    Cout, Cin = weight.shape[:2]
    ot, kt = -(-Cout // 32), -(-Cin // 32)
    E = 8 if half else 4
    out = np.zeros(9 * ot * kt * 1024, dtype=weight.dtype)
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        for o in range(Cout):
            for c in range(Cin):
                col = c % 32                                     # = (e & 3) + 8 (e >> 2) + 4 h
                h, e = (col >> 2) & 1, (col & 3) + 4 * (col >> 3)
                chunk, j = divmod(e, E)
                lane = 32 * h + (o % 32)
                tile = (tap * ot + o // 32) * kt + c // 32
                out[tile * 1024 + (chunk * 64 + lane) * E + j] = weight[o, c, dy, dx]
    return out
