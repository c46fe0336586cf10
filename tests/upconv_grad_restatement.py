"""The backward of the fused 2x bilinear upsample + 3x3 convolution (igs_amd/csrc/upconv_bwd.hip, igs_amd.motion.upsample_conv_autograd)
restated in float64, with per-element bounds derived for it, the transposed pack written out element by element, the wrong variants the
bounds must reject and the cases the host and the GPU tests share.  No test here: tests/test_upconv_grad_host.py and
tests/test_gpu_upconv_grad.py import it.

The gradients, with up = U x (the forward's clamped bilinear rule), out = conv(up, W) + b, g = d out:
    db[o]          = sum_{n,Y,X} g[n,o,Y,X]
    dW[o,c,dy,dx]  = sum_{n,Y,X} g[n,o,Y,X] up[n,c,Y+dy-1,X+dx-1]                 up zero outside the 2H x 2W map
    dup[n,c,y,x]   = sum_{o,dy,dx} W[o,c,dy,dx] g[n,o,y-dy+1,x-dx+1]              g zero outside the map
    dx             = U^T dup
U is written out as a matrix here (upsample_matrix), from the rule and not from F.interpolate; the host test holds the whole restatement
against float64 autograd through F.interpolate and F.conv2d.

Bounds.  u24 = 2^-24, u11 = 2^-11, gamma_m(u) = m u / (1 - m u), M = N 4 H W.
  float32
    dx: gamma_{9 Cout + 16} U^T(conv^T(|W|, |g|)).  A dup value is one fma chain over the 9 Cout products (the zero products of a padded
        channel tile round nothing); the kernel's gather passes it through 4 fma of the column pass and 4 of the row pass, 8 roundings
        of the at most 16 allowed (the weights 1/4, 3/4, 1 and their products are exact).
    dW: gamma_{M + 4} sum |g| up(|x|): any summation order over the M pixels, and the 4 roundings of the recomputed interpolation.
    db: gamma_M sum |g|.
  float16 (the forward's derivation, upconv_restatement.py): g is given in half and is exact.  Every product carries 2 u11 + u11^2 -- for
    dx the weight rounded to half, for dW the float32 upsampled value rounded to half -- beside the float32 gamma; a half operand below
    2^-14 is subnormal and its rounding error absolute, up to 2^-25, times the other factor: 9 Cout 2^-25 (max |W| + max |g|) per dup
    value, gathered with weights that sum to at most 4; M 2^-25 (max |g| + max up(|x|)) for dW.  dW and db stay float32; db has no
    half rounding at all.
  dx is returned in x's dtype, so where x is half -- under either compute dtype -- it is rounded once more: (...) (1 + u11) + u11 |dx64|.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import upconv_restatement as UR
from upconv_restatement import U11, U24, gamma

SLICES = 64                                                      # IGS_UPCONV_BWD_SLICES
SHIPPED = UR.SHIPPED
# the dgrad kernel is picked by ceil(Cin / 32): UR.WIDTHS has Cin = 1, 33, 65, 96, 128; these add the top of the first two ranges and the
# bottom of the last (32, 64, 97).  The wgrad kernel has one instance per dtype pair over 1 .. 128 both ways: (1, 128), (128, 1) are there.
WIDTHS = UR.WIDTHS + ((32, 40), (64, 5), (97, 33))
# dgrad's tile is 3 x 15 low-resolution pixels, wgrad's 4 x 32 upsampled ones (2 x 16): (7, 31) is partial in and spans several of both, both ways
MAPS = UR.MAPS + ((7, 31),)
EDGE_CASES = [(ci, co, 2, h, w) for ci, co in WIDTHS for h, w in MAPS]
# wgrad pixel tiles N ceil(2H / 4) ceil(2W / 32): 6 (fewer than SLICES), 2 * 8 * 4 = 64 (exactly), 3 * 8 * 4 = 96 (more, uneven slices)
SLICE_CASES = ((7, 5, 2, 5, 7), (5, 7, 2, 16, 50), (5, 7, 3, 16, 50))
CPU_CASES = ((128, 128, 2, 5, 7), (33, 65, 2, 17, 3), (7, 5, 2, 1, 1), (128, 64, 2, 33, 18), (1, 128, 2, 9, 1), (97, 32, 3, 40, 20))
DX_VARIANTS = ("unflipped_taps", "transposed_taps", "weight_not_transposed", "gather_without_fold", "align_corners")
DW_VARIANTS = ("replicate_padding", "low_resolution_zero_padding", "flipped_taps")


def wgrad_tiles(N, H, W):
    return N * -(-2 * H // 4) * -(-2 * W // 32)


def upsample_matrix(L, fold=True):
    """U [2L, L] float64 of one axis: destination d reads source (d + 0.5) / 2 - 0.5 clamped at 0, its neighbour clamped at L - 1.
    fold=False is the wrong gather: what the clamp moved onto the first / last sample is dropped instead."""
    U = torch.zeros(2 * L, L, dtype=torch.float64)
    for d in range(2 * L):
        m = d >> 1
        i0, i1, w1 = (m, m + 1, 0.25) if d & 1 else (m - 1, m, 0.75)
        for i, w in ((i0, 1.0 - w1), (i1, w1)):
            if fold:
                i = min(max(i, 0), L - 1)
            if 0 <= i < L:
                U[d, i] += w
    return U


def gather(dup, H, W, fold=True):
    """U^T dup: [N, C, 2H, 2W] -> [N, C, H, W]."""
    return torch.einsum("yi,ncyx,xj->ncij", upsample_matrix(H, fold), dup, upsample_matrix(W, fold))


def weight_t(w):
    """[Cin, Cout, 3, 3]: weight_t[c, o, dy, dx] = weight[o, c, 2 - dy, 2 - dx]."""
    return w.flip(2, 3).transpose(0, 1)


def wgrad64(g64, up_padded):
    """dW from g [N, Cout, 2H, 2W] and the padded map [N, Cin, 2H + 2, 2W + 2]."""
    OH, OW = g64.shape[2:]
    return torch.stack([torch.stack([torch.einsum("noyx,ncyx->oc", g64, up_padded[:, :, dy:dy + OH, dx:dx + OW]) for dx in range(3)], -1)
                        for dy in range(3)], -2)


def restate(x, weight, g, half=False):
    """dict(dx64, dw64, db64, bound_dx, bound_dw, bound_db) for x [N, Cin, H, W], weight [Cout, Cin, 3, 3], g [N, Cout, 2H, 2W], each taken
    as the exact value it holds.  half: the float16 instance's bounds.  The dx bound counts the final rounding where x is half."""
    x64, w64, g64 = x.detach().double(), weight.detach().double(), g.detach().double()
    N, Cin, H, W = x64.shape
    Cout, M = w64.shape[0], N * 4 * H * W
    up, upabs = UR.upsample64(x64), UR.upsample64(x64.abs())
    dx64 = gather(F.conv2d(g64, weight_t(w64), padding=1), H, W)
    Sx = gather(F.conv2d(g64.abs(), weight_t(w64.abs()), padding=1), H, W)
    dw64 = wgrad64(g64, F.pad(up, (1, 1, 1, 1)))
    Sw = wgrad64(g64.abs(), F.pad(upabs, (1, 1, 1, 1)))
    db64, Sb = g64.sum((0, 2, 3)), g64.abs().sum((0, 2, 3))
    gx, gw, gb = gamma(9 * Cout + 16, U24), gamma(M + 4, U24), gamma(M, U24)
    if half:
        p = 2 * U11 + U11 * U11
        bx = (p + gx) * Sx + 4 * 9 * Cout * 2.0 ** -25 * (w64.abs().max() + g64.abs().max())
        bw = (p + gw) * Sw + M * 2.0 ** -25 * (g64.abs().max() + upabs.max())
    else:
        bx, bw = gx * Sx, gw * Sw
    if x.dtype == torch.float16:                                 # dx leaves in x's dtype: the one rounding to half, whatever computed it
        bx = bx * (1 + U11) + U11 * dx64.abs()
    return dict(dx64=dx64, dw64=dw64, db64=db64, bound_dx=bx, bound_dw=bw, bound_db=gb * Sb)


def autograd64(x, weight, g, align_corners=False):
    """(dx, dW, db) of float64 autograd through F.interpolate and F.conv2d."""
    x64 = x.detach().double().requires_grad_(True)
    w64 = weight.detach().double().requires_grad_(True)
    b64 = torch.zeros(weight.shape[0], dtype=torch.float64, requires_grad=True)
    out = F.conv2d(F.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=align_corners), w64, b64, padding=1)
    return torch.autograd.grad(out, (x64, w64, b64), g.detach().double())


def autograd32(x, weight, g):
    """PyTorch's own float32 gradients on the CPU."""
    x32 = x.detach().float().requires_grad_(True)
    w32 = weight.detach().float().requires_grad_(True)
    b32 = torch.zeros(weight.shape[0], requires_grad=True)
    out = F.conv2d(F.interpolate(x32, scale_factor=2, mode="bilinear", align_corners=False), w32, b32, padding=1)
    return torch.autograd.grad(out, (x32, w32, b32), g.detach().float())


def emulate_half(x, weight, g):
    """The float16 instance's roundings on the CPU with exact (float64) sums: half weights for dx (rounded once more where x is half), the
    float32 interpolation rounded to half for dW."""
    H, W = x.shape[2:]
    g64 = g.detach().half().double()
    dx = gather(F.conv2d(g64, weight_t(weight.detach().half().double()), padding=1), H, W)
    if x.dtype == torch.float16:
        dx = dx.half()
    up = F.interpolate(x.detach().float(), scale_factor=2, mode="bilinear", align_corners=False).half().double()
    return dx, wgrad64(g64, F.pad(up, (1, 1, 1, 1))), g64.sum((0, 2, 3))


def dx_variant(kind, x, weight, g):
    """A plausible wrong dx, in float64."""
    w64, g64 = weight.detach().double(), g.detach().double()
    H, W = x.shape[2:]
    if kind == "unflipped_taps":
        return gather(F.conv2d(g64, w64.transpose(0, 1), padding=1), H, W)
    if kind == "transposed_taps":
        return gather(F.conv2d(g64, weight_t(w64).transpose(2, 3), padding=1), H, W)
    if kind == "weight_not_transposed":                         # (square widths only)
        return gather(F.conv2d(g64, w64.flip(2, 3), padding=1), H, W)
    if kind == "gather_without_fold":
        return gather(F.conv2d(g64, weight_t(w64), padding=1), H, W, fold=False)
    if kind == "align_corners":
        return autograd64(x, weight, g, align_corners=True)[0]
    raise KeyError(kind)


def dw_variant(kind, x, weight, g):
    """A plausible wrong dW, in float64."""
    x64, g64 = x.detach().double(), g.detach().double()
    if kind == "replicate_padding":
        return wgrad64(g64, F.pad(UR.upsample64(x64), (1, 1, 1, 1), mode="replicate"))
    if kind == "low_resolution_zero_padding":
        return wgrad64(g64, UR.upsample64(F.pad(x64, (1, 1, 1, 1)))[:, :, 1:-1, 1:-1])
    if kind == "flipped_taps":
        return wgrad64(g64, F.pad(UR.upsample64(x64), (1, 1, 1, 1))).flip(2, 3)
    raise KeyError(kind)


def variant_applies(kind, case):
    """False where the variant is the reference itself: align_corners on a 1 x 1 map, the untransposed weight at unequal widths."""
    Cin, Cout, _, H, W = case
    if kind == "align_corners":
        return H > 1 or W > 1
    if kind == "weight_not_transposed":
        return Cin == Cout
    return True


def make_g(case, half=False, single_pixel=False, seed=0):
    """d out [N, Cout, 2H, 2W] = randn, float32 (rounded to half first for the float16 instance, which then reads exactly that);
    single_pixel: zero outside one pixel of the last image."""
    Cin, Cout, N, H, W = case
    gen = torch.Generator().manual_seed(77 + 1000 * Cin + 10 * Cout + 7 * H + W + seed)
    g = torch.randn(N, Cout, 2 * H, 2 * W, generator=gen)
    if single_pixel:
        keep = torch.zeros_like(g)
        keep[N - 1, :, (2 * H) // 2, 2 * W - 1] = 1.0
        g = g * keep
    return g.half() if half else g


def worst(got, ref64, bound):
    """max |got - ref64| / bound over every element (nan where got is not finite).  Where the bound is zero (nothing non-zero is added
    up: g zero outside one pixel) the element must be exact: 0, or inf if it is not."""
    err = (got.detach().double().cpu() - ref64).abs()
    if not torch.isfinite(err).all():
        return float("nan")
    b = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    d = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(d.max())


@functools.lru_cache(maxsize=None)
def reference(case, half=False, x_half=False, single_pixel=False):
    """(x, conv, g, restate(...)) of a case, computed once and shared: x rounded to half first for x_half, g for half."""
    x, conv = UR.make_case(*case)
    if x_half:
        x = x.half()
    g = make_g(case, half=half, single_pixel=single_pixel)
    return x, conv, g, restate(x, conv.weight, g, half=half)


def pack_t_restate(weight, half):
    """wpack_t as include/igs_rast.h defines it, written out element by element from weight [Cout, Cin, 3, 3] (numpy): the layout of
    igs_upconv_fwd's wpack for the [Cin, Cout, 3, 3] convolution weight_t[c, o, dy, dx] = weight[o, c, 2 - dy, 2 - dx]."""
    Cout, Cin = weight.shape[:2]
    ct, ot = -(-Cin // 32), -(-Cout // 32)                       # ct: the output tiles of the transposed convolution, ot: its input tiles
    E = 8 if half else 4
    out = np.zeros(9 * ct * ot * 1024, dtype=weight.dtype)
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        for c in range(Cin):
            for o in range(Cout):
                col = o % 32                                     # = (e & 3) + 8 (e >> 2) + 4 h
                h, e = (col >> 2) & 1, (col & 3) + 4 * (col >> 3)
                chunk, j = divmod(e, E)
                lane = 32 * h + (c % 32)
                tile = (tap * ct + c // 32) * ot + o // 32
                out[tile * 1024 + (chunk * 64 + lane) * E + j] = weight[o, c, 2 - dy, 2 - dx]
    return out
