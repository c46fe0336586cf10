"""Float64 PyTorch restatements of the multi-view anchor feature lift (GridEncoder.forward's perspective_projection branch,
igs/models/grid_encoder.py:66-88 over igs/utils/ops.py:444-477), in this repository's words, and the error bounds the tests use.

  lift_restate         -- explicit corners: projection, four gathers with zero padding, mean over the views (include/igs_rast.h).
  lift_grid_sample     -- the same composition through F.grid_sample (align_corners=False, zeros): an independent second statement.
  grid_encoder_intr    -- the intrinsics GridEncoder.forward builds, with its swapped names and its FOV[0] rule.
  forward_bound / backward_bound -- per-element bounds on |float32 kernel - float64 restatement|, derived below, not measured.

All functions take w2c (the inverse of the camera-to-world matrices) so that the float32 inversion, whose error depends on the
conditioning of the poses, is not part of the comparison: the tests pass the float32 inverse the product computes, upcast.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -23           # one unit in the last place of a float32 in [1, 2): twice the unit roundoff


def project(points, w2c, intr, H, W, align_corners=False):
    """(ix, iy, p_cam): points [B, A, 3], w2c [B*V, 4, 4], intr [B*V, 4] = fx, fy, cx, cy -> ix, iy [B*V, A] in pixel units."""
    BV, B = w2c.shape[0], points.shape[0]
    p = points.repeat_interleave(BV // B, 0)
    pc = p @ w2c[:, :3, :3].transpose(1, 2) + w2c[:, :3, 3].unsqueeze(1)
    fx, fy, cx, cy = (intr[:, i].unsqueeze(1) for i in range(4))
    u = (fx * pc[..., 0] + cx * pc[..., 2]) / pc[..., 2]
    v = (fy * pc[..., 1] + cy * pc[..., 2]) / pc[..., 2]
    gx, gy = 2 * u / W - 1, 2 * v / H - 1
    if align_corners:
        return (gx + 1) / 2 * (W - 1), (gy + 1) / 2 * (H - 1), pc
    return ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2, pc


def _corners(ix, iy, H, W):
    """The four corners of every sample: lists of (flat index clamped into the map, weight, valid).  A sample that is not finite has no
    valid corner (the stated deviation)."""
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    ix = torch.where(fin, ix, torch.full_like(ix, -10.0)).clamp(-10.0, W + 10.0)
    iy = torch.where(fin, iy, torch.full_like(iy, -10.0)).clamp(-10.0, H + 10.0)
    x0, y0 = ix.floor(), iy.floor()
    tx, ty = ix - x0, iy - y0
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = fin & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            w = (tx if dx else 1 - tx) * (ty if dy else 1 - ty)
            idx = (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)).long()
            out.append((idx, w, ok))
    return out


def sample_views(feat, ix, iy):
    """[B*V, A, C]: bilinear samples with zero padding of feat [B*V, C, H, W] at (ix, iy) [B*V, A]."""
    BV, C, H, W = feat.shape
    flat = feat.reshape(BV, C, H * W)
    acc = 0
    for idx, w, ok in _corners(ix, iy, H, W):
        vals = flat.gather(2, idx.unsqueeze(1).expand(-1, C, -1))                  # [BV, C, A]
        acc = acc + vals * (w * ok).unsqueeze(1)
    return acc.transpose(1, 2)


def lift_restate(feat, points, w2c, intr, align_corners=False):
    """out [B, A, C] = the mean over the V views of the samples, in feat's dtype (use float64)."""
    BV, C, H, W = feat.shape
    B = points.shape[0]
    ix, iy, _ = project(points.to(feat.dtype), w2c.to(feat.dtype), intr.to(feat.dtype), H, W, align_corners)
    s = sample_views(feat, ix, iy)
    return s.reshape(B, BV // B, -1, C).sum(1) / (BV // B)


def lift_grid_sample(feat, points, w2c, intr):
    """The same through F.grid_sample: normalised coordinates 2 u / W - 1, bilinear, zeros, align_corners=False, then the view mean."""
    BV, C, H, W = feat.shape
    B = points.shape[0]
    dt = feat.dtype
    p = points.to(dt).repeat_interleave(BV // B, 0)
    K = torch.zeros(BV, 3, 3, dtype=dt, device=feat.device)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = intr[:, 0].to(dt), intr[:, 1].to(dt), intr[:, 2].to(dt), intr[:, 3].to(dt), 1
    w2c = w2c.to(dt)
    cam = w2c[:, :3, :3] @ p.transpose(1, 2) + w2c[:, :3, 3:4]
    img = K @ cam
    img = img[:, :2] / img[:, 2:3]
    grid = torch.stack([2 * img[:, 0] / W - 1, 2 * img[:, 1] / H - 1], -1).unsqueeze(1)          # [BV, 1, A, 2]
    s = F.grid_sample(feat, grid, mode="bilinear", padding_mode="zeros", align_corners=False)    # [BV, C, 1, A]
    return s.squeeze(2).transpose(1, 2).reshape(B, BV // B, -1, C).mean(1)


def grid_encoder_intr(shape, fovx, fovy, BV, dtype=torch.float64):
    """[B*V, 4] = fx, fy, cx, cy as grid_encoder.py:75-82 builds them: `W, H = shape[-2:]` (so "W" is the map's height), FOV[0] for all."""
    Wn, Hn = shape[-2], shape[-1]
    fx, fy = Wn / (2 * math.tan(fovx / 2)), Hn / (2 * math.tan(fovy / 2))
    k = torch.tensor([fx, fy, Wn / 2.0, Hn / 2.0], dtype=torch.float32)            # the reference stores them in a float32 matrix
    return k.to(dtype).expand(BV, 4)


# ------------------------------------------------------------------------------------------------------------------------------------
# Bounds.  Everything is evaluated in float64 on the float32 inputs.
#
# Coordinates.  With |.| the evaluation on absolute values (P = |R| |p| + |T|, N = fx P.x + |cx| P.z):
#   u = (fx x_c + cx z_c) / z_c takes 16 rounded float32 operations: 6 for x_c (3 products, 3 sums), 6 for z_c, 3 for the numerator
#   (2 products, 1 sum), 1 division.  Each rounds with relative error <= 2^-24 = U / 2.  The numerator's error is <= 9 (U/2) N (1 + ...),
#   the denominator's <= 6 (U/2) P.z, and a quotient's first-order error is dN / |z| + |N| dz / z^2, so
#       d u <= 16 U (N / |z|) (P.z / |z|)                      (P.z >= |z|; counting in U instead of U / 2 leaves a factor two for the
#                                                               higher-order terms, valid while 16 U P.z / |z| << 1)
#   ix = ((2 u / W - 1 + 1) W - 1) / 2: the products by 2 and 1/2 are exact; /W, -1, +1, *W, -1 round values of magnitude
#   <= 2 |u| / W + 2 (normalised units, W / 2 pixels each), so they add <= 5 (U/2) (2 |u| / W + 2) (W / 2) <= 4 U (|u| + W):
#       d ix <= 16 U (N / |z|) (P.z / |z|) + 4 U (N / |z| + W),        d iy likewise with fy, cy, H.
# Output.  Bilinear sampling with zero padding is continuous and piecewise linear in (ix, iy), so a sample that lands in a neighbouring
#   cell needs no special case: |d sample| <= d ix Lx + d iy Ly with Lx (Ly) the largest horizontal (vertical) difference of
#   neighbouring pixels of the zero-padded map over the sample's cell and the cells around it (rows y0 - 1 .. y0 + 2, columns
#   x0 - 1 .. x0 + 2).  The sum itself: 4 V fmaf terms (<= 4 V (U/2)), the weights' two roundings (U) and the division by V (U/2):
#   <= (4 V + 2) U sum |w F| / V.
#       |d out| <= (1/V) sum_v (d ix Lx + d iy Ly) + (4 V + 2) U (1/V) sum_v sum_corners w |F|
# ------------------------------------------------------------------------------------------------------------------------------------
def coordinate_error(points, w2c, intr, H, W):
    """(d ix, d iy) [B*V, A] in float64."""
    points, w2c, intr = points.double(), w2c.double(), intr.double()
    BV, B = w2c.shape[0], points.shape[0]
    P = points.abs().repeat_interleave(BV // B, 0) @ w2c[:, :3, :3].abs().transpose(1, 2) + w2c[:, :3, 3].abs().unsqueeze(1)
    _, _, pc = project(points, w2c, intr, H, W)
    z = pc[..., 2].abs()
    fx, fy, cx, cy = (intr[:, i].abs().unsqueeze(1) for i in range(4))
    ua, va = (fx * P[..., 0] + cx * P[..., 2]) / z, (fy * P[..., 1] + cy * P[..., 2]) / z
    cond = P[..., 2] / z
    return 16 * U * ua * cond + 4 * U * (ua + W), 16 * U * va * cond + 4 * U * (va + H)


def _cell(ix, iy, H, W):
    fin = torch.isfinite(ix) & torch.isfinite(iy)
    x0 = torch.where(fin, ix, torch.full_like(ix, -10.0)).floor().clamp(-2, W).long()
    y0 = torch.where(fin, iy, torch.full_like(iy, -10.0)).floor().clamp(-2, H).long()
    return x0, y0


def forward_bound(feat, points, w2c, intr):
    """[B, A, C] float64: the per-element bound derived above."""
    BV, C, H, W = feat.shape
    B, V = points.shape[0], BV // points.shape[0]
    f = feat.double()
    ix, iy, _ = project(points.double(), w2c.double(), intr.double(), H, W)
    dix, diy = coordinate_error(points, w2c, intr, H, W)
    x0, y0 = _cell(ix, iy, H, W)
    fp = F.pad(f, (3, 3, 3, 3))                                                   # pixel (y, x) at [y + 3, x + 3]
    dx = (fp[..., :, 1:] - fp[..., :, :-1]).abs()                                 # [BV, C, H + 6, W + 5]: between x + 3 and x + 4
    dy = (fp[..., 1:, :] - fp[..., :-1, :]).abs()                                 # [BV, C, H + 5, W + 6]
    Lx = F.max_pool2d(dx, kernel_size=(4, 3), stride=1)                           # rows y .. y + 3, differences x .. x + 2
    Ly = F.max_pool2d(dy, kernel_size=(3, 4), stride=1)
    # cell (x0, y0): rows y0 - 1 .. y0 + 2 start at padded row y0 + 2; differences of columns x0 - 1 .. x0 + 2 start at padded x0 + 2
    ix_x = ((y0 + 2) * Lx.shape[-1] + (x0 + 2)).unsqueeze(1).expand(-1, C, -1)
    ix_y = ((y0 + 2) * Ly.shape[-1] + (x0 + 2)).unsqueeze(1).expand(-1, C, -1)
    lx = Lx.reshape(BV, C, -1).gather(2, ix_x).transpose(1, 2)                    # [BV, A, C]
    ly = Ly.reshape(BV, C, -1).gather(2, ix_y).transpose(1, 2)
    geo = (dix.unsqueeze(-1) * lx + diy.unsqueeze(-1) * ly).reshape(B, V, -1, C).sum(1) / V
    return geo + (4 * V + 2) * U * lift_restate(f.abs(), points.double(), w2c.double(), intr.double()) + 1e-30


def backward_bound(grad, points, w2c, intr, H, W, half=False, ref=None):
    """[B*V, C, H, W] float64 bound on |d feat - float64 autograd| for the upstream gradient grad [B, A, C].
    The weight a sample gives a pixel is hat(ix - x) hat(iy - y), Lipschitz 1 in each coordinate wherever the sample lands, so its error
    is <= d ix + d iy and it can be non-zero only for the pixels x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2 of the float64 cell:
        |d dfeat[p]| <= (1/V) sum over those samples (d ix + d iy) |g| + (deg + 3) U (1/V) sum over edges w |g|
    (deg = the longest pixel list: deg fmaf terms at U / 2, two weight roundings, the division) and, for float16 features, the one
    rounding of the result to half: max(2^-11 |ref|, 2^-25).  The absolute floor is the format's: below 2^-14 half is subnormal with
    spacing 2^-24, so a correctly rounded 6.29e-7 is 11 * 2^-24 = 6.56e-7, 4 % away (seen at the shipped shape, where gradients of
    that size occur under near-zero bilinear weights)."""
    B, A, C = grad.shape
    BV = w2c.shape[0]
    V = BV // B
    g = grad.double().abs()
    pts, w2, k = points.double(), w2c.double(), intr.double()
    ix, iy, _ = project(pts, w2, k, H, W)
    dix, diy = coordinate_error(points, w2c, intr, H, W)
    x0, y0 = _cell(ix, iy, H, W)
    gv = g.repeat_interleave(V, 0) * (dix + diy).unsqueeze(-1)                    # [BV, A, C]
    Hp, Wp = H + 6, W + 6
    acc = torch.zeros(BV, Hp * Wp, C, dtype=torch.float64, device=grad.device)
    for oy in range(-1, 3):
        for ox in range(-1, 3):
            idx = (y0 + oy + 3) * Wp + (x0 + ox + 3)
            acc.scatter_add_(1, idx.unsqueeze(-1).expand(-1, -1, C), gv)
    geo = acc.reshape(BV, Hp, Wp, C)[:, 3:3 + H, 3:3 + W].permute(0, 3, 1, 2) / V
    # the exact sum of w |g| per pixel and the longest list, from the float64 corners
    absw = torch.zeros(BV, H * W, C, dtype=torch.float64, device=grad.device)
    cnt = torch.zeros(BV, H * W, dtype=torch.float64, device=grad.device)
    gg = g.repeat_interleave(V, 0)
    for idx, w, ok in _corners(ix, iy, H, W):
        absw.scatter_add_(1, idx.unsqueeze(-1).expand(-1, -1, C), gg * (w * ok).unsqueeze(-1))
        cnt.scatter_add_(1, idx, ok.double())
    deg = cnt.max().item() + 4                                                     # (+ 4: a neighbouring cell's corners in float32)
    tol = geo + (deg + 3) * U * absw.reshape(BV, H, W, C).permute(0, 3, 1, 2) / V + 1e-30
    if half:          # one rounding to nearest half: 2^-11 relative, and never finer than half the subnormal spacing 2^-24 (|x| < 2^-14)
        tol = tol + torch.clamp(2.0 ** -11 * ref.abs(), min=2.0 ** -25)
    return tol
