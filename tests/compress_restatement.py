"""A restatement, in torch float32 on the CPU, of what the compress rasterizer's count pass computes (the reference's CUDA cannot be
built here).  Reference: submodules/RaDe-GS/submodules/compress-diff-gaussian-rasterization (CRZ below).

  * preprocess (CRZ cuda_rasterizer/forward.cu:158-262): vanilla 3DGS.  The undilated 2-D covariance, the pixel position, the colour
    and the view depth come from oracle.torch_oracle.per_gaussian; then the covariance is dilated (+0.3 on both diagonal terms,
    computeCov2D :114-115), and the determinant (det == 0 culls), conic and radius ceil(3 sqrt(max(l1, l2))) with its 0.1 floor
    are recomputed from the dilated one.  The opacity is the raw one (conic_opacity.w = opacities[idx]).
  * count blend (CRZ renderCUDA_count, forward.cu:379-503): per 16x16 tile, the Gaussians whose tile rectangle covers it in
    ascending depth (ties by index: the binning keys are depth, then Gaussian id); pixel centre = the integer pixel; power > 0 and
    alpha < 1/255 skip; T (1 - alpha) < 1e-4 ends the pixel without blending or counting that splat; every blended splat counts one
    pixel for its Gaussian.  The reference's count increments race; this restates the race-free value.
"""
import numpy as np
import torch

from oracle.torch_oracle import per_gaussian

TILE = 16


def vanilla_preprocess(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, scale_modifier, viewmatrix,
                       projmatrix, campos, tanfovx, tanfovy, W, H, degree):
    """Per-Gaussian dict: valid, xy [P,2], conic [P,3], opacity [P], rgb [P,3], depth [P], radius [P] (float; 0 = not rendered)."""
    f = lambda t: None if t is None else t.detach().cpu().float()
    g = per_gaussian(f(means3D), f(shs), f(colors_precomp), f(opacities), f(scales), f(rotations), f(cov3D_precomp), scale_modifier,
                     f(viewmatrix), f(projmatrix), f(campos), tanfovx, tanfovy, 0.0, W, H, degree)
    a, b, c = g["cov2"][:, 0] + 0.3, g["cov2"][:, 1], g["cov2"][:, 2] + 0.3
    det = a * c - b * b
    det_inv = 1.0 / det
    conic = torch.stack([c * det_inv, -b * det_inv, a * det_inv], 1)
    mid = 0.5 * (a + c)
    l1 = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    l2 = mid - torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(l1, l2)))
    valid = (g["depth"] > 0.2) & (det != 0)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    x0, y0, x1, y1 = rects(g["xy"], radius, gx, gy)
    valid = valid & ((x1 - x0) * (y1 - y0) != 0)
    radius = torch.where(valid, radius, torch.zeros_like(radius))
    return dict(valid=valid, xy=g["xy"].float(), conic=conic.float(), opacity=f(opacities).reshape(-1), rgb=g["rgb"].float(),
                depth=g["depth"].float(), radius=radius)


def rects(xy, radius, gx, gy):
    """getRect (auxiliary.h): tile rectangle [x0, x1) x [y0, y1), truncating divisions, clamped to the grid."""
    r = radius
    x0 = torch.clamp(torch.trunc((xy[:, 0] - r) / TILE), 0, gx).long()
    y0 = torch.clamp(torch.trunc((xy[:, 1] - r) / TILE), 0, gy).long()
    x1 = torch.clamp(torch.trunc((xy[:, 0] + r + TILE - 1) / TILE), 0, gx).long()
    y1 = torch.clamp(torch.trunc((xy[:, 1] + r + TILE - 1) / TILE), 0, gy).long()
    return x0, y0, x1, y1


def tile_lists(g, W, H, tiles=None):
    """{tile: Gaussian ids in blend order} for the tiles in `tiles` (default: all)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    x0, y0, x1, y1 = rects(g["xy"], g["radius"], gx, gy)
    ids = torch.nonzero(g["valid"]).reshape(-1)
    want = set(range(gx * gy)) if tiles is None else set(int(t) for t in tiles)
    lists = {t: [] for t in want}
    for i in ids.tolist():
        for ty in range(int(y0[i]), int(y1[i])):
            for tx in range(int(x0[i]), int(x1[i])):
                t = ty * gx + tx
                if t in lists:
                    lists[t].append(i)
    depth = g["depth"]
    for t, lst in lists.items():
        lst.sort(key=lambda i: (float(depth[i]), i))
    return lists


def count_blend(g, W, H, bg, tiles=None):
    """(count [P] int64, color [3,H,W] float32, pixels [H,W] bool that were rendered) of the count pass, restricted to `tiles`."""
    P = g["xy"].shape[0]
    gx = (W + TILE - 1) // TILE
    lists = tile_lists(g, W, H, tiles)
    order = sorted(lists)
    nt = len(order)
    L = max([len(lists[t]) for t in order] + [0])
    idx = torch.full((nt, max(L, 1)), -1, dtype=torch.long)
    for k, t in enumerate(order):
        if lists[t]:
            idx[k, :len(lists[t])] = torch.tensor(lists[t], dtype=torch.long)
    ty = torch.tensor([t // gx for t in order], dtype=torch.long)
    tx = torch.tensor([t % gx for t in order], dtype=torch.long)
    ly, lx = torch.meshgrid(torch.arange(TILE), torch.arange(TILE), indexing="ij")
    px = (tx[:, None] * TILE + lx.reshape(1, -1))          # [nt, 256]
    py = (ty[:, None] * TILE + ly.reshape(1, -1))
    inside = (px < W) & (py < H)
    pxf, pyf = px.float(), py.float()
    T = torch.ones(nt, TILE * TILE)
    C = torch.zeros(3, nt, TILE * TILE)
    done = ~inside
    count = torch.zeros(P, dtype=torch.long)
    xy, conic, op, rgb = g["xy"], g["conic"], g["opacity"], g["rgb"]
    thr = torch.tensor(1.0 / 255.0, dtype=torch.float32)
    for k in range(L):
        gid = idx[:, k]
        live = gid >= 0
        gi = torch.where(live, gid, torch.zeros_like(gid))
        dx = xy[gi, 0][:, None] - pxf
        dy = xy[gi, 1][:, None] - pyf
        cx, cy, cz = conic[gi, 0][:, None], conic[gi, 1][:, None], conic[gi, 2][:, None]
        power = -0.5 * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
        alpha = torch.clamp(op[gi][:, None] * torch.exp(power), max=0.99)
        cand = live[:, None] & ~done & ~(power > 0) & ~(alpha < thr)
        test_T = T * (1 - alpha)
        stop = cand & (test_T < 0.0001)
        blend = cand & ~stop
        done = done | stop
        for ch in range(3):
            C[ch] = torch.where(blend, C[ch] + rgb[gi, ch][:, None] * alpha * T, C[ch])
        T = torch.where(blend, test_T, T)
        count.index_add_(0, gi, blend.sum(1).long())
    color = bg.float().reshape(3, 1, 1).expand(3, H, W).clone()
    rendered = torch.zeros(H, W, dtype=torch.bool)
    out = C + T[None] * bg.float().reshape(3, 1, 1)
    m = inside.reshape(-1)
    color[:, py.reshape(-1)[m], px.reshape(-1)[m]] = out.reshape(3, -1)[:, m]
    rendered[py.reshape(-1)[m], px.reshape(-1)[m]] = True
    return count, color, rendered


def count_pass(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, scale_modifier, viewmatrix, projmatrix,
               campos, tanfovx, tanfovy, W, H, degree, bg, tiles=None):
    """(count, score = count x opacity, color, radii, per-Gaussian dict) of the count pass."""
    g = vanilla_preprocess(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, scale_modifier, viewmatrix,
                           projmatrix, campos, tanfovx, tanfovy, W, H, degree)
    count, color, _ = count_blend(g, W, H, bg.detach().cpu().float(), tiles)
    score = count.float() * g["opacity"]
    return count, score, color, g["radius"].int(), g


def calculate_v_imp_score(gaussians_scales, imp_list, v_pow):
    """prune.py:calculate_v_imp_score (LightGaussian): volume^v_pow of the 90 %-normalised box volume times the importance."""
    volume = torch.prod(gaussians_scales, dim=1)
    index = int(len(volume) * 0.9)
    sorted_volume, _ = torch.sort(volume, descending=True)
    kth_percent_largest = sorted_volume[index]
    v_list = torch.pow(volume / kth_percent_largest, v_pow)
    return v_list * imp_list


def prune_mask(v_list, percent):
    """scene/gaussian_model.py:prune_gaussians: the Gaussians whose score is at or below the value at position
    int(percent * (N - 1)) of the ascending sort."""
    sorted_tensor, _ = torch.sort(v_list, dim=0)
    index_nth_percentile = int(percent * (sorted_tensor.shape[0] - 1))
    value_nth_percentile = sorted_tensor[index_nth_percentile]
    return (v_list <= value_nth_percentile).squeeze(), value_nth_percentile


def closed_form_single(xy, conic, opacity, W, H):
    """Pixel centres (integer coordinates) where one splat alone is blended: power <= 0 and min(0.99, o exp(power)) >= 1/255."""
    py, px = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    dx, dy = np.float32(xy[0]) - px, np.float32(xy[1]) - py
    cx, cy, cz = (np.float32(v) for v in conic)
    power = np.float32(-0.5) * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
    alpha = np.minimum(np.float32(0.99), np.float32(opacity) * np.exp(power))
    return (~(power > 0)) & ~(alpha < np.float32(1.0 / 255.0))
