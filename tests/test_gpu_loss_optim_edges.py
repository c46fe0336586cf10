"""The refine-step kernels behind the rasterizer -- image losses (loss_ops.hip), L1, Adam and the activations (refine_ops.hip, and the
activation backward fused into geom_bwd.hip) -- at the shapes and values where they branch, against float64 restatements of the same
operations: oracle/torch_losses.py on float64 CPU tensors differentiated by autograd, torch.optim.Adam on float64 copies, torch
sigmoid / exp / F.normalize in float64.  Every element of every gradient is compared.  Bounds are the ones test_gpu_parity.py /
test_gpu_dropin.py hold the same kernels to, unless a tighter one is stated; the float64 references are built once per module.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from igs_amd.camera import Camera
from igs_amd.scenes import activate, cfg1_scene
from test_gpu_parity import dev, rel  # noqa: F401

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of float32


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _misaligned(t):
    """A copy of `t` on the GPU whose data pointer is 4 bytes past a 16-byte boundary (storage_offset 1): the kernels' scalar paths."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---- SSIM + L1 (ssim_stats_kernel / ssim_grad_kernel: 32 x 32 tiles, 42 x 42 halo, XCD bands, 64 atomic shards) ------------------
# below the 11 x 11 window, single rows / columns, the 31/32/33 tile edges, and two band-heavy frames: 1352 x 1014 (4 tile rows per
# XCD) and a 2160-row strip (9 tile rows per XCD, the last band 4 rows short).  (A full 2160 x 3840 frame would spend ~80 s in the
# float64 11 x 11 convolutions on the CPU; the band mapping depends on the number of tile ROWS, which the strip has.)
SSIM_SHAPES = [(1, 1), (1, 37), (37, 1), (5, 5), (10, 10), (11, 11), (12, 300), (31, 32), (32, 31), (32, 32), (33, 33), (64, 64),
               (65, 97), (1014, 1352), (2160, 200)]


@functools.lru_cache(maxsize=None)
def ssim_case(H, W, seed=0):
    """Seeded image pair and the float64 reference: (pred, gt, sum SSIM map, sum |pred - gt|, d mean SSIM / d pred, d mean L1 / d pred)."""
    from oracle.torch_losses import ssim_map
    g = torch.Generator().manual_seed(7919 * H + W + 104729 * seed)
    gt = torch.rand((3, H, W), generator=g)
    pred = (gt + 0.15 * torch.randn((3, H, W), generator=g)).clamp(0, 1.2)
    n = 3 * H * W
    x = pred.double().requires_grad_(True)
    m = ssim_map(x, gt.double())
    s_ssim = m.sum()
    (s_ssim / n).backward()
    xl = pred.double().requires_grad_(True)
    s_l1 = (xl - gt.double()).abs().sum()
    (s_l1 / n).backward()
    return pred, gt, float(s_ssim.detach()), float(s_l1.detach()), x.grad, xl.grad


def check_ssim_grad(a, b, what):
    """test_gpu_parity.py::test_fused_ssim_l1_loss_matches_torch_autograd's bars (fp32 separable blur against the 121-tap window;
    gradients are O(1/n)): max error below 2e-4 of the largest element, 99 % of the elements within 1e-3 (rel)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.isfinite(a).all(), what
    assert np.abs(a - b).max() <= 2e-4 * np.abs(b).max(), (what, np.abs(a - b).max(), np.abs(b).max())
    assert np.quantile(rel(a, b), 0.99) < 1e-3, (what, np.quantile(rel(a, b), 0.99))


@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_l1_loss_matches_float64(dev, shape):
    """igs_ssim_l1_loss_fwd_bwd: loss value, both shard sums and every gradient element for lambda in {0, 0.2, 1} and a weight != 1.
    lambda = 0 leaves the L1 term alone, whose gradient is sign(pred - gt) * (1 - lambda) w / n exactly."""
    from igs_amd.refine import L1SsimFused
    H, W = shape
    pred, gt, s_ssim, s_l1, g_ssim, g_l1 = ssim_case(H, W)
    n = 3 * H * W
    pred_d, gt_d = pred.to(dev), gt.to(dev)
    sign = torch.sign(pred - gt).numpy()
    for lam, w in ((0.0, 1.0), (0.2, 1.0), (1.0, 1.0), (0.2, 2.5), (0.0, 0.3)):
        f = L1SsimFused(dev, lam)
        grad = torch.full_like(pred_d, float("nan"))
        f(pred_d, gt_d, grad, weight=w)
        sums = f.sums.cpu().numpy().astype(np.float64)
        assert np.count_nonzero(sums[np.arange(2048) % 16 != 0]) == 0          # only every 16th float is a shard
        # shard sums as means: the value bar of test_gpu_parity.py (1e-5)
        assert abs(sums[:1024].sum() / n - s_ssim / n) < 1e-5, (lam, sums[:1024].sum() / n, s_ssim / n)
        assert abs(sums[1024:].sum() / n - s_l1 / n) < 1e-5, (lam, sums[1024:].sum() / n, s_l1 / n)
        want = w * ((1.0 - lam) * s_l1 / n + lam * (1.0 - s_ssim / n))
        got = f.value(n, weight=w)
        assert abs(got - want) < 1e-5 * max(1.0, abs(want)), (lam, w, got, want)
        a = grad.cpu().numpy()
        if lam == 0.0:
            c_l1 = np.float32(np.float32(w) / np.float32(n))
            np.testing.assert_array_equal(a, (sign * c_l1).astype(np.float32))
        else:
            check_ssim_grad(a, w * ((1.0 - lam) * g_l1.numpy() - lam * g_ssim.numpy()), (shape, lam, w))


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (11, 11), (33, 33), (65, 97), (1014, 1352)])
def test_ssim_mean_on_the_device_matches_float64(dev, shape):
    """igs_ssim_mean_fwd_bwd through igs_amd.losses.ssim (the reference's call shape): the mean finished on the device by workgroup 0 of
    the gradient launch, and d(1 - mean SSIM)/d pred, against float64 autograd (bars of test_drop_in_ssim_matches_the_reference_formula)."""
    from igs_amd.losses import ssim
    H, W = shape
    pred, gt, s_ssim, _, g_ssim, _ = ssim_case(H, W)
    x = pred.to(dev).requires_grad_(True)
    v = ssim(x, gt.to(dev).unsqueeze(0), size_average=False)
    assert v.shape == (1,)
    want = s_ssim / (3 * H * W)
    assert abs(float(v.detach()) - want) <= 1e-6 + 1e-5 * abs(want), (float(v.detach()), want)
    (1.0 - v).sum().backward()
    check_ssim_grad(x.grad.cpu().numpy(), -g_ssim.numpy(), shape)


def test_ssim_ground_truth_cache_fill_read_refill(dev):
    """GT_FILL -> GT_CACHED -> refill: fill with prediction A, read with another prediction B (= the uncached call on B), then a new
    ground truth refilled with valid = 0 (= the uncached call on the new pair), then read again; ragged shape, every element."""
    from igs_amd.refine import L1SsimFused
    H, W = 65, 97
    n = 3 * H * W
    A, gt1, *_ = ssim_case(H, W)
    # B: another prediction for the SAME ground truth, and its float64 reference
    g = torch.Generator().manual_seed(31337)
    B = (gt1 + 0.2 * torch.randn(gt1.shape, generator=g)).clamp(0, 1.2)
    from oracle.torch_losses import ssim_map
    xb = B.double().requires_grad_(True)
    sb = ssim_map(xb, gt1.double()).sum()
    (sb / n).backward()
    g_ssim_b = xb.grad.numpy()
    s_l1_b = float((B.double() - gt1.double()).abs().sum())
    gt2 = torch.rand(gt1.shape, generator=g)
    stats = torch.full((_lib().igs_ssim_gt_stats_bytes(W, H) // 4,), float("nan"), device=dev)     # every value must be written by the fill
    lam = 0.2
    f = L1SsimFused(dev, lam)

    def run(pred, gt, cache=None):
        grad = torch.full((3, H, W), float("nan"), device=dev)
        f(pred.to(dev), gt.to(dev), grad, 1.0, gt_stats=cache)
        return grad.cpu(), f.value(n)

    def same(x, y, what):
        # cached and inline statistics come from the same code in the same order: agreement far inside the float64 bars
        (ga, va), (gb, vb) = x, y
        assert torch.isfinite(ga).all(), what
        assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max()), (what, float((ga - gb).abs().max()))
        assert abs(va - vb) < 2e-6, (what, va, vb)

    ptr = stats.data_ptr()
    same(run(A, gt1, (ptr, 0)), run(A, gt1), "fill with A")
    assert torch.isfinite(stats).all()
    cached_b = run(B, gt1, (ptr, 1))
    same(cached_b, run(B, gt1), "read with B")
    want = (1 - lam) * s_l1_b / n + lam * (1.0 - float(sb) / n)
    assert abs(cached_b[1] - want) < 1e-5, (cached_b[1], want)
    check_ssim_grad(cached_b[0].numpy(), (1 - lam) * np.sign((B - gt1).numpy()) / n - lam * g_ssim_b, "cached B vs float64")
    # the ground truth changes: refill (valid = 0), then read
    same(run(B, gt2, (ptr, 0)), run(B, gt2), "refill with a new ground truth")
    same(run(A, gt2, (ptr, 1)), run(A, gt2), "read the refilled statistics")


# ---- depth-normal consistency (depth_normal_kernel: 14 x 14 tiles) ------------------------------------------------------------
DN_SHAPES = [(1, 1), (2, 2), (3, 3), (13, 13), (14, 14), (15, 15), (14, 29), (29, 14), (1014, 1352)]


def dn_camera(H, W):
    return Camera(torch.eye(4), 2 * math.atan(W / (2 * 55.0)), 2 * math.atan(H / (2 * 60.0)), (H, W))


def dn_inputs(H, W):
    """Smooth positive depth maps with regions of depth exactly 0: isolated pixels, one-pixel horizontal and vertical lines, and a
    silhouette (everything outside an ellipse) -- different ones for the two maps."""
    g = torch.Generator().manual_seed(1000 * H + W)
    yy, xx = torch.meshgrid(torch.arange(H).double(), torch.arange(W).double(), indexing="ij")
    base = 3.0 + 0.01 * xx + 0.02 * yy + 0.3 * torch.sin(xx / 7.0) * torch.cos(yy / 5.0)
    depth = base + 0.02 * torch.randn(H, W, generator=g, dtype=torch.float64)
    mdepth = base * 1.03 + 0.02 * torch.randn(H, W, generator=g, dtype=torch.float64)
    iso = torch.rand(H, W, generator=g) < 0.03
    depth[iso] = 0.0
    depth[H // 2, :] = 0.0                                    # horizontal line
    depth[:, W // 3] = 0.0                                    # vertical line
    outside = ((yy - H / 2.0) / max(H / 2.5, 1.0)) ** 2 + ((xx - W / 2.0) / max(W / 2.5, 1.0)) ** 2 > 1.0
    mdepth[outside] = 0.0                                     # silhouette
    mdepth[:, (2 * W) // 3] = 0.0
    mdepth[torch.rand(H, W, generator=g) < 0.02] = 0.0
    normal = F.normalize(torch.randn(3, H, W, generator=g, dtype=torch.float64), dim=0)
    return depth.float(), mdepth.float(), normal.float()


def dn_geometry(cam, depth64):
    """Per interior pixel of the float64 restatement: clamped (|a x b| <= 1e-12, F.normalize's eps) and the norms |a|, |b|, |a x b|
    of the two difference vectors and their cross product."""
    from oracle.torch_losses import backproject
    P = backproject(cam, depth64[None])
    a = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    b = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    c = torch.linalg.cross(a, b, dim=0)
    deg = torch.zeros(depth64.shape, dtype=torch.bool)
    an, bn, cn, sa, sb = (torch.zeros(depth64.shape, dtype=torch.float64) for _ in range(5))
    if c.numel():
        cn[1:-1, 1:-1] = c.norm(dim=0)
        deg[1:-1, 1:-1] = cn[1:-1, 1:-1] <= 1e-12
        an[1:-1, 1:-1] = a.norm(dim=0)
        bn[1:-1, 1:-1] = b.norm(dim=0)
        d = depth64.abs()
        sa[1:-1, 1:-1] = d[2:, 1:-1] + d[:-2, 1:-1]              # the sizes a and b are differences of
        sb[1:-1, 1:-1] = d[1:-1, 2:] + d[1:-1, :-2]
    return deg, an, bn, cn, sa, sb


def _shift(t, dy, dx):
    """out[y, x] = t[y - dy, x - dx] (zero outside)."""
    H, W = t.shape
    out = torch.zeros_like(t)
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    if H - abs(dy) > 0 and W - abs(dx) > 0:
        out[yd, xd] = t[ys, xs]
    return out


@functools.lru_cache(maxsize=None)
def dn_reference(H, W, ratio):
    from oracle.torch_losses import depth_normal_loss
    cam = dn_camera(H, W)
    d, m, nrm = dn_inputs(H, W)
    dd, mm, nn = (t.double().requires_grad_(True) for t in (d[None], m[None], nrm))
    loss = depth_normal_loss(dict(depth_pred=dd, mdepth=mm, normal=nn), cam, depth_ratio=ratio)
    loss.backward()
    # what every interior pixel p feeds the depth gradients of its neighbours: |b| |e| to p -+ row, |a| |e| to p -+ col, with
    # |e| <= |s q| / max(|a x b|, eps); float32 rounds a and b to ~1e-7 of the depths they are differences of (cond: that size over
    # |a|, |b|) and 1 / |a x b| amplifies it by kappa = |a| |b| / |a x b| (kappa = 1 in the clamped branch, which divides by eps)
    scale = []
    for k, (dm, s) in enumerate(((d, (1 - ratio) / (H * W)), (m, ratio / (H * W)))):
        deg, an, bn, cn, sa, sb = dn_geometry(cam, dm.double())
        kappa = torch.where(deg, torch.ones_like(cn), an * bn / cn.clamp_min(1e-300)).clamp_min(1.0)
        rmax = math.sqrt(1.0 + cam.tanfovx ** 2 + cam.tanfovy ** 2)
        cond = (torch.where(an > 0, rmax * sa / an.clamp_min(1e-300), torch.ones_like(an)).clamp_min(1.0)
                + torch.where(bn > 0, rmax * sb / bn.clamp_min(1e-300), torch.ones_like(bn)).clamp_min(1.0))
        e = abs(s) * nrm.double().norm(dim=0) / cn.clamp_min(1e-12) * kappa * cond
        e[0, :] = 0; e[-1, :] = 0; e[:, 0] = 0; e[:, -1] = 0
        fb, fa = e * bn, e * an
        feed = _shift(fb, 1, 0) + _shift(fb, -1, 0) + _shift(fa, 0, 1) + _shift(fa, 0, -1)
        scale.append((int(deg.sum()), feed))
    return cam, (d, m, nrm), float(loss.detach()), (dd.grad[0], mm.grad[0], nn.grad), scale


@pytest.mark.parametrize("shape", DN_SHAPES)
def test_depth_normal_matches_float64_with_zero_depth_regions(dev, shape):
    """igs_depth_normal_loss_fwd_bwd on depth maps with regions of depth 0 (the normalisation's clamped branch, |cross| <= 1e-12: the
    reference divides by eps and its gradient there is h / eps, no projection) against float64 autograd through oracle/torch_losses.py:
    value, g_depth, g_mdepth and g_normal per element, depth_ratio in {0, 0.6, 1}.
    Bound per depth-gradient element: 1e-5 of what its four neighbours feed it (dn_reference: fp32 rounding is ~1e-7 of a term, times
    the cancellation in the difference vectors and the conditioning of 1 / |a x b|), never looser than the existing test's 2e-4 of the largest element.  The clamped terms reach
    1e12 s |q| |b|: a kernel that drops them misses all of each."""
    H, W = shape
    L = _lib()
    for ratio in (0.0, 0.6, 1.0):
        cam, (d, m, nrm), want, grads_ref, scale = dn_reference(H, W, ratio)
        if H >= 3 and W >= 3:
            assert scale[0][0] > 0 and scale[1][0] > 0, ("the clamped branch must be reached", scale[0][0], scale[1][0])
        dd, md, nd = d.to(dev), m.to(dev), nrm.to(dev)
        gd, gm, gn = (torch.full_like(t, float("nan")) for t in (dd, md, nd))
        shards = torch.full((1024,), float("nan"), device=dev)
        rc = L.igs_depth_normal_loss_fwd_bwd(_stream(dev), W, H, cam.tanfovx, cam.tanfovy, dd.data_ptr(), md.data_ptr(), nd.data_ptr(), 1.0,
                                             ratio, gd.data_ptr(), gm.data_ptr(), gn.data_ptr(), shards.data_ptr())
        assert rc == 0
        val = float(shards[::16].double().sum())
        assert abs(val - want) < 1e-5 * max(1.0, abs(want)), (ratio, val, want)
        cx = ((torch.arange(W).double() + 0.5 - W / 2.0) * (2 * cam.tanfovx / W))
        cy = ((torch.arange(H).double() + 0.5 - H / 2.0) * (2 * cam.tanfovy / H))
        ray = torch.sqrt(cx[None, :] ** 2 + cy[:, None] ** 2 + 1.0)
        for k, (name, a) in enumerate((("depth", gd), ("mdepth", gm))):
            b = grads_ref[k].numpy()
            a = a.cpu().double().numpy()
            feed = (ray * scale[k][1]).numpy()
            err = np.abs(a - b)
            bound = np.minimum(1e-5 * feed, 2e-4 * np.abs(b).max()) + 1e-12
            assert np.isfinite(a).all() and (err <= bound).all(), (name, ratio, float((err / bound).max()), int((err > bound).sum()))
        b = grads_ref[2].numpy()
        a = gn.cpu().double().numpy()
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 2e-4 * np.abs(b).max() + 1e-9, ("normal", ratio, np.abs(a - b).max())
        assert float(gn[:, 0, :].abs().max()) == 0.0                                   # border pixels: n = 0


# ---- SSIM gradient + depth-normal in ONE launch (ssim_grad_dn_kernel, Bresenham interleave of the two workgroup kinds) -------------
def _groups(H, W):
    band = lambda gx, gy, planes: planes * ((gy + 7) // 8) * gx        # band_grid / 8 (loss_ops.hip)
    return band((W + 31) // 32, (H + 31) // 32, 3), band((W + 13) // 14, (H + 13) // 14, 1)


# SSIM groups : depth-normal groups = 3 : 1 (everything below 15 x 15), 3 : 2, 2 : 1, 1 : 2 (113 x 29: two dn bands per XCD), full size
FUSED_SHAPES = [(13, 13), (15, 15), (27, 41), (113, 29), (1014, 1352)]


@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_fused_ssim_and_depth_normal_launch_at_lopsided_shapes(dev, shape):
    """igs_refine_step with L1 + D-SSIM and lambda_depth_normal > 0 (the SSIM gradient and the depth-normal pass share one launch),
    gradients only, against the autograd step whose losses are the two separate kernels (igs_amd.losses.ssim,
    igs_amd.losses.depth_normal_loss) -- the bars of test_fused_step_with_depth_normal_regulariser."""
    from igs_amd.refine import GaussianParams, Refiner, render
    from igs_amd.scenes import perturbed_copy
    H, W = shape
    ns, nd = _groups(H, W)
    assert {(13, 13): (3, 1), (15, 15): (3, 2), (27, 41): (6, 3), (113, 29): (3, 6)}.get(shape, (ns, nd)) == (ns, nd)
    raw, _, bg = cfg1_scene(P=3000, size=64)
    c2w = torch.eye(4); c2w[2, 3] = -5.0
    cam = Camera.from_c2w(c2w, (math.radians(55.0), 2 * math.atan(math.tan(math.radians(27.5)) * H / W)), (H, W)).to(dev)
    bg = bg.to(dev)
    gt_raw = {k: v.to(dev) for k, v in perturbed_copy(raw, sigma=0.03).items()}
    with torch.no_grad():
        gts = [render(activate(gt_raw), cam, bg)["images_pred"].clone()]
    assert gts[0].shape == (3, H, W)
    pa, pb = GaussianParams(raw, dev), GaussianParams(raw, dev)
    ra = Refiner(pa, [cam], gts, bg, loss="l1_ssim", lambda_depth_normal=0.05, fused=True)
    rb = Refiner(pb, [cam], gts, bg, loss="l1_ssim", lambda_depth_normal=0.05, native=False)
    ra.adam_fn = lambda: None
    rb.adam_fn = lambda: None
    pka = ra.step(view=0); rb.step(view=0)
    from igs_amd.losses import depth_normal_loss, l1_loss, ssim
    with torch.no_grad():                                         # the autograd step's loss from the separate kernels
        pk = render(pb.activated(), cam, bg)
        img = pk["images_pred"]
        lb = float(0.8 * l1_loss(img, gts[0]) + 0.2 * (1.0 - ssim(img, gts[0].unsqueeze(0), size_average=False)[0])
                   + 0.05 * depth_normal_loss(pk, cam))
    assert abs(float(pka["loss"].item()) - lb) < 2e-5, (float(pka["loss"].item()), lb)
    nonzero = 0
    for k in pa.leaves:
        A, B = pa.leaves[k].grad.cpu().numpy(), pb.leaves[k].grad.cpu().numpy()
        assert np.isfinite(A).all(), k
        nonzero += int(np.count_nonzero(B))
        r = rel(A, B)
        assert np.quantile(r, 0.99) < 5e-3 and np.median(r) < 1e-4, (shape, k, np.quantile(r, 0.99), np.median(r))
    assert nonzero > 0


# ---- L1 (l1_mean_kernel: two-level "who finishes last" counter, 1024-workgroup cap; l1_kernel: 64 shards) ----------------------------
L1_SIZES = [1, 3, 131077, 3 * 1352 * 1014, 17000001]


@functools.lru_cache(maxsize=None)
def l1_case(n):
    g = torch.Generator().manual_seed(n)
    pred = torch.randn(n, generator=g)
    gt = torch.randn(n, generator=g)
    if n > 2:
        gt[::7] = pred[::7]                                    # d = 0: sign 0, gradient 0
    d = pred.double() - gt.double()
    return pred, gt, float(d.abs().sum()), torch.sign(pred - gt)


def l1_mean_bound(n, mean_abs):
    """Worst-case float32 error of l1_mean_kernel's sum (serial per thread: ceil(n / (256 * grid)) terms; 6 shuffle levels; 4 waves;
    the last workgroup: its lanes' ceil(grid / 256) partials, 6 levels, 4 waves), the difference rounding and the final scale, in
    units of the mean of |d|."""
    grid = min(max((n // 4 + 1023) // 1024, 1), 1024)
    k = -(-n // (256 * grid)) + 6 + 3 + -(-grid // 256) + 6 + 3 + 2
    return k * U32 * mean_abs


def check_l1_mean(v, grad, n):
    pred, gt, s, sign = l1_case(n)
    want = s / n
    assert abs(float(v) - want) <= l1_mean_bound(n, want), (n, float(v), want)
    inv_n = np.float32(1.0 / n)                                 # the kernel's (float)(1.0 / (double)n)
    assert torch.equal(grad.cpu(), sign * torch.tensor(inv_n)), n


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_mean_matches_float64(dev, n):
    """igs_l1_mean_fwd_bwd through igs_amd.losses.l1_loss: the mean within float32 rounding of the float64 mean, the gradient exactly
    sign(d) / n.  131077: 33 workgroups (two counter groups, the second of size 1); 17 000 001: the 1024-workgroup cap, several trips."""
    from igs_amd.losses import l1_loss
    pred, gt, _, _ = l1_case(n)
    x = pred.to(dev).requires_grad_(True)
    v = l1_loss(x, gt.to(dev))
    v.backward()
    check_l1_mean(v, x.grad, n)


def test_l1_mean_scalar_path_and_back_to_back_sizes(dev):
    """Views at storage_offset 1 (not 16-byte aligned: the scalar loop) through the C ABI, and calls of different n back to back on one
    stream sharing one partials / counter buffer: the counters must reset themselves after every call."""
    from igs_amd.losses import l1_loss
    L = _lib()
    scratch = torch.zeros(1024 + 33 * 64, dtype=torch.float32, device=dev)
    for n in (3, 131077, 3 * 1352 * 1014):
        pred, gt, _, _ = l1_case(n)
        a, b = _misaligned(pred.to(dev)), _misaligned(gt.to(dev))
        grad = _misaligned(torch.full((n,), float("nan"), device=dev))
        out = torch.full((1,), float("nan"), device=dev)
        assert L.igs_l1_mean_fwd_bwd(_stream(dev), n, a.data_ptr(), b.data_ptr(), grad.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                     scratch.data_ptr() + 4096) == 0
        check_l1_mean(out[0], grad, n)
        x = _misaligned(pred.to(dev)).requires_grad_(True)
        v = l1_loss(x, gt.to(dev))
        v.backward()
        check_l1_mean(v, x.grad, n)
    assert int(scratch[1024:].view(torch.int32).abs().sum()) == 0              # every counter word back at zero
    # back to back on one stream, no synchronisation in between: large, small, middle, large, one element
    outs = []
    for n in (17000001, 3, 131077, 17000001, 1, 3 * 1352 * 1014):
        pred, gt, _, _ = l1_case(n)
        x = pred.to(dev).requires_grad_(True)
        v = l1_loss(x, gt.to(dev))
        v.backward()
        outs.append((n, v, x.grad))
    for n, v, gr in outs:
        check_l1_mean(v, gr, n)
    assert L.igs_l1_mean_fwd_bwd(_stream(dev), 0, 0, 0, 0, 0, 0, 0) != 0                 # n = 0: refused by validation


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1_loss_shards_match_float64(dev, n):
    """igs_l1_loss_fwd_bwd (64 shards; grid cap 2048 with trips; scalar tail): sum within float32 rounding, gradient exactly sign * scale,
    aligned and at storage_offset 1."""
    L = _lib()
    pred, gt, s, sign = l1_case(n)
    scale = np.float32(0.37 / n)
    for misaligned in (False, True):
        a, b = pred.to(dev), gt.to(dev)
        grad = torch.full((n,), float("nan"), device=dev)
        if misaligned:
            a, b, grad = _misaligned(a), _misaligned(b), _misaligned(grad)
        sums = torch.zeros(1024, device=dev)
        assert L.igs_l1_loss_fwd_bwd(_stream(dev), n, a.data_ptr(), b.data_ptr(), grad.data_ptr(), sums.data_ptr(), float(scale)) == 0
        sm = sums.cpu().double().numpy()
        assert np.count_nonzero(sm[np.arange(1024) % 16 != 0]) == 0
        grid = min(max((n // 4 + 255) // 256, 1), 2048)
        k = -(-n // (256 * grid)) + 6 + 3 + -(-grid // 64) + 6 + 2        # serial, shuffles, waves, atomics per shard, shard sum
        assert abs(sm.sum() - s) <= k * U32 * s, (n, misaligned, sm.sum(), s)
        assert torch.equal(grad.cpu(), sign * torch.tensor(scale)), (n, misaligned)


# ---- Adam (adam_kernel, adam_groups_kernel, adam_multi_kernel<DEV_STEP>) against float64 torch.optim.Adam -----------------------------
BETAS, EPS = (0.9, 0.999), 1e-15
STEPS = 5


def adam_grads(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(STEPS):
        step = []
        for sh in shapes:
            t = torch.randn(sh, generator=g) * 0.1
            if t.numel() > 2:
                t.view(-1)[::97] = 0.0                          # m = v = 0 on the first step: 0 / (0 + eps)
            step.append(t)
        out.append(step)
    return out


def reference_adam(init, lrs, grads):
    """torch.optim.Adam on float64 CPU copies; one parameter group per tensor."""
    ps = [torch.nn.Parameter(t.double().clone()) for t in init]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, betas=BETAS, eps=EPS)
    for step in grads:
        for p, gr in zip(ps, step):
            p.grad = gr.double().clone()
        opt.step()
    return ps, opt


# check_adam's bars as (rtol, atol factor): the atol factor multiplies lr for the parameter and the largest |reference| entry for a moment
# (tests/exchange_restatement.py::adam_allowance reads them from here)
ADAM_BARS = dict(param=(2e-6, 2e-4), exp_avg=(2e-5, 2e-6), exp_avg_sq=(2e-5, 1e-6))


def check_adam(p, m, v, ref_p, ref_st, lr, what):
    """test_gpu_dropin.py::test_multi_tensor_adam_matches_torch_adam's bars (a step moves a parameter by ~lr)."""
    p, m, v = (t.detach().cpu().double() for t in (p, m, v))
    bp, bm, bv = ADAM_BARS["param"], ADAM_BARS["exp_avg"], ADAM_BARS["exp_avg_sq"]
    torch.testing.assert_close(p, ref_p.detach(), rtol=bp[0], atol=bp[1] * lr, msg=lambda s: "%s param: %s" % (what, s))
    if m.numel():
        torch.testing.assert_close(m, ref_st["exp_avg"], rtol=bm[0], atol=bm[1] * float(ref_st["exp_avg"].abs().max()),
                                   msg=lambda s: "%s exp_avg: %s" % (what, s))
        torch.testing.assert_close(v, ref_st["exp_avg_sq"], rtol=bv[0], atol=bv[1] * float(ref_st["exp_avg_sq"].abs().max()),
                                   msg=lambda s: "%s exp_avg_sq: %s" % (what, s))


@pytest.mark.parametrize("n", [1, 3, 5, (1 << 21) + 3])
@pytest.mark.parametrize("misaligned", [False, True])
def test_adam_step_matches_float64_torch_adam(dev, n, misaligned):
    """igs_adam_step (one tensor, host-side bias corrections): float4 body + scalar tail, the 2048-workgroup cap with a second trip at
    2^21 + 3, and the scalar path for buffers at storage_offset 1; five steps."""
    L = _lib()
    lr = 1e-2
    gen = torch.Generator().manual_seed(n)
    init = torch.randn(n, generator=gen)
    grads = adam_grads([(n,)], n)
    mk = _misaligned if misaligned else (lambda t: t.clone())
    p, m, v = mk(init.to(dev)), mk(torch.zeros(n, device=dev)), mk(torch.zeros(n, device=dev))
    gbuf = mk(torch.zeros(n, device=dev))
    for t, step in enumerate(grads, 1):
        gbuf.copy_(step[0].to(dev))
        assert L.igs_adam_step(_stream(dev), n, p.data_ptr(), gbuf.data_ptr(), m.data_ptr(), v.data_ptr(), lr, BETAS[0], BETAS[1], EPS,
                               1.0 - BETAS[0] ** t, math.sqrt(1.0 - BETAS[1] ** t)) == 0
    ps, opt = reference_adam([init], [lr], grads)
    st = opt.state[ps[0]]
    assert int(st["step"]) == STEPS
    check_adam(p, m, v, ps[0], st, lr, (n, misaligned))


def test_adam_groups_ragged_offsets_match_float64(dev):
    """igs_adam_step_groups: 8 groups at offsets that are no multiples of 4 (the scalar path per group), one empty, one past the
    1024-workgroup cap, per-group learning rates; the floats between the groups stay untouched."""
    L = _lib()
    counts = [5, 0, 1024 * 256 * 4 + 5, 7, 130, 1, 3, 999]
    lrs = [1e-2, 5e-2, 1.6e-3, 2.5e-3, 1e-3, 3e-2, 7e-3, 4e-3]
    offs, o = [], 1
    for c in counts:
        if o % 4 == 0:
            o += 1
        offs.append(o)
        o += c + 2                                              # two untouched floats between groups
    assert all(x % 4 != 0 for x in offs)
    total = o
    gen = torch.Generator().manual_seed(11)
    init_flat = torch.randn(total, generator=gen)
    grads = adam_grads([(c,) for c in counts], 11)
    p = init_flat.to(dev)
    m, v, gbuf = torch.zeros(total, device=dev), torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    off_t = np.array(offs, np.uint64); cnt_t = np.array(counts, np.uint64); lr_t = np.array(lrs, np.float32)
    for t, step in enumerate(grads, 1):
        for o_, c, gr in zip(offs, counts, step):
            gbuf[o_:o_ + c] = gr.to(dev)
        assert L.igs_adam_step_groups(_stream(dev), 8, off_t.ctypes.data, cnt_t.ctypes.data, lr_t.ctypes.data, p.data_ptr(), gbuf.data_ptr(),
                                      m.data_ptr(), v.data_ptr(), BETAS[0], BETAS[1], EPS, 1.0 - BETAS[0] ** t, math.sqrt(1.0 - BETAS[1] ** t)) == 0
        torch.cuda.synchronize(dev)                             # (the host arrays live on this frame)
    ps, opt = reference_adam([init_flat[o_:o_ + c] for o_, c in zip(offs, counts)], [float(x) for x in lr_t], grads)
    touched = torch.zeros(total, dtype=torch.bool)
    for k, (o_, c) in enumerate(zip(offs, counts)):
        touched[o_:o_ + c] = True
        check_adam(p[o_:o_ + c], m[o_:o_ + c], v[o_:o_ + c], ps[k], opt.state[ps[k]], float(lr_t[k]), ("group", k))
    pc = p.cpu()
    assert torch.equal(pc[~touched], init_flat[~touched]) and float(m.cpu()[~touched].abs().max()) == 0.0
    assert L.igs_adam_step_groups(_stream(dev), 9, off_t.ctypes.data, cnt_t.ctypes.data, lr_t.ctypes.data, p.data_ptr(), gbuf.data_ptr(),
                                  m.data_ptr(), v.data_ptr(), BETAS[0], BETAS[1], EPS, 1.0, 1.0) != 0            # > 8 groups: refused


@pytest.mark.parametrize("capturable", [False, True])
def test_optim_adam_eleven_tensors_matches_float64(dev, capturable):
    """igs_amd.optim.Adam over 11 tensors (two launches of <= 8; with capturable=True they share one `done` scratch and each advances
    its own device-side step counts): one zero-size tensor, one misaligned view (scalar path), one larger than 1024 * 256 * 4
    elements (the workgroup cap).  Five steps against float64 torch.optim.Adam: parameters, both moments, step counts."""
    from igs_amd.optim import Adam
    shapes = [(1000, 3), (0,), (1000, 4), (1024 * 256 * 4 + 11,), (7,), (1000, 16, 3), (1,), (1000, 1), (333,), (3,), (64, 5)]
    lrs = [1.6e-3, 1e-2, 1e-2, 2.5e-3, 5e-2, 2.5e-3, 1e-3, 5e-2, 5e-3, 3e-2, 7e-3]
    view_at = 8                                                  # this one is a view at storage_offset 1
    gen = torch.Generator().manual_seed(21)
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = adam_grads(shapes, 22)
    ps = []
    for i, t in enumerate(init):
        ps.append(torch.nn.Parameter(_misaligned(t.to(dev)) if i == view_at else t.to(dev).clone()))
    assert ps[view_at].data_ptr() % 16 == 4 and ps[1].numel() == 0
    opt = Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, betas=BETAS, eps=EPS, capturable=capturable)
    for step in grads:
        for i, (p, gr) in enumerate(zip(ps, step)):
            p.grad = _misaligned(gr.to(dev)) if i == view_at else gr.to(dev)
        opt.step()
    torch.cuda.synchronize(dev)
    rp, ropt = reference_adam(init, lrs, grads)
    for i, (p, q) in enumerate(zip(ps, rp)):
        st, rst = opt.state[p], ropt.state[q]
        assert float(st["step"]) == float(rst["step"]) == STEPS, (i, st["step"])
        if capturable:
            assert torch.is_tensor(st["step"]) and st["step"].is_cuda
        check_adam(p, st["exp_avg"], st["exp_avg_sq"], q, rst, lrs[i], ("tensor", i, capturable))


# ---- activations (activate_fwd / activate_bwd, and the copy fused into geom_bwd.hip) ----------------------------------------------
def edge_activation_inputs(P=300, seed=8):
    """Saturated logits, log-scales on both sides of exp's float32 overflow (ln FLT_MAX = 88.7228), quaternions of norm 0, below
    F.normalize's eps (1e-13, 5e-13, 9e-13) and above it (1e-11), and ordinary values; upstream gradients chosen so that
    d_scale * scale lands clearly inside or outside float32's range."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(P, 1, generator=g) * 2
    ls = torch.randn(P, 3, generator=g) - 3
    rt = torch.randn(P, 4, generator=g)
    d_lo, d_ls, d_rt = torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g)
    logits = [20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 17.0, -17.0]
    lo[:len(logits), 0] = torch.tensor(logits)
    ls[0] = torch.tensor([88.0, 88.7, -88.0]); d_ls[0] = torch.tensor([0.5, 0.5, 1.0])        # finite: 1.66e38 * 0.5 ...
    ls[1] = torch.tensor([88.7, 88.75, 89.0]); d_ls[1] = torch.tensor([2.0, 1.0, -1.0])       # d_scale * scale = inf, inf, -inf
    ls[2] = torch.tensor([100.0, -100.0, 88.72]); d_ls[2] = torch.tensor([-0.25, 3.0, 0.5])
    d = F.normalize(torch.randn(16, 4, generator=g), dim=1)
    norms = [0.0, 1e-13, 5e-13, 9e-13, 1e-11, 3e-11, 1e-13, 5e-13, 0.0, 9e-13, 1e-11, 2e-13, 6e-13, 4e-13, 1e-13, 8e-13]
    rt[:16] = d * torch.tensor(norms)[:, None]
    rt[16] = torch.tensor([3e-13, -2e-13, 1e-13, 0.0])
    return lo, ls, rt, (d_lo, d_ls, d_rt)


def assert_close_with_infs(a, b, rtol, atol, what):
    """b: float64 reference rounded to float32 (overflow -> inf, as float32 arithmetic gives it): the same infinities, finite elsewhere."""
    b32 = b.float()
    inf = torch.isinf(b32)
    assert torch.equal(torch.isinf(a), inf) and torch.equal(a[inf], b32[inf]), (what, a[inf], b32[inf])
    assert not torch.isnan(a).any(), what
    torch.testing.assert_close(a[~inf].double(), b[~inf], rtol=rtol, atol=atol, msg=lambda s: "%s: %s" % (what, s))


def test_activations_at_their_edges_match_float64(dev):
    """igs_amd.activations.activate forward and backward against float64 sigmoid / exp / F.normalize and their autograd, at the bars of
    test_fused_activations_match_torch.  Below eps the reference's gradient of F.normalize is g / eps (the clamp passes none)."""
    from igs_amd.activations import activate
    lo, ls, rt, (d_lo, d_ls, d_rt) = edge_activation_inputs()
    assert int((torch.exp(ls.double()).float().isinf()).sum()) == 3
    x = [t.to(dev).requires_grad_(True) for t in (lo, ls, rt)]
    y = [t.double().requires_grad_(True) for t in (lo, ls, rt)]
    ox = activate(*x)
    oy = (torch.sigmoid(y[0]), torch.exp(y[1]), F.normalize(y[2]))
    for name, a, b in zip(("opacity", "scale", "rotation"), ox, oy):
        assert_close_with_infs(a.detach().cpu(), b.detach(), 2e-6, 1e-7, name)
    sum((o * w.to(dev)).sum() for o, w in zip(ox, (d_lo, d_ls, d_rt))).backward()
    sum((o * w.double()).sum() for o, w in zip(oy, (d_lo, d_ls, d_rt))).backward()
    for name, a, b in zip(("logit", "log_scale", "rotation"), x, y):
        assert_close_with_infs(a.grad.cpu(), b.grad, 2e-5, 1e-6, name + " grad")
    # the clamped quaternions: the reference's gradient is d_rot / eps exactly
    small = rt.double().norm(dim=1) < 1e-12
    assert int(small.sum()) >= 10
    torch.testing.assert_close(x[2].grad.cpu()[small].double(), d_rt.double()[small] * 1e12, rtol=2e-5, atol=0)


def test_fused_step_activation_backward_below_eps_equals_unfused(dev):
    """The activation backward fused into igs_refine_step (geom_bwd.hip) against the unfused native step (igs_activate_bwd, pinned to
    float64 above), gradients only, with quaternions of norm 0 and below F.normalize's eps among ordinary ones and saturated logits
    (the bars of test_fused_gradient_only_step_equals_unfused_native_step, the clamped rows held to them separately)."""
    from igs_amd.refine import GaussianParams, Refiner, render
    from igs_amd.scenes import perturbed_copy
    raw, cams, bg = cfg1_scene(P=3000, size=128)
    cams = [cams[0].to(dev)]
    bg = bg.to(dev)
    gt_raw = {k: v.to(dev) for k, v in perturbed_copy(raw, sigma=0.03).items()}
    with torch.no_grad():
        gts = [render(activate(gt_raw), cams[0], bg)["images_pred"].clone()]
    raw = {k: v.clone() for k, v in raw.items()}
    g = torch.Generator().manual_seed(77)
    tiny = torch.arange(0, 3000, 7)
    norms = torch.tensor([0.0, 1e-13, 5e-13, 9e-13])[torch.arange(len(tiny)) % 4]
    raw["rotation"][tiny] = F.normalize(torch.randn(len(tiny), 4, generator=g), dim=1) * norms[:, None]
    raw["opacity"][1::50, 0] = 20.0
    raw["opacity"][2::50, 0] = -20.0
    for loss in ("l1", "l1_ssim"):
        pa, pb = GaussianParams(raw, dev), GaussianParams(raw, dev)
        ra = Refiner(pa, cams, gts, bg, loss=loss, native=True, fused=True)
        rb = Refiner(pb, cams, gts, bg, loss=loss, native=True, fused=False)
        ra.adam_fn = lambda: None
        rb.adam_fn = lambda: None
        ra.step(view=0); rb.step(view=0)
        mask = torch.zeros(3000, dtype=torch.bool)
        mask[tiny] = True
        for k in pa.leaves:
            A, B = pa.leaves[k].grad.cpu(), pb.leaves[k].grad.cpu()
            assert torch.isfinite(A).all(), (loss, k)
            rows = [torch.ones(3000, dtype=torch.bool)] if k != "rotation" else [~mask, mask]
            for sel in rows:
                a, b = A[sel].numpy(), B[sel].numpy()
                r = rel(a, b)
                assert np.quantile(r, 0.999) < 2e-3 and np.median(r) < 1e-5, (loss, k, np.quantile(r, 0.999), np.median(r))
        Bt = pb.leaves["rotation"].grad.cpu()[mask]
        seen = (Bt.abs().sum(dim=1) > 0) & (pb.leaves["rotation"].detach().cpu()[mask].norm(dim=1) > 0)
        assert int(seen.sum()) >= 20, int(seen.sum())                  # clamped, non-zero quaternions that receive a gradient
        assert float(Bt.abs().max()) > 1e6 * float(pb.leaves["rotation"].grad.cpu()[~mask].abs().max())       # (g / eps against g / |q|)
