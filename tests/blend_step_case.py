"""Hand-placed scenes for the fused blend kernel (igs_amd/csrc/blend_step.hip) on a 40 x 24 image: 3 x 2 tiles, the right column
(x = 32..39) and the bottom row (y = 16..23) partial.  Shared by tests/test_gpu_blend_step_tiles.py (which also runs this file as a
child process: the library reads IGS_NO_TILE_FUSION once per process) and tests/test_blend_step_isa.py (which checks the layouts on
the CPU oracle).

A pinhole camera at the origin looks down +z with focal 40 px, so a point (x, y, z) lands on pixel 40 x / z + 19.5, 40 y / z + 11.5.
"Small" Gaussians are 0.7 .. 1 px wide on screen (radius 3 px) with centres at least 3 px inside their tile: each is an instance of
exactly one tile, and the tile's instance count is how many were put there.  Their opacities are 0.02 .. 0.08, so no pixel saturates
and the lists are walked to their ends.

  counts_a   tiles hold   64, 129,  65 | 128,   0,   1      (tile order: row 0 left to right, then row 1)
  counts_b   tiles hold  193,  65, 192 | 129, 260,  64
  saturate   40 opaque Gaussians of sigma = 15 px about the image centre in front of / between 0, 30, 100 | 150, 170, 230 small ones:
             every pixel of every tile is finished (T < 1e-4) well before its list ends -- lists of 40 .. 270 instances, the forward's
             early exit in one round and its break-off in front of a second one, a backward that starts far from the list's end

The forward stages 192 instances a round, the colour-only backward 128: the counts sit on both sides of 64, 128 and 192 -- forward at
one and two rounds, backward at one, two and three, its 64-splat words full, one over and empty.  P is padded to a multiple of four
with Gaussians far outside the image.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, FOCAL = 40, 24, 40.0
STEPS = 3
# pixel ranges (centres of the small Gaussians) per tile column / row
XR = [(4.0, 11.0), (20.0, 27.0), (35.0, 36.5)]
YR = [(4.0, 11.0), (19.0, 20.5)]
LAYOUTS = {
    "counts_a": dict(small=[64, 129, 65, 128, 0, 1], big=0, bg=(0.0, 0.0, 0.0)),
    "counts_b": dict(small=[193, 65, 192, 129, 260, 64], big=0, bg=(0.2, 0.5, 0.8)),
    "saturate": dict(small=[0, 30, 100, 150, 170, 230], big=40, bg=(0.3, 0.1, 0.6)),
}


def camera():
    from igs_amd.camera import Camera, focal2fov
    return Camera.from_c2w(torch.eye(4), (focal2fov(FOCAL, W), focal2fov(FOCAL, H)), (H, W))


def _xyz(px, py, z):
    return torch.stack([(px - (W - 1) / 2.0) * z / FOCAL, (py - (H - 1) / 2.0) * z / FOCAL, z], dim=1)


def scene(name):
    """raw parameters (CPU, the layout igs_amd.scenes documents), background, ground truth [3, H, W], instances of every tile"""
    L = LAYOUTS[name]
    gen = torch.Generator().manual_seed(sorted(LAYOUTS).index(name) + 11)

    def rnd(n, lo, hi):
        return torch.rand(n, generator=gen) * (hi - lo) + lo
    xyz, scal, opa = [], [], []
    for t, n in enumerate(L["small"]):
        (x0, x1), (y0, y1) = XR[t % 3], YR[t // 3]
        xyz.append(_xyz(rnd(n, x0, x1), rnd(n, y0, y1), rnd(n, 4.0, 6.0)))
        scal.append(rnd(n, -2.9, -2.7).unsqueeze(1).expand(n, 3) + rnd(3 * n, -0.1, 0.1).view(n, 3))
        p = rnd(n, 0.02, 0.08)
        opa.append(torch.log(p / (1.0 - p)))
    nb = L["big"]
    if nb:
        z = torch.linspace(4.0, 5.0, nb)
        xyz.append(_xyz(rnd(nb, 19.0, 21.0), rnd(nb, 11.0, 13.0), z))
        scal.append(torch.log(15.0 * z / FOCAL).unsqueeze(1).expand(nb, 3) + rnd(3 * nb, -0.05, 0.05).view(nb, 3))
        opa.append(torch.full((nb,), math.log(0.99 / 0.01)))
    n = sum(L["small"]) + nb
    pad = (-n) % 4 or 4                                      # (always some: Gaussians the view does not see take the culled paths)
    xyz.append(_xyz(rnd(pad, 900.0, 1000.0), rnd(pad, 0.0, 20.0), rnd(pad, 4.0, 6.0)))
    scal.append(torch.full((pad, 3), -4.6))
    opa.append(torch.zeros(pad))
    P = n + pad
    perm = torch.randperm(P, generator=gen)                  # (Gaussian index and list position are unrelated)
    shs = torch.randn(P, 16, 3, generator=gen) * 0.05
    shs[:, 0, :] = torch.randn(P, 3, generator=gen) / 0.2821 * 0.3
    raw = dict(xyz=torch.cat(xyz)[perm].contiguous(), scaling=torch.cat(scal)[perm].contiguous(),
               rotation=torch.randn(P, 4, generator=gen), opacity=torch.cat(opa)[perm].unsqueeze(1).contiguous(), shs=shs)
    gt = torch.rand(3, H, W, generator=gen)
    return raw, torch.tensor(L["bg"]), gt, [s + nb for s in L["small"]]


def run(name, absgrad, device="cuda:0"):
    """STEPS steps of igs_refine_step (L1) on the layout; {name: numpy array} of everything the step leaves behind"""
    from igs_amd.refine import GaussianParams, Refiner
    dev = torch.device(device)
    raw, bg, gt, tiles = scene(name)
    cam = camera().to(dev)
    pa = GaussianParams(raw, dev)
    assert pa.P % 4 == 0
    r = Refiner(pa, [cam], [gt.to(dev)], bg.to(dev), loss="l1", native=True, fused=True, want_viewspace_grad=absgrad)
    out = {}
    for s in range(STEPS):
        pk = r._fused_step(cam, r.gt[0])
        torch.cuda.synchronize(dev)
        out["rendered_%d" % s] = np.array([r.last_num_rendered], dtype=np.int64)
        out["images_%d" % s] = r._bufs.get(pa.P, H, W, dev)[0].cpu().numpy().copy()
        out["radii_%d" % s] = pk["radii"].cpu().numpy().copy()
        out["loss_%d" % s] = pk["loss"].cpu().numpy().copy()
        if absgrad:
            out["mean2d_%d" % s] = pk["viewspace_points"].cpu().numpy().copy()
    out["param"], out["exp_avg"], out["exp_avg_sq"] = pa.flat.cpu().numpy().copy(), pa.exp_avg.cpu().numpy().copy(), pa.exp_avg_sq.cpu().numpy().copy()
    from igs_amd import rasterizer as R
    out["abs_instance"] = np.array([1 if R.last_backward_instance()["absgrad"] else 0], dtype=np.int64)
    return out


if __name__ == "__main__":          # python blend_step_case.py OUT.npz : every (layout, absgrad) case into one file
    res = {}
    for name in sorted(LAYOUTS):
        for absgrad in (False, True):
            for k, v in run(name, absgrad).items():
                res["%s/%d/%s" % (name, int(absgrad), k)] = v
    np.savez(sys.argv[1], **res)
