"""Timing of the compress package's count pass (diff_gaussian_rasterization_compress, igs_rast_count_gaussians) on the cfg-3 stand-in
(sear_steak_like_scene: 200k Gaussians, 10 cameras, 1352 x 1014).  Prints one JSON line:
  count_ms            warm wall time per _C.count_gaussians call (one view; the call waits for its instance count, as the reference's)
  fwd_color_ms        warm wall time per colour-only rade forward (_C.rasterize_gaussians, require_coord = require_depth = False), same views
  ratio               count_ms / fwd_color_ms
  prune_list_ms       compress.py's prune_list over the 10 views: GaussianRasterizer(f_count=True) per view plus the two running sums
  R_mean              mean instance count per view

usage: python tools/bench_count.py [--reps N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed passes over the 10 views (after 3 warm-up passes)")
    args = ap.parse_args()
    from diff_gaussian_rasterization_compress import GaussianRasterizationSettings, GaussianRasterizer
    from diff_gaussian_rasterization_compress import _C as CC
    from igs_amd._cabi import ext
    from igs_amd.scenes import activate, sear_steak_like_scene

    dev = torch.device("cuda:0")
    raw, cams, bg = sear_steak_like_scene()
    a = {k: v.detach().to(dev).contiguous() for k, v in activate(raw).items()}
    bg = bg.to(dev)
    e = torch.Tensor([])
    views = [(c.world_view_transform.to(dev), c.full_proj_transform.to(dev), c.camera_center.to(dev), c) for c in cams]
    rade = ext()

    def count(v):
        view, proj, campos, c = v
        return CC.count_gaussians(bg, a["means3D"], e, a["opacities"], a["scales"], a["rotations"], 1.0, e, view, proj, c.tanfovx,
                                  c.tanfovy, c.height, c.width, a["shs"], 3, campos, False, False, True)

    def fwd(v):
        view, proj, campos, c = v
        return rade.rasterize_gaussians(bg, a["means3D"], e, a["opacities"], a["scales"], a["rotations"], 1.0, e, view, proj, c.tanfovx,
                                        c.tanfovy, 0.0, c.height, c.width, a["shs"], 3, campos, False, False, False, False)

    def timed(fn):
        for _ in range(3):
            for v in views:
                fn(v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for _ in range(args.reps):
            for v in views:
                fn(v)
                n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    # interleave the two measurements twice and keep the better of each (same process, same allocator state)
    c_ms = min(timed(count), timed(count))
    f_ms = min(timed(fwd), timed(fwd))
    c_ms = min(c_ms, timed(count))
    R = [count(v)[2] for v in views]

    def prune_list():
        gaussian_list = imp_list = None
        for view, proj, campos, c in reversed(views):
            rs = GaussianRasterizationSettings(image_height=c.height, image_width=c.width, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=bg,
                                               scale_modifier=1.0, viewmatrix=view, projmatrix=proj, sh_degree=3, campos=campos,
                                               prefiltered=False, debug=False, f_count=True)
            means2D = torch.zeros_like(a["means3D"], requires_grad=True)
            gaussians_count, important_score, _, _ = GaussianRasterizer(rs)(
                means3D=a["means3D"], means2D=means2D, shs=a["shs"], colors_precomp=None, opacities=a["opacities"], scales=a["scales"],
                rotations=a["rotations"], cov3D_precomp=None)
            gaussian_list = gaussians_count.detach() if gaussian_list is None else gaussian_list + gaussians_count.detach()
            imp_list = important_score.detach() if imp_list is None else imp_list + important_score.detach()
        return gaussian_list, imp_list

    for _ in range(3):
        prune_list()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(5):
        t0 = time.perf_counter()
        prune_list()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(metric="count_gaussians", scene="sear_steak_like_scene", P=int(a["means3D"].shape[0]), views=len(views),
                          width=cams[0].width, height=cams[0].height, count_ms=round(c_ms, 4), fwd_color_ms=round(f_ms, 4),
                          ratio=round(c_ms / f_ms, 4), prune_list_ms=round(best, 3), R_mean=int(sum(R) / len(R)))))


if __name__ == "__main__":
    main()
