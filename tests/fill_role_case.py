"""Scenes and the step loop of tests/test_gpu_fill_role.py.

The scene is that of tests/test_gpu_zero_fill_visible.py with its sizes as parameters: P Gaussians ordered along the viewing axis, two
cameras inside the cloud back to back (each culls about half of the Gaussians, whole workgroups of them), three steps that alternate
between the views.  `run` returns the images and radii of every step and the parameters and both Adam moments at the end.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, W, H, STEPS = 1031, 80, 48, 3
CASES = {
    "l1": dict(loss="l1"),                                           # compact accumulator rows, the fused blend kernel, the step order
    "depth_normal": dict(loss="l1_ssim", lambda_depth_normal=0.05),  # full rows, the plane cache in use, no step order
    "masked": dict(loss="l1", masked=True),                          # rows exist for the trainable Gaussians only
}


def scene(n=P, w=W, h=H, scale_shift=1.5):
    from igs_amd.camera import Camera
    from igs_amd.scenes import cfg1_scene
    raw, _, _ = cfg1_scene(P=n, seed=5, size=64)
    order = torch.argsort(raw["xyz"][:, 2])               # along the viewing axis: each view culls whole workgroups
    raw = {k: v[order].contiguous() for k, v in raw.items()}
    raw["scaling"] = raw["scaling"] + scale_shift         # (1.5: footprints of a few pixels to a tile or two)
    fov = (math.radians(70.0), math.radians(45.0))
    back = torch.eye(4)
    back[0, 0], back[2, 2] = -1.0, -1.0                   # half a turn about y: looks down -z
    cams = [Camera.from_c2w(torch.eye(4), fov, (h, w)), Camera.from_c2w(back, fov, (h, w))]
    gen = torch.Generator().manual_seed(11)
    gts = [torch.rand(3, h, w, generator=gen) for _ in cams]
    return raw, cams, gts, torch.tensor([0.1, 0.2, 0.3])


def run(case, fill, dev, n=P, w=W, h=H, scale_shift=1.5):
    """Three steps on a workspace filled with the byte `fill` before every step."""
    from igs_amd.refine import GaussianParams, Refiner
    opt = dict(CASES[case])
    raw, cams, gts, bg = scene(n, w, h, scale_shift)
    mask = (torch.arange(n) % 3 != 0) if opt.pop("masked", False) else None
    pa = GaussianParams(raw, dev, mask=mask)
    r = Refiner(pa, [c.to(dev) for c in cams], [g.to(dev) for g in gts], bg.to(dev), native=True, fused=True, **opt)
    r._bufs.get(pa.P, h, w, dev)
    out = {}
    for s in range(STEPS):
        r._bufs.workspace.fill_(fill)
        pk = r.step(view=s % 2)
        torch.cuda.synchronize(dev)
        assert r._mode() == "fused"
        out["images_%d" % s] = r._bufs.get(pa.P, h, w, dev)[0].cpu().numpy().copy()
        out["radii_%d" % s] = pk["radii"].cpu().numpy().copy()
    out["param"], out["exp_avg"], out["exp_avg_sq"] = pa.flat.cpu().numpy().copy(), pa.exp_avg.cpu().numpy().copy(), pa.exp_avg_sq.cpu().numpy().copy()
    return out


def bytes_that_differ(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    return int((np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)).sum())
