"""igs_refine_step zero-fills, in its preprocess kernel, only the accumulator rows of the Gaussians the view sees (radii > 0): nothing
reads another row (geom_bwd and extract_view_colors test `radii[idx] > 0`, the blend kernels add to rows of Gaussians in a tile list),
and the workspace's contents are undefined on entry (include/igs_rast.h).

So the steps must not care what the workspace holds: three steps whose workspace is filled with 0xFF bytes (NaN as double and as float)
before every step against the same three steps on a zeroed workspace, bit for bit -- images, radii, parameters and both Adam moments.
Two cameras stand inside the cloud back to back, so that each culls about half of the Gaussians (whole workgroups of them among the
1031: more than four workgroups, the last one partial) and a Gaussian whose poisoned row view A left alone is visible, and must find a
zeroed row, in view B.  Paths: the L1 step (64-byte rows), the depth-normal step (full rows, the plane cache in use), a masked step
(rows exist for the trainable Gaussians only).
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import dev  # noqa: F401

pytestmark = pytest.mark.gpu

P, W, H, STEPS = 1031, 80, 48, 3
CASES = {
    "l1": dict(loss="l1"),
    "depth_normal": dict(loss="l1_ssim", lambda_depth_normal=0.05),
    "masked": dict(loss="l1", masked=True),
}


def scene():
    from igs_amd.camera import Camera
    from igs_amd.scenes import cfg1_scene
    raw, _, _ = cfg1_scene(P=P, seed=5, size=64)
    order = torch.argsort(raw["xyz"][:, 2])               # along the viewing axis: each view culls whole workgroups
    raw = {k: v[order].contiguous() for k, v in raw.items()}
    raw["scaling"] = raw["scaling"] + 1.5                 # (footprints of a few pixels to a tile or two)
    fov = (math.radians(70.0), math.radians(45.0))
    back = torch.eye(4)
    back[0, 0], back[2, 2] = -1.0, -1.0                   # half a turn about y: looks down -z
    cams = [Camera.from_c2w(torch.eye(4), fov, (H, W)), Camera.from_c2w(back, fov, (H, W))]
    gen = torch.Generator().manual_seed(11)
    gts = [torch.rand(3, H, W, generator=gen) for _ in cams]
    return raw, cams, gts, torch.tensor([0.1, 0.2, 0.3])


def run(case, fill, dev):  # noqa: F811
    from igs_amd.refine import GaussianParams, Refiner
    opt = dict(CASES[case])
    raw, cams, gts, bg = scene()
    mask = (torch.arange(P) % 3 != 0) if opt.pop("masked", False) else None
    pa = GaussianParams(raw, dev, mask=mask)
    r = Refiner(pa, [c.to(dev) for c in cams], [g.to(dev) for g in gts], bg.to(dev), native=True, fused=True, **opt)
    r._bufs.get(pa.P, H, W, dev)
    out = {}
    for s in range(STEPS):
        r._bufs.workspace.fill_(fill)
        pk = r.step(view=s % 2)
        torch.cuda.synchronize(dev)
        assert r._mode() == "fused"
        out["images_%d" % s] = r._bufs.get(pa.P, H, W, dev)[0].cpu().numpy().copy()
        out["radii_%d" % s] = pk["radii"].cpu().numpy().copy()
    out["param"], out["exp_avg"], out["exp_avg_sq"] = pa.flat.cpu().numpy().copy(), pa.exp_avg.cpu().numpy().copy(), pa.exp_avg_sq.cpu().numpy().copy()
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_do_not_care_what_the_workspace_holds(dev, case):  # noqa: F811
    clean, poisoned = run(case, 0, dev), run(case, 0xFF, dev)
    ra, rb = clean["radii_0"], clean["radii_1"]
    assert ((ra == 0) & (rb > 0)).sum() > 256 and ((ra > 0) & (rb == 0)).sum() > 256, "each view culls Gaussians the other one sees"
    whole = lambda r: (r[: P // 256 * 256].reshape(-1, 256).max(1) == 0).any()
    assert whole(ra) or whole(rb), "a view culls a whole workgroup of 256"
    for k in sorted(clean):
        a, b = clean[k], poisoned[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.isfinite(b.astype(np.float64)).all(), k
        differ = int((np.ascontiguousarray(a).view(np.uint8) != np.ascontiguousarray(b).view(np.uint8)).sum())
        assert differ == 0, (case, k, "bytes that differ: %d" % differ)
    assert float(np.abs(clean["exp_avg_sq"]).max()) > 0.0 and float(np.abs(clean["images_2"][0:3]).max()) > 0.05      # the steps did something
