"""Writes eigen_branches.npz: a small hand-made scene whose Gaussians take every branch of the 3x3 eigen-solver of the plane fit
(geom_math.h: eig_sym3 / cov2d_planes_eig), and the 128-byte records the forward's preprocess kernel writes for it.

    python tests/golden/make_eigen_branches_golden.py [OUT.npz]        (needs a GPU; default: next to this file)

The records were taken from the build BEFORE hyp() was made branch-free (two arms, one IEEE divide and square root each), so that
tests/test_gpu_eigen_branches.py pins "the same bits" for every later rewrite of the solver.  Everything the test feeds the rasterizer
is stored in the file (no random generator, no camera helper): re-run this only when the record layout or the reference arithmetic
itself changes, and say so in the commit.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, FOCAL = 80, 48, 60.0          # 5 x 3 tiles
N_GENERIC = 250                      # + the hand-placed ones: more than one workgroup of 256


def hand_cases():
    """(name, position, log-scales, quaternion (w, x, y, z)).  Camera at the origin looking down +z."""
    rz = (math.cos(0.35), 0.0, 0.0, math.sin(0.35))                 # about z only: Sigma[2][0] = Sigma[2][1] = 0, Sigma[1][0] != 0
    gen = (0.61, 0.33, -0.52, 0.49)
    return [
        ("householder_near0_no_sweep", (-1.0, -0.5, 4.0), (-1.0, -1.5, -2.0), (1.0, 0.0, 0.0, 0.0)),      # axis-aligned: Sigma diagonal
        ("equal_scales_no_sweep",      (0.0, -0.5, 4.0),  (-1.0, -1.0, -1.0), (1.0, 0.0, 0.0, 0.0)),
        ("householder_near0_sweeps",   (1.0, -0.5, 4.0),  (-1.0, -1.8, -1.4), rz),                        # row 2 skipped, QL sweeps on the 2x2 block
        ("rotated_sweeps",             (-1.0, 0.5, 4.0),  (-1.0, -1.7, -2.3), gen),
        ("rank_deficient_axis",        (0.0, 0.5, 4.0),   (-1.0, -1.0, -10.0), (1.0, 0.0, 0.0, 0.0)),     # evmin = e^-20 <= 1e-8: e_min e_min^T
        ("rank_deficient_rotated",     (1.0, 0.5, 4.0),   (-3.0, -3.0, -12.0), gen),
        ("regular_thin_rotated",       (0.0, 0.0, 5.0),   (-1.0, -1.0, -7.0), gen),                       # evmin = e^-14 > 1e-8: the regular inverse
    ]


def scene():
    frac = lambda x: x - np.floor(x)
    i = np.arange(N_GENERIC, dtype=np.float64)
    pos = np.stack([-1.6 + 3.2 * (i % 10) / 9.0, -0.9 + 1.8 * ((i // 10) % 5) / 4.0, 3.0 + 0.6 * (i // 50) + 0.05 * frac(i * 0.754877)], 1)
    logs = np.stack([-1.2 - 1.6 * frac(i * 0.618034 + 0.1), -1.2 - 1.6 * frac(i * 0.414214 + 0.4), -1.2 - 1.6 * frac(i * 0.732051 + 0.7)], 1)
    quat = np.stack([np.cos(0.7 * i), np.sin(1.3 * i), np.sin(2.1 * i + 1.0), np.cos(0.37 * i + 2.0)], 1)
    names = ["generic_%03d" % k for k in range(N_GENERIC)]
    hc = hand_cases()
    names = [c[0] for c in hc] + names
    pos = np.concatenate([np.array([c[1] for c in hc]), pos])
    logs = np.concatenate([np.array([c[2] for c in hc]), logs])
    quat = np.concatenate([np.array([c[3] for c in hc]), quat])
    quat = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    P = len(names)
    k = np.arange(P, dtype=np.float64)
    shs = np.zeros((P, 16, 3))
    shs[:, 0, :] = np.stack([0.9 * np.sin(0.9 * k), 0.9 * np.cos(1.7 * k), 0.9 * np.sin(2.3 * k + 0.5)], 1)
    for m in range(1, 16):
        shs[:, m, :] = 0.05 * np.stack([np.sin(0.3 * m * k + m), np.cos(0.2 * m * k + 2 * m), np.sin(0.5 * k + 3 * m)], 1)
    opac = 0.2 + 0.7 * frac(k * 0.381966)
    tanx, tany = W / (2.0 * FOCAL), H / (2.0 * FOCAL)
    zn, zf = 0.01, 100.0
    view_T = np.eye(4)                                                    # world = camera frame
    proj = np.zeros((4, 4))
    proj[0, 0] = 1.0 / tanx; proj[1, 1] = 1.0 / tany; proj[3, 2] = 1.0; proj[2, 2] = zf / (zf - zn); proj[2, 3] = -(zf * zn) / (zf - zn)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(names=np.array(names), means3D=f32(pos), scales=f32(np.exp(logs)), rotations=f32(quat), opacities=f32(opac[:, None]),
                shs=f32(shs), viewmatrix=f32(view_T), projmatrix=f32(view_T @ proj.T), campos=f32(np.zeros(3)), bg=f32([0.2, 0.4, 0.6]),
                tanfov=np.array([tanx, tany], np.float64), size=np.array([H, W], np.int64))


def forward_records(s, dev):
    """Runs the stand-alone forward on the stored inputs; returns (rec as uint32 [P, 32], radii int32 [P])."""
    import torch
    from igs_amd import rasterizer as R
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E = torch.Tensor([])
    Hh, Ww = int(s["size"][0]), int(s["size"][1])
    P = s["means3D"].shape[0]
    out = R.rasterize_gaussians(t(s["bg"]), t(s["means3D"]), E, t(s["opacities"]), t(s["scales"]), t(s["rotations"]), 1.0, E,
                                t(s["viewmatrix"]), t(s["projmatrix"]), float(s["tanfov"][0]), float(s["tanfov"][1]), 0.0, Hh, Ww,
                                t(s["shs"]), 3, t(s["campos"]), False, True, True, True)
    d = R.debug_dump(P, out[0], Ww, Hh, out[9], out[10], out[11])
    torch.cuda.synchronize()
    return d["rec"].cpu().numpy().view(np.uint32).copy(), out[8].cpu().numpy().astype(np.int32)


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "eigen_branches.npz")
    s = scene()
    rec, radii = forward_records(s, torch.device("cuda:0"))
    assert (radii > 0).all(), "every Gaussian of the scene is meant to be visible: %s" % (s["names"][radii <= 0],)
    np.savez_compressed(out, rec=rec, radii=radii, **s)
    print("wrote", out, os.path.getsize(out), "bytes;", len(radii), "Gaussians")


if __name__ == "__main__":
    main()
