"""Generates tests/golden/ref_lift.npz: outputs of the reference's own perspective_projection (igs/utils/ops.py) and fov2focal
(igs/utils/graphics_utils.py), data only.

Run in the build container only (needs the reference checkout):  python tests/golden/make_lift_golden.py REFERENCE_ROOT   (or IGS_REFERENCE in the environment)
igs/utils/ops.py does not import here (jaxtyping), so only the AST node of `perspective_projection` is compiled, with its annotations
removed; the reference is read at run time and none of its text is stored.  Case: a non-square 12 x 20 map, B = 2, V = 3, C = 5,
A = 96, float32, some points behind the camera, some samples outside, and the autograd gradient to the features for a fixed upstream
gradient.  `w2c` is torch.inverse(c2ws), the reference function's own first line, stored so that the float64 restatement can be compared
without the float32 inversion error.
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")


def load_function(path, name, env):
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    for a in node.args.args:
        a.annotation = None
    node.returns = None
    mod = ast.Module(body=[node], type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), env)
    return env[name]


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    pp = load_function(os.path.join(REF, "igs", "utils", "ops.py"), "perspective_projection", {"torch": torch, "F": F})
    spec = importlib.util.spec_from_file_location("ref_graphics_utils", os.path.join(REF, "igs", "utils", "graphics_utils.py"))
    gu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gu)
    g = torch.Generator().manual_seed(20240)
    B, V, C, H, W, A = 2, 3, 5, 12, 20, 96
    feat = torch.randn(B * V, C, H, W, generator=g)
    c2w = torch.eye(4).repeat(B * V, 1, 1)
    for i in range(B * V):
        q = torch.randn(4, generator=g)
        q = q / q.norm()
        w, x, y, z = q.tolist()
        R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        R = torch.eye(3) + 0.25 * (R - torch.eye(3))                   # a mild rotation-like matrix (not orthonormal: a general pose)
        c2w[i, :3, :3] = R
        c2w[i, :3, 3] = torch.tensor([0.0, 0.0, -3.0]) + 0.3 * torch.randn(3, generator=g)
    fovx, fovy = 0.9, 0.7
    # GridEncoder's rule: `W, H = shape[-2:]`, so the names are swapped
    Wn, Hn = H, W
    fx, fy = float(gu.fov2focal(fovx, Wn)), float(gu.fov2focal(fovy, Hn))
    K = np.identity(3, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, Wn / 2.0, Hn / 2.0
    intrinsics = torch.from_numpy(K[None].repeat(B * V, axis=0))
    pts = torch.rand(B, A, 3, generator=g) * 3.0 - 1.5
    pts[:, :6, 2] -= 5.0                                                # behind the cameras: negative z, mirrored projection
    w2c = torch.inverse(c2w)
    for _ in range(20):                                                 # keep |z_cam| >= 0.25 (resample the few points that violate it)
        pc = pts.repeat_interleave(V, 0) @ w2c[:, :3, :3].transpose(1, 2) + w2c[:, :3, 3].unsqueeze(1)
        bad = (pc[..., 2].abs() < 0.25).reshape(B, V, A).any(1)
        if not bad.any():
            break
        pts[bad] = torch.rand(int(bad.sum()), 3, generator=g) * 3.0 - 1.5
    assert not bad.any()
    x = feat.clone().requires_grad_(True)
    pp_pts = pts.unsqueeze(1).repeat_interleave(V, 1).reshape(B * V, A, 3)
    proj = pp(pp_pts, c2w, intrinsics, x)                              # [B*V, A, C]
    out = proj.reshape(B, V, A, C).mean(dim=1)
    gout = torch.randn(B, A, C, generator=g)
    out.backward(gout)
    np.savez_compressed(os.path.join(HERE, "ref_lift.npz"), feat=feat.numpy(), c2w=c2w.numpy(), w2c=w2c.numpy(), intrinsics=intrinsics.numpy(),
                        points=pts.numpy(), fov=np.array([fovx, fovy]), focal=np.array([fx, fy], dtype=np.float64), out=out.detach().numpy(),
                        gout=gout.numpy(), dfeat=x.grad.numpy())
    print("ref_lift.npz:", os.path.getsize(os.path.join(HERE, "ref_lift.npz")), "bytes; z < 0:", int((pc[..., 2] < 0).sum()),
          "of", pc[..., 2].numel())


if __name__ == "__main__":
    main()
