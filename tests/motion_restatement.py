"""Float64 PyTorch restatement of the two anchor-graph consumers of IGS's AGM-Net, in this repository's words (no reference program text).

  interp_restate     -- GS3DRenderer.query_ir_grid's tail (igs/models/gs.py:812-822): gather the K neighbour rows of the flattened
                        anchor features, weight them, sum over K; split the result by example counts.
  qmul_restate       -- quaternion_multiply (igs/utils/general_utils.py:177-200): F.normalize both inputs (eps 1e-12), then the Hamilton
                        product with w first.
  deform_restate     -- GaussianModel.deform (gs.py:347-375) for the shipped residual keys xyz and rotation: clone the fields, add the
                        xyz residual on the masked rows, rotate the masked rows by the residual quaternion.

Every function is differentiable (torch.autograd), so the GPU tests take their gradient truths from here.  A -1 (or out-of-range)
column contributes nothing, as the native path documents.
"""
import torch


def interp_restate(feats_flat, weights, col):
    """out[n] = sum_k w[n, k] * F[col[n, k]] (gs.py:816-820), with slots outside [0, A) dropped.  F [A, D], weights [N, K] or
    [N, K, 1], col [N*K] or [N, K]; computed in F's dtype."""
    A, D = feats_flat.shape
    w = weights.reshape(weights.shape[0], -1)
    N, K = w.shape
    c = col.reshape(N, K)
    ok = (c >= 0) & (c < A)
    rows = feats_flat[c.clamp(0, A - 1).reshape(-1)].reshape(N, K, D)          # gs.py:818 features[col] viewed [N, K, D]
    prod = rows * w.to(feats_flat.dtype).unsqueeze(-1)                           # gs.py:820 features * weights
    prod = torch.where(ok.unsqueeze(-1), prod, torch.zeros((), dtype=prod.dtype))
    return prod.sum(dim=1)                                                       # ... sum over dim 1


def split_by_batch(out, batch_y):
    """gs.py:821-822: torch.unique(batch_y, return_counts=True), then torch.split by the counts."""
    _, counts = torch.unique(batch_y, return_counts=True)
    return torch.split(out, counts.tolist())


def normalize(q, eps=1e-12):
    """F.normalize along dim 1: q / max(|q|, eps)."""
    return q / q.norm(dim=1, keepdim=True).clamp_min(eps)


def qmul_restate(a, b):
    """general_utils.py:189-200: normalise both, then (w, x, y, z) of the Hamilton product a * b."""
    a, b = normalize(a), normalize(b)
    w1, x1, y1, z1 = a.unbind(1)
    w2, x2, y2, z2 = b.unbind(1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2,
                        w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                        w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2], dim=1)


def deform_xyz_rotation_restate(xyz, rotation, mask, res_xyz, res_rotation):
    """gs.py:356-370 for the xyz and rotation keys: clone, then masked rows get xyz + residual and qmul(rotation, residual)."""
    xo = xyz.clone()
    ro = rotation.clone()
    xo[mask] = res_xyz.to(xyz.dtype) + xo[mask]
    ro[mask] = qmul_restate(ro[mask], res_rotation.to(rotation.dtype))
    return xo, ro


def deform_restate(gs, res_feat, mask):
    """gs.py:347-375 as a dict of the GaussianModel fields it builds."""
    xo, ro = deform_xyz_rotation_restate(gs.xyz, gs.rotation, mask, res_feat["xyz"], res_feat["rotation"])
    return {"xyz": xo, "opacity": gs.opacity.clone(), "rotation": ro, "scaling": gs.scaling.clone(), "shs": gs.shs.clone(),
            "resi_rotation": res_feat["rotation"].clone(), "mask": mask, "resi_xyz": res_feat["xyz"].clone()}
