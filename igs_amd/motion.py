"""The two consumers of the anchor graph in IGS's AGM-Net on the MI355X-native library (igs_amd/csrc/motion.hip, include/igs_rast.h).

Per streamed frame and per training step, igs/models/gs.py runs: GS3DRenderer.query_ir_grid's tail (gs.py:812-822), a weighted sum of
the features of every in-box Gaussian's K nearest anchors, then the decoder MLP, then GaussianModel.deform (gs.py:347-375), which moves
the masked Gaussians by the decoded residuals.  `query_ir_grid` and `deform` here are those two steps, with autograd.

Deviations from the reference lines (INTEGRATION.md lists them):
  - a neighbour slot whose column is -1 (knn_native's padding) or out of range contributes nothing (the reference would index with it);
  - the interpolation backward is deterministic (an inverse index instead of index_put_'s atomics);
  - float16 residuals are widened to float32 before normalisation (the reference normalises them in float16).
"""
import torch

from ._cabi import ext as _ext

MAX_K = 100                            # IGS_INTERP_MAX_K
MAX_D = 1024                           # IGS_INTERP_MAX_D
FEATURE_DTYPES = (torch.float32, torch.float16)


def _flat_inputs(anchor_feats, weights, col):
    F = anchor_feats.reshape(-1, anchor_feats.shape[-1]) if anchor_feats.dim() == 3 else anchor_feats
    if F.dim() != 2:
        raise ValueError(f"interpolate_anchor_features: anchor_feats must be [B, A, D] or [B*A, D] (got {list(anchor_feats.shape)})")
    if weights.dim() == 3:
        if weights.shape[-1] != 1:
            raise ValueError(f"interpolate_anchor_features: weights must be [N, K, 1] or [N, K] (got {list(weights.shape)})")
        weights = weights.squeeze(-1)
    if weights.dim() != 2:
        raise ValueError(f"interpolate_anchor_features: weights must be [N, K, 1] or [N, K] (got {list(weights.shape)})")
    N, K = weights.shape
    if col.numel() != N * K:
        raise ValueError(f"interpolate_anchor_features: col has {col.numel()} entries for weights of shape {list(weights.shape)}")
    return F, weights, col.reshape(N, K)


class _Interp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F, w, col):
        out = _ext().motion_interp_fwd(F, col, w)
        ctx.save_for_backward(F, w, col)
        return out

    @staticmethod
    def backward(ctx, g):
        F, w, col = ctx.saved_tensors
        want_F, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_F or want_w):
            return None, None, None
        E = _ext()
        index = E.motion_interp_index(col.contiguous(), F.shape[0], F.shape[1])      # built only when a gradient is needed
        dF, dw = E.motion_interp_bwd(F, w, g.float(), index, want_F, want_w)
        return dF, dw, None


def interpolate_anchor_features(anchor_feats, weights, col):
    """out [N, D] float32 = sum_k weights[n, k] * anchor_feats_flat[col[n, k]] (gs.py:818-820).  anchor_feats [B, A, D] or [B*A, D]
    in float32 or float16 (col indexes the flattened rows: example i's columns are offset by i * A), weights [N, K, 1] or [N, K]
    float32, col [N*K] or [N, K] int64.  Gradients reach anchor_feats (in its dtype) and weights when they require them."""
    F, w, col = _flat_inputs(anchor_feats, weights, col)
    if F.dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"interpolate_anchor_features: features must be float32 or float16 (got {F.dtype})")
    if w.dtype != torch.float32:
        raise NotImplementedError(f"interpolate_anchor_features: weights must be float32 (got {w.dtype})")
    if col.dtype != torch.int64:
        raise NotImplementedError(f"interpolate_anchor_features: col must be int64 (got {col.dtype})")
    if torch.is_grad_enabled() and (F.requires_grad or w.requires_grad):
        return _Interp.apply(F, w, col)
    return _ext().motion_interp_fwd(F, col, w)                  # under no_grad: the one launch, nothing saved


def query_ir_grid(anchor_feats, weights, neighbor, counts=None):
    """The tail of GS3DRenderer.query_ir_grid (gs.py:812-822): a tuple of per-example [N_b, D] float32 tensors.  neighbor is
    anchor_graph's (row, col, batch_x, batch_y).  counts: the per-example Gaussian counts as host ints (anchor_graph's mask lengths)
    -- then no host synchronisation; None reads them from batch_y once, as the reference does."""
    _, col, _, batch_y = neighbor
    out = interpolate_anchor_features(anchor_feats, weights, col)
    if counts is None:
        _, c = torch.unique(batch_y, return_counts=True)
        counts = c.tolist()
    return torch.split(out, [int(c) for c in counts])


class _Deform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, rot, mask, dxyz, drot):
        xo, ro = _ext().motion_deform_fwd(xyz, rot, mask, dxyz, drot)
        ctx.save_for_backward(rot, mask, dxyz, drot)
        return xo, ro

    @staticmethod
    def backward(ctx, g_xyz, g_rot):
        rot, mask, dxyz, drot = ctx.saved_tensors
        nx, nr, _, ndx, ndr = ctx.needs_input_grad
        # d xyz = g_xyz itself (the map is xyz + a scatter of dxyz): no copy
        _, dr, ddx, ddr = _ext().motion_deform_bwd(rot, mask, dxyz, drot, g_xyz, g_rot, False, nr, ndx, ndr)
        d_xyz = None
        if nx:
            d_xyz = g_xyz if g_xyz is not None else torch.zeros_like(rot[:, :3])
        return d_xyz, dr, None, ddx, ddr


def deform_xyz_rotation(xyz, rotation, mask, res_xyz, res_rotation):
    """(xyz_new, rotation_new): xyz[mask] + res_xyz and quaternion_multiply(rotation[mask], res_rotation) (gs.py:362-370,
    general_utils.py:177-200) on the masked rows, every other row unchanged.  xyz [P, 3], rotation [P, 4] float32, mask [M] int64 of
    distinct indices, res_xyz [M, 3] and res_rotation [M, 4] float32 or float16 (widened to float32 before normalisation)."""
    if mask.dtype == torch.bool:
        mask = mask.nonzero().squeeze(1)
    mask = mask.long()
    res_xyz = res_xyz.reshape(-1, 3)
    if res_rotation.dtype != res_xyz.dtype and res_rotation.dtype in FEATURE_DTYPES and res_xyz.dtype in FEATURE_DTYPES:
        res_xyz = res_xyz.to(res_rotation.dtype)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (xyz, rotation, res_xyz, res_rotation)):
        return _Deform.apply(xyz, rotation, mask, res_xyz, res_rotation)
    return _ext().motion_deform_fwd(xyz, rotation, mask, res_xyz, res_rotation)


def deform(gs, res_feat, mask):
    """GaussianModel.deform (gs.py:347-375): the dict of GaussianModel fields (xyz, opacity, rotation, scaling, shs, resi_xyz,
    resi_rotation, mask).  gs: any object with .xyz .opacity .rotation .scaling .shs; res_feat: {"xyz": [M, 3], "rotation": [M, 4]}
    (the shipped config's residuals, configs/train.yaml:215-217); other keys raise NotImplementedError."""
    extra = set(res_feat) - {"xyz", "rotation"}
    if extra:
        raise NotImplementedError(f"deform: residuals {sorted(extra)} are not supported natively (only xyz and rotation)")
    if "xyz" not in res_feat or "rotation" not in res_feat:
        raise NotImplementedError("deform: both the xyz and the rotation residual are required")
    xyz, rotation = deform_xyz_rotation(gs.xyz, gs.rotation, mask, res_feat["xyz"], res_feat["rotation"])
    return {"xyz": xyz, "opacity": gs.opacity.clone(), "rotation": rotation, "scaling": gs.scaling.clone(), "shs": gs.shs.clone(),
            "resi_xyz": res_feat["xyz"].clone(), "resi_rotation": res_feat["rotation"].clone(), "mask": mask}
