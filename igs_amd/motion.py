"""The two consumers of the anchor graph in IGS's AGM-Net on the MI355X-native library (igs_amd/csrc/motion.hip, include/igs_rast.h).

Per streamed frame and per training step, igs/models/gs.py runs: GS3DRenderer.query_ir_grid's tail (gs.py:812-822), a weighted sum of
the features of every in-box Gaussian's K nearest anchors, then the decoder MLP, then GaussianModel.deform (gs.py:347-375), which moves
the masked Gaussians by the decoded residuals.  `query_ir_grid` and `deform` here are those two steps, with autograd.

`grid_encoder_lift` / `lift_anchor_features` are the step in front of them: GridEncoder.forward's lift of the 2-D motion features onto the
anchors (igs/models/grid_encoder.py:66-88 over igs/utils/ops.py:444-477; igs_amd/csrc/lift.hip), with autograd to the features.

`ray_condition` / `modln` / `condition3d` are the step in front of the lift: IGS.condition3D (igs/IGS.py:185-210 with ray_to_plucker,
rsh_cart_3 and ModLN; igs_amd/csrc/cond.hip).  The ray embedding and the fused LayerNorm + adaLN modulation are native, ModLN's small MLP
between them stays PyTorch.

Deviations from the reference lines (INTEGRATION.md lists them):
  - condition3d returns the reference's shape, dtype and values NCHW-contiguous, where the reference returns a channels-last-strided
    view of a [N, H, W, C] tensor: its only consumer, grid_encoder_lift, then reads it in place instead of copying it;
  - float16 features are normalised in float32 and the result is float32; a float16 modulation is widened before `1 + scale` is formed
    (the reference forms it in half);
  - a lifted sample whose pixel coordinate is not finite adds zero; channels-last features are copied to NCHW first;
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


class _Lift(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, points, w2c, intr):
        out = _ext().motion_lift_fwd(feat, points, w2c, intr)                # [B, C, A]
        ctx.save_for_backward(points, w2c, intr)                             # the backward needs no features
        ctx.hw, ctx.half = feat.shape[-2:], feat.dtype == torch.float16
        return out.permute(0, 2, 1)

    @staticmethod
    def backward(ctx, g):
        points, w2c, intr = ctx.saved_tensors
        d = _ext().motion_lift_bwd(g.float().permute(0, 2, 1), points, w2c, intr, ctx.hw[0], ctx.hw[1], ctx.half)
        return d, None, None, None


def _lift(motion_feature, anchor_points, w2c, intr, fn):
    for t, name in ((anchor_points, "anchor_points"), (w2c, "c2ws"), (intr, "intrinsics")):
        if t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"{fn}: gradients to {name} are not provided (only to motion_feature)")
    f = motion_feature
    if not (f.dim() == 4 and (f.shape[3] == 1 or f.stride(3) == 1) and (f.shape[2] == 1 or f.stride(2) == f.shape[3])):
        f = f.contiguous()                   # channels-last and other strided patterns: made plane-contiguous NCHW first
    if torch.is_grad_enabled() and f.requires_grad:
        return _Lift.apply(f, anchor_points, w2c, intr)
    return _ext().motion_lift_fwd(f, anchor_points, w2c, intr).permute(0, 2, 1)      # under no_grad nothing is saved


def _lift_shapes(motion_feature, anchor_points, c2ws, fn):
    if motion_feature.dim() != 4:
        raise ValueError(f"{fn}: motion_feature must be [B*V, C, H, W] (got {list(motion_feature.shape)})")
    if anchor_points.dim() != 3 or anchor_points.shape[-1] != 3:
        raise ValueError(f"{fn}: anchor_points must be [B, A, 3] (got {list(anchor_points.shape)})")
    if c2ws.dim() == 4:
        if c2ws.shape[0] != anchor_points.shape[0]:
            raise ValueError(f"{fn}: c2ws {list(c2ws.shape)} does not match {anchor_points.shape[0]} examples")
        c2ws = c2ws.reshape(-1, *c2ws.shape[2:])
    B, BV = anchor_points.shape[0], motion_feature.shape[0]
    if c2ws.dim() != 3 or tuple(c2ws.shape[1:]) != (4, 4) or c2ws.shape[0] != BV or B < 1 or BV % B:
        raise ValueError(f"{fn}: c2ws must be [B*V, 4, 4] or [B, V, 4, 4] with B*V = {BV} views for {B} examples (got {list(c2ws.shape)})")
    if motion_feature.dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: motion_feature must be float32 or float16 (got {motion_feature.dtype})")
    if anchor_points.dtype != torch.float32 or c2ws.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: anchor_points and c2ws must be float32 (got {anchor_points.dtype}, {c2ws.dtype})")
    if not (motion_feature.is_cuda and anchor_points.is_cuda and c2ws.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    return c2ws


def lift_anchor_features(motion_feature, anchor_points, c2ws, intrinsics):
    """perspective_projection (igs/utils/ops.py:444-477) for all views plus the mean over the views (grid_encoder.py:84-88): [B, A, C]
    float32, a permuted view of a [B, C, A] buffer (what GridEncoder's conv reads after its own permute).

    motion_feature [B*V, C, H, W] float32 / float16, any strides (plane-contiguous NCHW, slices of n and c included, is read in place;
    channels-last and everything else is copied to NCHW first); anchor_points [B, A, 3]; c2ws [B*V, 4, 4] or [B, V, 4, 4], inverted with
    torch.linalg.inv as the reference does; intrinsics [B*V, 3, 3] of the form [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (checked with one
    host read; anything else raises NotImplementedError) or [B*V, 4] = fx, fy, cx, cy (no read).  Gradients reach motion_feature only,
    in its dtype, summed in a fixed order (bitwise reproducible); the backward keeps the points and cameras, not the features."""
    fn = "lift_anchor_features"
    c2ws = _lift_shapes(motion_feature, anchor_points, c2ws, fn)
    BV = c2ws.shape[0]
    if intrinsics.dim() == 3 and tuple(intrinsics.shape) == (BV, 3, 3):
        K = intrinsics.detach().float().cpu()
        form = torch.zeros(3, 3, dtype=torch.bool)
        form[0, 1] = form[1, 0] = form[2, 0] = form[2, 1] = True
        if not ((K[:, form] == 0).all() and (K[:, 2, 2] == 1).all()):
            raise NotImplementedError(f"{fn}: intrinsics must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
        intr = torch.stack([intrinsics[:, 0, 0], intrinsics[:, 1, 1], intrinsics[:, 0, 2], intrinsics[:, 1, 2]], 1)
    elif intrinsics.dim() == 2 and tuple(intrinsics.shape) == (BV, 4):
        intr = intrinsics
    else:
        raise ValueError(f"{fn}: intrinsics must be [B*V, 3, 3] or [B*V, 4] with B*V = {BV} (got {list(intrinsics.shape)})")
    if intr.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: intrinsics must be float32 (got {intr.dtype})")
    return _lift(motion_feature, anchor_points, torch.linalg.inv(c2ws), intr.to(c2ws.device), fn)


def grid_encoder_lift(motion_feature, anchor_points, FOV, c2w_input, fov=None):
    """GridEncoder.forward's perspective_projection branch (grid_encoder.py:66-88): motion_grids [B, A, C] float32.

    Reproduces the reference's intrinsics as written: `W, H = motion_feature.shape[-2:]` (the names are swapped), fx =
    fov2focal(FOV[0, 0], shape[-2]), cx = shape[-2] / 2, fy = fov2focal(FOV[0, 1], shape[-1]), cy = shape[-1] / 2, and FOV[0] serves
    every example and view; the sampling itself normalises with the true width and height.  FOV [B, 2] on any device: the focal
    lengths are computed where it lies, in float32, without a host read.  fov=(fovx, fovy) as host floats replaces FOV[0] (FOV may then
    be None)."""
    fn = "grid_encoder_lift"
    if c2w_input.dim() != 4:
        raise ValueError(f"{fn}: c2w_input must be [B, V, 4, 4] (got {list(c2w_input.shape)})")
    c2ws = _lift_shapes(motion_feature, anchor_points, c2w_input, fn)
    Wn, Hn = motion_feature.shape[-2:]                                   # the reference's names
    if fov is not None:                      # host floats: fov2focal in double, rounded once into the float32 matrix
        import math
        intr = torch.tensor([Wn / (2 * math.tan(float(fov[0]) / 2)), Hn / (2 * math.tan(float(fov[1]) / 2)), Wn / 2.0, Hn / 2.0],
                            dtype=torch.float32)
    else:                                    # fov2focal's tensor branch (graphics_utils.py:73-75) where FOV lies, in its dtype: no host read
        if FOV.dim() != 2 or FOV.shape[-1] != 2:
            raise ValueError(f"{fn}: FOV must be [B, 2] (got {list(FOV.shape)})")
        f0 = FOV[0].detach()
        focal = torch.tensor([float(Wn), float(Hn)], dtype=f0.dtype, device=f0.device) / (2 * torch.tan(f0 / 2))
        intr = torch.cat([focal.float(), torch.tensor([Wn / 2.0, Hn / 2.0], dtype=torch.float32, device=f0.device)])
    intr = intr.to(c2ws.device).expand(c2ws.shape[0], 4)
    return _lift(motion_feature, anchor_points, torch.linalg.inv(c2ws), intr, fn)


class _ModLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, weight, bias, eps):
        out, mean, rstd = _ext().modln_fwd(x, mod, weight, bias, eps, True)
        ctx.save_for_backward(x, mod, weight, bias, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, g):
        x, mod, weight, bias, mean, rstd = ctx.saved_tensors
        nx, nm, nw, nb = ctx.needs_input_grad[:4]
        dx, dmod, dw, db = _ext().modln_bwd(x, mod, weight, bias, mean, rstd, g.float(), nx, nm, nw, nb)
        return dx, dmod, dw, db, None


def _plane_contiguous(f):
    return (f.shape[3] == 1 or f.stride(3) == 1) and (f.shape[2] == 1 or f.stride(2) == f.shape[3])


def ray_condition(rays, depth, size):
    """cond [B*V, H, W, 33] float32, contiguous: what IGS.condition3D hands ModLN's MLP (IGS.py:197-203, local_ray False).  rays
    [B, V, H, W, 6] float32 = (origin, direction) at the feature resolution size = (H, W); depth [B, V, Hd, Wd] float32 at any resolution.
    Channels 0-15: the degree <= 3 real spherical harmonics of the normalised direction, 16-31: of the raw moment origin x direction,
    32: depth resized bilinearly (align_corners=False).  One launch; no backward (rays / depth that require grad raise)."""
    fn = "ray_condition"
    if rays.dim() != 5 or rays.shape[-1] != 6:
        raise ValueError(f"{fn}: rays must be [B, V, H, W, 6] (got {list(rays.shape)})")
    if depth.dim() != 4 or tuple(depth.shape[:2]) != tuple(rays.shape[:2]):
        raise ValueError(f"{fn}: depth must be [B, V, Hd, Wd] with B, V = {list(rays.shape[:2])} (got {list(depth.shape)})")
    if tuple(size) != tuple(rays.shape[2:4]):
        raise ValueError(f"{fn}: rays are at {list(rays.shape[2:4])}, the feature resolution is {list(size)}")
    if rays.dtype != torch.float32 or depth.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: rays and depth must be float32 (got {rays.dtype}, {depth.dtype})")
    if torch.is_grad_enabled() and (rays.requires_grad or depth.requires_grad):
        raise NotImplementedError(f"{fn}: gradients to rays and depth are not provided")
    if not (rays.is_cuda and depth.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    return _ext().cond_ray_fwd(rays.reshape(-1, *rays.shape[2:]), depth.reshape(-1, *depth.shape[2:]))


def modln(x, mod, weight, bias, eps=1e-6):
    """out [N, C, H, W] float32, NCHW-contiguous = LayerNorm_C(x) * (1 + scale) + shift (ModLN.forward, IGS.py:282-284, on NCHW features).
    x [N, C, H, W] float32 / float16 (plane-contiguous NCHW, slices of n and c included, is read in place; anything else is copied);
    mod [N, H, W, 2C] float32 / float16, the MLP's output unchunked (shift = mod[..., :C], scale = mod[..., C:]); weight, bias [C] float32.
    Mean and biased variance over the C channels of a pixel, in float32 from centred values.  Gradients reach x and mod in their dtypes
    and weight / bias, the latter two summed in a fixed order (bitwise reproducible)."""
    fn = "modln"
    if x.dim() != 4:
        raise ValueError(f"{fn}: x must be [N, C, H, W] (got {list(x.shape)})")
    N, C, H, W = x.shape
    if tuple(mod.shape) != (N, H, W, 2 * C):
        raise ValueError(f"{fn}: mod must be [N, H, W, 2C] = {[N, H, W, 2 * C]} (got {list(mod.shape)})")
    if tuple(weight.shape) != (C,) or tuple(bias.shape) != (C,):
        raise ValueError(f"{fn}: weight and bias must be [C] = [{C}] (got {list(weight.shape)}, {list(bias.shape)})")
    if x.dtype not in FEATURE_DTYPES or mod.dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: x and mod must be float32 or float16 (got {x.dtype}, {mod.dtype})")
    if weight.dtype != torch.float32 or bias.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: weight and bias must be float32 (got {weight.dtype}, {bias.dtype})")
    if not (x.is_cuda and mod.is_cuda and weight.is_cuda and bias.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    if not _plane_contiguous(x):
        x = x.contiguous()
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, mod, weight, bias)):
        return _ModLN.apply(x, mod, weight, bias, float(eps))
    return _ext().modln_fwd(x, mod, weight, bias, float(eps), False)[0]          # under no_grad: one launch, nothing saved


def condition3d(motion_feature, rays, depth, modln_module):
    """IGS.condition3D (IGS.py:185-210, local_ray False): motion_feature [B*V, C, H, W] modulated by the ray / depth condition, float32,
    NCHW-contiguous (the reference returns the same values as a channels-last-strided view).  modln_module: any object with .norm
    (weight, bias, eps, normalized_shape == (C,)) and .mlp (a callable on [..., 33] returning [..., 2C]); the MLP runs in PyTorch."""
    fn = "condition3d"
    if motion_feature.dim() != 4:
        raise ValueError(f"{fn}: motion_feature must be [B*V, C, H, W] (got {list(motion_feature.shape)})")
    norm = modln_module.norm
    C = motion_feature.shape[1]
    if tuple(norm.normalized_shape) != (C,):
        raise ValueError(f"{fn}: the module normalises {tuple(norm.normalized_shape)}, motion_feature has C = {C}")
    if norm.weight is None or norm.bias is None:
        raise NotImplementedError(f"{fn}: LayerNorm without affine parameters is not supported")
    if rays.dim() == 5 and rays.shape[0] * rays.shape[1] != motion_feature.shape[0]:
        raise ValueError(f"{fn}: rays {list(rays.shape)} do not match {motion_feature.shape[0]} views")
    cond = ray_condition(rays, depth, motion_feature.shape[-2:])
    mod = modln_module.mlp(cond)
    return modln(motion_feature, mod, norm.weight, norm.bias, norm.eps)


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
