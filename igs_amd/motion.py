"""The two consumers of the anchor graph in IGS's AGM-Net on the MI355X-native library (igs_amd/csrc/motion.hip, include/igs_rast.h).

Per streamed frame and per training step, igs/models/gs.py runs: GS3DRenderer.query_ir_grid's tail (gs.py:812-822), a weighted sum of
the features of every in-box Gaussian's K nearest anchors, then the decoder MLP, then GaussianModel.deform (gs.py:347-375), which moves
the masked Gaussians by the decoded residuals.  `query_ir_grid` and `deform` here are the first and the last step, with autograd.

`mlp_heads` / `decode_residual_feature` / `use_native_decoder` are the step between them: GS3DRenderer.decode_residual_feature
(gs.py:858-869), the MLP of igs/models/networks.py:60-108 and the per-feature output Linears in one launch (igs_amd/csrc/mlp.hip).
These are forward only, for the streaming path under torch.no_grad().  `mlp_heads_autograd` / `decode_residual_feature_train` /
`use_native_decoder(r, training=True)` add the native backward (igs_mlp_heads_bwd), which recomputes the forward from x.

`grid_encoder_lift` / `lift_anchor_features` are the step in front of them: GridEncoder.forward's lift of the 2-D motion features onto the
anchors (igs/models/grid_encoder.py:66-88 over igs/utils/ops.py:444-477; igs_amd/csrc/lift.hip), with autograd to the features.

`ray_condition` / `modln` / `condition3d` are the step in front of the lift: IGS.condition3D (igs/IGS.py:185-210 with ray_to_plucker,
rsh_cart_3 and ModLN; igs_amd/csrc/cond.hip).  The ray embedding and the fused LayerNorm + adaLN modulation are native, ModLN's small MLP
between them stays PyTorch: the path with autograd.  `condition3d_fused` / `use_native_condition3d` are the same stage's forward in one
launch, the MLP on the matrix cores included (igs_amd/csrc/cond_fused.hip): forward only, for the streaming path under torch.no_grad();
`condition3d_fused_autograd` / `use_native_condition3d(model, training=True)` put a recomputing native backward behind that launch
(igs_amd/csrc/cond_fused_bwd.hip).

`upsample_conv` / `pack_upsample_conv` are the step in front of condition3D: the 2x bilinear upsample and the 3x3 convolution of the
motion features (igs/IGS.py:132-134, up_sample True) in one launch on the matrix cores, the upsampled map never stored
(igs_amd/csrc/upconv.hip): forward only; a call that needs a gradient is the eager two lines.  `upsample_conv_autograd` is the same step
for training: the native forward with the native backward (igs_upconv_bwd, igs_amd/csrc/upconv_bwd.hip), which recomputes the upsampled map
from x and stores neither it nor its gradient.

Deviations from the reference lines (INTEGRATION.md lists them):
  - condition3d returns the reference's shape, dtype and values NCHW-contiguous, where the reference returns a channels-last-strided
    view of a [N, H, W, C] tensor: its only consumer, grid_encoder_lift, then reads it in place instead of copying it;
  - float16 features are normalised in float32 and the result is float32; a float16 modulation is widened before `1 + scale` is formed
    (the reference forms it in half);
  - a lifted sample whose pixel coordinate is not finite adds zero; channels-last features are copied to NCHW first;
  - a neighbour slot whose column is -1 (knn_native's padding) or out of range contributes nothing (the reference would index with it);
  - the interpolation backward is deterministic (an inverse index instead of index_put_'s atomics);
  - float16 residuals are widened to float32 before normalisation (the reference normalises them in float16);
  - the float16 decoder accumulates, adds the bias and applies the activation in float32 and rounds each activation to half once (the
    reference rounds after every Linear and every activation); its backward recomputes the forward the same way and returns
    parameter gradients accumulated in float32 and rounded once.
"""
import torch

from ._binding import autocast_half as _autocast_half, param_key as _param_key
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


# ---------------------------------------------------------------- condition3D in one launch (cond_fused.hip)
COND_CH, COND_MLP_MAX_WIDTH = 33, 128                           # IGS_COND_MLP_MAX_WIDTH
COND_FUSED_MAX_STRIDE = 1 << 27                                 # IGS_COND_FUSED_MAX_STRIDE
COND_FUSED_CACHE = "_igs_condition3d_pack"
MODLN_NAME = "ModLN"                                            # IGS.ModLN (IGS.py:91-95)
# What use_native_condition3d sends to the fused kernel: per MLP dtype the largest N * H * W it takes (None: no limit, 0: never).
# DESIGN.md 15.7 has the measurements this follows: the fused forward is the faster one in every measured case.
COND_FUSED_MAX_PIXELS = {torch.float32: None, torch.float16: None}
COND_FUSED_TRAIN_CACHE = "_igs_condition3d_train_pack"
# Per MLP dtype, whether use_native_condition3d(model, training=True) sends a call that needs a gradient to condition3d_fused_autograd
# (True) or to condition3d (False).  DESIGN.md 15.8 has the rule and the measurements this follows: at N = 16 views of the shipped shape
# the native forward + backward took 3.84 ms against 2.09 ms (float32) and 2.92 against 2.08 ms (float16), so it is taken only on request
# (an explicit mlp_dtype on condition3d_fused_autograd); what it buys is memory (203 MB against 985 / 565 MB) and a reproducible backward.
COND_FUSED_BWD_NATIVE = {torch.float32: False, torch.float16: False}


def _cond_mlp_spec(fn, modln_module, C):
    """(Linear(33, hidden), Linear(hidden, 2C)) of a ModLN-shaped module, or NotImplementedError."""
    nn = torch.nn
    mlp = getattr(modln_module, "mlp", None)
    mods = list(mlp) if isinstance(mlp, nn.Sequential) else []
    if len(mods) != 3 or not (isinstance(mods[0], nn.Linear) and isinstance(mods[1], nn.SiLU) and isinstance(mods[2], nn.Linear)):
        raise NotImplementedError(f"{fn}: .mlp must be nn.Sequential(Linear(33, hidden), SiLU, Linear(hidden, 2C))")
    l0, l2 = mods[0], mods[2]
    if l0.in_features != COND_CH or l2.in_features != l0.out_features or l2.out_features != 2 * C:
        raise NotImplementedError(f"{fn}: .mlp must map 33 -> hidden -> 2C = {2 * C} (got {l0.in_features} -> {l0.out_features}, "
                                  f"{l2.in_features} -> {l2.out_features})")
    if not (1 <= C <= COND_MLP_MAX_WIDTH and 1 <= l0.out_features <= COND_MLP_MAX_WIDTH):
        raise NotImplementedError(f"{fn}: C and hidden must be in 1..{COND_MLP_MAX_WIDTH} (got {C}, {l0.out_features})")
    return l0, l2


def _cond_params(modln_module):
    mlp, norm = modln_module.mlp, modln_module.norm
    return [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, norm.weight, norm.bias]


def pack_condition_mlp(mlp, dtype=torch.float32, transposed=False):
    """(wpack in `dtype`, bpack float32 [3, 128]) as igs_condition3d_fwd takes them (include/igs_rast.h), from
    mlp = nn.Sequential(Linear(33, hidden), SiLU, Linear(hidden, 2C)): W1, W2[:C] (shift) and W2[C:] (scale), each in
    pack_mlp_tile_order, one after another; the biases b1, b2[:C], b2[C:] zero-padded (an absent bias: zeros).  transposed=True:
    (wpack, bpack, wpack_t), wpack_t = W2^T as igs_condition3d_bwd takes it: one Linear [hidden, 2 * 32 ct] in pack_mlp_tile_order whose
    input 32 ct s + c is channel c of the shift (s = 0) or the scale (s = 1) half.  Plain tensor ops."""
    l0, l2 = mlp[0], mlp[2]
    hidden, C = l0.out_features, l2.out_features // 2
    W1, W2 = l0.weight.detach().to(dtype), l2.weight.detach().to(dtype)
    wpack = torch.cat([pack_mlp_tile_order(W1), pack_mlp_tile_order(W2[:C]), pack_mlp_tile_order(W2[C:])]).contiguous()
    bpack = torch.zeros(3, COND_MLP_MAX_WIDTH, dtype=torch.float32, device=wpack.device)
    if l0.bias is not None:
        bpack[0, :hidden] = l0.bias.detach().float()
    if l2.bias is not None:
        bpack[1, :C] = l2.bias.detach().float()[:C]
        bpack[2, :C] = l2.bias.detach().float()[C:]
    if not transposed:
        return wpack, bpack
    cw = 32 * _tiles(C)
    M = W2.new_zeros(hidden, 2 * cw)
    M[:, :C] = W2[:C].t()
    M[:, cw:cw + C] = W2[C:].t()
    return wpack, bpack, pack_mlp_tile_order(M).contiguous()


def _cond_fused_args(fn, motion_feature, rays, depth, modln_module):
    """(norm, (N, C, H, W), Linear(33, hidden)) after the checks condition3d_fused and condition3d_fused_autograd share."""
    if motion_feature.dim() != 4:
        raise ValueError(f"{fn}: motion_feature must be [B*V, C, H, W] (got {list(motion_feature.shape)})")
    norm = modln_module.norm
    N, C, H, W = motion_feature.shape
    if tuple(norm.normalized_shape) != (C,):
        raise ValueError(f"{fn}: the module normalises {tuple(norm.normalized_shape)}, motion_feature has C = {C}")
    if norm.weight is None or norm.bias is None:
        raise NotImplementedError(f"{fn}: LayerNorm without affine parameters is not supported")
    if rays.dim() != 5 or rays.shape[-1] != 6:
        raise ValueError(f"{fn}: rays must be [B, V, H, W, 6] (got {list(rays.shape)})")
    if rays.shape[0] * rays.shape[1] != N:
        raise ValueError(f"{fn}: rays {list(rays.shape)} do not match {N} views")
    if depth.dim() != 4 or tuple(depth.shape[:2]) != tuple(rays.shape[:2]):
        raise ValueError(f"{fn}: depth must be [B, V, Hd, Wd] with B, V = {list(rays.shape[:2])} (got {list(depth.shape)})")
    if tuple(rays.shape[2:4]) != (H, W):
        raise ValueError(f"{fn}: rays are at {list(rays.shape[2:4])}, the feature resolution is {[H, W]}")
    if rays.dtype != torch.float32 or depth.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: rays and depth must be float32 (got {rays.dtype}, {depth.dtype})")
    if motion_feature.dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: motion_feature must be float32 or float16 (got {motion_feature.dtype})")
    if norm.weight.dtype != torch.float32 or norm.bias.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: the LayerNorm's weight and bias must be float32 (got {norm.weight.dtype}, {norm.bias.dtype})")
    l0, _ = _cond_mlp_spec(fn, modln_module, C)
    return norm, (N, C, H, W), l0


def condition3d_fused(motion_feature, rays, depth, modln_module, packed=None, mlp_dtype=None):
    """condition3d's result in one launch, forward only: the ray / depth condition, ModLN's MLP and the modulated LayerNorm per pixel,
    with neither cond, the hidden activations nor mod stored (igs_condition3d_fwd, cond_fused.hip).  motion_feature [B*V, C, H, W] float32
    / float16 (plane-contiguous NCHW is read in place, anything else is copied), rays [B, V, H, W, 6], depth [B, V, Hd, Wd] float32;
    out float32, NCHW-contiguous.  modln_module: .norm as condition3d takes it, .mlp = nn.Sequential(Linear(33, hidden), SiLU,
    Linear(hidden, 2C)) with C, hidden <= 128.  mlp_dtype: torch.float32 (an exact float32 fma chain) or torch.float16 (half operands,
    float32 accumulation; mod is not rounded to half); default float16 under autocast to half, float32 otherwise.  packed:
    pack_condition_mlp(modln_module.mlp, mlp_dtype), packed here when absent.  The argument checks are condition3d's; another .mlp
    structure, C or hidden out of range, or anything that requires grad under enabled grad raise NotImplementedError."""
    fn = "condition3d_fused"
    norm, (N, C, H, W), l0 = _cond_fused_args(fn, motion_feature, rays, depth, modln_module)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [motion_feature, rays, depth] + _cond_params(modln_module)):
        raise NotImplementedError(f"{fn}: forward only -- call it under torch.no_grad(), and train with condition3d")
    if not (motion_feature.is_cuda and rays.is_cuda and depth.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    if mlp_dtype is None:
        mlp_dtype = torch.float16 if _autocast_half(fn, motion_feature) else torch.float32
    if mlp_dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: mlp_dtype must be float32 or float16 (got {mlp_dtype})")
    wpack, bpack = pack_condition_mlp(modln_module.mlp, mlp_dtype) if packed is None else packed
    if wpack.dtype != mlp_dtype:
        raise ValueError(f"{fn}: packed holds {wpack.dtype} weights, mlp_dtype is {mlp_dtype}")
    x = motion_feature
    if not _plane_contiguous(x) or (C > 1 and x.stride(1) > COND_FUSED_MAX_STRIDE):
        x = x.contiguous()
    return _ext()._cond.condition3d_fwd(x, rays.reshape(N, *rays.shape[2:]), depth.reshape(N, *depth.shape[2:]), wpack, bpack, l0.out_features,
                                  norm.weight.detach(), norm.bias.detach(), float(norm.eps))


class _Condition3dFused(torch.autograd.Function):
    """igs_condition3d_fwd with igs_condition3d_bwd behind it.  Saves x as the kernels read it, rays, depth, the packs and the LayerNorm's
    affine: neither cond, the hidden activations, mod nor the statistics."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, nw, nb, rays, depth, wpack, bpack, wpack_t, hidden, eps):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, rays, depth, wpack, bpack, wpack_t, nw, nb)
        ctx.hidden, ctx.eps = hidden, eps
        ctx.param_dtypes = [None if t is None else t.dtype for t in (w1, b1, w2, b2, nw, nb)]
        return _ext()._cond.condition3d_fwd(x, rays, depth, wpack, bpack, hidden, nw.detach(), nb.detach(), eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 14
        x, rays, depth, wpack, bpack, wpack_t, nw, nb = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.float()
        if not g.is_contiguous():
            g = g.contiguous()                   # (the one copy of a strided d out)
        grads = list(_ext()._cond.condition3d_bwd(x, rays, depth, wpack, wpack_t, bpack, ctx.hidden, nw.detach(), nb.detach(), ctx.eps, g,
                                                  *ctx.needs_input_grad[:7]))
        for i, dt in enumerate(ctx.param_dtypes):    # accumulated in float32, cast once
            if grads[i + 1] is not None and grads[i + 1].dtype != dt:
                grads[i + 1] = grads[i + 1].to(dt)
        return (*grads, None, None, None, None, None, None, None)


def condition3d_fused_autograd(motion_feature, rays, depth, modln_module, packed=None, mlp_dtype=None):
    """condition3d_fused for training: the same checks, sizes, dtypes and value, and a native backward.  When grad is disabled or neither
    motion_feature nor a parameter of the module requires it this IS condition3d_fused(...).  Otherwise the forward is igs_condition3d_fwd
    and the backward igs_condition3d_bwd (cond_fused_bwd.hip): d motion_feature in its dtype, the gradients of mlp[0] / mlp[2]'s weights and
    biases and of norm.weight / norm.bias accumulated in float32 and cast once to each parameter's dtype.  Saved: motion_feature as the
    kernels read it (itself where it is plane-contiguous NCHW, a contiguous copy otherwise), rays, depth, the packs and the LayerNorm's
    affine; cond, the hidden activations and mod are recomputed.  Once differentiable, deterministic (no atomics).  rays or depth that
    require grad raise NotImplementedError.  `packed`, if given, is pack_condition_mlp(modln_module.mlp, mlp_dtype, transposed=True);
    otherwise the three packs are kept on the module under COND_FUSED_TRAIN_CACHE and rebuilt when a parameter's _version, data_ptr,
    dtype or device changes (every optimiser step).  Refusals as condition3d_fused's; there is no CPU fallback."""
    fn = "condition3d_fused_autograd"
    norm, (N, C, H, W), l0 = _cond_fused_args(fn, motion_feature, rays, depth, modln_module)
    if packed is not None and len(packed) != 3:
        raise ValueError(f"{fn}: packed must be pack_condition_mlp(mlp, mlp_dtype, transposed=True)")
    if torch.is_grad_enabled() and (rays.requires_grad or depth.requires_grad):
        raise NotImplementedError(f"{fn}: gradients to rays and depth are not provided")
    params = _cond_params(modln_module)
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [motion_feature] + params)):
        return condition3d_fused(motion_feature, rays, depth, modln_module, packed=None if packed is None else tuple(packed[:2]),
                                 mlp_dtype=mlp_dtype)
    if mlp_dtype is None:
        mlp_dtype = torch.float16 if _autocast_half(fn, motion_feature) else torch.float32
    if mlp_dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: mlp_dtype must be float32 or float16 (got {mlp_dtype})")
    if packed is not None and (packed[0].dtype != mlp_dtype or packed[2].dtype != mlp_dtype):
        raise ValueError(f"{fn}: packed holds {packed[0].dtype} weights, mlp_dtype is {mlp_dtype}")
    if not (motion_feature.is_cuda and rays.is_cuda and depth.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    if packed is None:
        key = (_param_key(params[:4]), mlp_dtype)
        cache = modln_module.__dict__.get(COND_FUSED_TRAIN_CACHE)
        if cache is None or cache["key"] != key:
            cache = dict(key=key, pack=pack_condition_mlp(modln_module.mlp, mlp_dtype, transposed=True))
            modln_module.__dict__[COND_FUSED_TRAIN_CACHE] = cache
        packed = cache["pack"]
    wpack, bpack, wpack_t = packed
    x = motion_feature
    if not _plane_contiguous(x) or (C > 1 and x.stride(1) > COND_FUSED_MAX_STRIDE) or x.stride(0) < 0 or x.stride(1) < 0:
        x = x.contiguous()
    return _Condition3dFused.apply(x, *params, rays.reshape(N, *rays.shape[2:]), depth.reshape(N, *depth.shape[2:]), wpack, bpack, wpack_t,
                                   l0.out_features, float(norm.eps))


def _condition3d_bound(self, motion_feature, rays, depth, training=False):
    """IGS.condition3D as use_native_condition3d binds it: the fused forward when nothing needs a gradient and the module qualifies,
    condition3d (ray_condition -> the PyTorch MLP -> modln, with autograd) otherwise.  training: a call that needs a gradient goes to
    condition3d_fused_autograd where COND_FUSED_BWD_NATIVE says so for its MLP dtype."""
    fn = "condition3D"
    module = _child(self, MODLN_NAME)
    try:
        params = _cond_params(module)
    except (AttributeError, IndexError, TypeError):
        return condition3d(motion_feature, rays, depth, module)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [motion_feature, rays, depth] + params):
        if not training or rays.requires_grad or depth.requires_grad:
            return condition3d(motion_feature, rays, depth, module)
        try:
            _cond_mlp_spec(fn, module, motion_feature.shape[1] if motion_feature.dim() == 4 else -1)
        except NotImplementedError:
            return condition3d(motion_feature, rays, depth, module)
        dtype = torch.float16 if _autocast_half(fn, motion_feature) else torch.float32
        if not COND_FUSED_BWD_NATIVE[dtype]:
            return condition3d(motion_feature, rays, depth, module)
        return condition3d_fused_autograd(motion_feature, rays, depth, module, mlp_dtype=dtype)
    try:
        _cond_mlp_spec(fn, module, motion_feature.shape[1] if motion_feature.dim() == 4 else -1)
    except NotImplementedError:
        return condition3d(motion_feature, rays, depth, module)
    dtype = torch.float16 if _autocast_half(fn, motion_feature) else torch.float32
    limit = COND_FUSED_MAX_PIXELS[dtype]
    if limit is not None and motion_feature.numel() // max(motion_feature.shape[1], 1) > limit:
        return condition3d(motion_feature, rays, depth, module)
    key = (_param_key(params[:4]), dtype)
    cache = module.__dict__.get(COND_FUSED_CACHE)
    if cache is None or cache["key"] != key:
        cache = dict(key=key, pack=pack_condition_mlp(module.mlp, dtype))
        module.__dict__[COND_FUSED_CACHE] = cache
    return condition3d_fused(motion_feature, rays, depth, module, packed=cache["pack"], mlp_dtype=dtype)


def _condition3d_bound_training(self, motion_feature, rays, depth):
    return _condition3d_bound(self, motion_feature, rays, depth, training=True)


def use_native_condition3d(model, training=False):
    """Binds condition3D(motion_feature, rays, depth) on this IGS-shaped instance (IGS.py:185-210) and returns the instance; the class and
    state_dict() keys are untouched.  A call under torch.no_grad() (or with nothing that requires grad) on a module whose .ModLN.mlp is
    Linear(33, hidden) . SiLU . Linear(hidden, 2C) with C, hidden <= 128 takes condition3d_fused -- float16 weights under autocast to half,
    float32 otherwise, within COND_FUSED_MAX_PIXELS -- and every other call is condition3d, exactly today's training path.  training=True
    binds a variant that sends a call that needs a gradient (to motion_feature or a parameter, not to rays or depth) to
    condition3d_fused_autograd where COND_FUSED_BWD_NATIVE[mlp dtype] is True, and to condition3d where it is False.  The packed
    weights are kept on the ModLN module and rebuilt when a parameter's _version, data_ptr, dtype or device changes.  Raises
    NotImplementedError, before anything is changed, for cfg.local_ray true or cfg.use_condition3d false."""
    import types
    cfg = model.cfg
    if getattr(cfg, "local_ray", False):
        raise NotImplementedError("use_native_condition3d: local_ray True (the 4-channel condition) is not supported")
    if not getattr(cfg, "use_condition3d", True):
        raise NotImplementedError("use_native_condition3d: cfg.use_condition3d is False: the model has no ModLN to bind")
    if _child(model, MODLN_NAME) is None:
        raise NotImplementedError(f"use_native_condition3d: the model has no {MODLN_NAME} module")
    model.condition3D = types.MethodType(_condition3d_bound_training if training else _condition3d_bound, model)
    return model


# ---------------------------------------------------------------- 2x bilinear upsample + 3x3 convolution in one launch (upconv.hip)
UPCONV_MAX_WIDTH, UPCONV_MAX_HW, UPCONV_MAX_PIXELS = 128, 4096, 1 << 22      # IGS_UPCONV_MAX_*
UPCONV_CACHE = "_igs_upconv_pack"
# Per compute dtype, whether upsample_conv's no-grad call takes the native kernel (True) or the eager two lines (False).
# DESIGN.md 25 has the measurements this follows.
UPCONV_NATIVE = {torch.float32: True, torch.float16: True}
UPCONV_TRAIN_CACHE = "_igs_upconv_train_pack"
# Per compute dtype, whether upsample_conv_autograd's default-dtype call that needs a gradient takes the native forward + backward (True)
# or the eager two lines (False).  DESIGN.md 25 has the measurements this follows.
UPCONV_BWD_NATIVE = {torch.float32: False, torch.float16: True}


def _upconv_spec(fn, conv):
    """(Cin, Cout) of nn.Conv2d(Cin, Cout, 3, stride=1, padding=1) with widths <= 128, or NotImplementedError."""
    if not isinstance(conv, torch.nn.Conv2d):
        raise NotImplementedError(f"{fn}: conv must be an nn.Conv2d (got {type(conv).__name__})")
    if (tuple(conv.kernel_size), tuple(conv.stride), conv.padding, tuple(conv.dilation), conv.groups, conv.padding_mode) != \
            ((3, 3), (1, 1), (1, 1), (1, 1), 1, "zeros"):
        raise NotImplementedError(f"{fn}: conv must be Conv2d(Cin, Cout, 3, stride=1, padding=1, dilation=1, groups=1, padding_mode='zeros') "
                                  f"(got {conv})")
    if not (1 <= conv.in_channels <= UPCONV_MAX_WIDTH and 1 <= conv.out_channels <= UPCONV_MAX_WIDTH):
        raise NotImplementedError(f"{fn}: Cin and Cout must be in 1..{UPCONV_MAX_WIDTH} (got {conv.in_channels}, {conv.out_channels})")
    return conv.in_channels, conv.out_channels


def _pack_taps(W):
    """The 9 taps W[:, :, dy, dx] of W [O, I, 3, 3], dy outermost, each in pack_mlp_tile_order, one after another -- as two copies instead
    of nine packs and a cat (the training path packs every step)."""
    O, I = W.shape[:2]
    OT, KT = _tiles(O), _tiles(I)
    P = W.permute(2, 3, 0, 1).reshape(9, O, I)
    if (O, I) != (32 * OT, 32 * KT):
        Z = W.new_zeros(9, 32 * OT, 32 * KT)
        Z[:, :O, :I] = P
        P = Z
    if W.dtype == torch.float16:                 # pack_mlp_tile_order's two permutations behind a leading tap index
        return P.view(9, OT, 32, KT, 2, 2, 2, 4).permute(0, 1, 3, 4, 6, 2, 5, 7).reshape(-1)
    return P.view(9, OT, 32, KT, 4, 2, 4).permute(0, 1, 3, 4, 5, 2, 6).reshape(-1)


def _upconv_args(fn, x, conv, conv_dtype):
    """(Cin, Cout, [weight, bias]) after the checks upsample_conv and upsample_conv_autograd share."""
    Cin, Cout = _upconv_spec(fn, conv)
    if x.dim() != 4 or x.shape[1] != Cin:
        raise ValueError(f"{fn}: x must be [N, {Cin}, H, W] (got {list(x.shape)})")
    params = [conv.weight, conv.bias]
    if x.dtype not in FEATURE_DTYPES or any(p is not None and p.dtype not in FEATURE_DTYPES for p in params):
        raise NotImplementedError(f"{fn}: x and conv's parameters must be float32 or float16 (got {x.dtype}, {conv.weight.dtype})")
    if conv_dtype is not None and conv_dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: conv_dtype must be float32 or float16 (got {conv_dtype})")
    return Cin, Cout, params


def pack_upsample_conv(conv, dtype=torch.float32, transposed=False):
    """(wpack in `dtype`, bpack float32 [128]) as igs_upconv_fwd takes them (include/igs_rast.h) from conv = nn.Conv2d(Cin, Cout, 3,
    padding=1): the 9 taps weight[:, :, dy, dx], dy outermost, each a Linear [Cout, Cin] in pack_mlp_tile_order, one after another;
    the bias zero-padded (an absent bias: zeros).  transposed=True: (wpack, bpack, wpack_t), wpack_t the same layout of the [Cin, Cout, 3, 3]
    convolution weight_t[c, o, dy, dx] = weight[o, c, 2 - dy, 2 - dx] that igs_upconv_bwd takes.  Plain tensor ops."""
    W = conv.weight.detach().to(dtype)
    wpack = _pack_taps(W)
    bpack = torch.zeros(UPCONV_MAX_WIDTH, dtype=torch.float32, device=wpack.device)
    if conv.bias is not None:
        bpack[:W.shape[0]] = conv.bias.detach().float()
    if transposed:
        return wpack, bpack, _pack_taps(W.flip(2, 3).transpose(0, 1))
    return wpack, bpack


def upsample_conv(x, conv, packed=None, conv_dtype=None):
    """conv(F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)) for conv = nn.Conv2d(Cin, Cout, 3, stride=1,
    padding=1), the motion features' step between the transformer and condition3D (IGS.py:132-134), in one launch without storing the
    upsampled map (igs_upconv_fwd, upconv.hip).  x [N, Cin, H, W] float32 / float16 (plane-contiguous NCHW, slices of n and c included,
    is read in place; channels-last and anything else is copied first); out [N, Cout, 2H, 2W] NCHW-contiguous in conv_dtype:
    torch.float32 (float32 interpolation, one float32 fma chain per output) or torch.float16 (the upsampled value and the weights in
    half, float32 accumulation, one rounding of the result); default float16 under autocast to half, float32 otherwise -- the dtype
    the eager convolution returns.  The packed weights (pack_upsample_conv) are kept on the module and rebuilt when weight's or bias's
    _version, data_ptr, dtype or device changes; `packed` overrides them.

    With grad enabled and x or a parameter of conv requiring it the result is the eager two lines, with autograd: there is no native
    backward.  So it is, for the default conv_dtype, where UPCONV_NATIVE[conv_dtype] is False (an explicit conv_dtype always takes the
    kernel).  Another Conv2d configuration or a width above 128 raises
    NotImplementedError, as do bfloat16 / float64; a CPU tensor raises RuntimeError (no CPU fallback); a wrong rank ValueError."""
    fn = "upsample_conv"
    Cin, Cout, params = _upconv_args(fn, x, conv, conv_dtype)
    if torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params)):
        return conv(torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))
    if not (x.is_cuda and all(p is None or p.is_cuda for p in params)):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    routed = conv_dtype is None                  # the default dtype goes where UPCONV_NATIVE sends it; an explicit one is always native
    if routed:
        conv_dtype = torch.float16 if _autocast_half(fn, x) else torch.float32
    N, _, H, W = x.shape
    if not (1 <= H <= UPCONV_MAX_HW and 1 <= W <= UPCONV_MAX_HW and N * H * W <= UPCONV_MAX_PIXELS):
        raise NotImplementedError(f"{fn}: sizes out of range (1 <= H, W <= {UPCONV_MAX_HW}, N * H * W <= 2^22; got {list(x.shape)})")
    if routed and not UPCONV_NATIVE[conv_dtype]:
        return conv(torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))
    if packed is None:
        key = (_param_key(params), conv_dtype)
        cache = conv.__dict__.get(UPCONV_CACHE)
        if cache is None or cache["key"] != key:
            cache = dict(key=key, pack=pack_upsample_conv(conv, conv_dtype))
            conv.__dict__[UPCONV_CACHE] = cache
        packed = cache["pack"]
    wpack, bpack = packed
    if wpack.dtype != conv_dtype:
        raise ValueError(f"{fn}: packed holds {wpack.dtype} weights, conv_dtype is {conv_dtype}")
    if not _plane_contiguous(x) or x.stride(0) < 0 or x.stride(1) < 0:
        x = x.contiguous()
    return _ext()._upconv.upconv_fwd(x, wpack, bpack, Cout)


class _UpsampleConv(torch.autograd.Function):
    """igs_upconv_fwd with igs_upconv_bwd behind it.  Saves x as it was handed over (not a copy, not the upsampled map) and wpack_t."""

    @staticmethod
    def forward(ctx, x, weight, bias, wpack, bpack, wpack_t):
        ctx.save_for_backward(x, wpack_t)
        ctx.param_dtypes = (weight.dtype, None if bias is None else bias.dtype)
        return _ext()._upconv.upconv_fwd(_upconv_readable(x), wpack, bpack, weight.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, wpack_t = ctx.saved_tensors
        want_x, want_w, want_b = ctx.needs_input_grad[:3]
        if g.dtype != wpack_t.dtype:
            g = g.to(wpack_t.dtype)
        if not g.is_contiguous():
            g = g.contiguous()                   # (the one copy of a strided d out)
        dx, dw, db = _ext()._upconv.upconv_bwd(_upconv_readable(x), wpack_t, g, want_x, want_w, want_b)
        wdt, bdt = ctx.param_dtypes              # accumulated in float32, cast once
        if dw is not None and dw.dtype != wdt:
            dw = dw.to(wdt)
        if db is not None and db.dtype != bdt:
            db = db.to(bdt)
        return dx, dw, db, None, None, None


def _upconv_readable(x):
    """x where the kernels read it in place (plane-contiguous NCHW, slices of n and c included), a contiguous copy otherwise."""
    return x.contiguous() if not _plane_contiguous(x) or x.stride(0) < 0 or x.stride(1) < 0 else x


def upsample_conv_autograd(x, conv, packed=None, conv_dtype=None):
    """upsample_conv for training: the same checks, sizes, dtypes and value, and a native backward.  When grad is disabled or neither x
    nor a parameter of conv requires it this IS upsample_conv(x, conv, packed, conv_dtype).  Otherwise the forward is igs_upconv_fwd and
    the backward igs_upconv_bwd (upconv_bwd.hip): dx in x's dtype, weight.grad and bias.grad accumulated in float32 and cast once to the
    parameters' dtype; x itself and the transposed pack are saved, the upsampled map is recomputed.  Once differentiable, deterministic.
    Under CUDA autocast to float16 the compute dtype and the output are half (bfloat16 autocast raises).  A conv without a bias works.
    `packed`, if given, is pack_upsample_conv(conv, conv_dtype, transposed=True); otherwise the three packs are kept on the module under
    UPCONV_TRAIN_CACHE and rebuilt when weight's or bias's _version, data_ptr, dtype or device changes (every optimiser step).

    The default conv_dtype goes where UPCONV_BWD_NATIVE[conv_dtype] sends it: False is the eager two lines with autograd (an explicit
    conv_dtype always takes the kernels).  Refusals as upsample_conv's; there is no CPU fallback."""
    fn = "upsample_conv_autograd"
    Cin, Cout, params = _upconv_args(fn, x, conv, conv_dtype)
    if not (torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params))):
        return upsample_conv(x, conv, packed=None if packed is None else tuple(packed[:2]), conv_dtype=conv_dtype)
    if not (x.is_cuda and all(p is None or p.is_cuda for p in params)):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    routed = conv_dtype is None
    if routed:
        conv_dtype = torch.float16 if _autocast_half(fn, x) else torch.float32
    N, _, H, W = x.shape
    if not (1 <= H <= UPCONV_MAX_HW and 1 <= W <= UPCONV_MAX_HW and N * H * W <= UPCONV_MAX_PIXELS):
        raise NotImplementedError(f"{fn}: sizes out of range (1 <= H, W <= {UPCONV_MAX_HW}, N * H * W <= 2^22; got {list(x.shape)})")
    if routed and not UPCONV_BWD_NATIVE[conv_dtype]:
        return conv(torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False))
    if packed is None:
        key = (_param_key(params), conv_dtype)
        cache = conv.__dict__.get(UPCONV_TRAIN_CACHE)
        if cache is None or cache["key"] != key:
            cache = dict(key=key, pack=pack_upsample_conv(conv, conv_dtype, transposed=True))
            conv.__dict__[UPCONV_TRAIN_CACHE] = cache
        packed = cache["pack"]
    if len(packed) != 3:
        raise ValueError(f"{fn}: packed must be pack_upsample_conv(conv, conv_dtype, transposed=True)")
    wpack, bpack, wpack_t = packed
    if wpack.dtype != conv_dtype or wpack_t.dtype != conv_dtype:
        raise ValueError(f"{fn}: packed holds {wpack.dtype} weights, conv_dtype is {conv_dtype}")
    return _UpsampleConv.apply(x, conv.weight, conv.bias, wpack, bpack, wpack_t)


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


# ---------------------------------------------------------------- the residual decoder (mlp.hip)
MLP_MAX_WIDTH, MLP_MAX_HIDDEN, MLP_MAX_HEADS = 128, 3, 8        # IGS_MLP_MAX_*
MLP_ACTIVATIONS = {"silu": 0, "relu": 1}                        # IGS_MLP_ACT_*
DECODER_MLP, DECODER_HEADS, DECODER_CACHE = "mlp_net", "out_layers", "_igs_decoder_pack"
DECODER_TRAIN_CACHE = "_igs_decoder_train_pack"


def _tiles(c):
    return (c + 31) // 32


def pack_mlp_tile_order(W):
    """One Linear's weight W [O, I] in the order mlp.hip's operands want it (include/igs_rast.h, igs_mlp_heads_fwd): a flat tensor of
    ceil(O / 32) * ceil(I / 32) tiles of 1024 elements, zero where W ends.  Plain tensor ops: works on any device."""
    O, I = W.shape
    OT, KT = _tiles(O), _tiles(I)
    P = W.new_zeros(32 * OT, 32 * KT)
    P[:O, :I] = W
    # column c of a 32-channel tile = 8 q + 4 h + p; element e = 4 q + p of lane (r, h)
    if W.dtype == torch.float16:                 # chunks of 8: [ot, kt, s, h, r, q & 1, p] with q = 2 s + (q & 1)
        return P.view(OT, 32, KT, 2, 2, 2, 4).permute(0, 2, 3, 5, 1, 4, 6).reshape(-1)
    return P.view(OT, 32, KT, 4, 2, 4).permute(0, 2, 3, 4, 1, 5).reshape(-1)      # chunks of 4: [ot, kt, q, h, r, p]


def pack_mlp(weights, biases, head_weights, head_biases, transposed=False, dtype=None):
    """(wpack in the weights' dtype, bpack float32 [layers, 128]) for mlp_heads: the hidden Linears, then the heads as one Linear.
    transposed=True: (wpack, bpack, wpack_t), wpack_t the same Linears transposed, which the backward's dgrad chain reads
    (mlp_heads_autograd).  dtype: pack the weights in this dtype instead of their own (float16 under autocast)."""
    Ws = list(weights) + [torch.cat(list(head_weights), 0)]
    if dtype is not None:
        Ws = [w.detach().to(dtype) for w in Ws]
    hb = [b if b is not None else w.new_zeros(w.shape[0]) for w, b in zip(head_weights, head_biases)]
    bs = list(biases) + [torch.cat(hb, 0)]
    wpack = torch.cat([pack_mlp_tile_order(w.detach()) for w in Ws])
    bpack = torch.zeros(len(Ws), MLP_MAX_WIDTH, dtype=torch.float32, device=wpack.device)
    for l, b in enumerate(bs):
        if b is not None:
            bpack[l, :b.shape[0]] = b.detach().float()
    if transposed:
        return wpack.contiguous(), bpack, torch.cat([pack_mlp_tile_order(w.detach().t()) for w in Ws]).contiguous()
    return wpack.contiguous(), bpack


def _mlp_checks(fn, x, weights, biases, head_weights, head_biases, activation, act_after, train=False, autocast=False):
    """Every refusal of the decoder that does not need the module; returns (widths, act_after, head_widths).  train: the caller has a
    backward, so requiring grad is no refusal; autocast: x and the parameters are cast to half, so they need not share a dtype."""
    weights, biases, head_weights, head_biases = list(weights), list(biases), list(head_weights), list(head_biases)
    if activation not in MLP_ACTIVATIONS:
        raise NotImplementedError(f"{fn}: activation must be one of {sorted(MLP_ACTIVATIONS)} (got {activation!r})")
    if len(biases) != len(weights) or len(head_biases) != len(head_weights):
        raise ValueError(f"{fn}: one bias (or None) per weight")
    if len(weights) > MLP_MAX_HIDDEN:
        raise NotImplementedError(f"{fn}: at most {MLP_MAX_HIDDEN} hidden Linears (got {len(weights)})")
    if not 1 <= len(head_weights) <= MLP_MAX_HEADS:
        raise NotImplementedError(f"{fn}: between 1 and {MLP_MAX_HEADS} heads (got {len(head_weights)})")
    act_after = [1] * len(weights) if act_after is None else [int(bool(a)) for a in act_after]
    if len(act_after) != len(weights):
        raise ValueError(f"{fn}: act_after needs one flag per hidden Linear")
    if x.dim() != 2:
        raise ValueError(f"{fn}: x must be [N, C] (got {list(x.shape)})")
    params = [(w, b) for w, b in zip(weights + head_weights, biases + head_biases)]
    width = x.shape[1]
    widths = [width]
    for i, (w, b) in enumerate(params):
        head = i >= len(weights)
        if w.dim() != 2 or w.shape[1] != width or (b is not None and tuple(b.shape) != (w.shape[0],)):
            raise ValueError(f"{fn}: {'head' if head else 'hidden'} Linear {i - len(weights) if head else i} has weight {list(w.shape)}"
                             f"{'' if b is None else ' and bias ' + str(list(b.shape))} for an input of {width} channels")
        if not head:
            width = w.shape[0]
            widths.append(width)
    head_widths = [w.shape[0] for w in head_weights]
    if min(widths + head_widths) < 1 or max(widths) > MLP_MAX_WIDTH or sum(head_widths) > MLP_MAX_WIDTH:
        raise NotImplementedError(f"{fn}: every width and the heads' sum must be in 1..{MLP_MAX_WIDTH} (widths {widths}, heads {head_widths})")
    tensors = [t for pair in params for t in pair if t is not None]
    if x.dtype not in FEATURE_DTYPES:
        raise NotImplementedError(f"{fn}: x must be float32 or float16 (got {x.dtype})")
    for t in tensors:
        if t.dtype != x.dtype and not (autocast and t.dtype in FEATURE_DTYPES):
            raise NotImplementedError(f"{fn}: x and every parameter must share a dtype (got {x.dtype} and {t.dtype})")
    if not train and torch.is_grad_enabled() and any(t.requires_grad for t in [x] + tensors):
        raise NotImplementedError(f"{fn}: forward only -- call it under torch.no_grad(), and train with the PyTorch lines")
    if not all(t.is_cuda for t in [x] + tensors):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    return widths, act_after, head_widths


def _mlp_launch(x, wpack, bpack, widths, act_after, head_widths, activation):
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()                       # a channel-strided x is copied; a row-strided one is read in place
    return tuple(_ext()._mlp.mlp_heads_fwd(x, wpack, bpack, widths, act_after, head_widths, MLP_ACTIVATIONS[activation]))


def mlp_heads(x, weights, biases, head_weights, head_biases, activation="silu", act_after=None, packed=None):
    """A tuple of contiguous [N, ch] tensors in x's dtype, one per head: h = x; h = act(h W_l^T + b_l) for every hidden Linear l
    (act_after[l] false: no activation behind that one; default all true); head k = h Wh_k^T + bh_k.  One launch, forward only.

    x [N, C0] float32 / float16 with any row stride (a channel-strided x is copied first); weights[l] [C_{l+1}, C_l] and head_weights[k]
    [ch_k, C_L] as nn.Linear keeps them, each bias [out] or None, all in x's dtype; at most 3 hidden Linears and 8 heads, every width and
    the heads' sum at most 128.  packed = pack_mlp(weights, biases, head_weights, head_biases) skips the packing, which otherwise runs
    on every call (a handful of small tensor ops); decode_residual_feature keeps it on the module."""
    fn = "mlp_heads"
    widths, act_after, head_widths = _mlp_checks(fn, x, weights, biases, head_weights, head_biases, activation, act_after)
    wpack, bpack = packed if packed is not None else pack_mlp(weights, biases, head_weights, head_biases)
    return _mlp_launch(x, wpack, bpack, widths, act_after, head_widths, activation)


class _MlpHeadsFn(torch.autograd.Function):
    """mlp_heads with the native backward (igs_mlp_heads_bwd).  Saved: x and the three packs; the forward is recomputed from x."""

    @staticmethod
    def forward(ctx, x, spec, packs, *params):
        widths, act_after, head_widths, activation = spec
        wpack, bpack, wpack_t = packs
        outs = _ext()._mlp.mlp_heads_fwd(x, wpack, bpack, widths, act_after, head_widths, MLP_ACTIVATIONS[activation])
        ctx.save_for_backward(x, wpack, bpack, wpack_t)
        ctx.spec = spec
        ctx.param_meta = [None if p is None else (p.dtype, tuple(p.shape)) for p in params]
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        x, wpack, bpack, wpack_t = ctx.saved_tensors
        widths, act_after, head_widths, activation = ctx.spec
        n, nh, meta = len(widths) - 1, len(head_widths), ctx.param_meta
        need = ctx.needs_input_grad[3:]                      # weights, biases, head weights, head biases, as mlp_heads_autograd lists them
        is_w = [True] * n + [False] * n + [True] * nh + [False] * nh
        want_x = ctx.needs_input_grad[0]
        want_w = any(nd and w for nd, w in zip(need, is_w))
        want_b = any(nd and not w for nd, w in zip(need, is_w))
        douts = [None if g is None else g.to(x.dtype).contiguous() for g in gouts]       # (a non-contiguous gradient is copied once)
        dx, dw, db = _ext()._mlp.mlp_heads_bwd(x, wpack, wpack_t, bpack, widths, act_after, head_widths, MLP_ACTIVATIONS[activation], douts,
                                               want_x, want_w, want_b)
        outs_w = [widths[l + 1] for l in range(n)] + list(head_widths)
        ins_w = list(widths[:n]) + [widths[-1]] * nh
        gw, gb, wo, bo = [], [], 0, 0
        for O, I in zip(outs_w, ins_w):
            gw.append(None if dw is None else dw[wo:wo + O * I].view(O, I))
            gb.append(None if db is None else db[bo:bo + O])
            wo, bo = wo + O * I, bo + O
        flat = gw[:n] + gb[:n] + gw[n:] + gb[n:]
        grads = [g.to(m[0]) if (nd and m is not None and g is not None) else None for g, nd, m in zip(flat, need, meta)]
        return (dx, None, None) + tuple(grads)


def _mlp_train_launch(x, params, packs, widths, act_after, head_widths, activation):
    if packs[0].dtype != x.dtype:
        x = x.to(packs[0].dtype)                  # (autocast; autograd casts the gradient back)
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()                       # a channel-strided x is copied; a row-strided one is read, and saved, in place
    return _MlpHeadsFn.apply(x, (list(widths), list(act_after), list(head_widths), activation), packs, *params)


def mlp_heads_autograd(x, weights, biases, head_weights, head_biases, activation="silu", act_after=None, packed=None):
    """mlp_heads with a native backward: the same checks, sizes and return value, but gradients reach x and every weight and bias that
    requires them, in that tensor's dtype (accumulated in float32 and rounded once for half parameters).  Nothing of N rows is kept
    for the backward but x: the forward is recomputed in chunks (igs_mlp_heads_bwd), deterministically and without float atomics.  A
    head that took no part in the loss costs nothing; d x is not computed when only parameters require grad, and the parameter
    gradients are not when only x does.  Under CUDA autocast to float16, x and the packed weights are cast to half and the outputs
    are half, as eager nn.Linear gives; the gradients of float32 parameters come back float32.  bfloat16 autocast raises
    NotImplementedError.  packed = pack_mlp(..., transposed=True) skips the packing.  Not twice differentiable."""
    fn = "mlp_heads_autograd"
    half = _autocast_half(fn, x)
    widths, act_after, head_widths = _mlp_checks(fn, x, weights, biases, head_weights, head_biases, activation, act_after, train=True, autocast=half)
    if packed is None:
        packed = pack_mlp(weights, biases, head_weights, head_biases, transposed=True, dtype=torch.float16 if half else None)
    wpack, bpack, wpack_t = packed
    params = list(weights) + list(biases) + list(head_weights) + list(head_biases)
    return _mlp_train_launch(x, params, (wpack, bpack, wpack_t), widths, act_after, head_widths, activation)


def _decoder_spec(renderer, fn):
    """(hidden Linears, act_after, activation name, head Linears, keys) of a GS3DRenderer-shaped object, or NotImplementedError."""
    nn = torch.nn
    cfg = renderer.cfg
    keys = list(cfg.feature_channels.keys())
    heads = list(getattr(renderer, DECODER_HEADS))
    if len(heads) != len(keys) or not all(isinstance(m, nn.Linear) for m in heads):
        raise NotImplementedError(f"{fn}: {DECODER_HEADS} must hold one nn.Linear per entry of cfg.feature_channels")
    linears, act_after, kinds = [], [], set()
    if cfg.mlp_network_config is not None:
        mlp = getattr(renderer, DECODER_MLP)
        oa = getattr(mlp, "output_activation", None)
        probe = torch.zeros(1)
        if not (oa is None or isinstance(oa, nn.Identity) or (callable(oa) and oa(probe) is probe)):
            raise NotImplementedError(f"{fn}: an output_activation other than the identity is not supported")
        mods = list(mlp.layers)
        for i, m in enumerate(mods):
            if i % 2 == 0 and isinstance(m, nn.Linear):
                linears.append(m)
                act_after.append(0)
            elif i % 2 == 1 and isinstance(m, (nn.SiLU, nn.ReLU)):
                act_after[-1] = 1
                kinds.add("silu" if isinstance(m, nn.SiLU) else "relu")
            else:
                raise NotImplementedError(f"{fn}: the MLP must alternate nn.Linear and nn.SiLU / nn.ReLU (entry {i} is {type(m).__name__})")
        if not linears:
            raise NotImplementedError(f"{fn}: the MLP has no Linear")
    if len(kinds) > 1:
        raise NotImplementedError(f"{fn}: mixed activations ({sorted(kinds)}) are not supported")
    if len(linears) > MLP_MAX_HIDDEN:
        raise NotImplementedError(f"{fn}: at most {MLP_MAX_HIDDEN} Linears in the MLP (got {len(linears)})")
    if not 1 <= len(heads) <= MLP_MAX_HEADS:
        raise NotImplementedError(f"{fn}: between 1 and {MLP_MAX_HEADS} output layers (got {len(heads)})")
    widths = [m.in_features for m in linears + heads[:1]] + [m.out_features for m in linears]
    if max(widths) > MLP_MAX_WIDTH or sum(m.out_features for m in heads) > MLP_MAX_WIDTH:
        raise NotImplementedError(f"{fn}: every width and the output layers' sum must be at most {MLP_MAX_WIDTH}")
    width = linears[0].in_features if linears else heads[0].in_features
    for m in linears:
        if m.in_features != width:
            raise NotImplementedError(f"{fn}: the Linears' widths do not chain")
        width = m.out_features
    if any(m.in_features != width for m in heads):
        raise NotImplementedError(f"{fn}: every output layer must read the MLP's {width} channels")
    return linears, act_after, (kinds.pop() if kinds else "silu"), heads, keys


def _child(m, name):
    """A submodule by dictionary lookup (nn.Module.__getattr__ is the slow way round), any other attribute as usual."""
    mods = m.__dict__.get("_modules")
    return mods[name] if mods is not None and name in mods else getattr(m, name, None)


def _structure_key(renderer):
    """The objects _decoder_spec looks at and the feature keys: the same objects give the same spec (the cache keeps them alive)."""
    cfg = renderer.cfg
    heads = _child(renderer, DECODER_HEADS)
    objs = [heads] + list(heads._modules.values())
    if cfg.mlp_network_config is not None:
        mlp = _child(renderer, DECODER_MLP)
        layers = _child(mlp, "layers")
        objs += [mlp, layers, _child(mlp, "output_activation")] + list(layers._modules.values())
    return objs, tuple(cfg.feature_channels)


def _same_objects(a, b):
    return a[1] == b[1] and len(a[0]) == len(b[0]) and all(x is y for x, y in zip(a[0], b[0]))


def decode_residual_feature(renderer, residual_feat, bbox=None, radius=None):
    """GS3DRenderer.decode_residual_feature (gs.py:858-869): {key: [N, ch]} in cfg.feature_channels' order, from renderer.mlp_net.layers
    (no MLP when cfg.mlp_network_config is None) and renderer.out_layers, in one launch.  Kept on the module: the validated structure,
    reused while the same module objects are in place, and the packed weights with the checked sizes, rebuilt when a parameter's
    _version, data_ptr, dtype or device changes; a call that finds both unchanged checks the input only.  Forward only: under enabled grad
    with anything that requires grad it raises NotImplementedError.  With B > 1 examples the unsplit interpolation buffer can be decoded
    once and the results split."""
    fn = "decode_residual_feature"
    x = residual_feat
    cache = renderer.__dict__.get(DECODER_CACHE)
    structure = _structure_key(renderer)
    if cache is None or not _same_objects(cache["structure"], structure):
        cache = dict(structure=structure, spec=_decoder_spec(renderer, fn), key=None)
    linears, act_after, activation, heads, keys = cache["spec"]
    params = [m._parameters[n] for n in ("weight", "bias") for m in linears + heads]
    key = _param_key(params)
    if not (cache["key"] == key and x.dim() == 2 and x.shape[1] == cache["widths"][0] and x.dtype == cache["dtype"] and x.is_cuda
            and not (torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params)))):
        n = len(linears)
        ws, bs, hws, hbs = params[:n], params[len(params) // 2:len(params) // 2 + n], params[n:len(params) // 2], params[len(params) // 2 + n:]
        widths, act_after, head_widths = _mlp_checks(fn, x, ws, bs, hws, hbs, activation, act_after)          # every refusal is raised here
        if cache["key"] != key:
            cache.update(key=key, pack=pack_mlp(ws, bs, hws, hbs))
        cache.update(widths=widths, act_after=act_after, head_widths=head_widths, dtype=x.dtype)
        renderer.__dict__[DECODER_CACHE] = cache             # (only after every check has passed: a refusal leaves the module as it was)
    wpack, bpack = cache["pack"]
    outs = _mlp_launch(x, wpack, bpack, cache["widths"], cache["act_after"], cache["head_widths"], activation)
    return dict(zip(keys, outs))


def decode_residual_feature_train(renderer, residual_feat, bbox=None, radius=None):
    """decode_residual_feature for a module that is trained.  With grad off, or nothing requiring grad, it is decode_residual_feature
    (the same cache, the same bits).  Otherwise the outputs carry the native backward of mlp_heads_autograd; the forward and transposed
    packs are kept on the module under the same rule (rebuilt when a parameter's _version, data_ptr, dtype or device changes, i.e. once
    per optimiser step), separately for float16 autocast."""
    fn = "decode_residual_feature_train"
    x = residual_feat
    cache = renderer.__dict__.get(DECODER_TRAIN_CACHE)
    structure = _structure_key(renderer)
    if cache is None or not _same_objects(cache["structure"], structure):
        cache = dict(structure=structure, spec=_decoder_spec(renderer, fn), key=None)
    linears, act_after, activation, heads, keys = cache["spec"]
    params = [m._parameters[n] for n in ("weight", "bias") for m in linears + heads]
    if not (torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params))):
        return decode_residual_feature(renderer, residual_feat, bbox, radius)
    n, half = len(linears), _autocast_half(fn, x)
    m = len(params) // 2
    ws, hws, bs, hbs = params[:n], params[n:m], params[m:m + n], params[m + n:]
    widths, act_after, head_widths = _mlp_checks(fn, x, ws, bs, hws, hbs, activation, act_after, train=True, autocast=half)
    key = (_param_key(params), half)
    if cache["key"] != key:
        cache.update(key=key, pack=pack_mlp(ws, bs, hws, hbs, transposed=True, dtype=torch.float16 if half else None))
    renderer.__dict__[DECODER_TRAIN_CACHE] = cache               # (only after every check has passed)
    outs = _mlp_train_launch(x, ws + bs + hws + hbs, cache["pack"], widths, act_after, head_widths, activation)
    return dict(zip(keys, outs))


def use_native_decoder(renderer, training=False):
    """Binds decode_residual_feature on this GS3DRenderer instance; state_dict() keys and the class are untouched.  Returns the number of
    Linears taken over (5 for the shipped config).  Raises NotImplementedError, before anything is changed, when the MLP is not nn.Linear
    and nn.SiLU / nn.ReLU alternating, mixes activations, has an output_activation, more than 3 Linears or a width above 128.
    training=True binds decode_residual_feature_train instead, which has a backward; the default binds the forward-only method."""
    import types
    linears, _, _, heads, _ = _decoder_spec(renderer, "use_native_decoder")
    renderer.decode_residual_feature = types.MethodType(decode_residual_feature_train if training else decode_residual_feature, renderer)
    return len(linears) + len(heads)
