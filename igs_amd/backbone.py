"""The non-GEMM steps of the unimatch CNN encoder on the MI355X-native library (igs_amd/csrc/inorm.hip, include/igs_rast.h).

IGS._forward_v3 -> UniMatch.forward -> CNNEncoder (igs/models/unimatch/backbone.py) runs for every streamed frame and holds the largest
activations of the network.  Its 15 nn.InstanceNorm2d layers (affine = False, no running statistics, eps 1e-5), the in-place ReLU behind
each, the residual add of every ResidualBlock and the norm of its downsample branch are `instance_norm` and `residual_tail`: one launch
per norm that reads the plane once and writes it once.  `feature_add_position` (igs/models/unimatch/utils.py:111-131) is one launch for
both features.  The convolutions stay with PyTorch.  Two calls bind them into the reference's model:

    import igs.models.unimatch.unimatch as U
    igs_amd.backbone.use_native_encoder_norms(model.backbone)        # the CNNEncoder: 15 norms
    igs_amd.backbone.use_native_position(U)                          # the module that did `from .utils import feature_add_position`

Forward only: the backbone is frozen in IGS (igs/IGS.py:76-77: requires_grad_(False), eval()) and its inputs are images, so no backward
is provided; an input that requires grad while grad is enabled raises NotImplementedError.  There is no CPU and no PyTorch fallback: CPU
tensors raise RuntimeError, bfloat16 / float64 / mixed dtypes raise NotImplementedError, wrong ranks, mismatching shapes and H * W < 2
raise ValueError.  Not provided: affine or running-statistics instance norm, the BatchNorm / GroupNorm variants of the encoder.
"""
import types

import torch
import torch.nn as nn

from ._cabi import ext as _ext

DTYPES = (torch.float32, torch.float16)
PLAIN, RELU, RELU_ADD_RELU, RELU_ADDNORM_RELU = 0, 1, 2, 3          # IGS_INORM_* (include/igs_rast.h)

# The attributes of the reference's ResidualBlock and CNNEncoder that the bound forwards touch, as igs/models/unimatch/backbone.py names them
BLOCK_CONV1, BLOCK_CONV2, BLOCK_NORM1, BLOCK_NORM2, BLOCK_RELU, BLOCK_DOWNSAMPLE = "conv1", "conv2", "norm1", "norm2", "relu", "downsample"
STEM_CONV, STEM_NORM, STEM_RELU = "conv1", "norm1", "relu1"
ENCODER_LAYERS = ("layer1", "layer2", "layer3")
ENCODER_OUT_CONV, ENCODER_BRANCHES, ENCODER_TRIDENT = "conv2", "num_branch", "trident_conv"
POSITION_NAME = "feature_add_position"

_FROZEN = ("the unimatch encoder is frozen in IGS (igs/IGS.py:76-77) and its inputs are images: no backward is provided; "
           "call under torch.no_grad() or detach the input")


def _check_shapes(fn, spatial, *named):
    """ValueError for (tensor, name) pairs that are not [N, C, H, W] or do not share the first one's shape."""
    like = named[0][0]
    for t, name in named:
        if t.dim() != 4:
            raise ValueError(f"{fn}: {name} must have four dimensions [N, C, H, W] (got {list(t.shape)})")
        if tuple(t.shape) != tuple(like.shape):
            raise ValueError(f"{fn}: {name} has shape {list(t.shape)}, expected {list(like.shape)}")
    if spatial and like.shape[2] * like.shape[3] < 2:
        raise ValueError(f"{fn}: Expected more than 1 spatial element (got {list(like.shape)})")


def _check(fn, spatial, *named):
    """The refusals, in an order that does not depend on where the tensors live: shapes, dtypes, grad, then the device."""
    _check_shapes(fn, spatial, *named)
    like = named[0][0]
    if any(t.dtype not in DTYPES or t.dtype != like.dtype for t, _ in named):
        raise NotImplementedError(f"{fn}: tensors must all be float32 or all float16 (got {', '.join(str(t.dtype) for t, _ in named)})")
    for t, name in named:
        if t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"{fn}: {name} requires grad, but {_FROZEN}")
    if any(not t.is_cuda or t.device != like.device for t, _ in named):
        raise RuntimeError(f"{fn}: tensors must be on one GPU (no CPU fallback)")


def instance_norm(x, *, relu=False, eps=1e-5, inplace=False):
    """F.instance_norm(x, eps=eps) without affine parameters or running statistics, then relu if asked, as one launch that reads every
    H x W plane once and writes it once.  x: [N, C, H, W] float32 or float16 on a GPU; a non-contiguous tensor (channels-last included) is
    copied once.  inplace=True writes into x when it was not copied.  Arithmetic is float32, the variance comes from centred values."""
    fn = "instance_norm"
    _check(fn, True, (x, "x"))
    xc = x.contiguous()
    return _ext()._encoder.instance_norm_fwd(xc, None, RELU if relu else PLAIN, float(eps), bool(inplace) and xc is x)


def residual_tail(y, skip, *, norm_skip=False, eps=1e-5, inplace=False):
    """relu(skip' + relu(IN(y))), the tail of a ResidualBlock (igs/models/unimatch/backbone.py:31-36) as one launch: skip' = skip for the
    identity skip, IN(skip) with norm_skip=True (the downsample branch's norm).  inplace=True writes into y when it was not copied."""
    fn = "residual_tail"
    _check(fn, True, (y, "y"), (skip, "skip"))
    yc, sc = y.contiguous(), skip.contiguous()
    if sc.data_ptr() == yc.data_ptr():                              # (relu(y + relu(IN(y))) is legitimate; the kernel's out may only alias x)
        inplace = False
    return _ext()._encoder.instance_norm_fwd(yc, sc, RELU_ADDNORM_RELU if norm_skip else RELU_ADD_RELU, float(eps), bool(inplace) and yc is y)


def feature_add_position(feature0, feature1, attn_splits, feature_channels):
    """The reference's signature (igs/models/unimatch/utils.py:111-131): both features plus the sine embedding of PositionEmbeddingSine
    (feature_channels // 2 frequencies, normalised, temperature 10000) of the position inside the attn_splits x attn_splits window, as one
    launch without the split, position and merge tensors.  Returns two new tensors."""
    fn = "feature_add_position"
    _check_shapes(fn, False, (feature0, "feature0"), (feature1, "feature1"))
    C, H, W = feature0.shape[1:]
    K = int(attn_splits)
    if int(feature_channels) != C:
        raise ValueError(f"{fn}: feature_channels = {feature_channels} is not the features' channel count {C}")
    if C % 4:
        raise ValueError(f"{fn}: the channel count must be a multiple of 4 (got {C})")
    if K < 1 or H % K or W % K:
        raise ValueError(f"{fn}: H = {H} and W = {W} do not split into {K} windows each")
    _check(fn, False, (feature0, "feature0"), (feature1, "feature1"))
    return _ext()._encoder.position_add(feature0.contiguous(), feature1.contiguous(), K, False)


def use_native_position(namespace):
    """Sets feature_add_position on `namespace`, the module object whose globals the caller looks it up in (igs.models.unimatch.unimatch does
    `from .utils import feature_add_position`, so patch that module, not unimatch.utils); returns how many names were set (1, or 0 when the
    namespace has no such name)."""
    if not hasattr(namespace, POSITION_NAME):
        return 0
    setattr(namespace, POSITION_NAME, feature_add_position)
    return 1


def _norm_ok(m):
    return isinstance(m, nn.InstanceNorm2d) and not m.affine and not m.track_running_stats


def _is_block(m):
    return all(hasattr(m, a) for a in (BLOCK_CONV1, BLOCK_CONV2, BLOCK_NORM1, BLOCK_NORM2, BLOCK_RELU, BLOCK_DOWNSAMPLE))


def _block_norms(m):
    norms = [getattr(m, BLOCK_NORM1), getattr(m, BLOCK_NORM2)]
    down = getattr(m, BLOCK_DOWNSAMPLE)
    if down is not None:
        if not (isinstance(down, nn.Sequential) and len(down) == 2):
            raise NotImplementedError("use_native_encoder_norms: a downsample branch must be Sequential(conv, norm)")
        norms.append(down[1])
    return norms


def _block_forward(self, x):
    """ResidualBlock.forward (igs/models/unimatch/backbone.py:28-36) with its norms, ReLUs and add fused; the convolutions as they are."""
    n1, n2 = getattr(self, BLOCK_NORM1), getattr(self, BLOCK_NORM2)
    y = instance_norm(getattr(self, BLOCK_CONV1)(x), relu=True, eps=n1.eps, inplace=True)
    y = getattr(self, BLOCK_CONV2)(y)
    down = getattr(self, BLOCK_DOWNSAMPLE)
    if down is None:
        return residual_tail(y, x, eps=n2.eps, inplace=True)
    if down[1].eps != n2.eps:
        raise NotImplementedError("ResidualBlock: norm2 and the downsample norm must share one eps")
    return residual_tail(y, down[0](x), norm_skip=True, eps=n2.eps, inplace=True)


def _encoder_forward(self, x):
    """CNNEncoder.forward (igs/models/unimatch/backbone.py:101-121) with the stem's norm and ReLU fused."""
    x = instance_norm(getattr(self, STEM_CONV)(x), relu=True, eps=getattr(self, STEM_NORM).eps, inplace=True)
    for name in ENCODER_LAYERS:
        x = getattr(self, name)(x)
    x = getattr(self, ENCODER_OUT_CONV)(x)
    branches = getattr(self, ENCODER_BRANCHES)
    if branches > 1:
        return getattr(self, ENCODER_TRIDENT)([x] * branches)
    return [x]


def use_native_encoder_norms(encoder):
    """Binds a new forward on every submodule of `encoder` with the ResidualBlock shape (conv1, conv2, norm1, norm2, relu, downsample =
    (conv, norm) or None) and on the encoder itself for its stem (conv1, norm1, relu1); the convolutions and, for num_branch > 1, the
    trident_conv branch are called as they are, state_dict() keys do not change.  Returns the number of norms taken over (15 for the
    shipped encoder).  Raises NotImplementedError, before anything is changed, when a norm is not nn.InstanceNorm2d with affine = False and
    track_running_stats = False."""
    fn = "use_native_encoder_norms"
    stem = all(hasattr(encoder, a) for a in (STEM_CONV, STEM_NORM, STEM_RELU) + ENCODER_LAYERS + (ENCODER_OUT_CONV, ENCODER_BRANCHES))
    if not stem:
        raise NotImplementedError(f"{fn}: {type(encoder).__name__} does not have the CNNEncoder attributes "
                                  f"({', '.join((STEM_CONV, STEM_NORM, STEM_RELU) + ENCODER_LAYERS + (ENCODER_OUT_CONV, ENCODER_BRANCHES))})")
    blocks = [m for m in encoder.modules() if m is not encoder and _is_block(m)]
    norms = [getattr(encoder, STEM_NORM)]
    for b in blocks:
        norms += _block_norms(b)
    for n in norms:
        if not _norm_ok(n):
            raise NotImplementedError(f"{fn}: every norm must be nn.InstanceNorm2d with affine=False and track_running_stats=False "
                                      f"(got {n}); the BatchNorm / GroupNorm / affine variants are not provided")
    for b in blocks:
        b.forward = types.MethodType(_block_forward, b)
    encoder.forward = types.MethodType(_encoder_forward, encoder)
    return len(norms)
