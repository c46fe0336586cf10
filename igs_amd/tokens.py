"""The per-token work of AGM-Net's two transformers, up to their GEMMs, on the MI355X-native library (igs_amd/csrc/tokens.hip,
igs_amd/csrc/gnorm.hip, include/igs_rast.h).

GridEncoder.conv is a Transformer1D of 4 BasicTransformerBlocks (igs/models/transformers.py:290-397, configs/train.yaml:168-178; dim 512,
8192 anchors per example): each runs two nn.LayerNorm(512) and a GEGLU feed-forward (transformers.py:482-506) whose chunk / gelu / multiply
go over a [B * 8192, 4096] projection.  The unimatch FeatureTransformer and FeatureTransformerMy run a TransformerLayer
(igs/models/unimatch/transformer.py:44-146) per attention: around the attention, norm1(merge(message)), with the FFN a cat, the MLP and
norm2, then `source + message`, and a three-launch `is_self_attn` test whose result attn_type = 'swin' never reads.  Here:

    layer_norm(x, weight, bias, eps, residual=None, out_dtype=None)     (residual +) LN(x) * weight + bias, one launch, one read of x
    geglu(proj)                                                         proj[..., :D] * gelu(proj[..., D:]), one launch; the backward
                                                                        writes both halves of d proj in one launch
    use_native_block_ops(grid_encoder)                                  binds norm1, norm3 and ff.net[0] of every BasicTransformerBlock
    use_native_transformer_layers(feature_transformer)                  binds the forward of every unimatch TransformerLayer
    layer_tail(attn_out, source, layer)                                 everything behind the layer's attention (merge, LN1, cat, the
                                                                        GELU MLP, LN2, the residual add) as one launch, forward only
    use_native_layer_tails(feature_transformer)                         binds a forward that takes layer_tail when nothing needs a gradient
    layer_tail_autograd(attn_out, source, layer)                        layer_tail with the recomputing native backward (ffn_bwd.hip) behind it
    project_tokens(x, weights, rot=None)                                up to five bias-free 128 -> 128 projections of x side by side in
                                                                        one buffer, one launch, forward only (proj.hip)
    project_tokens_autograd(x, weights, rot=None)                       the same launch with a native backward (proj_bwd.hip) behind it;
                                                                        returns the n results as a tuple of column slices
    use_native_layer_heads(feature_transformer)                         binds a forward whose q / k / v projections are one or two such
                                                                        launches when nothing needs a gradient, then the tail as above
    use_native_feature_transformer(transformer, bidirectional)          binds the transformer's forward: five projections of a block's
                                                                        input in one launch, the batch-swapped target never built
    group_norm_tokens(x, num_groups, weight, bias, eps)                 F.group_norm over [B, C, A] written token-major [B, A, C]: the
                                                                        statistics, then one tile-transposing launch
    add_residual_tokens(tokens, residual)                               tokens [B, A, C] + residual [B, C, A], one launch; a [B, C, A]-shaped
                                                                        view of a token-major buffer
    use_native_transformer_ends(grid_encoder)                           binds the forward of every Transformer1D: the two above around
                                                                        proj_in, the blocks and proj_out (transformers.py:860-908)

Both have autograd (Transformer1D and FeatureTransformerMy are trained); the LayerNorm saves nothing but x and recomputes the row
statistics in its backward, the GEGLU saves nothing but proj.  Both backwards are deterministic (no float atomics).  They compose with
igs_amd.attention: use_native_attention replaces the block's attention, and the bound layer forward looks the two unimatch attention
functions up, at call time, in the module that defines the layer's class, which is where use_native_window_attention sets them.

Measured on one MI355X (medians of 20 against the eager sequences): the GEGLU is 2.0-2.5 x faster in float32,
forward and with its backward, at 0.83-0.92 of the copy roof and half the peak memory; the LayerNorm forward 1.2-2.0 x, the layer tail
forward 4.1-5.4 x.  Forward + backward of the LayerNorm is launch- and overhead-bound below about 100 MB: SLOWER than eager at [8192, 512]
in both dtypes (0.79 x float32, 0.88 x float16), level for the float16 tail at [32768, 128], 1.4-2.9 x ahead at [40960, 512] and
[65536, 128].  A whole block gains 2-5 %, a whole layer 1-5 %, within the spread of the measurement.

There is no CPU and no PyTorch fallback: CPU tensors raise RuntimeError, bfloat16 / float64 raise NotImplementedError, wrong shapes raise
ValueError.

The ends of Transformer1D: the GroupNorm keeps its [B, G, 2] statistics for a deterministic backward (per-tile
partial sums added in tile order); the residual add's backward launches nothing.  The bound Transformer1D returns the reference's shape,
dtype and values as a permuted view of a token-major buffer, so GridEncoder.forward's own permute(0, 2, 1) yields the contiguous
[B, A, C] that interpolate_anchor_features reads in place.  The work is launch-bound at the shipped sizes: no speed-up is claimed beyond
the figures of section 20.

Not provided: norm types other than nn.GroupNorm with affine parameters at the ends of Transformer1D, gradient checkpointing and 2-D
attention masks there, fusing proj_in / proj_out; the GELU inside the unimatch MLP (a single eager kernel
already) and splitting the MLP's first weight to avoid the cat outside layer_tail (which does both); a double backward
of layer_tail or project_tokens_autograd, d_model other than 128 and biases there; bfloat16; fusing any other GEMM; the ada
norms, cross-attention (norm2 / attn2) and the other feed-forward activations of BasicTransformerBlock; attn_type other than 'swin' and
nhead > 1 of TransformerLayer.
"""
import sys
import types

import torch
import torch.nn as nn

from ._binding import autocast_half, param_key
from ._cabi import ext as _ext
from .motion import pack_mlp_tile_order

DTYPES = (torch.float32, torch.float16)
LN_MAX_C = 1024                                                    # IGS_LN_MAX_C (include/igs_rast.h)
GEGLU_MAX_D = 8192                                                 # IGS_GEGLU_MAX_D
GN_MAX_C = 1024                                                    # IGS_GN_MAX_C
GN_MAX_TOKENS = 1 << 24                                            # IGS_GN_MAX_TOKENS: B * A
GN_MAX_GROUP_ELEMS = 1 << 30                                       # IGS_GN_MAX_GROUP_ELEMS: (C / G) * A

# The attributes of the reference's BasicTransformerBlock, FeedForward and GEGLU that the installer touches, as igs/models/transformers.py
# names them (the classes come from diffusers, which is not part of this stack)
BLOCK_NORM1, BLOCK_NORM2, BLOCK_NORM3, BLOCK_ATTN1, BLOCK_ATTN2, BLOCK_FF = "norm1", "norm2", "norm3", "attn1", "attn2", "ff"
BLOCK_ADA_FLAGS = ("use_ada_layer_norm", "use_ada_layer_norm_zero", "use_ada_layer_norm_continuous")
FF_NET, GEGLU_PROJ = "net", "proj"
GELU_ONLY_ATTRS = ("approximate",)                                 # what GELU has and GEGLU has not
# ... and of the unimatch TransformerLayer (igs/models/unimatch/transformer.py:11-42) with the two functions its forward calls
LAYER_Q, LAYER_K, LAYER_V, LAYER_MERGE, LAYER_NORM1, LAYER_NO_FFN, LAYER_NHEAD = "q_proj", "k_proj", "v_proj", "merge", "norm1", "no_ffn", "nhead"
LAYER_MLP, LAYER_NORM2 = "mlp", "norm2"
ATTN_SPLIT, ATTN_FULL = "single_head_split_window_attention", "single_head_full_attention"
# ... and of Transformer1D (igs/models/transformers.py:700-784)
T1D_NORM, T1D_PROJ_IN, T1D_BLOCKS, T1D_PROJ_OUT, T1D_CHECKPOINTING = "norm", "proj_in", "transformer_blocks", "proj_out", "gradient_checkpointing"


def _rows(t):
    """t [..., C] as [N, C] with stride 1 inside a row and a row stride of at least C: a view where the strides allow it (slices of a wider
    buffer included), one copy otherwise."""
    C = t.shape[-1]
    if C == 1 or t.stride(-1) == 1:
        try:
            v = t.view(-1, C)
            if v.shape[0] <= 1 or v.stride(0) >= C:
                return v
        except RuntimeError:
            pass
    return t.contiguous().view(-1, C)


def _refuse(fn, named):
    """The refusals that do not depend on the shapes, in an order that does not depend on where the tensors live: dtypes, then the device."""
    for t, name in named:
        if t.dtype not in DTYPES:
            raise NotImplementedError(f"{fn}: {name} must be float32 or float16 (got {t.dtype})")
    like = named[0][0]
    if any(not t.is_cuda or t.device != like.device for t, _ in named):
        raise RuntimeError(f"{fn}: tensors must be on one GPU (no CPU fallback)")


class _LayerNorm(torch.autograd.Function):
    """x, residual: [N, C] rows; weight, bias: [C] float32 or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, eps, out_half):
        out = _ext()._tokens.layer_norm_fwd(x, weight, bias, eps, residual, out_half)
        ctx.save_for_backward(x, weight)                           # the view itself: nothing is copied, no statistics are kept
        ctx.eps = eps
        ctx.res_dtype = residual.dtype if residual is not None else None
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        nx, nw, nb, nr = ctx.needs_input_grad[:4]
        dx = dw = db = None
        if nx or nw or nb:
            dx, dw, db = _ext()._tokens.layer_norm_bwd(x, weight, ctx.eps, _rows(g), nx, nw and weight is not None, nb and weight is not None)
        return dx, dw, db, (g.to(ctx.res_dtype) if nr else None), None, None


def layer_norm(x, weight, bias, eps=1e-5, residual=None, out_dtype=None):
    """F.layer_norm(x, (C,), weight, bias, eps) over the last dimension, plus `residual` when given, as one launch that reads every row
    once and keeps it in registers between the statistics and the write (tokens.hip).  x: [..., C] float32 or float16 on a GPU, C <= 1024;
    rows with stride 1 on C are read in place through a row stride, anything else is copied once.  weight and bias: [C], both or neither
    (float16 parameters are widened to float32, the kernel's parameter dtype).  residual: x's shape, float32 or float16 of its own.
    out_dtype (float32 or float16) defaults to x.dtype; the result is contiguous.  Arithmetic is float32 with the variance from centred
    values; a constant row gives exactly bias (+ residual), a row with a NaN or an infinity comes out all NaN.  Autograd reaches x, weight,
    bias and residual (whose gradient is the upstream gradient itself); only x is saved, and under no_grad nothing is."""
    fn = "layer_norm"
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"{fn}: x must be [..., C] with C >= 1 (got {list(x.shape)})")
    C = x.shape[-1]
    if C > LN_MAX_C:
        raise ValueError(f"{fn}: C = {C} is above the supported {LN_MAX_C}")
    if (weight is None) != (bias is None):
        raise ValueError(f"{fn}: weight and bias go together (both or neither)")
    named = [(x, "x")]
    if weight is not None:
        for p, name in ((weight, "weight"), (bias, "bias")):
            if tuple(p.shape) != (C,):
                raise ValueError(f"{fn}: {name} has shape {list(p.shape)}, expected {[C]}")
            named.append((p, name))
    if residual is not None:
        if tuple(residual.shape) != tuple(x.shape):
            raise ValueError(f"{fn}: residual has shape {list(residual.shape)}, expected {list(x.shape)}")
        named.append((residual, "residual"))
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in DTYPES:
        raise NotImplementedError(f"{fn}: out_dtype must be float32 or float16 (got {out_dtype})")
    _refuse(fn, named)
    if weight is not None:
        weight, bias = weight.float(), bias.float()
    x2 = _rows(x)
    r2 = _rows(residual) if residual is not None else None
    half = out_dtype == torch.float16
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x2, weight, bias, r2)):
        out = _LayerNorm.apply(x2, weight, bias, r2, float(eps), half)
    else:
        out = _ext()._tokens.layer_norm_fwd(x2, weight, bias, float(eps), r2, half)
    return out.view(x.shape)


class _Geglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, proj):
        ctx.save_for_backward(proj)
        return _ext()._tokens.geglu_fwd(proj)

    @staticmethod
    def backward(ctx, g):
        (proj,) = ctx.saved_tensors
        if g.dtype != proj.dtype:
            g = g.to(proj.dtype)
        return _ext()._tokens.geglu_bwd(proj, g)


def geglu(proj):
    """hidden * gelu(gate) for hidden, gate = proj.chunk(2, dim=-1), the exact (erf) GELU: [..., 2 D] -> [..., D] contiguous in proj's dtype
    (float32 or float16), D <= 8192, as one launch that reads proj once (tokens.hip); rows with stride 1 are read in place through a row
    stride.  With autograd: only proj is saved, and the backward writes both halves of d proj in one launch, so chunk's backward (a cat)
    costs nothing."""
    fn = "geglu"
    if proj.dim() < 1 or proj.shape[-1] < 2 or proj.shape[-1] % 2:
        raise ValueError(f"{fn}: proj must be [..., 2 D] with D >= 1 (got {list(proj.shape)})")
    D = proj.shape[-1] // 2
    if D > GEGLU_MAX_D:
        raise ValueError(f"{fn}: D = {D} is above the supported {GEGLU_MAX_D}")
    _refuse(fn, [(proj, "proj")])
    p2 = _rows(proj)
    out = _Geglu.apply(p2) if torch.is_grad_enabled() and p2.requires_grad else _ext()._tokens.geglu_fwd(p2)
    return out.view(proj.shape[:-1] + (D,))


def _autocast_out_dtype(default):
    """float32 whenever GPU autocast is enabled, whatever its dtype: layer_norm is on autocast's float32 list, so eager runs and answers
    in float32 there, and the bound forwards give the dtypes eager PyTorch gives."""
    return torch.float32 if torch.is_autocast_enabled() else default


# ---------------------------------------------------------------- BasicTransformerBlock: norm1, norm3, GEGLU
def _norm_forward(self, x):
    """nn.LayerNorm.forward on the native path."""
    return layer_norm(x, self.weight, self.bias, self.eps, out_dtype=_autocast_out_dtype(None))


def _geglu_forward(self, hidden_states, scale=1.0):
    """GEGLU.forward (igs/models/transformers.py:503-506): the projection as it is, then chunk, gelu and multiply as one launch."""
    return geglu(getattr(self, GEGLU_PROJ)(hidden_states))


def _is_block(m):
    return all(hasattr(m, a) for a in (BLOCK_NORM1, BLOCK_NORM2, BLOCK_NORM3, BLOCK_ATTN1, BLOCK_ATTN2, BLOCK_FF))


def _layer_norm_ok(n):
    return isinstance(n, nn.LayerNorm) and len(n.normalized_shape) == 1 and (n.weight is None) == (n.bias is None)


def _block_targets(fn, b):
    """(norm1, norm3, the feed-forward's GEGLU) of one block, or NotImplementedError."""
    for flag in BLOCK_ADA_FLAGS:
        if getattr(b, flag, False):
            raise NotImplementedError(f"{fn}: {flag} is set: the ada norms are not provided")
    for name in (BLOCK_NORM2, BLOCK_ATTN2):
        if getattr(b, name) is not None:
            raise NotImplementedError(f"{fn}: {name} is present: cross-attention blocks are not provided")
    n1, n3 = getattr(b, BLOCK_NORM1), getattr(b, BLOCK_NORM3)
    for n in (n1, n3):
        if not _layer_norm_ok(n):
            raise NotImplementedError(f"{fn}: norm1 and norm3 must be nn.LayerNorm over the last dimension with weight and bias together (got {n})")
    if n1.elementwise_affine != n3.elementwise_affine:
        raise NotImplementedError(f"{fn}: a LayerNorm without affine parameters alongside one with them is not provided")
    net = getattr(getattr(b, BLOCK_FF), FF_NET, None)
    act = net[0] if net is not None and len(net) >= 3 else None
    proj = getattr(act, GEGLU_PROJ, None)
    if (not isinstance(proj, nn.Linear) or any(hasattr(act, a) for a in GELU_ONLY_ATTRS) or not isinstance(net[2], nn.Linear)
            or proj.out_features != 2 * net[2].in_features):
        raise NotImplementedError(f"{fn}: the feed-forward activation must be GEGLU (a projection to twice the inner width); "
                                  f"gelu, gelu-approximate and geglu-approximate are not provided")
    return n1, n3, act


def use_native_block_ops(module):
    """Binds a forward on norm1, norm3 and the feed-forward's GEGLU (ff.net[0]: its proj, then `geglu`) of every BasicTransformerBlock
    under `module`, found by the attribute names above; returns the number of bound modules (3 per block, 12 for the shipped
    Transformer1D).  state_dict() keys and the classes are untouched.  Raises NotImplementedError, before anything is changed, for the ada
    norms, a LayerNorm without affine parameters alongside one with, a feed-forward activation other than GEGLU, and norm2 / attn2
    present.  Under float16 autocast the bound norms answer in float32 and the GEGLU in the projection's dtype, as eager PyTorch does."""
    fn = "use_native_block_ops"
    targets = [_block_targets(fn, m) for m in module.modules() if _is_block(m)]
    n = 0
    for n1, n3, act in targets:
        n1.forward = types.MethodType(_norm_forward, n1)
        n3.forward = types.MethodType(_norm_forward, n3)
        act.forward = types.MethodType(_geglu_forward, act)
        n += 3
    return n


# ---------------------------------------------------------------- the unimatch TransformerLayer
def _layer_served(self, attn_type):
    fn = "TransformerLayer"
    if attn_type != "swin":
        raise NotImplementedError(f"{fn}: attn_type = {attn_type!r} is not provided (IGS uses 'swin' only)")
    if getattr(self, LAYER_NHEAD) > 1:
        raise NotImplementedError(f"{fn}: nhead > 1 is not provided")


def _layer_attention(self, query, key, value, height, width, shifted_window_attn_mask, with_shift, attn_num_splits):
    """The attention function of the layer's own module, looked up now, so whatever use_native_window_attention set there is used."""
    namespace = sys.modules[type(self).__module__]
    if attn_num_splits is not None and attn_num_splits > 1:
        return getattr(namespace, ATTN_SPLIT)(query, key, value, num_splits=attn_num_splits, with_shift=with_shift, h=height, w=width,
                                              attn_mask=shifted_window_attn_mask)
    return getattr(namespace, ATTN_FULL)(query, key, value)


def _layer_message(self, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits):
    """The three projections and the attention: the input of the layer's tail."""
    _layer_served(self, attn_type)
    query, key, value = getattr(self, LAYER_Q)(source), getattr(self, LAYER_K)(target), getattr(self, LAYER_V)(target)
    return _layer_attention(self, query, key, value, height, width, shifted_window_attn_mask, with_shift, attn_num_splits)


def _layer_tail_unfused(self, message, source):
    """merge, then source + LN1(message) as one launch, or LN1, cat, mlp and source + LN2(message) as one launch."""
    message = getattr(self, LAYER_MERGE)(message)
    n1 = getattr(self, LAYER_NORM1)
    if getattr(self, LAYER_NO_FFN):
        return layer_norm(message, n1.weight, n1.bias, n1.eps, residual=source,
                          out_dtype=_autocast_out_dtype(torch.promote_types(message.dtype, source.dtype)))
    message = layer_norm(message, n1.weight, n1.bias, n1.eps, out_dtype=_autocast_out_dtype(None))
    message = getattr(self, LAYER_MLP)(torch.cat([source, message], dim=-1))
    n2 = getattr(self, LAYER_NORM2)
    return layer_norm(message, n2.weight, n2.bias, n2.eps, residual=source,
                      out_dtype=_autocast_out_dtype(torch.promote_types(message.dtype, source.dtype)))


def _layer_forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, shifted_window_attn_mask_1d=None,
                   attn_type="swin", with_shift=False, attn_num_splits=None):
    """TransformerLayer.forward (igs/models/unimatch/transformer.py:44-146) for attn_type = 'swin': the three projections, the attention
    function of the layer's own module (looked up now, so whatever use_native_window_attention set there is used), merge, then
    source + LN1(message) as one launch, or LN1, cat, mlp and source + LN2(message) as one launch.  is_self_attn is not computed: 'swin'
    never reads it."""
    message = _layer_message(self, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)
    return _layer_tail_unfused(self, message, source)


def _is_layer(m):
    return all(hasattr(m, a) for a in (LAYER_Q, LAYER_K, LAYER_V, LAYER_MERGE, LAYER_NORM1, LAYER_NO_FFN, LAYER_NHEAD))


def _checked_layers(fn, module):
    """Every unimatch TransformerLayer under `module`, or NotImplementedError for one that the bound forwards do not serve."""
    layers = [m for m in module.modules() if _is_layer(m)]
    for m in layers:
        if getattr(m, LAYER_NHEAD) > 1:
            raise NotImplementedError(f"{fn}: nhead > 1 is not provided")
        names = (LAYER_NORM1,) if getattr(m, LAYER_NO_FFN) else (LAYER_NORM1, LAYER_NORM2, LAYER_MLP)
        if not all(hasattr(m, a) for a in names):
            raise NotImplementedError(f"{fn}: a layer with an FFN must have {LAYER_MLP} and {LAYER_NORM2}")
        for a in names[:2]:
            if not _layer_norm_ok(getattr(m, a)):
                raise NotImplementedError(f"{fn}: {a} must be nn.LayerNorm over the last dimension (got {getattr(m, a)})")
    return layers


def use_native_transformer_layers(module):
    """Binds a forward on every unimatch TransformerLayer under `module`, found by q_proj, k_proj, v_proj, merge, norm1, no_ffn, nhead (and
    mlp, norm2 when it has an FFN); returns how many.  state_dict() keys and the classes are untouched.  Raises NotImplementedError, before
    anything is changed, for nhead > 1 and for norms that are not nn.LayerNorm over the last dimension; attn_type other than 'swin' raises
    at the call."""
    layers = _checked_layers("use_native_transformer_layers", module)
    for m in layers:
        m.forward = types.MethodType(_layer_forward, m)
    return len(layers)


# ---------------------------------------------------------------- the layer's tail in one launch (ffn.hip)
TAIL_D = 128                                                       # d_model: the only width ffn.hip (and wattn.hip) serves
TAIL_MAX_HIDDEN = 2048                                             # IGS_LAYER_TAIL_MAX_HIDDEN
TAIL_MAX_ROWS = 1 << 24                                            # IGS_LAYER_TAIL_MAX_ROWS
TAIL_TRIP_ROWS = 128                                               # IGS_LAYER_TAIL_TRIP_ROWS
TAIL_CACHE = "_igs_layer_tail_pack"
# Per compute dtype, whether the forward that use_native_layer_tails binds takes the fused kernel when nothing needs a gradient (True) or
# today's tail (False; layer_tail with an explicit compute_dtype still runs the kernel).  DESIGN.md 27 has the measurement that set
# each: the fused tail against the unfused native tail at [32768, 128], hidden 1024.
LAYER_TAIL_FUSED = {torch.float32: True, torch.float16: True}
# A layer WITH FFN takes the fused kernel only when its rows fill at least this share of the kernel's last round of workgroups.  The kernel
# holds one wave per SIMD and a wave streams the whole FFN past its 32 rows, so a launch costs a fixed time per round of compute units x
# 128 rows (0.32 ms float32, 0.14 ms float16 measured) however few of them are there: [16384, 128] fills half a round of 256 compute
# units and measured 0.67 x (float32) and 0.91 x (float16) of the unfused tail, [32768, 128] fills it and measured 1.05 x and 1.10 x.
# Layers without FFN are not held to it, and float32 ones take the fused kernel although it buys no time there: 0.99 x at [32768, 128] and
# 0.94 x at [16384, 128] with overlapping min - max ranges, i.e. level within the timing noise; it is kept for half the peak memory
# (merge's result is never stored) and one launch less.  float16 ones gain 1.21 - 1.24 x.
LAYER_TAIL_FFN_MIN_FILL = {torch.float32: 0.95, torch.float16: 0.95}
# Per compute dtype, whether a call that needs a gradient takes layer_tail_autograd (the fused forward and the recomputing backward of
# ffn_bwd.hip) under use_native_layer_tails(training=True).  An entry is True only where the native training step's median is lower than
# the unfused tail's under autograd and its min - max range does not lie behind it.  Measured ("The backward";
# profiles/layer_tail_train_bench.jsonl): 0.44 x (float32) and 0.53 x (float16 autocast) at [32768, 128] with the FFN, 0.52 x and 0.77 x
# without, 0.66 x and 0.75 x over a six-block stand-in, so both are False: the route buys memory (that stand-in trains in 1.3 GB
# against 3.4 GB in float32) and a reproducible backward, not time.  layer_tail_autograd called directly always runs the kernels.
LAYER_TAIL_BWD_NATIVE = {torch.float32: False, torch.float16: False}


def _tail_spec(fn, layer):
    """(merge, norm1, Linear 256 -> hidden or None, Linear hidden -> 128 or None, norm2 or None) of a layer that ffn.hip serves, or
    NotImplementedError."""
    merge, n1 = getattr(layer, LAYER_MERGE, None), getattr(layer, LAYER_NORM1, None)
    if not isinstance(merge, nn.Linear) or (merge.in_features, merge.out_features) != (TAIL_D, TAIL_D):
        raise NotImplementedError(f"{fn}: {LAYER_MERGE} must be nn.Linear({TAIL_D}, {TAIL_D}): d_model other than {TAIL_D} is not provided (got {merge})")
    linears, norms = [(merge, LAYER_MERGE)], [(n1, LAYER_NORM1)]
    l0 = l2 = n2 = None
    if not getattr(layer, LAYER_NO_FFN):
        mlp, n2 = getattr(layer, LAYER_MLP, None), getattr(layer, LAYER_NORM2, None)
        mods = list(mlp) if isinstance(mlp, nn.Sequential) else []
        if (len(mods) != 3 or not (isinstance(mods[0], nn.Linear) and isinstance(mods[1], nn.GELU) and isinstance(mods[2], nn.Linear))
                or getattr(mods[1], GELU_ONLY_ATTRS[0], "none") != "none"):
            raise NotImplementedError(f"{fn}: {LAYER_MLP} must be exactly nn.Sequential(Linear, GELU(approximate='none'), Linear) (got {mlp})")
        l0, l2 = mods[0], mods[2]
        hidden = l0.out_features
        if l0.in_features != 2 * TAIL_D or l2.in_features != hidden or l2.out_features != TAIL_D:
            raise NotImplementedError(f"{fn}: {LAYER_MLP} must map {2 * TAIL_D} -> hidden -> {TAIL_D} (got {l0.in_features} -> {hidden}, "
                                      f"{l2.in_features} -> {l2.out_features})")
        if hidden % 32 or not 32 <= hidden <= TAIL_MAX_HIDDEN:
            raise NotImplementedError(f"{fn}: hidden = {hidden} must be a multiple of 32 in 32..{TAIL_MAX_HIDDEN}")
        linears += [(l0, f"{LAYER_MLP}[0]"), (l2, f"{LAYER_MLP}[2]")]
        norms.append((n2, LAYER_NORM2))
    for lin, name in linears:
        if lin.bias is not None:
            raise NotImplementedError(f"{fn}: {name} has a bias: biases are not provided")
    for n, name in norms:
        if not _layer_norm_ok(n) or tuple(n.normalized_shape) != (TAIL_D,) or n.weight is None:
            raise NotImplementedError(f"{fn}: {name} must be nn.LayerNorm({TAIL_D}) with weight and bias (got {n})")
    for p in _tail_params(layer):
        if p.dtype not in DTYPES:
            raise NotImplementedError(f"{fn}: parameters must be float32 or float16 (got {p.dtype})")
    return merge, n1, l0, l2, n2


def _tail_params(layer):
    """The parameters the tail reads: merge, norm1 and, with an FFN, the two Linears of mlp and norm2."""
    n1 = getattr(layer, LAYER_NORM1)
    params = [getattr(layer, LAYER_MERGE).weight, n1.weight, n1.bias]
    if not getattr(layer, LAYER_NO_FFN):
        mlp, n2 = getattr(layer, LAYER_MLP), getattr(layer, LAYER_NORM2)
        params += [mlp[0].weight, mlp[2].weight, n2.weight, n2.bias]
    return params


def pack_layer_tail(layer, dtype=torch.float32, transposed=False):
    """The weights of a layer's tail in `dtype` as igs_layer_tail_fwd takes them (include/igs_rast.h), one flat tensor of 1024-element tiles in
    pack_mlp_tile_order's per-tile layout: merge (16 tiles, output tile outermost), then with an FFN mlp[0] split by output tile (hidden / 32
    x 8 tiles) and mlp[2] with its INPUT tile outermost (hidden / 32 x 4 tiles), so that the kernel finds everything hidden units
    32 j .. 32 j + 31 need in two contiguous pieces.  transposed=True: (pack, pack_t), pack_t the transposes as igs_layer_tail_bwd takes them
    at the same offsets: merge^T, mlp[0]^T with its INPUT tile outermost (tile 8 j + ot), mlp[2]^T with its output tile outermost (tile
    4 j + kt).  Plain tensor ops: works on any device."""
    merge, _, l0, l2, _ = _tail_spec("pack_layer_tail", layer)
    if dtype not in DTYPES:
        raise NotImplementedError(f"pack_layer_tail: dtype must be float32 or float16 (got {dtype})")
    parts = [pack_mlp_tile_order(merge.weight.detach().to(dtype))]
    if l0 is not None:
        ht = l0.out_features // 32
        parts.append(pack_mlp_tile_order(l0.weight.detach().to(dtype)))
        parts.append(pack_mlp_tile_order(l2.weight.detach().to(dtype)).view(TAIL_D // 32, ht, -1).transpose(0, 1).reshape(-1))
    pack = torch.cat(parts).contiguous()
    if not transposed:
        return pack
    parts = [pack_mlp_tile_order(merge.weight.detach().to(dtype).t().contiguous())]
    if l0 is not None:
        parts.append(pack_mlp_tile_order(l0.weight.detach().to(dtype).t().contiguous()).view(2 * TAIL_D // 32, ht, -1).transpose(0, 1).reshape(-1))
        parts.append(pack_mlp_tile_order(l2.weight.detach().to(dtype).t().contiguous()))
    return pack, torch.cat(parts).contiguous()


def _tail_compute_dtype(fn, attn_out):
    return torch.float16 if autocast_half(fn, attn_out) or attn_out.dtype == torch.float16 else torch.float32


def _tail_checks(fn, attn_out, source, layer, packed, packed_t, compute_dtype, forward_only):
    """The refusals of layer_tail and layer_tail_autograd, in one order; returns _tail_spec's tuple and the compute dtype."""
    merge, n1, l0, l2, n2 = _tail_spec(fn, layer)
    if attn_out.dim() < 1 or attn_out.shape[-1] != TAIL_D or tuple(source.shape) != tuple(attn_out.shape):
        raise ValueError(f"{fn}: attn_out and source must both be [..., {TAIL_D}] (got {list(attn_out.shape)} and {list(source.shape)})")
    if attn_out.numel() // TAIL_D > TAIL_MAX_ROWS:
        raise ValueError(f"{fn}: {attn_out.numel() // TAIL_D} rows is above the supported {TAIL_MAX_ROWS}")
    params = _tail_params(layer)
    named = [(attn_out, "attn_out"), (source, "source")] + [(p, "a parameter") for p in params]
    for t, name in named[:2]:
        if t.dtype not in DTYPES:
            raise NotImplementedError(f"{fn}: {name} must be float32 or float16 (got {t.dtype})")
    if forward_only and torch.is_grad_enabled() and any(t.requires_grad for t, _ in named):
        raise NotImplementedError(f"{fn}: forward only -- call it under torch.no_grad(), and train with use_native_transformer_layers")
    if compute_dtype is None:
        compute_dtype = _tail_compute_dtype(fn, attn_out)
    if compute_dtype not in DTYPES:
        raise NotImplementedError(f"{fn}: compute_dtype must be float32 or float16 (got {compute_dtype})")
    for pk in (packed, packed_t):
        if pk is not None and pk.dtype != compute_dtype:
            raise ValueError(f"{fn}: packed holds {pk.dtype} weights, compute_dtype is {compute_dtype}")
    _refuse(fn, named)
    return merge, n1, l0, l2, n2, compute_dtype


def layer_tail(attn_out, source, layer, packed=None, compute_dtype=None):
    """Everything a unimatch TransformerLayer does behind its attention, in one launch and forward only (igs_layer_tail_fwd, ffn.hip):
    source + LN1(merge(attn_out)) for a layer without FFN, source + LN2(mlp(cat(source, LN1(merge(attn_out))))) with one; neither merge's
    result, the cat nor the [rows, hidden] activations reach memory.  attn_out, source: [..., 128] float32 / float16 on one GPU (rows with
    stride 1 are read in place through a row stride, anything else is copied once).  compute_dtype: torch.float32 (exact float32 matrix
    instructions) or torch.float16 (half operands, float32 accumulation; LayerNorms, GELU and the residual add stay float32); default
    float16 under autocast to half or when attn_out is half, float32 otherwise.  packed: pack_layer_tail(layer, compute_dtype), packed
    here when absent.  The result is contiguous, in the dtype the unfused bound forward gives: float32 under autocast, the promoted dtype
    of attn_out and source otherwise.  Raises NotImplementedError when grad is enabled and an input or a parameter of the tail requires
    grad, for a Linear with a bias, an mlp that is not Sequential(Linear, GELU(approximate='none'), Linear), d_model other than 128, a
    hidden that is not a multiple of 32 in 32..2048, and bfloat16 / float64; RuntimeError for CPU tensors; ValueError for shapes."""
    fn = "layer_tail"
    merge, n1, l0, l2, n2, compute_dtype = _tail_checks(fn, attn_out, source, layer, packed, None, compute_dtype, True)
    if packed is None:
        packed = pack_layer_tail(layer, compute_dtype)
    out_dtype = _autocast_out_dtype(torch.promote_types(attn_out.dtype, source.dtype))
    ln2 = (None, None, 1e-5) if n2 is None else (n2.weight.detach().float(), n2.bias.detach().float(), float(n2.eps))
    out = _ext()._ffn.layer_tail_fwd(_rows(attn_out.detach()), _rows(source.detach()), packed, 0 if l0 is None else l0.out_features,
                                     n1.weight.detach().float(), n1.bias.detach().float(), float(n1.eps), *ln2, out_dtype == torch.float16)
    return out.view(attn_out.shape)


class _LayerTail(torch.autograd.Function):
    """igs_layer_tail_fwd with igs_layer_tail_bwd behind it.  Saves attn_out and source as the kernel read them, the two packs and the
    LayerNorms' affines: neither merge's result, the cat, the hidden activations, mlp's result nor any statistics."""

    @staticmethod
    def forward(ctx, a, s, wm, ln1w, ln1b, w1, w2, ln2w, ln2b, pack, pack_t, hidden, eps1, eps2, out_half):
        ctx.set_materialize_grads(False)
        f1w, f1b = ln1w.detach().float(), ln1b.detach().float()
        f2w, f2b = (None, None) if ln2w is None else (ln2w.detach().float(), ln2b.detach().float())
        ctx.save_for_backward(a, s, pack, pack_t, f1w, f1b, f2w, f2b)
        ctx.hidden, ctx.eps1, ctx.eps2 = hidden, eps1, eps2
        ctx.param_dtypes = [None if t is None else t.dtype for t in (wm, ln1w, ln1b, w1, w2, ln2w, ln2b)]
        return _ext()._ffn.layer_tail_fwd(a, s, pack, hidden, f1w, f1b, eps1, f2w, f2b, eps2, out_half)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 15
        a, s, pack, pack_t, f1w, f1b, f2w, f2b = ctx.saved_tensors
        if g.dtype not in DTYPES:
            g = g.float()
        want = [bool(n) and (i < 5 or ctx.hidden != 0) for i, n in enumerate(ctx.needs_input_grad[:9])]
        grads = list(_ext()._ffn.layer_tail_bwd(a, s, _rows(g), pack, pack_t, ctx.hidden, f1w, f1b, ctx.eps1, f2w, f2b, ctx.eps2, want,
                                                a.dtype == torch.float16, s.dtype == torch.float16))
        for i, dt in enumerate(ctx.param_dtypes):                  # accumulated in float32, cast once
            if grads[i + 2] is not None and grads[i + 2].dtype != dt:
                grads[i + 2] = grads[i + 2].to(dt)
        return (*grads, None, None, None, None, None, None)


def layer_tail_autograd(attn_out, source, layer, packed=None, packed_t=None, compute_dtype=None):
    """layer_tail for training: the same checks, sizes, dtypes and value, and a native backward.  When grad is disabled or neither an input
    nor a parameter of the tail requires it this IS the forward kernel alone.  Otherwise the forward is igs_layer_tail_fwd and the backward
    igs_layer_tail_bwd (ffn_bwd.hip), which recomputes the forward chunk by chunk: gradients for attn_out and source in their dtypes and
    for merge.weight, norm1.weight / bias, mlp[0].weight, mlp[2].weight and norm2.weight / bias, accumulated in float32 and cast once to
    each parameter's dtype.  Saved: attn_out and source as the kernel read them (themselves where their rows have stride 1), the two packs
    and the LayerNorms' affines.  Once differentiable, deterministic (no atomics).  packed, packed_t: pack_layer_tail(layer,
    compute_dtype, transposed=True), packed here when either is absent.  Refusals as layer_tail's, except that gradients are served."""
    fn = "layer_tail_autograd"
    merge, n1, l0, l2, n2, compute_dtype = _tail_checks(fn, attn_out, source, layer, packed, packed_t, compute_dtype, False)
    if packed is None or packed_t is None:
        packed, packed_t = pack_layer_tail(layer, compute_dtype, transposed=True)
    out_half = _autocast_out_dtype(torch.promote_types(attn_out.dtype, source.dtype)) == torch.float16
    hidden = 0 if l0 is None else l0.out_features
    a, s = _rows(attn_out), _rows(source)
    ffn = (None,) * 4 if l0 is None else (l0.weight, l2.weight, n2.weight, n2.bias)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (a, s, merge.weight, n1.weight, n1.bias) + ffn):
        out = _LayerTail.apply(a, s, merge.weight, n1.weight, n1.bias, *ffn, packed, packed_t, hidden, float(n1.eps),
                               1e-5 if n2 is None else float(n2.eps), out_half)
    else:
        ln2 = (None, None, 1e-5) if n2 is None else (n2.weight.detach().float(), n2.bias.detach().float(), float(n2.eps))
        out = _ext()._ffn.layer_tail_fwd(a.detach(), s.detach(), packed, hidden, n1.weight.detach().float(), n1.bias.detach().float(),
                                         float(n1.eps), *ln2, out_half)
    return out.view(attn_out.shape)


_TAIL_CUS = {}                                                     # device index -> compute units, asked once


def _tail_fill(attn_out):
    """The share of the fused FFN kernel's last round of workgroups (one of TAIL_TRIP_ROWS rows per compute unit) that these rows fill."""
    rows = attn_out.numel() // max(attn_out.shape[-1], 1)
    if rows == 0 or not attn_out.is_cuda:
        return 0.0
    index = attn_out.device.index
    groups = _TAIL_CUS.get(index)
    if groups is None:
        groups = _TAIL_CUS[index] = torch.cuda.get_device_properties(attn_out.device).multi_processor_count
    trips = -(-rows // TAIL_TRIP_ROWS)
    return rows / float(-(-trips // groups) * groups * TAIL_TRIP_ROWS)


def _tail_entry(layer, dtype, params, transposed):
    """The layer's cached pack(s) for a compute dtype, rebuilt when a parameter changed (param_key)."""
    key = param_key(params)
    cache = layer.__dict__.setdefault(TAIL_CACHE, {})                            # one entry per compute dtype
    entry = cache.get(dtype)
    if entry is None or entry["key"] != key:
        entry = cache[dtype] = dict(key=key)
    if transposed and "pack_t" not in entry:
        entry["pack"], entry["pack_t"] = pack_layer_tail(layer, dtype, transposed=True)
    elif "pack" not in entry:
        entry["pack"] = pack_layer_tail(layer, dtype)
    return entry


def _layer_tail_forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, shifted_window_attn_mask_1d=None,
                        attn_type="swin", with_shift=False, attn_num_splits=None):
    """TransformerLayer.forward as use_native_layer_tails binds it: _layer_forward's projections and attention, then layer_tail when
    nothing needs a gradient (and LAYER_TAIL_FUSED and LAYER_TAIL_FFN_MIN_FILL take the call), _layer_forward's own tail otherwise."""
    return _layer_tail_route(self, False, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)


def _layer_tail_forward_training(self, source, target, height=None, width=None, shifted_window_attn_mask=None, shifted_window_attn_mask_1d=None,
                                 attn_type="swin", with_shift=False, attn_num_splits=None):
    """_layer_tail_forward as use_native_layer_tails(training=True) binds it: a call that needs a gradient takes layer_tail_autograd where
    LAYER_TAIL_BWD_NATIVE says so (a layer with FFN still held to LAYER_TAIL_FFN_MIN_FILL), the unfused tail otherwise."""
    return _layer_tail_route(self, True, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)


def _layer_tail_route(self, training, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits):
    message = _layer_message(self, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)
    return _tail_route(self, training, message, source)


def _tail_route(self, training, message, source):
    """The layer's tail behind the attention's `message`, by the rules of use_native_layer_tails(module, training)."""
    fn = "TransformerLayer"
    params = _tail_params(self)
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in [message, source] + params)
    if needs_grad and not training:
        return _layer_tail_unfused(self, message, source)
    dtype = _tail_compute_dtype(fn, message)
    if needs_grad and not LAYER_TAIL_BWD_NATIVE[dtype]:
        return _layer_tail_unfused(self, message, source)
    if not needs_grad and not LAYER_TAIL_FUSED[dtype]:
        return _layer_tail_unfused(self, message, source)
    if not getattr(self, LAYER_NO_FFN) and _tail_fill(message) < LAYER_TAIL_FFN_MIN_FILL[dtype]:
        return _layer_tail_unfused(self, message, source)
    entry = _tail_entry(self, dtype, params, needs_grad)
    if needs_grad:
        return layer_tail_autograd(message, source, self, packed=entry["pack"], packed_t=entry["pack_t"], compute_dtype=dtype)
    return layer_tail(message, source, self, packed=entry["pack"], compute_dtype=dtype)


def use_native_layer_tails(module, training=False):
    """Binds a forward on every unimatch TransformerLayer under `module` (found as use_native_transformer_layers finds them) that does the
    three projections and the attention lookup as that binder's forward does and then, when nothing needs a gradient, runs the whole tail
    as one launch (layer_tail); with grad enabled and anything requiring it, the tail is use_native_transformer_layers' own, with autograd.
    So is the tail of a layer with FFN whose rows fill less than LAYER_TAIL_FFN_MIN_FILL of the kernel's last round of workgroups (the
    kernel's time does not shrink with the rows below compute units x 128), and of a compute dtype that LAYER_TAIL_FUSED turns off.
    Returns how many layers were bound; state_dict() keys and the classes are untouched; composes with use_native_window_attention.  The
    packed weights are kept on the layer, one pack per compute dtype, and rebuilt when a parameter's _version, data_ptr, dtype or device
    changes.  Compute dtype:
    float16 under autocast to half or when the attention's output is half, float32 otherwise; the result has the dtype of the unfused bound
    forward.  Raises NotImplementedError, before anything is changed, for everything use_native_transformer_layers refuses and for
    everything layer_tail refuses about a layer (biases, another mlp, d_model other than 128, hidden out of range, bfloat16 / float64
    parameters).
    training=True: a call that needs a gradient goes to layer_tail_autograd (the fused forward with the recomputing native backward of
    ffn_bwd.hip behind it) for the compute dtypes that LAYER_TAIL_BWD_NATIVE turns on, a layer with FFN still held to
    LAYER_TAIL_FFN_MIN_FILL; everything else is routed as with the default.  The transposed pack is cached beside the pack, per compute
    dtype, and both are rebuilt after every optimiser step (a parameter's _version changes)."""
    fn = "use_native_layer_tails"
    layers = _checked_layers(fn, module)
    for m in layers:
        _tail_spec(fn, m)
    bound = _layer_tail_forward_training if training else _layer_tail_forward
    for m in layers:
        m.forward = types.MethodType(bound, m)
    return len(layers)


# ---------------------------------------------------------------- the layer's q / k / v projections in one launch (proj.hip)
PROJ_MAX_OUT = 5                                                   # IGS_TOKEN_PROJ_MAX_OUT
HEAD_CACHE = "_igs_layer_head_pack"
FT_LAYERS, BLOCK_SELF, BLOCK_CROSS = "layers", "self_attn", "cross_attn_ffn"
FT_MASK = "generate_shift_window_attn_mask"
FT_STATE = "_igs_feature_transformer"
# Per compute dtype, whether the forwards that use_native_layer_heads and use_native_feature_transformer bind take the fused projections
# when nothing needs a gradient (True) or the layer's three nn.Linear calls (False; project_tokens itself always runs the kernel), and the
# fewest outputs a launch must have to be taken: a launch with fewer stays nn.Linear.  DESIGN.md 28 has the measurement that set each
# (profiles/layer_head_bench.jsonl): the launch against as many F.linear calls at [32768, 128] and [163840, 128].  n = 5 (with the swap
# copy on the other side) and n = 2 hold at both shapes in both dtypes (1.14 - 1.44 x and 1.07 - 1.27 x float32, 2.26 - 3.07 x and
# 1.34 - 2.13 x float16 autocast, ranges disjoint), so both dtypes are on.  n = 1 holds at [32768, 128] (1.23 x, 1.58 x) and DOES NOT HOLD
# at [163840, 128] (1.02 x float32 and 0.94 x float16, ranges overlapping), so a single projection stays nn.Linear in both.  n = 3 in
# float32 does not hold at [163840, 128] either (0.98 x, ranges overlapping: level) and is 1.35 x ahead at [32768, 128]; it stays on.
LAYER_HEAD_FUSED = {torch.float32: True, torch.float16: True}
LAYER_HEAD_MIN_OUTPUTS = {torch.float32: 2, torch.float16: 2}
# Per compute dtype, whether a call that needs a gradient takes project_tokens_autograd (the fused forward with proj_bwd.hip behind it) under
# use_native_layer_heads(training=True) and use_native_feature_transformer(training=True), and the fewest outputs such a launch must have.
# A case holds only where the native forward + backward is ahead of as many F.linear calls under autograd (plus the swap cat for n = 5)
# with disjoint min - max ranges.  Measured ("The backward"; profiles/layer_head_train_bench.jsonl) at [32768, 128] and
# [163840, 128]: n = 5 holds everywhere (2.07 x and 2.05 x float32, 2.50 x and 2.15 x float16 autocast), n = 3 too (1.68 x, 1.67 x, 1.86 x,
# 1.28 x), so both dtypes are on.  n = 2 holds in float32 (1.32 x, 1.35 x) and at [32768, 128] under autocast (1.43 x) and DOES NOT HOLD at
# [163840, 128] under autocast (0.91 x: 1.046 ms (1.033 - 1.073) against 0.947 (0.933 - 0.964), slower), so float16 asks for three outputs.
# n = 1 DOES NOT HOLD anywhere (0.88 x, 0.79 x float32; 0.90 x, 0.50 x float16: the weight-gradient launch costs a wave's walk over its
# slice however few outputs there are), so a single projection stays nn.Linear in both.  project_tokens_autograd called directly always
# runs the kernels.
LAYER_HEAD_BWD_NATIVE = {torch.float32: True, torch.float16: True}
LAYER_HEAD_BWD_MIN_OUTPUTS = {torch.float32: 2, torch.float16: 3}


def _proj_weights(fn, weights):
    """The [128, 128] weight tensors of `weights` (tensors, or bias-free nn.Linear modules), or the refusal."""
    ws = []
    for w in weights:
        if isinstance(w, nn.Linear):
            if w.bias is not None:
                raise NotImplementedError(f"{fn}: a projection has a bias: biases are not provided")
            w = w.weight
        if not torch.is_tensor(w) or w.dim() != 2 or w.shape[0] != w.shape[1]:
            raise ValueError(f"{fn}: every weight must be a square [{TAIL_D}, {TAIL_D}] matrix (got {list(w.shape) if torch.is_tensor(w) else type(w)})")
        if w.shape[0] != TAIL_D:
            raise NotImplementedError(f"{fn}: a weight is {list(w.shape)}: widths other than {TAIL_D} are not provided")
        if w.dtype not in DTYPES:
            raise NotImplementedError(f"{fn}: weights must be float32 or float16 (got {w.dtype})")
        ws.append(w)
    if not 1 <= len(ws) <= PROJ_MAX_OUT:
        raise ValueError(f"{fn}: 1..{PROJ_MAX_OUT} weights are served (got {len(ws)})")
    return ws


def pack_projections(weights, dtype=torch.float32, transposed=False):
    """n = 1..5 weights [128, 128] (tensors as nn.Linear keeps them, or bias-free nn.Linear modules) in `dtype` as igs_token_proj_fwd takes
    them (include/igs_rast.h): one flat tensor, matrix after matrix, each 16 tiles of 1024 elements in pack_layer_tail's layout for merge.
    transposed=True: (pack, pack_t), pack_t the same pack of the transposes W_j^T as igs_token_proj_bwd takes it.  Plain tensor ops: works
    on any device."""
    ws = _proj_weights("pack_projections", weights)
    if dtype not in DTYPES:
        raise NotImplementedError(f"pack_projections: dtype must be float32 or float16 (got {dtype})")
    pack = torch.cat([pack_mlp_tile_order(w.detach().to(dtype)) for w in ws]).contiguous()
    if not transposed:
        return pack
    return pack, torch.cat([pack_mlp_tile_order(w.detach().to(dtype).t().contiguous()) for w in ws]).contiguous()


def _proj_checks(fn, x, weights, rot, packed, packed_t, compute_dtype, forward_only):
    """The refusals of project_tokens and project_tokens_autograd, in one order; returns the weight tensors, the offsets as a list (empty:
    none) and the compute dtype."""
    ws = _proj_weights(fn, weights)
    n = len(ws)
    if x.dim() < 1 or x.shape[-1] != TAIL_D:
        raise ValueError(f"{fn}: x must be [..., {TAIL_D}] (got {list(x.shape)})")
    rows = x.numel() // TAIL_D
    if rows > TAIL_MAX_ROWS:
        raise ValueError(f"{fn}: {rows} rows is above the supported {TAIL_MAX_ROWS}")
    rot = [] if rot is None else [int(r) for r in rot]
    if rot and (len(rot) != n or any(r < 0 or (r >= rows and not (rows == 0 and r == 0)) for r in rot)):
        raise ValueError(f"{fn}: rot must hold one offset in 0..{rows - 1} per weight (got {rot})")
    if x.dtype not in DTYPES:
        raise NotImplementedError(f"{fn}: x must be float32 or float16 (got {x.dtype})")
    if forward_only and torch.is_grad_enabled() and any(t.requires_grad for t in [x] + ws):
        raise NotImplementedError(f"{fn}: forward only -- call it under torch.no_grad(), and train with project_tokens_autograd")
    if compute_dtype is None:
        compute_dtype = _tail_compute_dtype(fn, x)
    if compute_dtype not in DTYPES:
        raise NotImplementedError(f"{fn}: compute_dtype must be float32 or float16 (got {compute_dtype})")
    for pk in (packed, packed_t):
        if pk is not None and pk.dtype != compute_dtype:
            raise ValueError(f"{fn}: packed holds {pk.dtype} weights, compute_dtype is {compute_dtype}")
        if pk is not None and pk.numel() != n * 16 * 1024:
            raise ValueError(f"{fn}: packed holds {pk.numel()} elements, {n} matrices are {n * 16 * 1024}")
    _refuse(fn, [(x, "x")] + [(w, "a weight") for w in ws])
    return ws, rot, compute_dtype


def project_tokens(x, weights, rot=None, packed=None, compute_dtype=None):
    """torch.cat([F.linear(x, W) for W in weights], -1) in one launch and forward only (igs_token_proj_fwd, proj.hip): x [..., 128] is read
    once, the n = 1..5 results [..., 128 n] are written side by side and the caller slices them (wattn.hip reads such slices in place).
    rot: n row offsets in [0, rows), rows the product of x's leading sizes: the columns of output j are written rolled by rot[j] rows,
    torch.roll(F.linear(x, W_j).view(rows, 128), rot[j], 0); rot[j] = rows / 2 is the projection of x with its two batch halves swapped.
    weights: tensors [128, 128] or bias-free nn.Linear modules.  compute_dtype: torch.float32 (exact float32 matrix instructions) or
    torch.float16 (half operands, float32 accumulation); default float16 under autocast to half or when x is half, float32 otherwise.  The
    result is contiguous, float16 when the compute dtype is, float32 otherwise: what nn.Linear returns.  packed:
    pack_projections(weights, compute_dtype), packed here when absent.  Raises NotImplementedError when grad is enabled and x or a
    weight requires it, for a bias, widths other than 128 and bfloat16 / float64; RuntimeError for CPU tensors; ValueError for shapes."""
    fn = "project_tokens"
    ws, rot, compute_dtype = _proj_checks(fn, x, weights, rot, packed, None, compute_dtype, True)
    if packed is None:
        packed = pack_projections(ws, compute_dtype)
    out = _ext()._proj.token_proj_fwd(_rows(x.detach()), packed, len(ws), rot, compute_dtype == torch.float16)
    return out.view(x.shape[:-1] + (TAIL_D * len(ws),))


class _ProjectTokens(torch.autograd.Function):
    """igs_token_proj_fwd with igs_token_proj_bwd behind it.  Returns the n column slices of the one buffer as n outputs, so that each
    output's gradient arrives on its own (None for an unused one).  Saves x as the kernel read it and the transposed pack."""

    @staticmethod
    def forward(ctx, x, pack, pack_t, rot, out_half, *ws):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, pack_t)
        ctx.rot, ctx.param_dtypes = rot, [w.dtype for w in ws]
        buf = _ext()._proj.token_proj_fwd(x, pack, len(ws), rot, out_half)
        return tuple(_cols(buf, j) for j in range(len(ws)))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        n = len(gs)
        if all(g is None for g in gs):
            return (None,) * (5 + n)
        x, pack_t = ctx.saved_tensors
        dts = {g.dtype for g in gs if g is not None}
        to = None if len(dts) == 1 and dts <= set(DTYPES) else torch.float32     # the C call takes one dtype for all of them
        # rows with stride 1 inside and at least 128 between them are read in place; anything else (an expanded gradient) is copied once
        gs = [None if g is None else _rows(g if to is None else g.to(to)) for g in gs]
        dx, dws = _ext()._proj.token_proj_bwd(x, gs, pack_t, ctx.rot, bool(ctx.needs_input_grad[0]), [bool(w) for w in ctx.needs_input_grad[5:]],
                                              x.dtype == torch.float16)
        dws = [d if d is None or d.dtype == dt else d.to(dt) for d, dt in zip(dws, ctx.param_dtypes)]      # accumulated in float32, cast once
        return (dx, None, None, None, None, *dws)


def project_tokens_autograd(x, weights, rot=None, packed=None, packed_t=None, compute_dtype=None):
    """project_tokens for training: the same checks, sizes, dtypes and values, returned as a tuple of the n results [..., 128], which are
    the column slices of one [rows, 128 n] buffer (wattn.hip reads them in place), and a native backward.  When grad is disabled or neither
    x nor a weight requires it this IS project_tokens plus the slicing.  Otherwise the forward is igs_token_proj_fwd and the backward
    igs_token_proj_bwd (proj_bwd.hip): each output's gradient arrives on its own and is read in place with its stride and the roll (an
    unused output's is skipped), d x comes back in x's dtype (no launch for it when x needs none) and each d W_j, accumulated in float32,
    is cast once to its weight's dtype.  Saved: x as the kernel read it (itself where its rows have stride 1) and the transposed pack.
    Once differentiable, deterministic (no atomics).  packed, packed_t: pack_projections(weights, compute_dtype, transposed=True), packed
    here when either is absent; a wrong dtype or length raises ValueError.  Refusals as project_tokens', except that gradients are
    served."""
    fn = "project_tokens_autograd"
    ws, rot, compute_dtype = _proj_checks(fn, x, weights, rot, packed, packed_t, compute_dtype, False)
    n, shape = len(ws), x.shape[:-1] + (TAIL_D,)
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in [x] + ws)):
        if packed is None:
            packed = pack_projections(ws, compute_dtype)
        buf = _ext()._proj.token_proj_fwd(_rows(x.detach()), packed, n, rot, compute_dtype == torch.float16)
        return tuple(_cols(buf, j).view(shape) for j in range(n))
    if packed is None or packed_t is None:
        packed, packed_t = pack_projections(ws, compute_dtype, transposed=True)
    outs = _ProjectTokens.apply(_rows(x), packed, packed_t, rot, compute_dtype == torch.float16, *ws)
    return tuple(o.view(shape) for o in outs)


def _head_linears(fn, layer):
    """(q_proj, k_proj, v_proj) of a layer that proj.hip serves, or NotImplementedError."""
    lins = tuple(getattr(layer, a, None) for a in (LAYER_Q, LAYER_K, LAYER_V))
    for lin, name in zip(lins, (LAYER_Q, LAYER_K, LAYER_V)):
        if not isinstance(lin, nn.Linear) or (lin.in_features, lin.out_features) != (TAIL_D, TAIL_D):
            raise NotImplementedError(f"{fn}: {name} must be nn.Linear({TAIL_D}, {TAIL_D}): d_model other than {TAIL_D} is not provided (got {lin})")
        if lin.bias is not None:
            raise NotImplementedError(f"{fn}: {name} has a bias: biases are not provided")
        if lin.weight.dtype not in DTYPES:
            raise NotImplementedError(f"{fn}: parameters must be float32 or float16 (got {lin.weight.dtype})")
    return lins


def _head_pack(holder, which, dtype, weights, transposed=False):
    """The pack of `weights` for a compute dtype (transposed: the pack and the pack of the transposes), cached on the layer `holder` under
    the name `which` and rebuilt when a weight changed (param_key)."""
    key = param_key(weights)
    cache = holder.__dict__.setdefault(HEAD_CACHE, {})
    entry = cache.get((which, dtype))
    if entry is None or entry["key"] != key:
        entry = cache[(which, dtype)] = dict(key=key)
    if transposed and "pack_t" not in entry:
        pack, entry["pack_t"] = pack_projections(weights, dtype, transposed=True)
        entry.setdefault("pack", pack)
    elif "pack" not in entry:
        entry["pack"] = pack_projections(weights, dtype)
    return (entry["pack"], entry["pack_t"]) if transposed else entry["pack"]


def _head_project(holder, which, x, linears, rot=None):
    """The n products [..., 128] of x with the n Linears' weights.  One launch whose buffer's column slices are returned where
    LAYER_HEAD_MIN_OUTPUTS allows (project_tokens; with a gradient needed: LAYER_HEAD_BWD_MIN_OUTPUTS and project_tokens_autograd), n
    nn.Linear calls (and the rolls and the cat that rot and the layout ask for) otherwise."""
    dtype = _tail_compute_dtype("TransformerLayer", x)
    weights = [lin.weight for lin in linears]
    n = len(linears)
    if torch.is_grad_enabled() and any(t.requires_grad for t in [x] + weights):
        if n >= LAYER_HEAD_BWD_MIN_OUTPUTS[dtype]:
            pack, pack_t = _head_pack(holder, which, dtype, weights, transposed=True)
            return project_tokens_autograd(x, weights, rot=rot, packed=pack, packed_t=pack_t, compute_dtype=dtype)
    elif n >= LAYER_HEAD_MIN_OUTPUTS[dtype]:
        buf = project_tokens(x, weights, rot=rot, packed=_head_pack(holder, which, dtype, weights), compute_dtype=dtype)
        return tuple(_cols(buf, j) for j in range(n))
    outs = [lin(x) for lin in linears]
    if rot is not None:
        outs = [o if r == 0 else torch.roll(o.reshape(-1, TAIL_D), r, 0).view(o.shape) for o, r in zip(outs, rot)]
    if n == 1:
        return (outs[0],)
    buf = torch.cat(outs, -1)
    return tuple(_cols(buf, j) for j in range(n))


def _heads_fused(tensors, weights, training=False):
    """Whether a forward over `tensors` with the projection `weights` takes the fused launches: the activations are float32 / float16 rows
    of 128 on a GPU and, when nothing needs a gradient, LAYER_HEAD_FUSED has the compute dtype on; when something does, the forward was
    bound with training=True and LAYER_HEAD_BWD_NATIVE has it on."""
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in list(tensors) + list(weights))
    if needs_grad and not training:
        return False
    if any(t.dtype not in DTYPES or not t.is_cuda or t.dim() < 1 or t.shape[-1] != TAIL_D for t in tensors):
        return False
    return (LAYER_HEAD_BWD_NATIVE if needs_grad else LAYER_HEAD_FUSED)[_tail_compute_dtype("TransformerLayer", tensors[0])]


def _cols(buf, j):
    return buf[..., TAIL_D * j: TAIL_D * (j + 1)]


def _layer_head_route(self, training, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits):
    _layer_served(self, attn_type)
    q, k, v = (getattr(self, a) for a in (LAYER_Q, LAYER_K, LAYER_V))
    if not _heads_fused([source, target], [q.weight, k.weight, v.weight], training):
        message = _layer_message(self, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)
        return _tail_route(self, training, message, source)
    if source is target:
        query, key, value = _head_project(self, "qkv", source, (q, k, v))
    else:
        (query,) = _head_project(self, "q", source, (q,))
        key, value = _head_project(self, "kv", target, (k, v))
    message = _layer_attention(self, query, key, value, height, width, shifted_window_attn_mask, with_shift, attn_num_splits)
    return _tail_route(self, training, message, source)


def _layer_head_forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, shifted_window_attn_mask_1d=None,
                        attn_type="swin", with_shift=False, attn_num_splits=None):
    """TransformerLayer.forward as use_native_layer_heads binds it: when nothing needs a gradient the projections are one launch
    (source is target) or two (q of source, k and v of target) whose column slices the attention reads in place; then the attention
    lookup and the tail routing of use_native_layer_tails.  With a gradient needed: that binder's forward as it is."""
    return _layer_head_route(self, False, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)


def _layer_head_forward_training(self, source, target, height=None, width=None, shifted_window_attn_mask=None, shifted_window_attn_mask_1d=None,
                                 attn_type="swin", with_shift=False, attn_num_splits=None):
    """_layer_head_forward with the tail routing of use_native_layer_tails(training=True)."""
    return _layer_head_route(self, True, source, target, height, width, shifted_window_attn_mask, attn_type, with_shift, attn_num_splits)


def use_native_layer_heads(module, training=False):
    """Binds a forward on every unimatch TransformerLayer under `module` (found as use_native_transformer_layers finds them) that, when
    nothing needs a gradient, runs q_proj, k_proj and v_proj as one project_tokens launch with n = 3 when `source is target`, as one with
    n = 1 on source and one with n = 2 on target otherwise, hands the attention column slices of those buffers, and then does exactly what
    the forward of use_native_layer_tails(module, training) does behind the projections: the same attention lookup, the same tail routing.
    With grad enabled and an input or a parameter requiring it the three nn.Linear calls run as before.  LAYER_HEAD_FUSED turns the
    launches off per compute dtype and LAYER_HEAD_MIN_OUTPUTS leaves launches with too few outputs to nn.Linear.  Returns how many layers
    were bound; state_dict() keys and the classes are untouched.  The packs are kept on the layer per compute dtype and rebuilt when a
    weight's _version, data_ptr, dtype or device changes.  Raises NotImplementedError, before anything is changed, for everything
    use_native_layer_tails refuses and for a q_proj / k_proj / v_proj that is not a bias-free nn.Linear(128, 128) in float32 / float16.
    training=True: a call that needs a gradient takes the same launches through project_tokens_autograd (proj_bwd.hip behind them) for the
    compute dtypes that LAYER_HEAD_BWD_NATIVE turns on, a launch with fewer outputs than LAYER_HEAD_BWD_MIN_OUTPUTS staying nn.Linear; the
    transposed pack is cached beside the pack.  Everything else is routed as with the default."""
    fn = "use_native_layer_heads"
    layers = _checked_layers(fn, module)
    for m in layers:
        _tail_spec(fn, m)
        _head_linears(fn, m)
    bound = _layer_head_forward_training if training else _layer_head_forward
    for m in layers:
        m.forward = types.MethodType(bound, m)
    return len(layers)


def _feature_blocks(fn, transformer):
    """The blocks of a unimatch feature transformer, each a (self_attn, cross_attn_ffn) pair of layers, or NotImplementedError."""
    blocks = getattr(transformer, FT_LAYERS, None)
    if not isinstance(blocks, (nn.ModuleList, list, tuple)) or len(blocks) == 0:
        raise NotImplementedError(f"{fn}: the transformer must have a non-empty `{FT_LAYERS}` list of blocks")
    pairs = []
    for b in blocks:
        pair = (getattr(b, BLOCK_SELF, None), getattr(b, BLOCK_CROSS, None))
        if not all(p is not None and _is_layer(p) for p in pair):
            raise NotImplementedError(f"{fn}: every block must have the TransformerLayers {BLOCK_SELF} and {BLOCK_CROSS}")
        pairs.append(pair)
    return pairs


def _feature_forward(self, feature0, feature1, attn_type="swin", attn_num_splits=None, **kwargs):
    """The forward that use_native_feature_transformer binds: FeatureTransformer.forward (igs/models/unimatch/transformer.py:229-301) or
    FeatureTransformerMy.forward (:328-400) with a block's projections of its input fused, or the forward it was bound over."""
    state = self.__dict__[FT_STATE]
    pairs = _feature_blocks("FeatureTransformer", self)
    weights = [getattr(layer, a).weight for pair in pairs for layer in pair for a in (LAYER_Q, LAYER_K, LAYER_V)]
    tensors = [feature0, feature1]
    fused = (attn_type == "swin" and all(torch.is_tensor(t) and t.dim() == 4 and t.shape[1] == TAIL_D for t in tensors)
             and tuple(feature0.shape) == tuple(feature1.shape) and feature0.dtype == feature1.dtype
             and _heads_fused([t.permute(0, 2, 3, 1) for t in tensors], weights + [p for pair in pairs for layer in pair for p in _tail_params(layer)],
                              state["training"]))
    if not fused:
        return state["forward"](feature0, feature1, attn_type=attn_type, attn_num_splits=attn_num_splits, **kwargs)
    for pair in pairs:
        for layer in pair:
            _layer_served(layer, attn_type)
    training, bidirectional = state["training"], state["bidirectional"]
    b, c, h, w = feature0.shape
    feature0 = feature0.flatten(-2).permute(0, 2, 1)
    feature1 = feature1.flatten(-2).permute(0, 2, 1)
    split = attn_num_splits is not None and attn_num_splits > 1
    mask = None
    if split:
        wh, ww = h // attn_num_splits, w // attn_num_splits
        mask = getattr(sys.modules[type(self).__module__], FT_MASK)(input_resolution=(h, w), window_size_h=wh, window_size_w=ww,
                                                                   shift_size_h=wh // 2, shift_size_w=ww // 2, device=feature0.device)
    if bidirectional:
        x = torch.cat((feature0, feature1), dim=0)
    else:
        x, feature1 = feature0.contiguous(), feature1.contiguous()        # (token-major once, not once per block)
    rows = x.shape[0] * x.shape[1]
    for i, (sa, ca) in enumerate(pairs):
        geom = (h, w, mask, split and i % 2 == 1, attn_num_splits)
        sq, sk, sv = (getattr(sa, a) for a in (LAYER_Q, LAYER_K, LAYER_V))
        cq, ck, cv = (getattr(ca, a) for a in (LAYER_Q, LAYER_K, LAYER_V))
        if bidirectional:                                                  # five products of the block's input; the last two land swapped
            q, k, v, key, value = _head_project(sa, "block", x, (sq, sk, sv, ck, cv), rot=(0, 0, 0, rows // 2, rows // 2))
        else:
            q, k, v = _head_project(sa, "qkv", x, (sq, sk, sv))
            key, value = _head_project(ca, "kv", feature1, (ck, cv))
        x = _tail_route(sa, training, _layer_attention(sa, q, k, v, *geom), x)
        x = _tail_route(ca, training, _layer_attention(ca, _head_project(ca, "q", x, (cq,))[0], key, value, *geom), x)
    if not bidirectional:
        return x.view(b, h, w, c).permute(0, 3, 1, 2).contiguous()
    feature0, feature1 = x.chunk(chunks=2, dim=0)
    return feature0.view(b, h, w, c).permute(0, 3, 1, 2).contiguous(), feature1.view(b, h, w, c).permute(0, 3, 1, 2).contiguous()


def use_native_feature_transformer(transformer, bidirectional, training=False):
    """Binds the forward of a unimatch feature transformer, found by its `layers` list of blocks that each have the TransformerLayers
    self_attn and cross_attn_ffn, and use_native_layer_heads(transformer, training) on its layers; returns how many layers were bound (two
    per block).  The reference's two classes have the same attributes, so the caller says which forward it is: bidirectional=True is
    FeatureTransformer.forward (both features on the batch, each the other's target, two results), False is FeatureTransformerMy.forward
    (feature1 is every block's target and is never updated, one result).  Under no_grad with attn_type = 'swin' a block is: one
    project_tokens launch with n = 5 on the block's input (self_attn's q, k, v and cross_attn_ffn's k, v, the last two written with
    rot = rows / 2, i.e. where the block's batch-swapped target would have put them: that target is never built), self attention and its
    tail, one launch with n = 1 (cross_attn_ffn's q), cross attention on columns 384..639 of the first buffer and its tail.  With
    bidirectional=False: n = 3 on the block's input, n = 2 on feature1, n = 1.  The first cat and the final chunk / view / permute /
    contiguous stay PyTorch; the shift mask comes from generate_shift_window_attn_mask of the module that defines the transformer's class
    and the attention functions from the module that defines the layers' class, both looked up at the call, so eager and native window
    attention both work; a launch with fewer outputs than LAYER_HEAD_MIN_OUTPUTS (as shipped: the single q projection) stays nn.Linear;
    tails are routed as use_native_layer_tails(module, training) routes them.  A call that needs a gradient, another attn_type,
    or a compute dtype that LAYER_HEAD_FUSED turns off runs the forward that was bound over (whose layers are bound).  Raises
    NotImplementedError, before anything is changed, for a module without such blocks and for everything use_native_layer_heads refuses.
    training=True: a call that needs a gradient runs the same block loop for the compute dtypes that LAYER_HEAD_BWD_NATIVE turns on, its
    launches through project_tokens_autograd (n = 5 with rot, or n = 3 / 2 / 1; fewer outputs than LAYER_HEAD_BWD_MIN_OUTPUTS stay
    nn.Linear), its tails as use_native_layer_tails(training=True) routes them; a feature1 that needs no gradient gets no d x launch."""
    fn = "use_native_feature_transformer"
    pairs = _feature_blocks(fn, transformer)
    for pair in pairs:
        for layer in pair:
            _tail_spec(fn, layer)
            _head_linears(fn, layer)
    state = transformer.__dict__.get(FT_STATE)
    original = state["forward"] if state is not None else transformer.forward      # (binding twice keeps the first original)
    n = use_native_layer_heads(transformer, training)
    transformer.__dict__[FT_STATE] = dict(forward=original, bidirectional=bool(bidirectional), training=bool(training))
    transformer.forward = types.MethodType(_feature_forward, transformer)
    return n


# ---------------------------------------------------------------- the two ends of Transformer1D
def _channel_major(t):
    """t [B, C, A] as the kernels read it: stride 1 on A, a channel stride of at least A and a batch stride of at least a batch's extent
    (slices of a wider buffer included); one copy otherwise."""
    B, C, A = t.shape
    cs = t.stride(1) if C > 1 else A
    if (A == 1 or t.stride(2) == 1) and cs >= A and (B == 1 or t.stride(0) >= (C - 1) * cs + A):
        return t
    return t.contiguous()


def _token_major(t):
    """t [B, A, C] as rows with stride 1 on C and one row stride through the batches; one copy otherwise."""
    B, A, C = t.shape
    rs = t.stride(1) if A > 1 else C
    if (C == 1 or t.stride(2) == 1) and rs >= C and (B == 1 or t.stride(0) == A * rs):
        return t
    return t.contiguous()


def _ends_size_check(fn, B, C, G, A):
    if C < 1 or A < 1:
        raise ValueError(f"{fn}: C and A must be at least 1 (got C = {C}, A = {A})")
    if C > GN_MAX_C:
        raise ValueError(f"{fn}: C = {C} is above the supported {GN_MAX_C}")
    if G < 1 or C % G:
        raise ValueError(f"{fn}: num_groups = {G} must be at least 1 and divide C = {C}")
    if B * A > GN_MAX_TOKENS or (C // G) * A > GN_MAX_GROUP_ELEMS:
        raise ValueError(f"{fn}: B * A = {B * A} is above {GN_MAX_TOKENS} or (C / G) * A = {(C // G) * A} above {GN_MAX_GROUP_ELEMS}")


class _GroupNormTokens(torch.autograd.Function):
    """x: [B, C, A] channel-major; weight, bias: [C] float32 or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, num_groups, eps, out_half):
        out, stats = _ext()._gnorm.group_norm_tokens_fwd(x, num_groups, weight, bias, eps, out_half)
        ctx.save_for_backward(x, weight, stats)                    # x itself (no copy), the [B, G, 2] statistics
        ctx.num_groups = num_groups
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, stats = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        dx = dw = db = None
        if nx or nw or nb:
            dx, dw, db = _ext()._gnorm.group_norm_tokens_bwd(x, ctx.num_groups, weight, stats, _token_major(g), nx, nw and weight is not None,
                                                             nb and weight is not None)
        return dx, dw, db, None, None, None


def group_norm_tokens(x, num_groups, weight=None, bias=None, eps=1e-5, out_dtype=None):
    """F.group_norm(x, num_groups, weight, bias, eps).permute(0, 2, 1) as a contiguous [B, A, C] tensor: one launch for the statistics of
    every (example, group), one that reads x along the tokens, normalises, and writes along the channels through an LDS tile (gnorm.hip).
    x: [B, C, A] float32 or float16 on a GPU, C <= 1024; read in place when A has stride 1 (slices of a wider buffer included), copied once
    otherwise.  weight and bias: [C], both or neither (float16 parameters are widened to float32).  out_dtype (float32 or float16) defaults
    to x.dtype.  Arithmetic is float32 with the variance from centred values; a constant group gives exactly bias, a group with a NaN or
    an infinity comes out all NaN.  Autograd reaches x, weight and bias; x, weight and the [B, G, 2] statistics are saved, and the
    backward is deterministic.  Under no_grad only the statistics are allocated besides the result."""
    fn = "group_norm_tokens"
    if x.dim() != 3:
        raise ValueError(f"{fn}: x must be [B, C, A] (got {list(x.shape)})")
    B, C, A = x.shape
    _ends_size_check(fn, B, C, int(num_groups), A)
    if (weight is None) != (bias is None):
        raise ValueError(f"{fn}: weight and bias go together (both or neither)")
    named = [(x, "x")]
    if weight is not None:
        for p, name in ((weight, "weight"), (bias, "bias")):
            if tuple(p.shape) != (C,):
                raise ValueError(f"{fn}: {name} has shape {list(p.shape)}, expected {[C]}")
            named.append((p, name))
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if out_dtype not in DTYPES:
        raise NotImplementedError(f"{fn}: out_dtype must be float32 or float16 (got {out_dtype})")
    _refuse(fn, named)
    if weight is not None:
        weight, bias = weight.float(), bias.float()
    xc = _channel_major(x)
    half = out_dtype == torch.float16
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (xc, weight, bias)):
        return _GroupNormTokens.apply(xc, weight, bias, int(num_groups), float(eps), half)
    return _ext()._gnorm.group_norm_tokens_fwd(xc, int(num_groups), weight, bias, float(eps), half)[0]


class _AddResidualTokens(torch.autograd.Function):
    """tokens [B, A, C] + residual [B, C, A] -> the [B, C, A]-shaped view of a token-major buffer.  The backward launches nothing."""

    @staticmethod
    def forward(ctx, tokens, residual, out_half):
        ctx.dtypes = (tokens.dtype, residual.dtype)
        return _ext()._gnorm.tokens_add_residual(tokens, residual, out_half).permute(0, 2, 1)

    @staticmethod
    def backward(ctx, g):
        nt, nr = ctx.needs_input_grad[:2]
        return (g.permute(0, 2, 1).to(ctx.dtypes[0]) if nt else None), (g.to(ctx.dtypes[1]) if nr else None), None


def add_residual_tokens(tokens, residual):
    """tokens.permute(0, 2, 1) + residual for tokens [B, A, C] and residual [B, C, A] (float32 or float16 each, the result in their
    promoted dtype), as one launch that reads both once and writes a contiguous token-major buffer (gnorm.hip).  Returns that buffer's
    [B, C, A]-shaped permuted view: out.permute(0, 2, 1) is contiguous [B, A, C].  Both are read in place where their strides allow
    (rows with stride 1 on C; stride 1 on A), copied once otherwise.  Autograd reaches both; the backward launches nothing: d residual is
    the upstream gradient, d tokens its permuted view."""
    fn = "add_residual_tokens"
    if tokens.dim() != 3 or residual.dim() != 3:
        raise ValueError(f"{fn}: tokens must be [B, A, C] and residual [B, C, A] (got {list(tokens.shape)} and {list(residual.shape)})")
    B, A, C = tokens.shape
    if tuple(residual.shape) != (B, C, A):
        raise ValueError(f"{fn}: residual has shape {list(residual.shape)}, expected {[B, C, A]}")
    _ends_size_check(fn, B, C, 1, A)
    _refuse(fn, [(tokens, "tokens"), (residual, "residual")])
    half = torch.promote_types(tokens.dtype, residual.dtype) == torch.float16
    tm, cm = _token_major(tokens), _channel_major(residual)
    if torch.is_grad_enabled() and (tm.requires_grad or cm.requires_grad):
        return _AddResidualTokens.apply(tm, cm, half)
    return _ext()._gnorm.tokens_add_residual(tm, cm, half).permute(0, 2, 1)


def _ends_forward(self, hidden_states, encoder_hidden_states=None, timestep=None, modulation_cond=None, class_labels=None,
                  cross_attention_kwargs=None, attention_mask=None, encoder_attention_mask=None):
    """Transformer1D.forward (igs/models/transformers.py:786-908): the GroupNorm written token-major, proj_in, the blocks called as the
    reference calls them, proj_out, and the residual add written token-major.  The result is a [B, C, A]-shaped view of that buffer."""
    fn = "Transformer1D"
    for name, mask in (("attention_mask", attention_mask), ("encoder_attention_mask", encoder_attention_mask)):
        if mask is not None and mask.ndim == 2:
            raise NotImplementedError(f"{fn}: a 2-D {name} (a keep / discard mask) is not provided: pass the additive bias [batch, 1, key_tokens]")
    norm = getattr(self, T1D_NORM)
    tokens = group_norm_tokens(hidden_states, norm.num_groups, norm.weight, norm.bias, norm.eps, out_dtype=_autocast_out_dtype(None))
    tokens = getattr(self, T1D_PROJ_IN)(tokens)
    for block in getattr(self, T1D_BLOCKS):
        tokens = block(tokens, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                       encoder_attention_mask=encoder_attention_mask, timestep=timestep, modulation_cond=modulation_cond,
                       cross_attention_kwargs=cross_attention_kwargs, class_labels=class_labels)
    return add_residual_tokens(getattr(self, T1D_PROJ_OUT)(tokens), hidden_states)


def _is_transformer1d(m):
    return all(hasattr(m, a) for a in (T1D_NORM, T1D_PROJ_IN, T1D_BLOCKS, T1D_PROJ_OUT))


def use_native_transformer_ends(module):
    """Binds a forward on every Transformer1D under `module`, found by norm, proj_in, transformer_blocks and proj_out: group_norm_tokens,
    proj_in, the blocks, proj_out, add_residual_tokens; returns how many (1 for the shipped GridEncoder).  state_dict() keys and the
    classes are untouched; composes with use_native_block_ops and use_native_attention.  The result has the reference's shape, dtype and
    values but is a permuted view of a token-major buffer (add .contiguous() for the reference's layout).  Under float16 autocast the
    norm answers in float32, as eager PyTorch does.  Raises NotImplementedError, before anything is changed, for a norm that is not
    nn.GroupNorm with affine parameters and for gradient_checkpointing; a 2-D attention_mask or encoder_attention_mask raises at the
    call."""
    fn = "use_native_transformer_ends"
    found = [m for m in module.modules() if _is_transformer1d(m)]
    for m in found:
        norm = getattr(m, T1D_NORM)
        if not isinstance(norm, nn.GroupNorm) or norm.weight is None or norm.bias is None:
            raise NotImplementedError(f"{fn}: norm must be nn.GroupNorm with affine parameters (got {norm})")
        if getattr(m, T1D_CHECKPOINTING, False):
            raise NotImplementedError(f"{fn}: gradient_checkpointing is set: checkpointed blocks are not provided")
    for m in found:
        m.forward = types.MethodType(_ends_forward, m)
    return len(found)
