"""Fused attention for AGM-Net's anchor transformer on the MI355X-native library (igs_amd/csrc/attn.hip, include/igs_rast.h).

GridEncoder.conv is a Transformer1D (igs/models/transformers.py:673-907, configs/train.yaml:168-178): 4 BasicTransformerBlocks whose
self-attention runs 8 heads of 64 channels over all 8192 anchors, with no mask, no dropout and no cross-attention.  The reference reaches
it through diffusers' Attention module and its default processor (F.scaled_dot_product_attention).  `sdpa` is that product as one fused
pass on the matrix cores, with autograd; `AnchorAttnProcessor` is a processor object for the reference's Attention modules, and
`use_native_attention(model)` installs it:

    grid_encoder = GridEncoder(...)
    igs_amd.attention.use_native_attention(grid_encoder)

Deviations from the reference lines (INTEGRATION.md lists them):
  - float16: scores, running max, running sum and rescale are float32; the probabilities are rounded to half once, as the operand of the
    P V product (PyTorch's math path rounds the scores and the probabilities to half);
  - float32 runs on the exact float32 matrix instructions: no half or reduced-precision value anywhere;
  - the backward is deterministic (no float atomics; two runs agree bit for bit);
  - the processor reads to_q / to_k / to_v's token-major outputs in place and writes the result token-major for to_out: no transposes.
There is no CPU and no PyTorch fallback here: CPU tensors raise RuntimeError, bfloat16 / float64 / head sizes other than 64 raise
NotImplementedError.

The other attention of AGM-Net, the swin window attention of the unimatch motion-feature transformers (one head of 128 channels over the
K x K windows of the feature map, shifted by half a window in the odd blocks; igs/models/unimatch/attention.py:8-16 and 45-104), is
`window_attention` (igs_amd/csrc/wattn.hip): the rolls, the window split, the shift mask, the merge and the roll back are index arithmetic
inside one launch.  `single_head_split_window_attention` and `single_head_full_attention` carry the reference's signatures, and
`use_native_window_attention(namespace)` sets them on the module that binds them at import:

    import igs.models.unimatch.transformer as T
    igs_amd.attention.use_native_window_attention(T)

Not provided: the 1-D variants (single_head_full_attention_1d, single_head_split_window_attention_1d: the stereo and depth tasks),
nhead > 1 and bfloat16.
"""
import torch

from ._cabi import ext as _ext

HEAD_DIM = 64                                  # the only head size any shipped config uses
DTYPES = (torch.float32, torch.float16)
WINDOW_DIM = 128                               # the unimatch feature_channels of every shipped config, one head

# The attributes of diffusers.models.attention_processor.Attention that the processor touches, as upstream names them (diffusers is not part
# of this stack; the names are recalled from its source, like torch_cluster's constants were).
ATTN_TO_Q, ATTN_TO_K, ATTN_TO_V, ATTN_TO_OUT = "to_q", "to_k", "to_v", "to_out"
ATTN_HEADS, ATTN_SCALE = "heads", "scale"
ATTN_NORM_CROSS = "norm_cross"
ATTN_REFUSED_MODULES = ("group_norm", "spatial_norm")               # set (not None) = a configuration Transformer1D never builds
ATTN_RESIDUAL, ATTN_RESCALE = "residual_connection", "rescale_output_factor"
ATTN_SET_PROCESSOR = "set_processor"


def _acceptable(t):
    """What attn.hip reads in place: stride 1 on d, base pointer and the other strides multiples of 16 bytes (data_ptr is a host number:
    nothing is read from the device)."""
    es = t.element_size()
    return t.stride(3) == 1 and t.data_ptr() % 16 == 0 and all(s >= 0 and (s * es) % 16 == 0 for s in t.stride()[:3])


def _in_place_or_copy(t, token_major):
    if _acceptable(t):
        return t
    if token_major:
        return t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    return t.contiguous()


class _SDPA(torch.autograd.Function):
    """q [B, H, Aq, 64], k, v [B, H, Ak, 64] as indexed, any acceptable strides."""

    @staticmethod
    def forward(ctx, q, k, v, scale, token_major):
        out, lse = _ext().attn_fwd(q, k, v, scale, token_major, True)
        ctx.save_for_backward(q, k, v, out, lse)                    # the views themselves: nothing is copied
        ctx.scale, ctx.token_major = scale, token_major
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse = ctx.saved_tensors
        nq, nk, nv = ctx.needs_input_grad[:3]
        if not (nq or nk or nv):
            return None, None, None, None, None
        if g.dtype != q.dtype:
            g = g.to(q.dtype)
        g = _in_place_or_copy(g, ctx.token_major)
        dq, dk, dv = _ext().attn_bwd(q, k, v, out, lse, g, ctx.scale, ctx.token_major, nq, nk, nv)
        return dq, dk, dv, None, None


def sdpa(q, k, v, scale=None, layout="bhad"):
    """softmax(scale * q k^T) v as one fused pass (attn.hip); out has q's shape, layout and dtype.

    layout "bhad": q [B, H, Aq, 64], k, v [B, H, Ak, 64]; layout "bahd": q [B, Aq, H, 64], k, v [B, Ak, H, 64], e.g. the views
    `to_q(x).view(B, A, H, 64)` of token-major projections or slices of one fused QKV buffer.  Either way any strides are read in place as
    long as d has stride 1 and the base pointer and the other strides are multiples of 16 bytes; anything else is copied once.
    float32 or float16 (the same for all three); scale defaults to 1 / sqrt(64).  Aq != Ak is fine; there is no mask and no dropout.
    Under no_grad nothing is saved and the log-sum-exp is not written; with a gradient q, k, v, out (as views) and lse [B, H, Aq] float32 are
    kept, the backward recomputes the probabilities from lse and is bitwise reproducible.  No host synchronisation anywhere."""
    fn = "sdpa"
    if layout not in ("bhad", "bahd"):
        raise ValueError(f"{fn}: layout must be 'bhad' or 'bahd' (got {layout!r})")
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"{fn}: q, k, v must have four dimensions (got {list(q.shape)}, {list(k.shape)}, {list(v.shape)})")
    token_major = layout == "bahd"
    if token_major:
        q, k, v = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    B, H, Aq, D = q.shape
    if tuple(k.shape) != tuple(v.shape) or k.shape[0] != B or k.shape[1] != H or k.shape[3] != D:
        raise ValueError(f"{fn}: k and v must be [B, H, Ak, D] with q's B, H, D = {[B, H, D]} (got {list(k.shape)}, {list(v.shape)} as [B, H, A, D])")
    if Aq < 1 or k.shape[2] < 1 or H < 1:
        raise ValueError(f"{fn}: empty q or k (Aq = {Aq}, Ak = {k.shape[2]}, H = {H})")
    if q.dtype not in DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise NotImplementedError(f"{fn}: q, k, v must all be float32 or all float16 (got {q.dtype}, {k.dtype}, {v.dtype})")
    if D != HEAD_DIM:
        raise NotImplementedError(f"{fn}: the head size must be {HEAD_DIM} (got {D})")
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    scale = float(D) ** -0.5 if scale is None else float(scale)
    q, k, v = _in_place_or_copy(q, token_major), _in_place_or_copy(k, token_major), _in_place_or_copy(v, token_major)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        out = _SDPA.apply(q, k, v, scale, token_major)
    else:
        out = _ext().attn_fwd(q, k, v, scale, token_major, False)[0]
    return out.permute(0, 2, 1, 3) if token_major else out


class AnchorAttnProcessor:
    """An attention processor (diffusers' protocol) for the reference's Attention modules that does exactly what Transformer1D needs:
    to_q / to_k / to_v on [B, A, C], the native fused attention with attn.scale and attn.heads on the token-major views (no transposes),
    to_out[0], to_out[1].  Everything else raises NotImplementedError: an attention mask, encoder_hidden_states with norm_cross, 4-D inputs,
    group_norm / spatial_norm / residual_connection / rescale_output_factor != 1, and a dropout probability > 0 in training mode.

    Measured on one MI355X (H = 8, A = 8192, B = 1 and 5): in float32 faster than F.scaled_dot_product_attention as
    dispatched in every case (attention forward 1.37 x / 1.10 x, forward + backward 1.17 x / 1.10 x, a whole block 1.07-1.26 x).  In float16
    SLOWER than the dispatched call, a library flash kernel, in every case: forward 0.61 x / 0.50 x, forward + backward 0.90 x / 0.80 x,
    a whole block 0.74 x / 0.66 x forward and 0.90 x / 0.88 x with its backward.  Against SDPBackend.MATH faster in all cases, both dtypes.
    So install it for float32; for float16 it brings a deterministic backward and no transposes, not time."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kwargs):
        fn = "AnchorAttnProcessor"
        if attention_mask is not None:
            raise NotImplementedError(f"{fn}: attention masks are not provided")
        if hidden_states.dim() == 4:
            raise NotImplementedError(f"{fn}: 4-D inputs are not provided (Transformer1D passes [B, A, C])")
        if hidden_states.dim() != 3:
            raise ValueError(f"{fn}: hidden_states must be [B, A, C] (got {list(hidden_states.shape)})")
        if encoder_hidden_states is not None and getattr(attn, ATTN_NORM_CROSS, None):
            raise NotImplementedError(f"{fn}: encoder_hidden_states with norm_cross is not provided")
        for name in ATTN_REFUSED_MODULES:
            if getattr(attn, name, None) is not None:
                raise NotImplementedError(f"{fn}: attn.{name} is not provided")
        if getattr(attn, ATTN_RESIDUAL, False):
            raise NotImplementedError(f"{fn}: residual_connection is not provided")
        if getattr(attn, ATTN_RESCALE, 1.0) != 1.0:
            raise NotImplementedError(f"{fn}: rescale_output_factor != 1 is not provided")
        to_out = getattr(attn, ATTN_TO_OUT)
        if getattr(attn, "training", False) and any(float(getattr(m, "p", 0.0)) > 0.0 for m in to_out):
            raise NotImplementedError(f"{fn}: dropout with p > 0 in training mode is not provided")
        context = hidden_states if encoder_hidden_states is None else encoder_hidden_states
        q = getattr(attn, ATTN_TO_Q)(hidden_states)
        k = getattr(attn, ATTN_TO_K)(context)
        v = getattr(attn, ATTN_TO_V)(context)
        heads = int(getattr(attn, ATTN_HEADS))
        B, A, C = q.shape
        if C % heads:
            raise ValueError(f"{fn}: {C} channels do not divide into {heads} heads")
        D = C // heads
        out = sdpa(q.view(B, A, heads, D), k.view(B, k.shape[1], heads, D), v.view(B, v.shape[1], heads, D),
                   scale=float(getattr(attn, ATTN_SCALE)), layout="bahd")
        out = out.reshape(B, A, C)                                  # (a view: sdpa wrote it token-major)
        return to_out[1](to_out[0](out))


def use_native_attention(module):
    """Installs AnchorAttnProcessor on every submodule that has set_processor (the reference's Attention modules); returns how many."""
    n = 0
    for m in module.modules():
        setter = getattr(m, ATTN_SET_PROCESSOR, None)
        if callable(setter):
            setter(AnchorAttnProcessor())
            n += 1
    return n


# ---------------------------------------------------------------- swin window attention (wattn.hip)
def _acceptable3(t):
    """What wattn.hip reads in place: a [B, L, 128] view with stride 1 on d, base pointer and the other strides multiples of 16 bytes."""
    es = t.element_size()
    return t.stride(2) == 1 and t.data_ptr() % 16 == 0 and all(s >= 0 and (s * es) % 16 == 0 for s in t.stride()[:2])


class _WindowAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, h, w, num_splits, with_shift, scale):
        out, lse = _ext()._window.window_attn_fwd(q, k, v, h, w, num_splits, with_shift, scale, True)
        ctx.save_for_backward(q, k, v, out, lse)                    # the views themselves: nothing is copied
        ctx.geom = (h, w, num_splits, with_shift, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, lse = ctx.saved_tensors
        nq, nk, nv = ctx.needs_input_grad[:3]
        if not (nq or nk or nv):
            return (None,) * 8
        if g.dtype != q.dtype:
            g = g.to(q.dtype)
        if not _acceptable3(g):
            g = g.contiguous()
        dq, dk, dv = _ext()._window.window_attn_bwd(q, k, v, out, lse, g, *ctx.geom, nq, nk, nv)
        return dq, dk, dv, None, None, None, None, None


def window_attention(q, k, v, h, w, num_splits=1, with_shift=False, scale=None):
    """softmax(scale * q k^T + mask) v inside every one of the num_splits x num_splits windows of the h x w map, as one fused pass
    (wattn.hip).  q, k, v: [B, h * w, 128] in the map's own token order, float32 or float16 (the same for all three); out is contiguous
    [B, h * w, 128] in q's dtype, in the same token order.  with_shift rolls the map by half a window before the split and back after the
    merge and adds -100 to the scaled score of every pair of tokens from different regions of the rolled map, exactly what
    generate_shift_window_attn_mask builds (igs/models/unimatch/utils.py:84-108): the mask is regenerated from h, w and num_splits by index
    arithmetic, none is read.  scale defaults to 128 ** -0.5.  Views with stride 1 on the channels whose base pointer and other strides are
    multiples of 16 bytes, e.g. the three slices of one fused [B, L, 384] projection, are read in place; anything else is copied once.
    Under no_grad nothing is saved and the log-sum-exp is not written; with a gradient q, k, v, out (as views) and lse [B, h * w] float32
    are kept, the backward recomputes the probabilities from lse and is bitwise reproducible.  No host synchronisation anywhere.
    num_splits = 1 is single_head_full_attention.

    Measured on one MI355X (64 x 64 map, num_splits = 2, medians of 20 alternating calls) against the reference's own
    sequence of operations (rolls, split copies, matmul, mask add, softmax, matmul, merge, roll back): the forward at B = 8 holds in all
    four cases (float32 0.21 against 0.31 ms unshifted and 0.46 ms shifted: 1.45 x / 2.18 x; float16 0.10 against 0.17 / 0.30 ms: 1.63 x /
    2.89 x); forward + backward at B = 4 holds in float16 (0.34 against 0.49 ms, 0.37 against 0.50 ms shifted: 1.44 x / 1.36 x) and DOES
    NOT HOLD in float32, where the native path is SLOWER (0.72 against 0.60 ms, 0.75 against 0.65 ms shifted: 0.83 x / 0.87 x).  Peak
    memory is the output (+ lse): 17 MB against 352-369 MB forward in float32.  Against F.scaled_dot_product_attention on windows split
    beforehand (rolls and copies not timed) float32 is 1.06-1.44 x ahead, float16 0.49-0.76 x behind except the shifted forward (1.10 x)."""
    fn = "window_attention"
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError(f"{fn}: q, k, v must have three dimensions [B, h * w, C] (got {list(q.shape)}, {list(k.shape)}, {list(v.shape)})")
    if tuple(k.shape) != tuple(q.shape) or tuple(v.shape) != tuple(q.shape):
        raise ValueError(f"{fn}: q, k, v must share one shape (got {list(q.shape)}, {list(k.shape)}, {list(v.shape)})")
    h, w, num_splits = int(h), int(w), int(num_splits)
    B, L, C = q.shape
    if h < 1 or w < 1 or h * w != L:
        raise ValueError(f"{fn}: h * w = {h} * {w} is not the token count {L}")
    if num_splits < 1 or h % num_splits or w % num_splits:
        raise ValueError(f"{fn}: h = {h} and w = {w} do not split into {num_splits} windows each")
    with_shift = bool(with_shift)
    if with_shift and (h // num_splits < 2 or w // num_splits < 2):
        raise ValueError(f"{fn}: a shifted call needs windows of at least 2 x 2 tokens (got {h // num_splits} x {w // num_splits})")
    if q.dtype not in DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise NotImplementedError(f"{fn}: q, k, v must all be float32 or all float16 (got {q.dtype}, {k.dtype}, {v.dtype})")
    if C != WINDOW_DIM:
        raise NotImplementedError(f"{fn}: the channel count must be {WINDOW_DIM} (got {C})")
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise RuntimeError(f"{fn}: tensors must be on a GPU (no CPU fallback)")
    scale = float(C) ** -0.5 if scale is None else float(scale)
    q, k, v = (t if _acceptable3(t) else t.contiguous() for t in (q, k, v))
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return _WindowAttention.apply(q, k, v, h, w, num_splits, with_shift, scale)
    return _ext()._window.window_attn_fwd(q, k, v, h, w, num_splits, with_shift, scale, False)[0]


def single_head_full_attention(q, k, v):
    """The reference's signature (igs/models/unimatch/attention.py:8-16): full attention over all L tokens, scale 1 / sqrt(C)."""
    if q.dim() != 3:
        raise ValueError(f"single_head_full_attention: q, k, v must be [B, L, C] (got {list(q.shape)})")
    return window_attention(q, k, v, 1, q.shape[1], num_splits=1, with_shift=False)


def single_head_split_window_attention(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None):
    """The reference's signature (igs/models/unimatch/attention.py:45-104).  With with_shift an attn_mask must be given, as in the
    reference, and must have the shape [num_splits ** 2, (h / num_splits) * (w / num_splits), the same]; its VALUES ARE NOT READ: the
    kernel regenerates the mask of generate_shift_window_attn_mask from h, w and num_splits, so a mask with other values is ignored."""
    fn = "single_head_split_window_attention"
    if h is None or w is None:
        raise ValueError(f"{fn}: h and w must be given")
    if with_shift:
        if attn_mask is None:
            raise ValueError(f"{fn}: with_shift needs attn_mask (its shape is checked, its values are regenerated)")
        K = int(num_splits)
        lw = (int(h) // K) * (int(w) // K) if K >= 1 else -1
        if tuple(attn_mask.shape) != (K * K, lw, lw):
            raise ValueError(f"{fn}: attn_mask must have shape {[K * K, lw, lw]} (got {list(attn_mask.shape)})")
    return window_attention(q, k, v, h, w, num_splits=num_splits, with_shift=with_shift)


def use_native_window_attention(namespace):
    """Sets single_head_full_attention and single_head_split_window_attention on `namespace`, the module object whose globals the callers
    look them up in (igs.models.unimatch.transformer binds both names at import, so patch that module, not unimatch.attention); returns
    how many names were set.  Names the namespace does not have are not added."""
    n = 0
    for f in (single_head_full_attention, single_head_split_window_attention):
        if hasattr(namespace, f.__name__):
            setattr(namespace, f.__name__, f)
            n += 1
    return n
