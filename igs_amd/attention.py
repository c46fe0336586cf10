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
"""
import torch

from ._cabi import ext as _ext

HEAD_DIM = 64                                  # the only head size any shipped config uses
DTYPES = (torch.float32, torch.float16)

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
