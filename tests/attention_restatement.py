"""A float64 restatement of the attention of GridEncoder.conv's Transformer1D (igs/models/transformers.py:673-907: softmax(scale q k^T) v,
no mask, no dropout), and the error bounds the tests use for igs_amd/csrc/attn.hip.

  restate          -- explicit matmul, softmax, matmul; returns every intermediate the bounds need.  The backward is autograd through it
                      (`gradients`); `explicit_gradients` is the second statement (d V = P^T d O, d S = P (d P - delta), ...).
  forward_bound    -- per-element bound on |native out - float64 out| for the float16 and the float32 instance.
  backward_bounds  -- per-element bounds on d q, d k, d v.
  half_pipeline    -- CPU / any-device emulations of the half pipeline and of its two wrong variants (scale 1 / D; scores rounded to half).
  Stand-ins for diffusers' Attention module (AttentionStandIn) for the processor tests.

All bounds are derived from operation counts of the kernels' arithmetic, never measured.  u32 = 2^-24 and u16 = 2^-11 are the unit
roundoffs.  Notation: s_ij = scale q_i . k_j, p = softmax_j(s), o = p v, a_ij = sum_d |q_id| |k_jd|.

Forward.  A score is a float32 fma chain of D = 64 products (D u32 a_ij), multiplied once by the rounded constant scale log2(e) (2 u32) and
reduced by the running max (1 u32): |d s_ij| <= ds_ij = (D + 3) u32 scale a_ij.  exp2 is good to one ulp.  A weight p_ij = e_ij / l_i
then has relative error <= 2 max_j ds_ij (numerator and denominator) + the roundings of the sums: the running sum l and the accumulator o
each take Ak additions (half instance, as the issue states it: Ak + 16; float instance: also one rescale multiplication per 32 keys, so
Ak + Ak / 32 + 16), and the operand rounding up = u16 (P rounded to half once) or 2 u32 (the exp2 ulp).  The output is rounded once
(uo = u16 or u32, the division).  The leading factor 2 covers the second-order terms:
    |d o_id| <= 2 (2 max_j ds_ij + n_acc u32 + up) sum_j p_ij |v_jd| + uo |o_id|.

Backward.  P is recomputed as exp2(s c - lse log2 e): the exponent carries the score error again (with the rounded constant and the fma's
rounding: (D + 5) u32 scale a_ij), the forward's error of lse (max_j ds_ij + (n_acc + 4) u32) and the roundings of lse itself (stored, times
log2 e, subtracted: 3 u32 |lse_i|); so |d p_ij| <= 2 ep_ij p_ij with ep_ij = (D + 5) u32 scale a_ij + max_j ds_ij + (n_acc + 6) u32 +
3 u32 |lse_i|.  d P = d O V^T is a float32 chain of D products: |d dP_ij| <= D u32 sum_d |dO_id| |v_jd|.  delta_i = sum_d dO_id o_id is
taken from the kernel's own output: |d delta_i| <= sum_d |dO_id| (forward bound)_id + (D + 1) u32 sum_d |dO_id| |o_id|.  Then
    |d dS_ij| <= E_ij = 2 ep_ij p_ij |dP_ij - delta_i| + p_ij (|d dP_ij| + |d delta_i|) + (2 u32 + uh) |dS_ij|
(uh = u16 where dS and P are rounded to half as matrix operands, 0 in float32), and with n = the number of summed rows
    |d dq_id| <= 2 scale (sum_j E_ij |k_jd| + (Ak + 2) u32 sum_j |dS_ij| |k_jd|) + uo |dq_id|     (d k likewise over the queries)
    |d dv_jd| <= 2 (sum_i (2 ep_ij + uh) p_ij |dO_id| + (Aq + 2) u32 sum_i p_ij |dO_id|) + uo |dv_jd|.
Half has a floor: below its smallest normal number 2^-14 the spacing is 2^-24, so a rounding to half errs by up to max(u16 |x|, 2^-25).
Weights and gradients of far-away keys are that small (p_ij ~ 1e-6 is common at |scaled score| ~ 11), so in the half instance every
rounding to half of the backward carries the absolute term ah = 2^-25 next to its relative one: d S_ij and p_ij as matrix operands
(E_ij + ah; (2 ep_ij + uh) p_ij + ah) and the three stored gradients (uo |x| + ah).  In float32 ah = 0 (the float32 floor, 2^-150, is
far below every term).
"""
import math

import torch

u32 = 2.0 ** -24
u16 = 2.0 ** -11
AH = 2.0 ** -25            # half the spacing of half's subnormals: the absolute error of a rounding to half below 2^-14
D = 64


def restate(q, k, v, scale):
    """q [..., Aq, D], k, v [..., Ak, D] float64 -> dict(s, p, o, lse)."""
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    return dict(s=s, p=p, o=torch.matmul(p, v), lse=(m + torch.log(l)).squeeze(-1))


def gradients(q, k, v, scale, dout):
    """(d q, d k, d v) by autograd through `restate`, float64."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = restate(q, k, v, scale)["o"]
    return torch.autograd.grad(o, (q, k, v), dout)


def explicit_gradients(q, k, v, scale, dout, r=None):
    r = restate(q, k, v, scale) if r is None else r
    dp = torch.matmul(dout, v.transpose(-1, -2))
    delta = (dout * r["o"]).sum(-1, keepdim=True)
    ds = r["p"] * (dp - delta)
    return dict(dq=scale * torch.matmul(ds, k), dk=scale * torch.matmul(ds.transpose(-1, -2), q), dv=torch.matmul(r["p"].transpose(-1, -2), dout),
                dp=dp, delta=delta, ds=ds)


def _units(dtype):
    half = dtype == torch.float16
    return half, (u16 if half else 2 * u32), (u16 if half else u32)


def _n_acc(Ak, half):
    return Ak + 16 if half else Ak + (Ak + 31) // 32 + 16


def forward_bound(q, k, v, scale, dtype, r=None):
    """Per-element bound on |native out - float64 out|; q, k, v float64 (the widened inputs)."""
    r = restate(q, k, v, scale) if r is None else r
    half, up, uo = _units(dtype)
    a = torch.matmul(q.abs(), k.abs().transpose(-1, -2))
    ds = ((D + 3) * u32 * abs(scale)) * a.max(-1, keepdim=True).values
    rel = 2 * ds + _n_acc(k.shape[-2], half) * u32 + up
    return 2 * rel * torch.matmul(r["p"], v.abs()) + uo * r["o"].abs()


def backward_bounds(q, k, v, scale, dout, dtype, r=None):
    """Per-element bounds (bq, bk, bv) on |native gradient - float64 gradient|."""
    r = restate(q, k, v, scale) if r is None else r
    g = explicit_gradients(q, k, v, scale, dout, r)
    half, up, uo = _units(dtype)
    uh = u16 if half else 0.0
    ah = AH if half else 0.0
    Aq, Ak = q.shape[-2], k.shape[-2]
    sc = abs(scale)
    a = torch.matmul(q.abs(), k.abs().transpose(-1, -2))
    ds_max = ((D + 3) * u32 * sc) * a.max(-1, keepdim=True).values
    ep = ((D + 5) * u32 * sc) * a + ds_max + (_n_acc(Ak, half) + 6) * u32 + 3 * u32 * r["lse"].abs().unsqueeze(-1)
    del a
    p = r["p"]
    e_dp = D * u32 * torch.matmul(dout.abs(), v.abs().transpose(-1, -2))
    e_delta = (dout.abs() * forward_bound(q, k, v, scale, dtype, r)).sum(-1, keepdim=True) + (D + 1) * u32 * (dout.abs() * r["o"].abs()).sum(-1, keepdim=True)
    E = 2 * ep * p * (g["dp"] - g["delta"]).abs() + p * (e_dp + e_delta) + (2 * u32 + uh) * g["ds"].abs() + ah
    del e_dp
    dsa = g["ds"].abs()
    bq = 2 * sc * (torch.matmul(E, k.abs()) + (Ak + 2) * u32 * torch.matmul(dsa, k.abs())) + uo * g["dq"].abs() + ah
    bk = 2 * sc * (torch.matmul(E.transpose(-1, -2), q.abs()) + (Aq + 2) * u32 * torch.matmul(dsa.transpose(-1, -2), q.abs())) + uo * g["dk"].abs() + ah
    del E, dsa
    w = (2 * ep + uh + (Aq + 2) * u32) * p + ah
    bv = 2 * torch.matmul(w.transpose(-1, -2), dout.abs()) + uo * g["dv"].abs() + ah
    return bq, bk, bv


def half_pipeline(q, k, v, scale, variant="right"):
    """The half instance's arithmetic emulated with torch ops on half inputs: float32 scores, P rounded to half once, float32 P V, half
    output.  variant "scale_1_over_D": the softmax scale 1 / D instead of `scale`; "half_scores": the scores rounded to half before the
    softmax.  Returns float64."""
    assert q.dtype == torch.float16
    if variant == "scale_1_over_D":
        scale = 1.0 / q.shape[-1]
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if variant == "half_scores":
        s = s.half().float()
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    o = torch.matmul(e.half().float(), v.float()) / l
    return o.half().double()


def random_inputs(B, H, Aq, Ak, dtype, device, seed=0, with_dout=False):
    """q, k = 1.5 randn, v = randn + 0.3 (|scaled score| reaches about 11 at scale 1 / 8), as [B, H, A, D] in `dtype`."""
    g = torch.Generator().manual_seed(seed)
    q = (1.5 * torch.randn(B, H, Aq, D, generator=g)).to(dtype).to(device)
    k = (1.5 * torch.randn(B, H, Ak, D, generator=g)).to(dtype).to(device)
    v = (torch.randn(B, H, Ak, D, generator=g) + 0.3).to(dtype).to(device)
    if with_dout:
        return q, k, v, torch.randn(B, H, Aq, D, generator=g).to(dtype).to(device)
    return q, k, v


class AttentionStandIn(torch.nn.Module):
    """What AnchorAttnProcessor touches of diffusers' Attention module, under upstream's attribute names."""

    def __init__(self, channels=512, heads=8, dropout=0.0, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.heads = heads
        self.scale = (channels // heads) ** -0.5
        self.to_q = torch.nn.Linear(channels, channels, bias=False)
        self.to_k = torch.nn.Linear(channels, channels, bias=False)
        self.to_v = torch.nn.Linear(channels, channels, bias=False)
        self.to_out = torch.nn.ModuleList([torch.nn.Linear(channels, channels), torch.nn.Dropout(dropout)])
        self.norm_cross = None
        self.group_norm = None
        self.spatial_norm = None
        self.residual_connection = False
        self.rescale_output_factor = 1.0
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (channels ** -0.5))
        self.processor = None

    def set_processor(self, processor):
        self.processor = processor

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask)

    def restated(self, x):
        """The same module function through `restate`, in x's dtype (use float64)."""
        B, A, C = x.shape
        H = self.heads
        sp = lambda t: t.view(B, A, H, C // H).permute(0, 2, 1, 3)
        o = restate(sp(self.to_q(x)), sp(self.to_k(x)), sp(self.to_v(x)), self.scale)["o"]
        return self.to_out[1](self.to_out[0](o.permute(0, 2, 1, 3).reshape(B, A, C)))
