"""A float64 restatement of the swin window attention of the unimatch motion-feature transformers (single_head_split_window_attention,
igs/models/unimatch/attention.py:45-104, with the mask of generate_shift_window_attn_mask, igs/models/unimatch/utils.py:84-108; K = 1 is
single_head_full_attention, attention.py:8-16), and the error bounds the tests use for igs_amd/csrc/wattn.hip.

  token_map           -- the gather form: the original token and the region of token j of every window (include/igs_rast.h states both).
  restate             -- gather, explicit matmul, mask addend, softmax, matmul, scatter; returns every intermediate the bounds need.
  restate_roll        -- the second statement: roll, view / permute split, a mask painted by slices, merge, roll back.
  gradients           -- autograd through `restate`; `explicit_gradients` is the second statement of the backward.
  forward_bound, backward_bounds -- per-element bounds on |native - float64| for the float16 and the float32 instance.
  half_pipeline       -- emulation of the half pipeline with torch ops, and of three wrong variants: "no_mask" (the mask ignored),
                         "roll_sign" (the roll's sign flipped), "hw_swapped" (h and w swapped in the window arithmetic).
  TransformerLayerStandIn -- what unimatch's TransformerLayer does around the attention, looking the function up in a namespace.

The restatement is generic in the channel count C (the golden file has C = 16; the kernels have C = 128).

Bounds.  They are attention_restatement.py's, derived from operation counts of the kernels' arithmetic and never measured, with three
changes.  u32 = 2^-24 and u16 = 2^-11 are the unit roundoffs; s_ij = scale q_i . k_j + mask_ij, p = softmax_j(s), o = p v,
a_ij = sum_d |q_id| |k_jd|; all sums run over the Lw tokens of one window.
  (1) D is the channel count (128): a score is one float32 fma chain of D products.
  (2) The sum length is the window length Lw: n_acc = Lw + 16 (half) or Lw + ceil(Lw / 32) + 16 (float).
  (3) The mask addend M = 100 enters the exponent inside the fma that scales the score, so that rounding and the rounding of the
      subtraction of the running max act on a number of size scale a_ij + M instead of scale a_ij: in a shifted call
          ds_ij = (D + 3) u32 scale a_ij + 2 u32 M.
      The backward recomputes the exponent as fma(s, c, mask) - lse log2 e where the unmasked kernel has one fma: one more rounding of a
      number of that size, ep_ij = (D + 5) u32 scale a_ij + 3 u32 M + max_j ds_ij + (n_acc + 6) u32 + 3 u32 |lse_i|.
  Forward:   |d o_id| <= 2 (2 max_j ds_ij + n_acc u32 + up) sum_j p_ij |v_jd| + uo |o_id| + ah sum_j |v_jd|
  (up = u16 or 2 u32, uo = u16 or u32).  The last term is half's floor: a weight e_ij = exp2(.) <= 1 below half's smallest normal number
  is rounded with an absolute error up to ah = 2^-25, not a relative one (masked pairs, e^-100, are flushed to zero entirely), and the
  row sum that divides it is >= 1; in float32 ah = 0.
  Backward: as attention_restatement.py states it (E_ij, the three gradient bounds and half's floor ah on every rounding to half), with
  the ep_ij above and sums over the window.
"""
import torch

u32 = 2.0 ** -24
u16 = 2.0 ** -11
AH = 2.0 ** -25
MASK = 100.0


# ---------------------------------------------------------------- geometry
def token_map(h, w, K, shift, variant="right"):
    """(tok, region): [K * K, Lw] long tensors; window wy * K + wx, token j -> original token y * w + x, and the region of its rolled
    position.  variant "roll_sign" rolls the other way (a wrong variant for the tests)."""
    assert h % K == 0 and w % K == 0
    wh, ww = h // K, w // K
    sh, sw = (wh // 2, ww // 2) if shift else (0, 0)
    j = torch.arange(wh * ww)
    wy, wx = torch.arange(K).repeat_interleave(K), torch.arange(K).repeat(K)
    yp = wy[:, None] * wh + (j // ww)[None]
    xp = wx[:, None] * ww + (j % ww)[None]
    sgn = -1 if variant == "roll_sign" else 1
    tok = ((yp + sgn * sh) % h) * w + (xp + sgn * sw) % w
    rh = (yp >= h - wh).long() + (yp >= h - sh).long()
    rw = (xp >= w - ww).long() + (xp >= w - sw).long()
    return tok, 3 * rh + rw


def gather(t, tok):
    """[B, L, C] -> [B, K * K, Lw, C]"""
    return t[:, tok.reshape(-1).to(t.device)].reshape(t.shape[0], tok.shape[0], tok.shape[1], *t.shape[2:])


def scatter(tw, tok):
    """[B, K * K, Lw, ...] -> [B, L, ...] in original token order"""
    out = torch.empty(tw.shape[0], tok.numel(), *tw.shape[3:], dtype=tw.dtype, device=tw.device)
    out[:, tok.reshape(-1).to(tw.device)] = tw.reshape(tw.shape[0], tok.numel(), *tw.shape[3:])
    return out


def mask_of(region, shift, dtype, device):
    """[K * K, Lw, Lw]: -100 where the regions differ (shifted), zeros otherwise"""
    if not shift:
        return torch.zeros(region.shape[0], region.shape[1], region.shape[1], dtype=dtype, device=device)
    r = region.to(device)
    return (r[:, :, None] != r[:, None, :]).to(dtype) * -MASK


# ---------------------------------------------------------------- the function
def restate_windows(qw, kw, vw, mask, scale):
    s = torch.matmul(qw, kw.transpose(-1, -2)) * scale + mask
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    return dict(s=s, p=p, ow=torch.matmul(p, vw), lsew=(m + torch.log(l)).squeeze(-1))


def restate(q, k, v, h, w, K=1, shift=False, scale=None, variant="right"):
    """q, k, v [B, h w, C] float64 -> dict(o [B, L, C], lse [B, L], and the windowed s, p, ow, qw, kw, vw, tok, mask)."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    if variant == "hw_swapped":
        tok, region = token_map(w, h, K, shift)
    else:
        tok, region = token_map(h, w, K, shift, variant)
    mask = mask_of(region, shift and variant != "no_mask", q.dtype, q.device)
    qw, kw, vw = gather(q, tok), gather(k, tok), gather(v, tok)
    r = restate_windows(qw, kw, vw, mask, scale)
    r.update(o=scatter(r["ow"], tok), lse=scatter(r["lsew"], tok), qw=qw, kw=kw, vw=vw, tok=tok, mask=mask, scale=scale)
    return r


def paint_mask(h, w, K):
    """The shift mask painted by slices on the rolled map and split into windows: [K * K, Lw, Lw]."""
    wh, ww = h // K, w // K
    img = torch.zeros(h, w, dtype=torch.float64)
    n = 0
    for ys in (slice(0, -wh), slice(-wh, -(wh // 2)), slice(-(wh // 2), None)):
        for xs in (slice(0, -ww), slice(-ww, -(ww // 2)), slice(-(ww // 2), None)):
            img[ys, xs] = n
            n += 1
    win = img.view(K, wh, K, ww).permute(0, 2, 1, 3).reshape(K * K, wh * ww)
    return (win[:, None, :] != win[:, :, None]).double() * -MASK


def restate_roll(q, k, v, h, w, K=1, shift=False, scale=None):
    """The second statement: [B, L, C] -> [B, L, C] by roll, split, attention per window, merge, roll back."""
    B, L, C = q.shape
    scale = C ** -0.5 if scale is None else scale
    wh, ww = h // K, w // K

    def split(t):
        t = t.view(B, h, w, C)
        if shift:
            t = torch.roll(t, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
        return t.view(B, K, wh, K, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, K * K, wh * ww, C)

    qs, ks, vs = split(q), split(k), split(v)
    s = torch.matmul(qs, ks.transpose(-1, -2)) * scale
    if shift:
        s = s + paint_mask(h, w, K).to(s)
    o = torch.matmul(torch.softmax(s, -1), vs)
    o = o.view(B, K, K, wh, ww, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h, w, C)
    if shift:
        o = torch.roll(o, shifts=(wh // 2, ww // 2), dims=(1, 2))
    return o.reshape(B, L, C)


def gradients(q, k, v, h, w, K, shift, dout, scale=None):
    """(d q, d k, d v) by autograd through `restate`, float64."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = restate(q, k, v, h, w, K, shift, scale)["o"]
    return torch.autograd.grad(o, (q, k, v), dout)


def explicit_gradients(r, dout):
    """The second statement of the backward from restate's dict: d V = P^T d O, d S = P (d P - delta), d Q = scale d S K, d K = scale d S^T Q,
    scattered back; also the windowed dp, delta, ds, dow."""
    dow = gather(dout, r["tok"])
    dp = torch.matmul(dow, r["vw"].transpose(-1, -2))
    delta = (dow * r["ow"]).sum(-1, keepdim=True)
    ds = r["p"] * (dp - delta)
    sc, tok = r["scale"], r["tok"]
    return dict(dq=scatter(sc * torch.matmul(ds, r["kw"]), tok), dk=scatter(sc * torch.matmul(ds.transpose(-1, -2), r["qw"]), tok),
                dv=scatter(torch.matmul(r["p"].transpose(-1, -2), dow), tok), dp=dp, delta=delta, ds=ds, dow=dow)


# ---------------------------------------------------------------- bounds
def _units(dtype):
    half = dtype == torch.float16
    return half, (u16 if half else 2 * u32), (u16 if half else u32)


def _n_acc(Lw, half):
    return Lw + 16 if half else Lw + (Lw + 31) // 32 + 16


def _forward_bound_windows(r, dtype, shift):
    half, up, uo = _units(dtype)
    D, Lw, sc = r["qw"].shape[-1], r["kw"].shape[-2], abs(r["scale"])
    a = torch.matmul(r["qw"].abs(), r["kw"].abs().transpose(-1, -2))
    ds = ((D + 3) * u32 * sc) * a.max(-1, keepdim=True).values + (2 * u32 * MASK if shift else 0.0)
    rel = 2 * ds + _n_acc(Lw, half) * u32 + up
    floor = AH * r["vw"].abs().sum(-2, keepdim=True) if half else 0.0
    return 2 * rel * torch.matmul(r["p"], r["vw"].abs()) + uo * r["ow"].abs() + floor


def forward_bound(r, dtype, shift):
    """Per-element bound on |native out - float64 out|, [B, L, C]; r = restate(...) of the widened inputs."""
    return scatter(_forward_bound_windows(r, dtype, shift), r["tok"])


def backward_bounds(r, dout, dtype, shift):
    """Per-element bounds (bq, bk, bv) on |native gradient - float64 gradient|, [B, L, C] each."""
    g = explicit_gradients(r, dout)
    half, up, uo = _units(dtype)
    uh = u16 if half else 0.0
    ah = AH if half else 0.0
    qw, kw, vw, p, tok = r["qw"], r["kw"], r["vw"], r["p"], r["tok"]
    D, Lw, sc = qw.shape[-1], kw.shape[-2], abs(r["scale"])
    m = MASK if shift else 0.0
    a = torch.matmul(qw.abs(), kw.abs().transpose(-1, -2))
    ds_max = ((D + 3) * u32 * sc) * a.max(-1, keepdim=True).values + 2 * u32 * m
    ep = ((D + 5) * u32 * sc) * a + 3 * u32 * m + ds_max + (_n_acc(Lw, half) + 6) * u32 + 3 * u32 * r["lsew"].abs().unsqueeze(-1)
    del a
    dow = g["dow"]
    e_dp = D * u32 * torch.matmul(dow.abs(), vw.abs().transpose(-1, -2))
    e_delta = (dow.abs() * _forward_bound_windows(r, dtype, shift)).sum(-1, keepdim=True) + (D + 1) * u32 * (dow.abs() * r["ow"].abs()).sum(-1, keepdim=True)
    E = 2 * ep * p * (g["dp"] - g["delta"]).abs() + p * (e_dp + e_delta) + (2 * u32 + uh) * g["ds"].abs() + ah
    del e_dp
    dsa = g["ds"].abs()
    bq = scatter(2 * sc * (torch.matmul(E, kw.abs()) + (Lw + 2) * u32 * torch.matmul(dsa, kw.abs())), tok) + uo * g["dq"].abs() + ah
    bk = scatter(2 * sc * (torch.matmul(E.transpose(-1, -2), qw.abs()) + (Lw + 2) * u32 * torch.matmul(dsa.transpose(-1, -2), qw.abs())), tok) + uo * g["dk"].abs() + ah
    del E, dsa
    wgt = (2 * ep + uh + (Lw + 2) * u32) * p + ah
    bv = scatter(2 * torch.matmul(wgt.transpose(-1, -2), dow.abs()), tok) + uo * g["dv"].abs() + ah
    return bq, bk, bv


# ---------------------------------------------------------------- emulation, inputs, stand-ins
def half_pipeline(q, k, v, h, w, K, shift, variant="right", scale=None):
    """The half instance's arithmetic emulated with torch ops on half inputs: float32 scores and softmax, P rounded to half once, float32
    P V, half output.  Returns float64 [B, L, C]."""
    assert q.dtype == torch.float16
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    tok, region = token_map(w, h, K, shift) if variant == "hw_swapped" else token_map(h, w, K, shift, variant)
    mask = mask_of(region, shift and variant != "no_mask", torch.float32, q.device)
    qw, kw, vw = gather(q, tok).float(), gather(k, tok).float(), gather(v, tok).float()
    s = torch.matmul(qw, kw.transpose(-1, -2)) * scale + mask
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    o = torch.matmul(e.half().float(), vw) / l
    return scatter(o.half().double(), tok)


def random_inputs(B, h, w, dtype, device, seed=0, with_dout=False, C=128):
    """q, k = 1.5 randn, v = randn + 0.3 (|scaled score| reaches about 11 at scale 1 / sqrt(128)), as [B, h w, C] in `dtype`."""
    g = torch.Generator().manual_seed(seed)
    q = (1.5 * torch.randn(B, h * w, C, generator=g)).to(dtype).to(device)
    k = (1.5 * torch.randn(B, h * w, C, generator=g)).to(dtype).to(device)
    v = (torch.randn(B, h * w, C, generator=g) + 0.3).to(dtype).to(device)
    if with_dout:
        return q, k, v, torch.randn(B, h * w, C, generator=g).to(dtype).to(device)
    return q, k, v


def restated_split(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None):
    return restate(q, k, v, h, w, num_splits, with_shift)["o"]


def restated_full(q, k, v):
    return restate(q, k, v, 1, q.shape[1], 1, False)["o"]


class TransformerLayerStandIn(torch.nn.Module):
    """The attention half of unimatch's TransformerLayer (igs/models/unimatch/transformer.py:30-100): q_proj / k_proj / v_proj without bias,
    the swin attention looked up in `namespace` at call time (the reference binds the names in its module's globals), merge, LayerNorm."""

    def __init__(self, namespace, channels=128, seed=0):
        super().__init__()
        self.ns = namespace
        g = torch.Generator().manual_seed(seed)
        self.q_proj = torch.nn.Linear(channels, channels, bias=False)
        self.k_proj = torch.nn.Linear(channels, channels, bias=False)
        self.v_proj = torch.nn.Linear(channels, channels, bias=False)
        self.merge = torch.nn.Linear(channels, channels, bias=False)
        self.norm1 = torch.nn.LayerNorm(channels)
        with torch.no_grad():
            for p in (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight, self.merge.weight):
                p.copy_(torch.randn(p.shape, generator=g) * (channels ** -0.5))

    def forward(self, source, target, height, width, attn_num_splits, with_shift, mask=None):
        query, key, value = self.q_proj(source), self.k_proj(target), self.v_proj(target)
        if attn_num_splits > 1:
            message = self.ns.single_head_split_window_attention(query, key, value, num_splits=attn_num_splits, with_shift=with_shift,
                                                                 h=height, w=width, attn_mask=mask)
        else:
            message = self.ns.single_head_full_attention(query, key, value)
        return self.norm1(self.merge(message))
