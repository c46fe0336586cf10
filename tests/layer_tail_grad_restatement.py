"""Float64 restatement of what igs_amd/csrc/ffn_bwd.hip computes (the gradients of the fused layer tail, written out from the formulas of
include/igs_rast.h, not through autograd), an independent pack / unpack of the TRANSPOSED weight layout that the header documents for
igs_layer_tail_bwd, and the allowance of the gradient tests.  A helper file, not a test file.
"""
import math

import torch

import layer_tail_restatement as LR
import token_ops_restatement as TR

D, TILE = LR.D, LR.TILE
CHUNK_ROWS = 8192                                                   # IGS_LAYER_TAIL_BWD_CHUNK_ROWS
SLICE_ROWS = 512                                                    # the rows of one slice of the weight-gradient sums
NAMES = ("da", "ds", "dWm", "dln1_w", "dln1_b", "dW1", "dW2", "dln2_w", "dln2_b")
FLOOR = {torch.float32: 1e-5, torch.float16: 2e-3}                  # test_gpu_token_ops.py's floors of the four-times rule


# ---------------------------------------------------------------- the computation
def _stats(v, eps):
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (v - mean) * rstd, rstd


def _ln_bwd(d, xh, w, rstd):
    p = d * w
    return rstd * (p - p.mean(-1, keepdim=True) - xh * (p * xh).mean(-1, keepdim=True))


def gelu_grad(z):
    return TR.cdf(z) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def tail_grad_restate(a, s, g, Wm, ln1, W1=None, W2=None, ln2=None, wgrad_rows=None, gelu_grad_fn=gelu_grad):
    """The nine gradients (NAMES' order; None for the FFN's without one) of sum(out * g), float64 in, float64 out.  wgrad_rows: the rows
    that enter the parameter sums (default all; the teeth tests leave one out).  gelu_grad_fn: GELU' (the teeth tests swap channels)."""
    rows = slice(None) if wgrad_rows is None else wgrad_rows
    m = a @ Wm.t()
    xh1, r1 = _stats(m, ln1[2])
    n1 = xh1 * ln1[0] + ln1[1]
    if W1 is None:
        ds, dn1 = g, g
        dW1 = dW2 = dg2 = db2 = None
    else:
        u = torch.cat([s, n1], -1)
        z = u @ W1.t()
        h = z * TR.cdf(z)
        xh2, r2 = _stats(h @ W2.t(), ln2[2])
        dg2, db2 = (g * xh2)[rows].sum(0), g[rows].sum(0)
        dy = _ln_bwd(g, xh2, ln2[0], r2)
        dW2 = dy[rows].t() @ h[rows]
        dz = (dy @ W2) * gelu_grad_fn(z)
        dW1 = dz[rows].t() @ u[rows]
        du = dz @ W1
        ds, dn1 = g + du[:, :D], du[:, D:]
    dg1, db1 = (dn1 * xh1)[rows].sum(0), dn1[rows].sum(0)
    dm = _ln_bwd(dn1, xh1, ln1[0], r1)
    return dm @ Wm, ds, dm[rows].t() @ a[rows], dg1, db1, dW1, dW2, dg2, db2


def tail_grad_autograd(a, s, g, Wm, ln1, W1=None, W2=None, ln2=None):
    """The same nine gradients through float64 autograd of layer_tail_restatement.tail_restate."""
    leaves = [a, s, Wm, ln1[0], ln1[1]] + ([] if W1 is None else [W1, W2, ln2[0], ln2[1]])
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    ffn = () if W1 is None else (leaves[5], leaves[6], (leaves[7], leaves[8], ln2[2]))
    out = LR.tail_restate(leaves[0], leaves[1], leaves[2], (leaves[3], leaves[4], ln1[2]), *ffn)
    grads = list(torch.autograd.grad((out * g).sum(), leaves, allow_unused=True))
    if grads[1] is None:
        grads[1] = torch.zeros_like(s)
    return tuple(grads + [None] * (9 - len(grads)))


# ---------------------------------------------------------------- the transposed pack
def pack_tail_t(Wm, W1=None, W2=None):
    """Wm^T with its output tile outermost, then W1^T [256, hidden] with its INPUT tile outermost (tile 8 j + ot), then W2^T [hidden, 128]
    with its output tile outermost (tile 4 j + kt): the header's formula for wpack_t, through layer_tail_restatement's per-tile index."""
    parts = [LR.pack_matrix(Wm.t().contiguous())]
    if W1 is not None:
        parts += [LR.pack_matrix(W1.t().contiguous(), input_tile_outermost=True), LR.pack_matrix(W2.t().contiguous())]
    return torch.cat(parts)


def unpack_tail_t(flat, hidden=0):
    """(Wm, W1, W2) back from the transposed pack (transposed back); hidden = 0: no FFN."""
    Wm = LR.unpack_matrix(flat[: 16 * TILE], D, D).t()
    if not hidden:
        return Wm, None, None
    n1 = hidden // 32 * 8 * TILE
    return (Wm, LR.unpack_matrix(flat[16 * TILE: 16 * TILE + n1], 2 * D, hidden, input_tile_outermost=True).t(),
            LR.unpack_matrix(flat[16 * TILE + n1:], hidden, D).t())


# ---------------------------------------------------------------- the allowance
def rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def allowed(err_comparator, compute_dtype):
    """The four-times rule per gradient tensor: at most 4 x the comparator's max |err| / max |ref|, with the floors above."""
    return max(4.0 * err_comparator, FLOOR[compute_dtype])


def scratch_bytes(T, hidden):
    """igs_layer_tail_bwd_scratch_bytes from the header's statement: one chunk's rows (whole trips of 128) of 2 hidden + 1152 (FFN) or 512
    float32 values and one partial of all the parameter gradients per slice of 512 rows."""
    rows = -(-min(T, CHUNK_ROWS) // LR.TRIP_ROWS) * LR.TRIP_ROWS
    per_row = 2 * hidden + 1152 if hidden else 512
    part = D * D + 2 * D + (hidden * 2 * D + D * hidden + 2 * D if hidden else 0)
    return 4 * (rows * per_row + -(-rows // SLICE_ROWS) * part)
