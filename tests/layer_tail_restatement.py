"""Float64 restatement of what igs_amd/csrc/ffn.hip computes (the tail of a unimatch TransformerLayer: merge, LN1, and with an FFN the cat, the
exact-GELU MLP and LN2, then the residual add), an independent restatement of the packed weight layout that include/igs_rast.h documents
for igs_layer_tail_fwd (pack and unpack, written from the documented element formula, not from igs_amd.motion.pack_mlp_tile_order), and
the stand-in layers and inputs of the tests.  A helper file, not a test file.
"""
import torch
import torch.nn as nn

import token_ops_restatement as TR

D = 128                                                             # d_model
TILE = 1024                                                         # elements of one packed 32 x 32 tile
TRIP_ROWS = 128                                                     # IGS_LAYER_TAIL_TRIP_ROWS


# ---------------------------------------------------------------- the computation
def tail_restate(a, s, Wm, ln1, W1=None, W2=None, ln2=None):
    """out [T, 128] in the dtype of a (pass float64).  ln1, ln2: (weight, bias, eps).  W1 None: no FFN.  Columns 0..127 of W1 multiply s,
    128..255 multiply n1 (the reference's cat order)."""
    m = a @ Wm.t()
    n1 = TR.layer_norm_restate(m, ln1[0], ln1[1], ln1[2])
    if W1 is None:
        return s + n1
    x = torch.cat([s, n1], -1) @ W1.t()
    h = x * TR.cdf(x)
    return s + TR.layer_norm_restate(h @ W2.t(), ln2[0], ln2[1], ln2[2])


def layer_weights(layer, dtype=torch.float64):
    """(Wm, ln1, W1, W2, ln2) of a stand-in layer as tail_restate takes them, in `dtype`."""
    n1 = layer.norm1
    Wm, ln1 = layer.merge.weight.detach().to(dtype), (n1.weight.detach().to(dtype), n1.bias.detach().to(dtype), n1.eps)
    if layer.no_ffn:
        return Wm, ln1, None, None, None
    n2 = layer.norm2
    return (Wm, ln1, layer.mlp[0].weight.detach().to(dtype), layer.mlp[2].weight.detach().to(dtype),
            (n2.weight.detach().to(dtype), n2.bias.detach().to(dtype), n2.eps))


# ---------------------------------------------------------------- the pack layout
def _tile_index(half):
    """(position in the tile, row, column) of every element of a 32 x 32 tile: the tile is [chunk][lane 64][E], E = 8 (half) or 4 (float);
    element e = chunk E + j of lane (r = lane & 31, h = lane >> 5) is W[r][(e & 3) + 8 (e >> 2) + 4 h]."""
    E = 8 if half else 4
    e, lane = torch.arange(16).view(16, 1), torch.arange(64).view(1, 64)
    r, h = lane & 31, lane >> 5
    pos = ((e // E) * 64 + lane) * E + e % E
    col = (e & 3) + 8 * (e >> 2) + 4 * h
    return pos.reshape(-1), r.expand(16, 64).reshape(-1), col.reshape(-1)


def _tile_number(ot, kt, OT, KT, input_tile_outermost):
    return kt * OT + ot if input_tile_outermost else ot * KT + kt


def pack_matrix(W, input_tile_outermost=False):
    """W [O, I] (multiples of 32) as O / 32 x I / 32 tiles of 1024 elements."""
    O, I = W.shape
    OT, KT = O // 32, I // 32
    pos, row, col = _tile_index(W.dtype == torch.float16)
    out = W.new_zeros(OT * KT * TILE)
    for ot in range(OT):
        for kt in range(KT):
            t = _tile_number(ot, kt, OT, KT, input_tile_outermost)
            out[t * TILE + pos] = W[32 * ot: 32 * ot + 32, 32 * kt: 32 * kt + 32][row, col]
    return out


def unpack_matrix(flat, O, I, input_tile_outermost=False):
    OT, KT = O // 32, I // 32
    pos, row, col = _tile_index(flat.dtype == torch.float16)
    W = flat.new_zeros(O, I)
    for ot in range(OT):
        for kt in range(KT):
            t = _tile_number(ot, kt, OT, KT, input_tile_outermost)
            W[32 * ot + row, 32 * kt + col] = flat[t * TILE + pos]
    return W


def pack_tail(Wm, W1=None, W2=None):
    """merge, then W1 with its output tile outermost, then W2 with its INPUT tile outermost; all in the dtype of Wm."""
    parts = [pack_matrix(Wm)]
    if W1 is not None:
        parts += [pack_matrix(W1), pack_matrix(W2, input_tile_outermost=True)]
    return torch.cat(parts)


def unpack_tail(flat, hidden=0):
    """(Wm, W1, W2) back from the pack; hidden = 0: no FFN."""
    Wm = unpack_matrix(flat[: 16 * TILE], D, D)
    if not hidden:
        return Wm, None, None
    n1 = hidden // 32 * 8 * TILE
    return (Wm, unpack_matrix(flat[16 * TILE: 16 * TILE + n1], hidden, 2 * D),
            unpack_matrix(flat[16 * TILE + n1:], D, hidden, input_tile_outermost=True))


def pack_elems(hidden, has_ffn=True):
    return (16 + (12 * (hidden // 32) if has_ffn else 0)) * TILE


# ---------------------------------------------------------------- stand-in layers and inputs
def make_tail_layer(hidden=1024, no_ffn=False, seed=0):
    """token_ops_restatement's TransformerLayer with an FFN of `hidden` units (the constructor only makes multiples of 256)."""
    layer = TR.TransformerLayer(d_model=D, no_ffn=no_ffn)
    if not no_ffn and hidden != layer.mlp[0].out_features:
        layer.mlp = nn.Sequential(nn.Linear(2 * D, hidden, bias=False), nn.GELU(), nn.Linear(hidden, D, bias=False))
    return TR.randomise(layer, seed)


def tail_inputs(T, seed, device):
    """(a, s) [T, 128] float64: rows of several scales and offsets, as TR.row_inputs makes them, tamed to float16's range."""
    a = TR.row_inputs(T, D, torch.float64, "cpu", seed)
    s = TR.row_inputs(T, D, torch.float64, "cpu", seed + 1)
    return (a / 8.0).to(device), (s / 8.0).to(device)
