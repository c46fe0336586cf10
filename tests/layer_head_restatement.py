"""Float64 restatement of what igs_amd/csrc/proj.hip computes (up to five bias-free 128 -> 128 products of one activation, written side by
side, each rolled by its own row offset), the pack as that kernel reads it, the test inputs, the C ABI's refusals as a list that the
host test and the GPU test share, and stand-ins in this repository's own wording for unimatch's TransformerBlock and for the two forwards
of its feature transformers, built on token_ops_restatement.TransformerLayer (the reference's modules are not available where the GPU
tests run).  The names the binders look up in a transformer's own module are defined here: generate_shift_window_attn_mask."""
import torch
import torch.nn as nn

import layer_tail_restatement as LR
import token_ops_restatement as TR
import window_attention_restatement as WR

D = 128
MAX_OUT = 5                                                         # IGS_TOKEN_PROJ_MAX_OUT
MAX_ROWS = 1 << 24                                                  # IGS_TOKEN_PROJ_MAX_ROWS
TRIP_ROWS = 128
MATRIX = 16 * LR.TILE                                               # elements of one packed matrix


# ---------------------------------------------------------------- the computation
def project_restate(x, weights, rot=None):
    """[T, 128 n] in the dtype of x (pass float64): columns 128 j .. 128 j + 127 of row (t + rot[j]) mod T are W_j x[t]."""
    T = x.shape[0]
    out = x.new_zeros(T, D * len(weights))
    for j, W in enumerate(weights):
        y = x @ W.t()
        r = 0 if rot is None else rot[j]
        dest = (torch.arange(T, device=x.device) + r) % max(T, 1)
        out[dest, D * j: D * (j + 1)] = y
    return out


def pack_projections(weights):
    """The n matrices one after the other, each in the layer tail's layout for merge; all in the dtype of the first."""
    return torch.cat([LR.pack_matrix(W.to(weights[0].dtype)) for W in weights])


def make_weights(n, seed, dtype=torch.float64, device="cpu"):
    """n matrices [128, 128] at 1 / sqrt(fan-in), as TR.randomise draws them."""
    g = torch.Generator().manual_seed(4000 + seed)
    return [(torch.randn(D, D, generator=g, dtype=torch.float64) * D ** -0.5).to(dtype).to(device) for _ in range(n)]


def project_inputs(T, seed, device):
    """x [T, 128] float64: rows of several scales and offsets, tamed to float16's range (LR.tail_inputs)."""
    return LR.tail_inputs(T, seed, device)[0]


# ---------------------------------------------------------------- the C ABI's refusals
def good_call(X, W, OUT):
    return dict(T=5, n=3, cdt=0, x=X, xdt=0, xstr=128, w=W, rot=(0, 0, 0), out=OUT, odt=0, ostr=384)


def refusals(X, W, OUT):
    """[(what differs from good_call, a word of the reason)]: each case differs from a call that would pass in the one thing its reason
    names.  X, W, OUT: addresses of spans that do not meet, with room for the few bytes some cases add."""
    big = (1 << 31) + 4
    return ([(dict([(k, v)]), "dtype") for k in ("cdt", "xdt", "odt") for v in (-1, 2)]
            + [(dict(n=v), "n out of range") for v in (0, -1, MAX_OUT + 1)]
            + [(dict(T=-1), "T out of range"), (dict(T=MAX_ROWS + 1), "T out of range")]
            + [(dict(xstr=v), "row stride") for v in (127, 0, -128, big)]
            + [(dict(ostr=v), "row stride") for v in (383, 128, 0, -384, big)]
            + [(dict(n=5, rot=(0,) * 5, ostr=639), "row stride"), (dict(n=1, rot=(0,), ostr=127), "row stride")]
            + [(dict(rot=r), "rot") for r in ((0, 0, 5), (-1, 0, 0), (0, 1 << 40, 0), (0, 0, -(1 << 40)))]
            + [(dict(T=1, rot=(0, 1, 0)), "rot")]
            + [(dict([(k, None)]), "NULL") for k in ("x", "w", "out")]
            + [(dict(x=X + 2), "aligned to its element size"), (dict(xdt=1, x=X + 1), "aligned to its element size"),
               (dict(out=OUT + 2), "aligned to its element size"), (dict(odt=1, out=OUT + 1), "aligned to its element size")]
            + [(dict(w=W + 4), "16 bytes"), (dict(w=W + 8), "16 bytes"), (dict(cdt=1, w=W + 2), "16 bytes")]
            # out over x: the same base, x's last element, x's rows between out's at wider strides, out's last columns over x's first row
            + [(dict(out=X), "out overlaps"), (dict(out=X + (4 * 128 + 127) * 4), "out overlaps"),
               (dict(xstr=1024, out=X + 128 * 4, ostr=1024), "out overlaps"), (dict(x=OUT + (4 * 384 + 383) * 4), "out overlaps"),
               (dict(xdt=1, out=X + 4 * 128 * 2), "out overlaps")])


def call_abi(lib, stream, k):
    import ctypes
    rot = None if k["rot"] is None else (ctypes.c_longlong * len(k["rot"]))(*k["rot"])
    return lib.igs_token_proj_fwd(stream, k["T"], k["n"], k["cdt"], k["x"], k["xdt"], k["xstr"], k["w"], rot, k["out"], k["odt"], k["ostr"])


# ---------------------------------------------------------------- stand-ins for the block and the two transformers
def generate_shift_window_attn_mask(input_resolution, window_size_h, window_size_w, shift_size_h, shift_size_w, device=None):
    """The additive mask of a shifted call, [K * K, Lw, Lw] float32 (the stand-ins only take square splits, as IGS does)."""
    h, w = input_resolution
    assert h // window_size_h == w // window_size_w and shift_size_h == window_size_h // 2 and shift_size_w == window_size_w // 2
    return WR.paint_mask(h, w, h // window_size_h).float().to(device)


class Block(nn.Module):
    """Self attention without FFN on the source, then cross attention with the FFN against the target."""

    def __init__(self, seed):
        super().__init__()
        self.self_attn = TR.make_layer(D, no_ffn=True, seed=seed)
        self.cross_attn_ffn = TR.make_layer(D, no_ffn=False, seed=seed + 100)

    def forward(self, source, target, **kw):
        return self.cross_attn_ffn(self.self_attn(source, source, **kw), target, **kw)


class _Transformer(nn.Module):
    def __init__(self, blocks=2, seed=0):
        super().__init__()
        self.d_model, self.nhead = D, 1
        self.layers = nn.ModuleList([Block(seed + 7 * i) for i in range(blocks)])

    def _tokens_and_mask(self, feature0, feature1, attn_type, attn_num_splits):
        b, c, h, w = feature0.shape
        assert c == self.d_model
        tok = [f.flatten(-2).permute(0, 2, 1) for f in (feature0, feature1)]
        mask = None
        if "swin" in attn_type and attn_num_splits > 1:
            wh, ww = h // attn_num_splits, w // attn_num_splits
            mask = generate_shift_window_attn_mask(input_resolution=(h, w), window_size_h=wh, window_size_w=ww, shift_size_h=wh // 2,
                                                   shift_size_w=ww // 2, device=feature0.device)
        return tok[0], tok[1], mask

    @staticmethod
    def _maps(tokens, b, h, w, c):
        return tokens.view(b, h, w, c).permute(0, 3, 1, 2).contiguous()


class TwoWayTransformer(_Transformer):
    """Both images on the batch, each the other's target: after every block the target is the block's result with its halves swapped."""

    def forward(self, feature0, feature1, attn_type="swin", attn_num_splits=None, **kwargs):
        b, c, h, w = feature0.shape
        t0, t1, mask = self._tokens_and_mask(feature0, feature1, attn_type, attn_num_splits)
        both, swapped = torch.cat((t0, t1), dim=0), torch.cat((t1, t0), dim=0)
        for i, block in enumerate(self.layers):
            both = block(both, swapped, height=h, width=w, attn_type=attn_type, attn_num_splits=attn_num_splits,
                         with_shift="swin" in attn_type and attn_num_splits > 1 and i % 2 == 1, shifted_window_attn_mask=mask,
                         shifted_window_attn_mask_1d=None)
            swapped = torch.cat(both.chunk(chunks=2, dim=0)[::-1], dim=0)
        t0, t1 = both.chunk(chunks=2, dim=0)
        return self._maps(t0, b, h, w, c), self._maps(t1, b, h, w, c)


class OneWayTransformer(_Transformer):
    """The first image attends to the second, which stays as it came; one result."""

    def forward(self, feature0, feature1, attn_type="swin", attn_num_splits=None, **kwargs):
        b, c, h, w = feature0.shape
        t0, t1, mask = self._tokens_and_mask(feature0, feature1, attn_type, attn_num_splits)
        for i, block in enumerate(self.layers):
            t0 = block(t0, t1, height=h, width=w, attn_type=attn_type, attn_num_splits=attn_num_splits,
                       with_shift="swin" in attn_type and attn_num_splits > 1 and i % 2 == 1, shifted_window_attn_mask=mask,
                       shifted_window_attn_mask_1d=None)
        return self._maps(t0, b, h, w, c)


def make_transformer(bidirectional, blocks=2, seed=0):
    return (TwoWayTransformer if bidirectional else OneWayTransformer)(blocks, seed)


def feature_inputs(b, h, w, seed, device, dtype=torch.float32):
    """Two [b, 128, h, w] feature maps of unit scale."""
    g = torch.Generator().manual_seed(9000 + seed)
    return tuple(torch.randn(b, D, h, w, generator=g).to(dtype).to(device) for _ in range(2))
