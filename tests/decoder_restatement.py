"""The residual decoder (igs_amd/csrc/mlp.hip; GS3DRenderer.decode_residual_feature, igs/models/gs.py:858-869 over the MLP of
igs/models/networks.py:60-108) restated in float64 with plain matmuls, an elementwise forward error bound carried layer by layer, the
packed weight layout restated from its definition, the builder of the exact integer cases, and a stand-in for the renderer module
(make_renderer: the attributes decode_residual_feature reads, with the reference's lines as its method).  numpy, and torch for the stand-in.

The bound is derived, not fitted.  u = 2^-24, gamma_n = n u / (1 - n u).  With h the exact activation, h^ the kernel's and e >= |h^ - h|:

  a Linear of K inputs, z = W h + b, computed as an fma chain of K + 1 terms from the bias in some order:
      |z^ - z| <= |W| e + gamma_{K+1} (|W| |h^| + |b|),    |h^| <= |h| + e.
  the half path rounds h^ to half when it becomes the operand: another |W| (2^-11 |h^| + 2^-25) (the second term: the half subnormal
      spacing); the input itself and the weights are half values already, so layer 0 has no such term.  The half output adds
      2^-11 |y^| + 2^-25.
  SiLU: |silu'| <= 1.0998, so |silu(z^) - silu(z)| <= 1.1 |z^ - z|; evaluating silu(z^) in float32 costs a u |silu(z^)| with a = 8:
      mlp_silu forms exp(-v) as exp2(t) (1 + tl ln 2) with t + tl = -v log2(e) to ~2^-48, so the argument's error does not grow with |v|;
      v_exp_f32 is within 1 ulp = 2 u, the fma that applies tl 1 u, 1 + e 1 u (and only the share e / (1 + e) of exp's error reaches
      the sum), v_rcp_f32 1 ulp = 2 u, the last product 1 u: 7 u to first order, 8 with the second-order terms.
      The kernel holds sigmoid's argument to [-128, 128] and the exponent of exp2 to 126 so that nothing overflows: below z = -87.3 it
      returns z / (1 + 2^126 (1 + small)) where the true value is smaller still, an absolute error below |z| 2^-126, carried as
      |z^| 2^-125.  Above 128 exp2 gives 0 and the result is z^ itself, which is silu(z^) to far below u.
  ReLU: exact, e <- |z^ - z|.
"""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11                    # unit roundoff of half
SUBH = 2.0 ** -25                  # half the spacing of the half subnormals
SILU_A = 8.0


def gamma(n):
    return n * U / (1.0 - n * U)


def silu(z):
    with np.errstate(over="ignore"):                       # exp(-z) = inf below z = -709.8: z / inf = -0, the limit
        return z / (1.0 + np.exp(-z))


def act(z, name):
    if name == "silu":
        return silu(z)
    if name == "relu":
        return np.maximum(z, 0.0)
    raise ValueError(name)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def forward(x, weights, biases, head_weights, head_biases, activation="silu", act_after=None):
    """The heads' outputs, a list of float64 [N, ch]."""
    return forward_with_bound(x, weights, biases, head_weights, head_biases, activation, act_after, half=False)[0]


def forward_with_bound(x, weights, biases, head_weights, head_biases, activation="silu", act_after=None, half=False):
    """(outputs, bounds): float64 lists per head; bounds[k] >= |kernel's output - outputs[k]| elementwise for the float32 (half False) or
    float16 kernel."""
    h = _f64(x)
    e = np.zeros_like(h)
    act_after = [1] * len(weights) if act_after is None else list(act_after)
    Wh = np.concatenate([_f64(w) for w in head_weights], 0)
    bh = np.concatenate([np.zeros(w.shape[0]) if b is None else _f64(b) for w, b in zip(head_weights, head_biases)], 0)
    layers = [(_f64(w), _f64(b), a) for w, b, a in zip(weights, biases, act_after)] + [(Wh, bh, 0)]
    for l, (W, b, on) in enumerate(layers):
        K = W.shape[1]
        absb = 0.0 if b is None else np.abs(b)
        z = h @ W.T + (0.0 if b is None else b)
        hh = np.abs(h) + e                                   # >= |h^|
        ez = e @ np.abs(W).T + gamma(K + 1) * (hh @ np.abs(W).T + absb)
        if half and l > 0:
            ez = ez + (UH * hh + SUBH) @ np.abs(W).T
        last = l == len(layers) - 1
        if last:
            if half:
                ez = ez + UH * (np.abs(z) + ez) + SUBH
            h, e = z, ez
        elif not on:
            h, e = z, ez
        elif activation == "relu":
            h, e = act(z, "relu"), ez
        else:
            s = silu(z)
            h, e = s, 1.1 * ez + SILU_A * U * (np.abs(s) + 1.1 * ez) + 2.0 ** -125 * (np.abs(z) + ez)
    outs, bounds, c = [], [], 0
    for w in head_weights:
        outs.append(h[:, c:c + w.shape[0]])
        bounds.append(e[:, c:c + w.shape[0]])
        c += w.shape[0]
    return outs, bounds


def worst_ratio(got, want, bound):
    """max |got - want| / bound (0 / 0 = 0)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------- the packed layout, from its definition (include/igs_rast.h)
def pack_tile_order(W, half):
    """W [O, I] -> flat [ceil(O/32) * ceil(I/32) * 1024]: tile (ot, kt), output tile outermost, is [chunk][lane 64][E], E = 8 (half) or 4;
    element e = chunk E + j of lane (r = lane & 31, h = lane >> 5) is W[32 ot + r][32 kt + (e & 3) + 8 (e >> 2) + 4 h], zero outside W."""
    W = np.asarray(W)
    O, I = W.shape
    OT, KT, E = (O + 31) // 32, (I + 31) // 32, 8 if half else 4
    out = np.zeros(OT * KT * 1024, dtype=W.dtype)
    for ot in range(OT):
        for kt in range(KT):
            for chunk in range(16 // E):
                for lane in range(64):
                    r, h = lane & 31, lane >> 5
                    for j in range(E):
                        e = chunk * E + j
                        row, col = 32 * ot + r, 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * h
                        if row < O and col < I:
                            out[(ot * KT + kt) * 1024 + (chunk * 64 + lane) * E + j] = W[row, col]
    return out


# ---------------------------------------------------------------- exact integer cases
def exact_case(C0, hidden, heads, N, bias=True, seed=0, nnz=3):
    """A ReLU decoder on integers: x in [-2, 2], every weight row has `nnz` non-zeros from {-2, -1, 1, 2} at scattered columns (asymmetric:
    W != W^T and no two rows alike by construction of the draw), biases in [-2, 2].  Asserts its own premise: for every output of every
    Linear, sum |W| |h| + |b| < 2^11, so every partial sum in any order and every activation is an integer below 2^11: exact in half and
    in float32 whatever the order.  Returns dict(x, weights, biases, head_weights, head_biases, outs) as float64 arrays (biases None when
    bias is False)."""
    rng = np.random.RandomState(1000 + seed)
    x = rng.randint(-2, 3, size=(N, C0)).astype(np.float64)
    vals = np.array([-2.0, -1.0, 1.0, 2.0])

    def linear(O, I):
        W = np.zeros((O, I))
        for o in range(O):
            cols = rng.choice(I, size=min(nnz, I), replace=False)
            W[o, cols] = vals[rng.randint(0, 4, size=len(cols))]
        b = rng.randint(-2, 3, size=O).astype(np.float64) if bias else None
        return W, b

    widths = [C0] + list(hidden)
    hid = [linear(widths[l + 1], widths[l]) for l in range(len(hidden))]
    hd = [linear(ch, widths[-1]) for ch in heads]
    h = x
    for W, b in hid + [(np.concatenate([w for w, _ in hd], 0), None if not bias else np.concatenate([b for _, b in hd], 0))]:
        mass = np.abs(h) @ np.abs(W).T + (0.0 if b is None else np.abs(b))
        assert mass.max() < 2 ** 11, "exact_case: a partial sum could reach 2^11 (%g)" % mass.max()
        z = h @ W.T + (0.0 if b is None else b)
        assert np.all(z == np.round(z))
        h = np.maximum(z, 0.0)
    ws, bs = [w for w, _ in hid], [b for _, b in hid]
    hws, hbs = [w for w, _ in hd], [b for _, b in hd]
    return dict(x=x, weights=ws, biases=bs, head_weights=hws, head_biases=hbs, outs=forward(x, ws, bs, hws, hbs, "relu"))


def linear_init(O, I, rng, bias=True):
    """nn.Linear's default initialisation: weight and bias uniform in +- 1 / sqrt(I)."""
    k = 1.0 / np.sqrt(I)
    return rng.uniform(-k, k, size=(O, I)), (rng.uniform(-k, k, size=O) if bias else None)


# ---------------------------------------------------------------- the stand-in module
def make_renderer(dim_in=20, n_neurons=24, dim_out=24, n_hidden_layers=2, activation="silu", feature_channels=None, bias=True, mlp=True, seed=0):
    """A module with what GS3DRenderer's decoder has (gs.py:535-559): cfg.mlp_network_config (None: no MLP), cfg.feature_channels,
    mlp_net.layers = Linear, act, ..., Linear as networks.py:72-90 builds them, mlp_net.output_activation (identity), out_layers, and
    decode_residual_feature with the reference's lines (gs.py:858-869).  The heads keep nn.Linear's default initialisation."""
    import types
    import torch
    import torch.nn as nn
    feature_channels = dict(feature_channels or {"xyz": 3, "rotation": 4})
    torch.manual_seed(seed)

    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            make = {"silu": nn.SiLU, "relu": nn.ReLU}[activation]
            layers = [nn.Linear(dim_in, n_neurons, bias=bias), make()]
            for _ in range(n_hidden_layers - 1):
                layers += [nn.Linear(n_neurons, n_neurons, bias=bias), make()]
            layers += [nn.Linear(n_neurons, dim_out, bias=bias)]
            self.layers = nn.Sequential(*layers)
            self.output_activation = lambda x: x

        def forward(self, x):
            return self.output_activation(self.layers(x))

    class Renderer(nn.Module):
        def __init__(self):
            super().__init__()
            self.cfg = types.SimpleNamespace(mlp_network_config=dict(n_neurons=n_neurons) if mlp else None, feature_channels=feature_channels)
            if mlp:
                self.mlp_net = MLP()
            self.out_layers = nn.ModuleList([nn.Linear(dim_out if mlp else dim_in, ch) for ch in feature_channels.values()])

        def decode_residual_feature(self, residual_feat, bbox=None, radius=None):
            if self.cfg.mlp_network_config is not None:
                residual_feat = self.mlp_net(residual_feat)
            return {k: layer(residual_feat) for k, layer in zip(self.cfg.feature_channels.keys(), self.out_layers)}

    return Renderer()


def renderer_parts(r):
    """(weights, biases, head_weights, head_biases, act_after) of a make_renderer module as float64 numpy arrays."""
    import torch.nn as nn
    mods = list(r.mlp_net.layers) if r.cfg.mlp_network_config is not None else []
    lin = [i for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
    arr = lambda t: None if t is None else t.detach().double().cpu().numpy()
    return ([arr(mods[i].weight) for i in lin], [arr(mods[i].bias) for i in lin], [arr(m.weight) for m in r.out_layers],
            [arr(m.bias) for m in r.out_layers], [int(i + 1 < len(mods) and not isinstance(mods[i + 1], nn.Linear)) for i in lin])
