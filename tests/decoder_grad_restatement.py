"""The residual decoder's backward (igs_mlp_heads_bwd, igs_amd/csrc/mlp.hip) restated in float64: the gradients of
decoder_restatement.forward by the chain rule, an elementwise error bound for every gradient carried through the recomputed forward and
the backward, and the builder of the exact integer cases.  numpy only.

    dh_L = dY Wh        dWh = dY^T h_L          dbh = sum_rows dY
    for l = L-1 .. 0:   dz_l = dh_{l+1} * act'(z_l)   (dh_{l+1} where act_after[l] == 0)
                        dW_l = dz_l^T h_l       db_l = sum_rows dz_l       dh_l = dz_l W_l
    dx = dh_0

The bound is derived, not fitted.  u = 2^-24, gamma_n = n u / (1 - n u); a hat marks the kernel's value, e_v >= |v^ - v|.

  forward again (the kernel recomputes it exactly as the forward kernel does): decoder_restatement's rules give e_z for every
      pre-activation and e_h for every activation.
  dz = g a'(z), SiLU.  sup |silu''| <= 0.5, so |silu'(z^) - silu'(z)| <= 0.5 e_z.  The kernel (mlp_silu_grad) evaluates
      silu'(v) = fma(v e s, s, s) with e = exp(-v) on mlp_silu's clamped exponent and s = 1 / (1 + e):
        e: v_exp_f32 1 ulp = 2 u, the fma that applies the argument's low part 1 u: 3 u (the argument itself is good to 2^-48);
        s: of e's error only the share e / (1 + e) <= 1 arrives (3 u), the sum 1 + e 1 u, v_rcp_f32 1 ulp = 2 u: 6 u;
        1 - s is formed as e s, 3 + 6 + 1 = 10 u relative whatever s is (no cancellation); t = v e s another 1 u: 11 u;
        the last fma: s (1 + t) with s off by 6 u, t by 11 u |t|, one rounding: 7 u |silu'| + 11 u |s t|, and
        |s t| = |v| s^2 e <= 0.2239 (its maximum at |v| = 1.54), so 11 u |s t| <= 2.5 u.
      With the second-order terms: |a'^ - a'(z^)| <= u (SILUP_C |a'(z^)| + SILUP_ABS), SILUP_C = 8, SILUP_ABS = 3.  The absolute part
      cannot be dropped: silu' has a zero at z = -1.278, where a purely relative bound would promise an exact zero.  Below z = -87.3
      the clamped exponent gives |a'^| <= 2^-126 (1 + |z|) where the true value is smaller still; that is inside SILUP_ABS u.
      Together  e_a = 0.5 e_z + u (SILUP_C (|a'| + 0.5 e_z) + SILUP_ABS)  and, the product being rounded once,
        e_dz = |a'| e_g + (|g| + e_g) e_a + u (|g| + e_g) (|a'| + e_a).
  dz, ReLU: the derivative is 0 or 1 and the product exact.  Where |z| <= e_z the kernel may have decided the other way:
      e_dz = |g| + e_g there, a' e_g elsewhere.
  dh = dz W, a sum of K = O terms in some order: e_dh = e_dz |W| + gamma_{K+1} (|dz| + e_dz) |W|.
  dW = dz^T h over N rows in some order: e_dW = e_dz^T (|h| + e_h) + |dz|^T e_h + gamma_{N+1} (|dz| + e_dz)^T (|h| + e_h);
      db = sum_rows dz: e_db = sum e_dz + gamma_N sum (|dz| + e_dz).  Both are float32 outputs.
  half: a value that is rounded to half to become an operand (dz for the dgrad and the wgrad, h for the wgrad; not x, dY or the
      weights, which are half already) or an output (dx; dW and db only where the caller rounds them for half parameters,
      round_params) adds 2^-11 |v^| + 2^-25.
"""
import numpy as np

import decoder_restatement as R

U, UH, SUBH = R.U, R.UH, R.SUBH
SILUP_C = 8.0
SILUP_ABS = 3.0


def silu_grad(z):
    with np.errstate(over="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
        zs = np.where(s == 0.0, 0.0, z * (1.0 - s))          # exp(-z) = inf: the limit, not -inf * 0... s is 0 and so is the product
    return s * (1.0 + zs)


def act_grad(z, name):
    if name == "silu":
        return silu_grad(z)
    if name == "relu":
        return (z > 0).astype(np.float64)
    raise ValueError(name)


def _layers(weights, biases, head_weights, head_biases, act_after):
    act_after = [1] * len(weights) if act_after is None else list(act_after)
    Wh = np.concatenate([R._f64(w) for w in head_weights], 0)
    bh = np.concatenate([np.zeros(w.shape[0]) if b is None else R._f64(b) for w, b in zip(head_weights, head_biases)], 0)
    return [(R._f64(w), R._f64(b), a) for w, b, a in zip(weights, biases, act_after)] + [(Wh, bh, 0)]


def _dy(douts, head_weights, N):
    return np.concatenate([np.zeros((N, w.shape[0])) if g is None else R._f64(g) for g, w in zip(douts, head_weights)], 1)


def gradients_with_bound(x, weights, biases, head_weights, head_biases, douts, activation="silu", act_after=None, half=False,
                         round_params=False, dact_hook=None):
    """(grads, bounds): dicts with dx [N, C0], dw / db (lists over the hidden Linears), dhw / dhb (lists over the heads), float64;
    bounds[k] >= |kernel's - grads[k]| elementwise for the float32 (half False) or float16 kernel.  douts[k] None: zeros.  dact_hook, for
    the tests of the bound itself: a function applied to each layer's derivative array [N, C] before it is used."""
    x = R._f64(x)
    N = x.shape[0]
    layers = _layers(weights, biases, head_weights, head_biases, act_after)
    L = len(layers) - 1
    # the forward again, as decoder_restatement.forward_with_bound carries it
    hs, ehs, zs, ezs = [x], [np.zeros_like(x)], [], []
    h, e = x, np.zeros_like(x)
    for l, (W, b, on) in enumerate(layers[:-1]):
        K = W.shape[1]
        absb = 0.0 if b is None else np.abs(b)
        z = h @ W.T + (0.0 if b is None else b)
        hh = np.abs(h) + e
        ez = e @ np.abs(W).T + R.gamma(K + 1) * (hh @ np.abs(W).T + absb)
        if half and l > 0:
            ez = ez + (UH * hh + SUBH) @ np.abs(W).T
        zs.append(z)
        ezs.append(ez)
        if not on:
            h, e = z, ez
        elif activation == "relu":
            h, e = R.act(z, "relu"), ez
        else:
            s = R.silu(z)
            h, e = s, 1.1 * ez + R.SILU_A * U * (np.abs(s) + 1.1 * ez) + 2.0 ** -125 * (np.abs(z) + ez)
        hs.append(h)
        ehs.append(e)

    def as_operand(v, ev, rounded):
        """(|v^| bound, error) of v^ once it is an operand: rounded to half on the half path unless it is a half value already"""
        if half and rounded:
            ev = ev + UH * (np.abs(v) + ev) + SUBH
        return np.abs(v) + ev, ev

    g = _dy(douts, head_weights, N)
    eg = np.zeros_like(g)
    dws, dbs, edws, edbs = [None] * (L + 1), [None] * (L + 1), [None] * (L + 1), [None] * (L + 1)
    for l in range(L, -1, -1):
        W = layers[l][0]
        dz, edz = g, eg
        if l < L and layers[l][2]:
            a = act_grad(zs[l], activation)
            if dact_hook is not None:
                a = dact_hook(l, a)
            if activation == "relu":
                dz = g * a
                edz = np.where(np.abs(zs[l]) <= ezs[l], np.abs(g) + eg, a * eg)
            else:
                ea = 0.5 * ezs[l] + U * (SILUP_C * (np.abs(a) + 0.5 * ezs[l]) + SILUP_ABS)
                dz = g * a
                edz = np.abs(a) * eg + (np.abs(g) + eg) * ea + U * (np.abs(g) + eg) * (np.abs(a) + ea)
        # the weight and bias gradients
        dzo, edzo = as_operand(dz, edz, l < L)
        ho, eho = as_operand(hs[l], ehs[l], l > 0)
        dws[l] = dz.T @ hs[l]
        edws[l] = edzo.T @ ho + np.abs(dz).T @ eho + R.gamma(N + 1) * (dzo.T @ ho)
        dbs[l] = dz.sum(0)
        edbs[l] = edz.sum(0) + R.gamma(max(N, 1)) * (np.abs(dz) + edz).sum(0)
        if round_params and half:
            edws[l] = edws[l] + UH * (np.abs(dws[l]) + edws[l]) + SUBH
            edbs[l] = edbs[l] + UH * (np.abs(dbs[l]) + edbs[l]) + SUBH
        # the dgrad
        K = W.shape[0]
        g = dz @ W
        eg = edzo @ np.abs(W) + R.gamma(K + 1) * (dzo @ np.abs(W))
    dx, edx = g, eg
    if half:
        edx = edx + UH * (np.abs(dx) + edx) + SUBH
    n = len(weights)
    split = np.cumsum([w.shape[0] for w in head_weights])[:-1]
    grads = dict(dx=dx, dw=dws[:n], db=dbs[:n], dhw=np.split(dws[L], split, 0), dhb=np.split(dbs[L], split, 0))
    bounds = dict(dx=edx, dw=edws[:n], db=edbs[:n], dhw=np.split(edws[L], split, 0), dhb=np.split(edbs[L], split, 0))
    return grads, bounds


def gradients(x, weights, biases, head_weights, head_biases, douts, activation="silu", act_after=None):
    return gradients_with_bound(x, weights, biases, head_weights, head_biases, douts, activation, act_after)[0]


def flat(grads):
    """[(name, array)] of a gradients dict, every tensor once."""
    out = [("dx", grads["dx"])]
    for k in ("dw", "db", "dhw", "dhb"):
        out += [("%s[%d]" % (k, i), a) for i, a in enumerate(grads[k])]
    return out


# ---------------------------------------------------------------- exact integer cases
def exact_grad_case(C0, hidden, heads, N, density=0.05, seed=0, bias=True, act_after=None):
    """decoder_restatement.exact_case (ReLU, integers) plus integer upstream gradients dY in {-1, 0, 1}, non-zero with probability
    `density`.  Asserts its own premise: for every product of the backward -- dY Wh, every dz_l W_l, every dz_l^T h_l and the bias
    sums -- sum |a| |b| < 2^11, so every partial sum in any order is an integer below 2^11, exact in half and in float32; with an
    act_after other than all ones also the forward's.  Asserts that at least one gradient of every kind is non-zero.  Returns
    exact_case's dict plus douts, act_after and grads (gradients' dict)."""
    case = R.exact_case(C0, hidden, heads, N, bias=bias, seed=seed)
    rng = np.random.RandomState(2000 + seed)
    douts = [(rng.randint(0, 2, size=(N, ch)) * 2 - 1) * (rng.uniform(size=(N, ch)) < density) for ch in heads]
    douts = [d.astype(np.float64) for d in douts]
    layers = _layers(case["weights"], case["biases"], case["head_weights"], case["head_biases"], act_after)
    L = len(layers) - 1
    h, hs, zs = case["x"], [case["x"]], []
    for W, b, on in layers[:-1]:
        mass = np.abs(h) @ np.abs(W).T + (0.0 if b is None else np.abs(b))
        assert mass.max() < 2 ** 11, "exact_grad_case: a forward partial sum could reach 2^11 (%g)" % mass.max()
        z = h @ W.T + (0.0 if b is None else b)
        h = np.maximum(z, 0.0) if on else z
        zs.append(z)
        hs.append(h)
    g = np.concatenate(douts, 1)
    worst = 0.0
    for l in range(L, -1, -1):
        W = layers[l][0]
        dz = g * (zs[l] > 0) if (l < L and layers[l][2]) else g
        worst = max(worst, (np.abs(dz).T @ np.abs(hs[l])).max(), np.abs(dz).sum(0).max(), (np.abs(dz) @ np.abs(W)).max())
        g = dz @ W
    assert worst < 2 ** 11, "exact_grad_case: a backward partial sum could reach 2^11 (%g)" % worst
    grads = gradients(case["x"], case["weights"], case["biases"], case["head_weights"], case["head_biases"], douts, "relu", act_after)
    for name, a in flat(grads):
        assert np.all(a == np.round(a)), name
    for kind in ("dx", "dw", "db", "dhw", "dhb"):
        arrs = [grads[kind]] if kind == "dx" else grads[kind]
        assert not arrs or any(np.any(a != 0) for a in arrs), "exact_grad_case: every %s is zero" % kind
    outs = R.forward(case["x"], case["weights"], case["biases"], case["head_weights"], case["head_biases"], "relu", act_after)
    case.update(douts=douts, act_after=act_after, grads=grads, worst=worst, outs=outs)
    return case
