"""The residual decoder's native backward on the MI355X (mlp_heads_autograd and the training binder of igs_amd/motion.py over
igs_mlp_heads_bwd, igs_amd/csrc/mlp.hip) against the float64 restatement of tests/decoder_grad_restatement.py: exact integer cases bit for
bit, SiLU cases inside the derived bound, the bound's own teeth, optional gradients, views, streams, reproducibility, the memory contract,
the bound module and the chain query_ir_grid -> decoder -> deform.

Worst |error| / bound seen on the MI355X is recorded in DESIGN.md section 21; every float test prints its own."""
import numpy as np
import pytest
import torch

import decoder_grad_restatement as GR
import decoder_restatement as DR
from test_gpu_decoder import LARGE, _dev, _float_case, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16]
IDS = ["f32", "f16"]
SHIPPED = (128, [128, 128, 128], (3, 4))
KEYS = ("weights", "biases", "head_weights", "head_biases")


def _params(case, dtype, requires_grad=True):
    out = []
    for k in KEYS:
        out.append([None if a is None else _dev(a, dtype).requires_grad_(requires_grad) for a in case[k]])
    return out


def _native(case, dtype, activation, act_after=None, douts=None, x=None, x_grad=True, p_grad=True):
    """(outs, grads dict as GR.gradients lays it out, tensors or None) of one forward + backward of mlp_heads_autograd."""
    from igs_amd.motion import mlp_heads_autograd
    x = (_dev(case["x"], dtype) if x is None else x).detach().requires_grad_(x_grad)
    ws, bs, hws, hbs = _params(case, dtype, p_grad)
    outs = mlp_heads_autograd(x, ws, bs, hws, hbs, activation, act_after)
    douts = case["douts"] if douts is None else douts
    used = [(o, g) for o, g in zip(outs, douts) if g is not None]
    torch.autograd.backward([o for o, _ in used], [g if torch.is_tensor(g) else _dev(g, dtype) for _, g in used])
    grad = lambda t: None if t is None else t.grad
    return outs, dict(dx=x.grad, dw=[grad(w) for w in ws], db=[grad(b) for b in bs], dhw=[grad(w) for w in hws], dhb=[grad(b) for b in hbs])


def _ratios(got, want, bound, skip_none=False):
    out = {}
    for (name, g), (_, w), (_, e) in zip(GR.flat(got), GR.flat(want), GR.flat(bound)):
        if g is None:
            assert skip_none, name
            continue
        assert tuple(g.shape) == w.shape, name
        out[name] = DR.worst_ratio(g.double().cpu().numpy(), w, e)
    return out


# ---------------------------------------------------------------- exact cases
EXACT = ([dict(C0=128, hidden=[128], heads=(3, 4), N=129), dict(C0=33, hidden=[24, 24], heads=(3, 4, 48, 1, 3), N=129),
          dict(C0=33, hidden=[128, 128, 128], heads=(128,), N=129), dict(C0=128, hidden=[128, 128, 128], heads=(3, 4), N=257),
          dict(C0=100, hidden=[128, 24, 64], heads=(7,), N=65), dict(C0=128, hidden=[], heads=(3, 4), N=97)]
         + [dict(C0=c, hidden=[128], heads=(3, 4), N=129) for c in (1, 3, 31, 33)]
         + [dict(C0=128, hidden=[128], heads=(3, 4), N=n, density=0.2) for n in (1, 31, 32, 33, 127, 128)]
         + [dict(C0=128, hidden=[128, 128, 128], heads=(3, 4), N=257, bias=False), dict(C0=40, hidden=[48, 24], heads=(3, 4), N=70, act_after=[1, 0])]
         + [dict(C0=128, hidden=[128], heads=(3, 4), N=70001, density=0.002)])


def _exact_id(c):
    return "C%d-%s-heads%s-N%d%s%s" % (c["C0"], "x".join(map(str, c["hidden"])) or "none", "+".join(map(str, c["heads"])), c["N"],
                                       "" if c.get("bias", True) else "-nobias", "-aa" + "".join(map(str, c["act_after"])) if "act_after" in c else "")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cfg", EXACT, ids=_exact_id)
def test_exact_integer_gradients_are_bit_equal(cfg, dtype):
    """ReLU on small integers with dY in {-1, 0, 1}: every partial sum of the backward is exact in either precision in any order
    (exact_grad_case asserts it), so a transposition, k-permutation, padding, tail, head-split or slice error, or a wrong derivative at
    z == 0, changes a value.  N = 70001 spans several chunks, many workgroups and every slice of the reduction."""
    case = GR.exact_grad_case(cfg["C0"], cfg["hidden"], cfg["heads"], cfg["N"], density=cfg.get("density", 0.05), seed=len(cfg["hidden"]) + cfg["C0"],
                              bias=cfg.get("bias", True), act_after=cfg.get("act_after"))
    outs, got = _native(case, dtype, "relu", act_after=cfg.get("act_after"))
    for o, want in zip(outs, case["outs"]):
        assert np.array_equal(o.detach().double().cpu().numpy(), want)
    for (name, g), (_, want) in zip(GR.flat(got), GR.flat(case["grads"])):
        if g is None:
            assert not cfg.get("bias", True) and name.startswith(("db", "dhb")), name
            continue
        assert g.dtype == dtype and tuple(g.shape) == want.shape, name
        assert np.array_equal(g.double().cpu().numpy(), want), name


# ---------------------------------------------------------------- SiLU inside the bound
def _with_douts(case, heads, N, dtype, seed):
    rng = np.random.RandomState(seed + 7)
    rnd = np.float16 if dtype == torch.float16 else np.float32
    case["douts"] = [rng.standard_normal((N, ch)).astype(rnd).astype(np.float64) for ch in heads]
    return case


def _eager(case, dtype, aa):
    """eager PyTorch's gradients on the same inputs, as _native lays them out"""
    x = _dev(case["x"], dtype).requires_grad_(True)
    ws, bs, hws, hbs = _params(case, dtype)
    h = x
    for w, b, on in zip(ws, bs, aa):
        h = torch.nn.functional.linear(h, w, b)
        h = torch.nn.functional.silu(h) if on else h
    outs = [torch.nn.functional.linear(h, w, b) for w, b in zip(hws, hbs)]
    torch.autograd.backward(outs, [_dev(g, dtype) for g in case["douts"]])
    return dict(dx=x.grad, dw=[w.grad for w in ws], db=[b.grad for b in bs], dhw=[w.grad for w in hws], dhb=[b.grad for b in hbs])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cfg", [SHIPPED + (2000,), SHIPPED + (70001,), (33, [50, 77], (3, 4, 5), 1001)], ids=["shipped-N2000", "shipped-N70001", "odd-widths"])
def test_silu_gradients_within_the_derived_bound(cfg, dtype):
    C0, hidden, heads, N = cfg
    half = dtype == torch.float16
    case = _with_douts(_float_case(C0, hidden, heads, N, dtype, seed=N + C0), heads, N, dtype, N)
    aa = [1] * (len(hidden) - 1) + [0]
    want, bound = GR.gradients_with_bound(*[case[k] for k in ("x",) + KEYS], case["douts"], "silu", aa, half=half, round_params=True)
    _, got = _native(case, dtype, "silu", act_after=aa)
    ratios = _ratios(got, want, bound)
    print("decoder backward %s %s: worst |error| / bound %.3g; per tensor %s" % (cfg, dtype, max(ratios.values()), {k: "%.3g" % v for k, v in ratios.items()}))
    er = _ratios(_eager(case, dtype, aa), want, bound)
    print("    eager PyTorch against the same bound (not asserted): worst %.3g; %s" % (max(er.values()), {k: "%.3g" % v for k, v in er.items()}))
    assert all(torch.isfinite(g).all() for _, g in GR.flat(got))
    assert max(ratios.values()) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_silu_gradients_with_large_pre_activations_stay_finite_and_within_the_bound(dtype):
    C, N = 16, 16 * len(LARGE) * 2
    case = _float_case(C, [C, 24, 16], (3, 4), N, dtype, seed=41)
    case["weights"][0], case["biases"][0] = np.eye(C), np.zeros(C)
    for n in range(N):
        case["x"][n, n % C] = LARGE[(n // C) % len(LARGE)]
    case = _with_douts(case, (3, 4), N, dtype, 41)
    aa = [1, 1, 0]
    want, bound = GR.gradients_with_bound(*[case[k] for k in ("x",) + KEYS], case["douts"], "silu", aa, half=dtype == torch.float16, round_params=True)
    _, got = _native(case, dtype, "silu", act_after=aa)
    ratios = _ratios(got, want, bound)
    print("decoder backward with pre-activations up to 1e4 %s: worst |error| / bound %.3g" % (dtype, max(ratios.values())))
    assert all(torch.isfinite(g).all() for _, g in GR.flat(got))
    assert max(ratios.values()) <= 1.0


def test_the_bound_has_teeth():
    """The shipped shape at N = 129: a reference without the last row's contribution to the weight gradients, and one with the derivative
    of two hidden channels swapped, are both outside the bound of the native result."""
    C0, hidden, heads = SHIPPED
    N, aa = 129, [1, 1, 0]
    case = _with_douts(_float_case(C0, hidden, heads, N, torch.float32, seed=9), heads, N, torch.float32, 9)
    args = [case[k] for k in ("x",) + KEYS]
    want, bound = GR.gradients_with_bound(*args, case["douts"], "silu", aa)
    _, got = _native(case, torch.float32, "silu", act_after=aa)
    assert max(_ratios(got, want, bound).values()) <= 1.0
    short = GR.gradients(case["x"][:-1], *args[1:], [d[:-1] for d in case["douts"]], "silu", aa)
    r_short = {k: v for k, v in _ratios({k: (None if k == "dx" else v) for k, v in got.items()}, dict(short, dx=want["dx"]), bound, skip_none=True).items()}

    def swap(l, a):
        a = a.copy()
        if l == 1:
            a[:, [5, 6]] = a[:, [6, 5]]
        return a
    swapped = GR.gradients_with_bound(*args, case["douts"], "silu", aa, dact_hook=swap)[0]
    r_swap = _ratios(got, swapped, bound)
    print("teeth: last row left out %.3g, two derivative channels swapped %.3g" % (max(r_short.values()), max(r_swap.values())))
    assert max(r_short.values()) > 1.0 and max(r_swap.values()) > 1.0


# ---------------------------------------------------------------- optional gradients
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_optional_gradients(dtype):
    half = dtype == torch.float16
    case = _with_douts(_float_case(33, [50, 77], (3, 4, 5), 301, dtype, seed=12), (3, 4, 5), 301, dtype, 12)
    case["biases"][1] = None
    case["head_biases"][0] = None
    aa = [1, 0]
    args = [case[k] for k in ("x",) + KEYS]
    want, bound = GR.gradients_with_bound(*args, case["douts"], "silu", aa, half=half, round_params=True)
    _, full = _native(case, dtype, "silu", act_after=aa)
    assert full["db"][1] is None and full["dhb"][0] is None and full["db"][0] is not None
    for name, g in GR.flat(full):
        assert g is None or g.dtype == dtype, name
    assert max(_ratios(full, want, bound, skip_none=True).values()) <= 1.0
    _, only_x = _native(case, dtype, "silu", act_after=aa, p_grad=False)
    assert all(g is None for name, g in GR.flat(only_x) if name != "dx") and _same_bits(only_x["dx"], full["dx"])
    _, only_p = _native(case, dtype, "silu", act_after=aa, x_grad=False)
    assert only_p["dx"] is None
    for (name, a), (_, b) in zip(GR.flat(only_p), GR.flat(full)):
        assert name == "dx" or (a is None and b is None) or _same_bits(a, b), name
    # one head unused: its gradient arrives as None and is a zero dY
    douts = [case["douts"][0], None, case["douts"][2]]
    want1, bound1 = GR.gradients_with_bound(*args, [douts[0], np.zeros((301, 4)), douts[2]], "silu", aa, half=half, round_params=True)
    _, unused = _native(case, dtype, "silu", act_after=aa, douts=douts)
    ratios = _ratios(unused, want1, bound1, skip_none=True)
    print("optional gradients %s: one head unused, worst |error| / bound %.3g" % (dtype, max(ratios.values())))
    assert max(ratios.values()) <= 1.0 and not unused["dhw"][1].any() and not unused["dhb"][1].any()


# ---------------------------------------------------------------- views, stream, empty input
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_views_side_stream_and_empty_input(dtype):
    C0, hidden, heads = SHIPPED
    N = 1000
    case = _with_douts(_float_case(C0, hidden, heads, N, dtype, seed=6), heads, N, dtype, 6)
    x = _dev(case["x"], dtype)
    _, want = _native(case, dtype, "silu", x=x)
    big = torch.randn(N + 7, 128, device=DEV).to(dtype)
    big[3:N + 3] = x
    wide = torch.full((N, 160), float("nan"), dtype=dtype, device=DEV)
    wide[:, :128] = x
    odd = torch.zeros(N, 131, dtype=dtype, device=DEV)
    odd[:, 1:129] = x
    g_nc = [_dev(g, dtype) for g in case["douts"]]
    g_nc = [torch.stack([g, g], 2)[:, :, 0] for g in g_nc]                                       # non-contiguous upstream gradients
    assert not g_nc[0].is_contiguous()
    runs = [_native(case, dtype, "silu", x=big[3:N + 3])[1], _native(case, dtype, "silu", x=wide[:, :128])[1],
            _native(case, dtype, "silu", x=odd[:, 1:129])[1], _native(case, dtype, "silu", x=x, douts=g_nc)[1]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(_native(case, dtype, "silu", x=x)[1])
    side.synchronize()
    for got in runs:
        for (name, a), (_, b) in zip(GR.flat(got), GR.flat(want)):
            assert _same_bits(a, b), name
    outs, empty = _native(case, dtype, "silu", x=x[:0], douts=[torch.zeros(0, 3, dtype=dtype, device=DEV), torch.zeros(0, 4, dtype=dtype, device=DEV)])
    assert [tuple(o.shape) for o in outs] == [(0, 3), (0, 4)] and tuple(empty["dx"].shape) == (0, 128) and empty["dx"].dtype == dtype
    for (name, g), (_, w) in zip(GR.flat(empty), GR.flat(want)):
        assert g.dtype == dtype and (g.shape == w.shape and not g.any() if name != "dx" else True), name


# ---------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reproducible_and_rows_do_not_see_one_another(dtype):
    C0, hidden, heads = SHIPPED
    N = 4000
    case = _with_douts(_float_case(C0, hidden, heads, N, dtype, seed=5), heads, N, dtype, 5)
    _, a = _native(case, dtype, "silu")
    _, b = _native(case, dtype, "silu")
    for (name, u), (_, v) in zip(GR.flat(a), GR.flat(b)):
        assert _same_bits(u, v), name
    small = dict(case, x=case["x"][:33], douts=[d[:33] for d in case["douts"]])
    _, c = _native(small, dtype, "silu")
    assert _same_bits(c["dx"], a["dx"][:33])


# ---------------------------------------------------------------- the memory contract
def test_memory_contract_at_70001_rows():
    """Between forward and backward nothing of N rows exists but x (and the outputs); the backward's peak is the reported scratch, the
    gradients themselves and small change."""
    from igs_amd._cabi import ext
    from igs_amd.motion import mlp_heads_autograd, pack_mlp
    C0, hidden, heads = SHIPPED
    N = 70001
    case = _float_case(C0, hidden, heads, N, torch.float32, seed=8)
    x = _dev(case["x"], torch.float32).requires_grad_(True)
    ws, bs, hws, hbs = _params(case, torch.float32)
    packed = pack_mlp(ws, bs, hws, hbs, transposed=True)
    douts = [torch.randn(N, ch, device=DEV) for ch in heads]
    act = N * 128 * 4
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    outs = mlp_heads_autograd(x, ws, bs, hws, hbs, "silu", [1, 1, 0], packed=packed)
    torch.cuda.synchronize()
    out_bytes = sum(o.numel() * 4 for o in outs)
    grown = torch.cuda.memory_allocated() - base
    print("memory: forward under grad keeps %.2f MB beside the outputs' %.2f MB (one activation: %.1f MB)" % ((grown - out_bytes) / 1e6, out_bytes / 1e6, act / 1e6))
    assert grown - out_bytes < act
    scratch = ext()._mlp.bwd_scratch_bytes(N, False, [C0] + hidden, list(heads))
    assert scratch == ext()._mlp.bwd_scratch_bytes(10 * N, False, [C0] + hidden, list(heads)) > 0
    grads = x.numel() * 4 + sum(p.numel() * 4 for p in ws + bs + hws + hbs)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch.autograd.backward(outs, douts)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("memory: backward peak %.1f MB above the baseline; scratch %.1f MB, gradients %.1f MB" % (peak / 1e6, scratch / 1e6, grads / 1e6))
    assert peak < scratch + grads + act
    assert x.grad is not None and ws[0].grad is not None


# ---------------------------------------------------------------- the bound module
def _renderer(dtype, **kw):
    r = DR.make_renderer(**kw)
    with torch.no_grad():
        r.out_layers[1].bias.copy_(torch.tensor([1.0, 1e-2, 1e-2, 1e-2]))
    return r.to(DEV).to(dtype)


def _module_grads(r):
    lin = [m for m in r.mlp_net.layers if isinstance(m, torch.nn.Linear)]
    return dict(dw=[m.weight.grad for m in lin], db=[m.bias.grad for m in lin], dhw=[m.weight.grad for m in r.out_layers], dhb=[m.bias.grad for m in r.out_layers])


def _module_check(r, x, douts, half, what):
    """loss.backward() through the bound method, every parameter's .grad inside the bound on the module's current weights"""
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    r.zero_grad(set_to_none=True)
    x = x.detach().requires_grad_(True)
    d = r.decode_residual_feature(x)
    loss = sum((d[k].float() * g.float()).sum() for k, g in zip(d, douts))
    loss.backward()
    dn = [g.to(d[k].dtype).double().cpu().numpy() for k, g in zip(d, douts)]
    want, bound = GR.gradients_with_bound(x.detach().double().cpu().numpy(), ws, bs, hws, hbs, dn, "silu", aa, half=half, round_params=False)
    got = dict(_module_grads(r), dx=x.grad)
    assert all(g is not None for _, g in GR.flat(got))
    ratios = _ratios(got, want, bound)
    print("bound module %s: worst |error| / bound %.3g" % (what, max(ratios.values())))
    assert max(ratios.values()) <= 1.0
    return d, got


def test_training_binder_fills_every_grad_and_follows_optimiser_steps():
    from igs_amd.motion import decode_residual_feature, use_native_decoder
    r = _renderer(torch.float32, dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=3)
    assert len(list(r.parameters())) == 10
    g = torch.Generator().manual_seed(2)
    x = torch.randn(777, 128, generator=g).to(DEV)
    douts = [torch.randn(777, 3, generator=g).to(DEV), torch.randn(777, 4, generator=g).to(DEV)]
    assert use_native_decoder(r, training=True) == 5
    d, first = _module_check(r, x, douts, False, "float32")
    assert list(d) == ["xyz", "rotation"] and d["xyz"].dtype == torch.float32 and d["xyz"].requires_grad
    opt = torch.optim.SGD(r.parameters(), lr=0.5)
    opt.step()                                                                                   # in place: both packs must be rebuilt
    _, second = _module_check(r, x, douts, False, "float32 after an optimiser step")
    assert not torch.equal(first["dw"][0], second["dw"][0])
    with torch.no_grad():
        a = r.decode_residual_feature(x)
        b = decode_residual_feature(r, x)
    assert all(_same_bits(a[k], b[k]) and not a[k].requires_grad for k in a)


def test_training_binder_under_autocast():
    from igs_amd.motion import use_native_decoder
    r = _renderer(torch.float32, dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=4)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(500, 128, generator=g).half().float().to(DEV)                                # (exact in half: the cast is no error of the kernel's)
    douts = [torch.randn(500, 3, generator=g).to(DEV), torch.randn(500, 4, generator=g).to(DEV)]
    use_native_decoder(r, training=True)
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    hr = lambda arrs: [None if a is None else a.astype(np.float16).astype(np.float64) for a in arrs]
    with torch.autocast("cuda", dtype=torch.float16):
        xg = x.clone().requires_grad_(True)
        d = r.decode_residual_feature(xg)
        assert all(v.dtype == torch.float16 for v in d.values())
        loss = sum((d[k].float() * gk).sum() for k, gk in zip(d, douts))
    loss.backward()
    got = dict(_module_grads(r), dx=xg.grad)
    assert all(t.dtype == torch.float32 for _, t in GR.flat(got))
    dn = [gk.half().double().cpu().numpy() for gk in douts]
    # the kernel sees the half-rounded weights (biases stay float32); the derived half bound is about those
    want, bound = GR.gradients_with_bound(x.double().cpu().numpy(), hr(ws), bs, hr(hws), hbs, dn, "silu", aa, half=True, round_params=False)
    ratios = _ratios(got, want, bound)
    print("bound module under float16 autocast: worst |error| / bound %.3g" % max(ratios.values()))
    assert max(ratios.values()) <= 1.0
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(NotImplementedError, match="autocast"):
        r.decode_residual_feature(x.clone().requires_grad_(True))


# ---------------------------------------------------------------- the chain
def test_chain_interpolation_decoder_deform_gradient_to_the_anchor_features():
    """query_ir_grid -> bound decoder -> deform -> a scalar loss; the gradient to the anchor features against the same chain with the
    module's PyTorch decoder lines.  Both decoders' d x are within the derived bound e of the exact one for the upstream gradient they
    were given, so they differ by at most 2 e per interpolated row; the interpolation's backward is linear, d F[a] = sum w[n, k] d x[n]
    over the slots that name anchor a, which carries 2 e through exactly (in float64), plus its own float32 roundings of a sum of that
    many terms."""
    from igs_amd import motion
    P, M, K, A, D = 5000, 3000, 8, 512, 128
    g = torch.Generator().manual_seed(11)
    feats = (torch.randn(1, A, D, generator=g) * 0.5).to(DEV)
    col = torch.randint(0, A, (M, K), generator=g).to(DEV)
    w = torch.softmax(torch.randn(M, K, generator=g), dim=1).unsqueeze(-1).to(DEV)
    nb = (None, col.reshape(-1), None, torch.zeros(M, dtype=torch.long, device=DEV))
    mask = torch.randperm(P, generator=g)[:M].to(DEV)
    tx, tr = torch.randn(P, 3, generator=g).to(DEV), torch.randn(P, 4, generator=g).to(DEV)

    class G:
        pass
    gs = G()
    gs.xyz, gs.rotation = (torch.rand(P, 3, generator=g) * 4 - 2).to(DEV), torch.randn(P, 4, generator=g).to(DEV)
    gs.opacity, gs.scaling, gs.shs = torch.randn(P, 1, device=DEV), torch.randn(P, 3, device=DEV), torch.randn(P, 16, 3, device=DEV)
    r = _renderer(torch.float32, dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=4)

    def run():
        F = feats.clone().requires_grad_(True)
        (f,) = motion.query_ir_grid(F, w, nb, counts=[M])
        f.retain_grad()
        res = r.decode_residual_feature(f)
        for v in res.values():
            v.retain_grad()
        out = motion.deform(gs, res, mask)
        loss = (out["xyz"] * tx).sum() + (out["rotation"] * tr).sum()
        loss.backward()
        return F.grad, f.detach(), [v.grad for v in res.values()], f.grad
    ref_dF, f, ref_douts, ref_dx = run()
    motion.use_native_decoder(r, training=True)
    dF, f2, douts, dx = run()
    assert torch.equal(f, f2) and dF.shape == ref_dF.shape == feats.shape
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    fx = f.double().cpu().numpy()
    bounds = [GR.gradients_with_bound(fx, ws, bs, hws, hbs, [d.double().cpu().numpy() for d in dd], "silu", aa)[1]["dx"] for dd in (ref_douts, douts)]
    # the two runs' upstream gradients differ (deform's backward saw two slightly different forwards); the exact backward is linear in
    # d Y, so that difference reaches d x as the exact backward of the difference
    ddx = GR.gradients(fx, ws, bs, hws, hbs, [(a.double() - b.double()).cpu().numpy() for a, b in zip(douts, ref_douts)], "silu", aa)
    rows = torch.from_numpy(bounds[0] + bounds[1] + np.abs(ddx["dx"])).to(DEV)                   # >= |d x native - d x eager| per interpolated row
    wk = w.squeeze(-1).double()
    spread = lambda v: torch.zeros(A, D, dtype=torch.float64, device=DEV).index_add_(0, col.reshape(-1), (wk.unsqueeze(-1) * v.unsqueeze(1)).reshape(M * K, D))
    cnt = torch.bincount(col.reshape(-1), minlength=A).double().unsqueeze(1)
    tol = spread(rows) + (cnt + 2) * 2.0 ** -24 * spread(dx.abs().double() + ref_dx.abs().double())      # ... and the two float32 sums' own roundings
    d = (dF[0].double() - ref_dF[0].double()).abs()
    print("chain backward: worst |d F native - d F eager| / bound %.3g" % (d / tol).max().item())
    assert (d <= tol).all() and dF.abs().max() > 0
