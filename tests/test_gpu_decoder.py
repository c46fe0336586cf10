"""The fused residual decoder on the MI355X (igs_amd/motion.py over igs_amd/csrc/mlp.hip) against the float64 restatement of
tests/decoder_restatement.py: exact integer cases bit for bit, SiLU cases inside the derived bound, row independence, views, streams, the
weight cache of the bound module, and the chain query_ir_grid -> decode_residual_feature -> deform.

Worst |error| / bound seen on the MI355X is recorded in DESIGN.md section 21; every float test prints its own."""
import numpy as np
import pytest
import torch

import decoder_restatement as DR

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16]
IDS = ["f32", "f16"]


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.asarray(a)).to(dtype).to(DEV)


def _native(case, dtype, activation, act_after=None, x=None):
    from igs_amd.motion import mlp_heads
    x = _dev(case["x"], dtype) if x is None else x
    with torch.no_grad():
        return mlp_heads(x, [_dev(w, dtype) for w in case["weights"]], [_dev(b, dtype) for b in case["biases"]],
                         [_dev(w, dtype) for w in case["head_weights"]], [_dev(b, dtype) for b in case["head_biases"]], activation, act_after)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------- exact cases
EXACT = ([dict(C0=128, hidden=[128], heads=(3, 4), N=n) for n in (1, 31, 32, 33, 127, 128, 129, 70001)]
         + [dict(C0=c, hidden=[128], heads=(3, 4), N=129) for c in (1, 3, 16, 31, 32, 33, 127)]
         + [dict(C0=33, hidden=[w] * L, heads=hd, N=129) for w in (24, 64, 128) for L, hd in ((1, (7,)), (2, (3, 4, 48, 1, 3)), (3, (128,)))]
         + [dict(C0=c, hidden=[], heads=hd, N=97) for c, hd in ((128, (3, 4)), (33, (7,)), (64, (3, 4, 48, 1, 3)), (128, (128,)))]
         + [dict(C0=128, hidden=[128, 128, 128], heads=hd, N=257, bias=b) for hd in ((3, 4), (3, 4, 48, 1, 3)) for b in (True, False)]
         + [dict(C0=20, hidden=[24, 64], heads=(128,), N=33, bias=False), dict(C0=100, hidden=[128, 24, 64], heads=(7,), N=65)])


def _exact_id(c):
    return "C%d-%s-heads%s-N%d%s" % (c["C0"], "x".join(map(str, c["hidden"])) or "none", "+".join(map(str, c["heads"])), c["N"],
                                     "" if c.get("bias", True) else "-nobias")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cfg", EXACT, ids=_exact_id)
def test_exact_integer_cases_are_bit_equal(cfg, dtype):
    """ReLU on small integers: every partial sum is exact in either precision in any order (exact_case asserts it), so any operand-layout,
    k-permutation, padding, tail or head-split error changes a value."""
    case = DR.exact_case(cfg["C0"], cfg["hidden"], cfg["heads"], cfg["N"], bias=cfg.get("bias", True), seed=len(cfg["hidden"]) + cfg["C0"])
    outs = _native(case, dtype, "relu")
    assert len(outs) == len(cfg["heads"])
    for o, want, ch in zip(outs, case["outs"], cfg["heads"]):
        assert o.dtype == dtype and o.shape == (cfg["N"], ch) and o.is_contiguous()
        assert np.array_equal(o.double().cpu().numpy(), want)
    assert any(np.abs(w).max() > 0 for w in case["outs"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_case_without_activation_behind_the_last_hidden_linear(dtype):
    """The reference's MLP ends on a Linear (networks.py:85-90): the per-layer flag."""
    case = DR.exact_case(40, [48, 24], (3, 4), 70, seed=77, nnz=2)
    want = DR.forward(case["x"], case["weights"], case["biases"], case["head_weights"], case["head_biases"], "relu", act_after=[1, 0])
    assert max(np.abs(w).max() for w in want) < 2 ** 11
    for o, w in zip(_native(case, dtype, "relu", act_after=[1, 0]), want):
        assert np.array_equal(o.double().cpu().numpy(), w)
    assert not all(np.array_equal(a, b) for a, b in zip(want, case["outs"]))                     # (the flag matters on this case)


# ---------------------------------------------------------------- SiLU inside the bound
def _float_case(C0, hidden, heads, N, dtype, seed):
    rng = np.random.RandomState(seed)
    widths = [C0] + list(hidden)
    rnd = (lambda a: None if a is None else a.astype(np.float16).astype(np.float64)) if dtype == torch.float16 else (lambda a: a.astype(np.float32).astype(np.float64) if a is not None else None)
    hid = [DR.linear_init(widths[l + 1], widths[l], rng) for l in range(len(hidden))]
    hd = [DR.linear_init(ch, widths[-1], rng) for ch in heads]
    return dict(x=rnd(rng.standard_normal((N, C0))), weights=[rnd(w) for w, _ in hid], biases=[rnd(b) for _, b in hid],
                head_weights=[rnd(w) for w, _ in hd], head_biases=[rnd(b) for _, b in hd])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cfg", [(128, [128, 128, 128], (3, 4), 2000), (128, [128, 128, 128], (3, 4), 70001), (33, [50, 77], (3, 4, 5), 1001)],
                         ids=["shipped-N2000", "shipped-N70001", "odd-widths"])
def test_silu_decoder_within_the_derived_bound(cfg, dtype):
    """The shipped shape (configs/train.yaml:205-217: 128 -> 128 -> 128 -> 128 with no activation behind the last, heads 3 + 4) and an odd
    one, weights as nn.Linear draws them."""
    C0, hidden, heads, N = cfg
    case = _float_case(C0, hidden, heads, N, dtype, seed=N + C0)
    aa = [1] * (len(hidden) - 1) + [0]
    want, bound = DR.forward_with_bound(case["x"], case["weights"], case["biases"], case["head_weights"], case["head_biases"], "silu", aa,
                                        half=dtype == torch.float16)
    outs = _native(case, dtype, "silu", act_after=aa)
    ratios = [DR.worst_ratio(o.double().cpu().numpy(), w, b) for o, w, b in zip(outs, want, bound)]
    print("decoder %s %s: worst |error| / bound per head %s" % (cfg, dtype, ["%.3g" % r for r in ratios]))
    assert all(np.isfinite(o.float().cpu().numpy()).all() for o in outs)
    assert max(ratios) <= 1.0


LARGE = (60.0, -60.0, 90.0, -90.0, 100.0, -100.0, 1e4, -1e4, 87.0, -87.5, 128.0, -129.0, 700.0, -700.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_silu_with_large_pre_activations_stays_finite_and_within_the_bound(dtype):
    """Hidden pre-activations far outside the range random weights give: the first Linear is the identity, so z0 is x itself, and one
    channel of every row holds one of LARGE (exact in half), the others standard normal values.  exp(-z) overflows float32 below
    z = -88.7: the kernel must return the tiny value (or -0) there, not a NaN that would run through the later layers into the residuals."""
    C, N = 16, 16 * len(LARGE) * 2
    case = _float_case(C, [C, 24, 16], (3, 4), N, dtype, seed=41)
    case["weights"][0], case["biases"][0] = np.eye(C), np.zeros(C)
    for n in range(N):
        case["x"][n, n % C] = LARGE[(n // C) % len(LARGE)]
    aa = [1, 1, 0]
    want, bound = DR.forward_with_bound(case["x"], case["weights"], case["biases"], case["head_weights"], case["head_biases"], "silu", aa,
                                        half=dtype == torch.float16)
    z1 = DR.silu(case["x"]) @ case["weights"][1].T + case["biases"][1]
    assert np.abs(case["x"]).max() == 1e4 and (z1 < -100).any() and (z1 > 100).any()           # large in the second layer too
    outs = _native(case, dtype, "silu", act_after=aa)
    ratios = [DR.worst_ratio(o.double().cpu().numpy(), w, b) for o, w, b in zip(outs, want, bound)]
    print("decoder with pre-activations up to 1e4 %s: worst |error| / bound per head %s" % (dtype, ["%.3g" % r for r in ratios]))
    assert all(np.isfinite(o.float().cpu().numpy()).all() for o in outs)
    assert max(ratios) <= 1.0


@pytest.mark.parametrize("activation", ["silu", "relu"])
def test_a_nan_row_comes_out_nan_and_touches_no_other_row(activation):
    case = _float_case(32, [32, 32], (3, 4), 70, torch.float32, seed=43)
    x = _dev(case["x"], torch.float32)
    clean = _native(case, torch.float32, activation, x=x)
    x2 = x.clone()
    x2[33, 5] = float("nan")
    got = _native(case, torch.float32, activation, x=x2)
    keep = torch.arange(70, device=DEV) != 33
    for g, c in zip(got, clean):
        assert torch.isnan(g[33]).all() and _same_bits(g[keep], c[keep])                         # as torch.relu and F.silu propagate it


# ---------------------------------------------------------------- rows do not see one another
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reproducible_and_independent_of_the_other_rows(dtype):
    case = _float_case(128, [128, 128, 128], (3, 4), 70001, dtype, seed=5)
    x = _dev(case["x"], dtype)
    a = _native(case, dtype, "silu", x=x)
    b = _native(case, dtype, "silu", x=x)
    perm = torch.randperm(70001, generator=torch.Generator().manual_seed(1)).to(DEV)
    p = _native(case, dtype, "silu", x=x[perm].contiguous())
    head = _native(case, dtype, "silu", x=x[:33].contiguous())
    for k in range(2):
        assert _same_bits(a[k], b[k])
        assert _same_bits(p[k], a[k][perm])
        assert _same_bits(head[k], a[k][:33])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_strided_view_side_stream_and_empty_input(dtype):
    case = _float_case(128, [128, 128, 128], (3, 4), 1000, dtype, seed=6)
    x = _dev(case["x"], dtype)
    want = _native(case, dtype, "silu", x=x)
    wide = torch.full((1000, 160), float("nan"), dtype=dtype, device=DEV)
    wide[:, :128] = x
    view = wide[:, :128]
    assert view.stride() == (160, 1) and view.data_ptr() == wide.data_ptr()
    got = _native(case, dtype, "silu", x=view)
    odd = torch.zeros(1000, 131, dtype=dtype, device=DEV)                                        # a row stride that rules out the four-element loads
    odd[:, 1:129] = x
    got_odd = _native(case, dtype, "silu", x=odd[:, 1:129])
    cols = x.t().contiguous().t()                                                                # channel-strided: copied first
    assert cols.stride() == (1, 1000)
    got_cols = _native(case, dtype, "silu", x=cols)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_side = _native(case, dtype, "silu", x=x)
    side.synchronize()
    for k in range(2):
        for g in (got, got_odd, got_cols, got_side):
            assert _same_bits(g[k], want[k])
    empty = _native(case, dtype, "silu", x=x[:0])
    assert [tuple(e.shape) for e in empty] == [(0, 3), (0, 4)] and all(e.dtype == dtype for e in empty)


def test_graph_capture_replays_the_call():
    """No allocation but the outputs, no host synchronisation: the call can be captured."""
    case = _float_case(128, [128, 128, 128], (3, 4), 500, torch.float32, seed=8)
    from igs_amd.motion import mlp_heads, pack_mlp
    args = [[_dev(w, torch.float32) for w in case[k]] for k in ("weights", "biases", "head_weights", "head_biases")]
    packed = pack_mlp(*args)
    x = _dev(case["x"], torch.float32)
    with torch.no_grad():
        want = mlp_heads(x, *args, packed=packed)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = mlp_heads(x, *args, packed=packed)
        x.copy_(x.flip(0))
        graph.replay()
        torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert _same_bits(o, w.flip(0))


# ---------------------------------------------------------------- the bound module
def _renderer(dtype, **kw):
    r = DR.make_renderer(**kw)
    with torch.no_grad():
        r.out_layers[1].bias.copy_(torch.tensor([1.0, 1e-2, 1e-2, 1e-2]))                        # the shipped rotation bias (gs.py:553)
    return r.to(DEV).to(dtype).eval()


def _restated(r, x, half):
    ws, bs, hws, hbs, aa = DR.renderer_parts(r)
    act = "relu" if any(isinstance(m, torch.nn.ReLU) for m in r.mlp_net.layers) else "silu"
    return DR.forward_with_bound(x.double().cpu().numpy(), ws, bs, hws, hbs, act, aa, half=half)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bound_module_returns_the_reference_dict_and_follows_in_place_updates(dtype):
    from igs_amd.motion import use_native_decoder
    r = _renderer(dtype, dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=3)
    x = torch.randn(777, 128, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    with torch.no_grad():
        eager = r.decode_residual_feature(x)
        assert use_native_decoder(r) == 5
        for trial in range(2):
            got = r.decode_residual_feature(x)
            cur = type(r).decode_residual_feature(r, x)                                          # the PyTorch lines on the current weights
            assert list(got) == list(eager) == ["xyz", "rotation"]
            want, bound = _restated(r, x, dtype == torch.float16)
            for k, w, b in zip(got, want, bound):
                assert got[k].shape == eager[k].shape and got[k].dtype == eager[k].dtype == dtype and got[k].is_contiguous()
                ratio = DR.worst_ratio(got[k].double().cpu().numpy(), w, b)
                print("bound module %s %s trial %d: worst |error| / bound %.3g" % (k, dtype, trial, ratio))
                assert ratio <= 1.0
                # for a maintainer, not asserted: the distance to eager PyTorch in the same dtype, in units of the dtype's rounding of the largest value
                ulp = (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -11) * np.abs(w).max()
                print("    |native - eager| max %.3g units, |eager - float64| max %.3g units, |native - float64| max %.3g units" % (
                    (got[k].double() - cur[k].double()).abs().max().item() / ulp, np.abs(cur[k].double().cpu().numpy() - w).max() / ulp,
                    np.abs(got[k].double().cpu().numpy() - w).max() / ulp))
            before = [got[k].clone() for k in got]
            r.mlp_net.layers[0].weight.mul_(2)                                                   # in place: the pack must be rebuilt
        assert not torch.equal(before[0], r.decode_residual_feature(x)["xyz"])
    with pytest.raises(NotImplementedError, match="forward only"):
        r.decode_residual_feature(x)                                                             # grad enabled, parameters require grad


def test_chain_interpolation_decoder_deform_against_the_pytorch_decoder_lines():
    """query_ir_grid -> decode_residual_feature -> deform on 3 000 in-box Gaussians, native decoder against the module's own PyTorch lines.
    Both decoders are within the derived bound e of the exact result, so the residuals differ by at most 2 e; deform adds xyz + res_xyz
    (two roundings of a sum of that size) and multiplies rotation by res_rotation / |res_rotation|, whose change is at most
    2 |d res| / |res| in norm, times |rotation|, plus a few roundings of the product."""
    from igs_amd import motion
    P, M, K, A, D = 5000, 3000, 8, 512, 128
    g = torch.Generator().manual_seed(11)
    feats = (torch.randn(1, A, D, generator=g) * 0.5).to(DEV)
    col = torch.randint(0, A, (M, K), generator=g).to(DEV)
    w = torch.softmax(torch.randn(M, K, generator=g), dim=1).unsqueeze(-1).to(DEV)
    nb = (None, col.reshape(-1), None, torch.zeros(M, dtype=torch.long, device=DEV))
    mask = torch.randperm(P, generator=g)[:M].to(DEV)

    class G:
        pass
    gs = G()
    gs.xyz, gs.rotation = (torch.rand(P, 3, generator=g) * 4 - 2).to(DEV), torch.randn(P, 4, generator=g).to(DEV)
    gs.opacity, gs.scaling, gs.shs = torch.randn(P, 1, device=DEV), torch.randn(P, 3, device=DEV), torch.randn(P, 16, 3, device=DEV)
    r = _renderer(torch.float32, dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=4)
    with torch.no_grad():
        (f,) = motion.query_ir_grid(feats, w, nb, counts=[M])
        ref_res = r.decode_residual_feature(f)
        ref = motion.deform(gs, ref_res, mask)
        motion.use_native_decoder(r)
        res = r.decode_residual_feature(f)
        out = motion.deform(gs, res, mask)
    assert list(res) == list(ref_res) and all(res[k].shape == ref_res[k].shape and res[k].dtype == ref_res[k].dtype for k in res)
    assert sorted(out) == sorted(ref)
    _, (e_xyz, e_rot) = _restated(r, f, False)
    u = 2.0 ** -24
    tol_xyz = 2 * torch.from_numpy(e_xyz).to(DEV) + 4 * u * out["xyz"][mask].abs().double()
    d_xyz = (out["xyz"][mask].double() - ref["xyz"][mask].double()).abs()
    rn = gs.rotation[mask].double().norm(dim=1, keepdim=True)
    dn = ref_res["rotation"].double().norm(dim=1, keepdim=True)
    tol_rot = rn * (2 * (2 * torch.from_numpy(e_rot).to(DEV)).norm(dim=1, keepdim=True) / dn + 16 * u)
    d_rot = (out["rotation"][mask].double() - ref["rotation"][mask].double()).abs()
    print("chain: worst xyz %.3g, rotation %.3g of the bound" % ((d_xyz / tol_xyz).max().item(), (d_rot / tol_rot).max().item()))
    assert (d_xyz <= tol_xyz).all() and (d_rot <= tol_rot).all()
    unm = torch.ones(P, dtype=torch.bool, device=DEV)
    unm[mask] = False
    assert torch.equal(out["xyz"][unm], gs.xyz[unm]) and torch.equal(out["rotation"][unm], gs.rotation[unm])
