"""The N > 1 colour exchange on the MI355X -- igs_sh_grad_from_view_colors, igs_adam_sh_from_view_colors, igs_adam_exchange_step (both
instances of sh_grad_views_kernel in igs_amd/csrc/sh_exchange.hip) and the two writers of igs_refine_step's `color_grad_out` -- at the
sizes, alignments and view counts where the kernels branch, against the float64 restatement of tests/exchange_restatement.py.

Every element is compared.  The allowances are derived, never measured: `rebuild_allowance` (K(V) 2^-24 sum_v B_k |g_v|, K(V) = 25 +
V - 1 from the kernel's operation count) for the rebuilt gradient, check_adam's bars plus that allowance carried through the update
for Adam, the every-element certificate at certify_grads' bars for `color_grad_out`.  tests/test_exchange_host.py asserts on the CPU
that the bound holds for a float32 evaluation, rejects three wrong variants, and that every case lands in the branch its id names.
Every output lies inside a larger allocation that holds a sentinel everywhere else and starts as NaN; the worst error-to-allowance
ratio of every comparison is printed (recorded in DESIGN.md section 6)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import exchange_restatement as X
from test_gpu_parity import dev  # noqa: F401

pytestmark = pytest.mark.gpu

BAND = 64
SENTINEL = 12345.0
E_INVALID = -1          # IGS_RAST_E_INVALID (include/igs_rast.h)
NAN = float("nan")


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Guard:
    """n floats starting `off` floats past a 16-byte boundary, BAND + off floats into an allocation that holds SENTINEL outside
    `spans` ([(offset, length)] within the n floats; default: all of them)."""

    def __init__(self, dev, n, off=0, spans=None, fill=NAN):
        self.big = torch.full((2 * BAND + off + n + 8,), SENTINEL, dtype=torch.float32, device=dev)
        assert self.big.data_ptr() % 16 == 0
        self.v = self.big[BAND + off: BAND + off + n]
        assert self.v.data_ptr() % 16 == (4 * off) % 16
        self.inside = torch.zeros(self.big.numel(), dtype=torch.bool, device=dev)
        for o, k in ([(0, n)] if spans is None else spans):
            self.inside[BAND + off + o: BAND + off + o + k] = True
            self.v[o:o + k] = fill

    def check(self, label):
        assert (self.big[~self.inside] == SENTINEL).all(), (label, "an element outside the output was written")


def _campos_arg(campos):
    if campos.shape[0] == 0:
        return None, None
    arr = (C.c_float * campos.numel())(*[float(x) for x in campos.reshape(-1).tolist()])       # host memory
    return arr, C.cast(arr, C.c_void_p)


def _worst(got, ref, allow, label):
    """Every element within its allowance; where the allowance is an exact zero the element is +0.0.  Prints and returns the worst ratio."""
    got = got.detach().cpu()
    assert not torch.isnan(got).any(), (label, "an element was not written")
    ref, allow = ref.reshape(got.shape), allow.reshape(got.shape)
    err = (got.double() - ref).abs()
    zero = allow == 0
    assert (_bits(got)[zero] == 0).all(), (label, "an exact +0.0 is expected where no view contributes")
    worst = float((err[~zero] / allow[~zero]).max()) if (~zero).any() else 0.0
    print("%s: max |err| %.3e, max |err| / allowance %.3f" % (label, float(err.max()) if err.numel() else 0.0, worst))
    assert worst <= 1.0, (label, worst)
    return worst


def _sh_grad(dev, c, means, campos, gc, off=None, clamp=None):
    """igs_sh_grad_from_view_colors into a guarded NaN buffer; returns the [P, M, 3] result on the CPU."""
    out = Guard(dev, c.P * c.M * 3, c.off if off is None else off)
    md, gd = means.to(dev), gc.to(dev).contiguous()
    keep, cp = _campos_arg(campos)
    rc = _lib().igs_sh_grad_from_view_colors(_stream(dev), c.P, c.D, c.M, c.V, md.data_ptr(), cp, gd.data_ptr() if c.V else None,
                                             c.clamp if clamp is None else clamp, out.v.data_ptr())
    assert rc == 0
    torch.cuda.synchronize(dev)
    out.check(c.id)
    return out.v.cpu().view(c.P, c.M, 3)


# ---------------------------------------------------------------- igs_sh_grad_from_view_colors
@pytest.mark.parametrize("c", X.GRAD_CASES, ids=lambda c: c.id)
def test_rebuilt_gradient_against_float64(dev, c):
    """Sizes around the 128-Gaussian workgroup, every (D, M) class, 0 / 1 / 3 / 64 views, the clamp, both store paths."""
    means, campos, gc = X.build_inputs(c)
    got = _sh_grad(dev, c, means, campos, gc)
    ref = X.rebuild_sh(c.D, c.M, means, campos, gc, c.clamp)
    _worst(got, ref, X.rebuild_allowance(c.D, c.M, means, campos, gc), "dL_dsh " + c.id)
    used = min((c.D + 1) ** 2, c.M)
    assert (_bits(got[:, used:]) == 0).all()                       # rows beyond the active degree: +0.0
    assert (_bits(got[2::3]) == 0).all()                           # Gaussians no view sees: +0.0
    if c.V == 0:
        assert (_bits(got) == 0).all()
    if c.clamp > 0:
        assert float(got.abs().max()) <= c.V * c.clamp and (ref.abs() >= c.clamp).any()


def test_a_negative_zero_colour_gradient_counts_as_unseen(dev):
    c = X.GRAD_CASES[8]
    means, campos, gc = X.build_inputs(c)
    plus = gc.clone()
    plus[:, 7] = 0.0
    plus[0, 9] = 0.0
    minus = plus.clone()
    minus[:, 7] = -0.0
    minus[0, 9] = -0.0
    assert torch.signbit(minus[:, 7]).all()
    a, b = _sh_grad(dev, c, means, campos, plus), _sh_grad(dev, c, means, campos, minus)
    assert (_bits(b[7]) == 0).all() and torch.equal(_bits(a), _bits(b))
    assert float(b[9].abs().max()) > 0


@pytest.mark.parametrize("clamp", [0.0, 15.0])
def test_a_nan_colour_gradient_stays_in_its_gaussian(dev, clamp):
    """One Gaussian's colour gradient is NaN in one view: its rows are NaN (through the clamp too, as through torch.clamp) and no
    other bit changes."""
    c = X.GRAD_CASES[12 if clamp else 8]
    assert c.clamp == clamp and c.D == 3 and c.M == 16
    means, campos, gc = X.build_inputs(c)
    g = 130
    assert g % 3 != 2
    bad = gc.clone()
    bad[1, g] = NAN
    a, b = _sh_grad(dev, c, means, campos, gc), _sh_grad(dev, c, means, campos, bad)
    assert torch.isnan(b[g]).all()
    others = torch.arange(c.P) != g
    assert torch.equal(_bits(a[others]), _bits(b[others])) and not torch.isnan(a).any()


# ---------------------------------------------------------------- igs_adam_sh_from_view_colors
def _bias(t):
    betas, _ = X.adam_constants()
    return 1.0 - betas[0] ** t, math.sqrt(1.0 - betas[1] ** t)


def _run_sh_adam(dev, c, off):
    """Three steps with fresh colour gradients and carried moments.  Returns (p, m, v) on the CPU and the reference."""
    L = _lib()
    betas, eps = X.adam_constants()
    means, campos, _ = X.build_inputs(c)
    grads = [X.view_gradients(c, s) for s in range(X.STEPS)]
    n = c.P * c.M * 3
    p0, m0, v0 = X.build_state(c, n)
    bufs = [Guard(dev, n, off) for _ in range(3)]
    for b, src in zip(bufs, (p0, m0, v0)):
        b.v.copy_(src)
    md = means.to(dev)
    keep, cp = _campos_arg(campos)
    for s, gc in enumerate(grads):
        gd = gc.to(dev).contiguous()
        rc = L.igs_adam_sh_from_view_colors(_stream(dev), c.P, c.D, c.M, c.V, md.data_ptr(), cp, gd.data_ptr() if c.V else None, c.clamp,
                                            bufs[0].v.data_ptr(), bufs[1].v.data_ptr(), bufs[2].v.data_ptr(), X.LR_SH, betas[0], betas[1], eps,
                                            *_bias(X.T0 + 1 + s))
        assert rc == 0
        torch.cuda.synchronize(dev)
    for b in bufs:
        b.check(c.id)
    return [b.v.cpu() for b in bufs], X.sh_reference(c, means, campos, grads, p0, m0, v0)


def _check_sh_adam(got, R, label):
    return [_worst(got[0], R["p"], R["allow_p"], label + " param"), _worst(got[1], R["m"], R["allow_m"], label + " exp_avg"),
            _worst(got[2], R["v"], R["allow_v"], label + " exp_avg_sq")]


@pytest.mark.parametrize("c", X.ADAM_CASES, ids=lambda c: c.id)
def test_sh_adam_three_steps_against_float64(dev, c):
    """The vector sweep with and without a second half, the scalar sweep (spans 4 bytes off; F = 3, 27), V = 0 (a zero gradient still
    decays the moments and moves the parameter as torch's Adam does) and V = 64."""
    got, R = _run_sh_adam(dev, c, c.off)
    _check_sh_adam(got, R, c.id)
    if c.V == 0:
        assert float((got[0].double() - X.build_state(c, got[0].numel())[0].double()).abs().max()) > 1e-4      # the parameters moved


def test_vector_and_scalar_sweep_agree(dev):
    """Same values, SH spans 16-byte aligned and 4 bytes off: within one float32 ulp of each other, each within its allowance."""
    c = X.ADAM_CASES[0]
    a, R = _run_sh_adam(dev, c, 0)
    b, _ = _run_sh_adam(dev, c, 1)
    _check_sh_adam(a, R, "aligned")
    _check_sh_adam(b, R, "4 bytes off")
    for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
        x, y = x.numpy(), y.numpy()
        ulp = np.spacing(np.maximum(np.abs(x), np.abs(y)))
        d = np.abs(x.astype(np.float64) - y.astype(np.float64)) / ulp
        print("%s: vector against scalar sweep, worst difference %.2f ulp, %d of %d elements differ" % (name, d.max(), (d > 0).sum(), d.size))
        assert d.max() <= 1.0, name


# ---------------------------------------------------------------- igs_adam_exchange_step
@pytest.mark.parametrize("c", X.EXCHANGE_CASES, ids=lambda c: c.id)
def test_exchange_step_three_steps_against_float64(dev, c):
    """The rank's whole optimiser step in one launch, in the store's own layout (SH span at 11 P floats: off the 16-byte grid unless
    P is a multiple of 4) and in a layout with gaps: SH part against the float64 restatement, the four small groups against float64
    Adam at check_adam's bars, nothing else written.  lr_xyz = 1.0: the directions of a step are those of the positions it was
    launched with.  M = 0 leaves the SH spans alone."""
    from igs_amd.refine import GaussianParams
    from test_gpu_loss_optim_edges import check_adam
    L = _lib()
    betas, eps = X.adam_constants()
    P = c.P
    off, total = X.store_offsets(P) if c.layout == "store" else X.gap_offsets(P, c.M)
    if c.layout == "store":
        z = torch.zeros
        p = GaussianParams(dict(xyz=z(P, 3), rotation=z(P, 4), opacity=z(P, 1), scaling=z(P, 3), shs=z(P, 16, 3)), dev)
        assert {k: v[0] for k, v in p.spans.items()} == off and p.flat.numel() == total
    nsh = (16 if c.layout == "store" else c.M) * 3 * P          # the span the layout reserves; M = 0 uses none of it
    spans = [(off[n], k * P) for n, k in X.SMALL] + [(off["shs"], nsh)]
    means0, campos, _ = X.build_inputs(c)
    grads = [X.view_gradients(c, s) for s in range(X.STEPS)]
    state = {n: X.build_state(c, k * P, seed_add=i + 1) for i, (n, k) in enumerate(X.SMALL)}
    state["xyz"] = (means0.reshape(-1),) + state["xyz"][1:]
    state["shs"] = X.build_state(c, nsh)
    bufs = [Guard(dev, total, 0, spans) for _ in range(3)]
    for n, st in state.items():
        for b, src in zip(bufs, st):
            b.v[off[n]: off[n] + src.numel()] = src.to(dev)
    before = [b.big.clone() for b in bufs]
    grad = torch.full((total,), NAN, device=dev)              # (the SH span and the gaps of the gradient buffer are never read)
    small = [{n: X.small_gradients(c, k * P, s) for n, k in X.SMALL} for s in range(X.STEPS)]
    keep, cp = _campos_arg(campos)
    means_at = []
    for s, gc in enumerate(grads):
        means_at.append(bufs[0].v[off["xyz"]: off["xyz"] + 3 * P].cpu().view(P, 3).clone())
        for n, k in X.SMALL:
            grad[off[n]: off[n] + k * P] = small[s][n].to(dev)
        gd = gc.to(dev).contiguous()
        rc = L.igs_adam_exchange_step(_stream(dev), P, c.D, c.M, c.V, cp, gd.data_ptr() if c.V else None, c.clamp, bufs[0].v.data_ptr(),
                                      bufs[1].v.data_ptr(), bufs[2].v.data_ptr(), grad.data_ptr(), off["xyz"], off["rotation"], off["shs"],
                                      off["opacity"], off["scaling"], X.LRS["xyz"], X.LRS["rotation"], X.LRS["shs"], X.LRS["opacity"],
                                      X.LRS["scaling"], betas[0], betas[1], eps, *_bias(X.T0 + 1 + s))
        assert rc == 0
        torch.cuda.synchronize(dev)
    for b in bufs:
        b.check(c.id)                                           # bands and the floats between the groups
    assert float((means_at[1] - means_at[0]).abs().max()) > 0.1          # the positions do move by about lr_xyz = 1 per step
    for n, k in X.SMALL:
        sl = slice(off[n], off[n] + k * P)
        rp, rst = X.adam_reference(*state[n], X.T0, [small[s][n] for s in range(X.STEPS)], X.LRS[n])
        check_adam(bufs[0].v[sl], bufs[1].v[sl], bufs[2].v[sl], rp, rst, X.LRS[n], (c.id, n))
    sl = slice(off["shs"], off["shs"] + nsh)
    if c.M == 0:
        for b, b0 in zip(bufs, before):
            assert torch.equal(_bits(b.v[sl]), _bits(b0[BAND: BAND + total][sl])), "M = 0 must leave the SH spans alone"
        return
    R = X.sh_reference(c, means_at, campos, grads, *state["shs"])
    _check_sh_adam([b.v[sl].cpu() for b in bufs], R, c.id)


# ---------------------------------------------------------------- color_grad_out: two writers, and the oracle
@functools.lru_cache(maxsize=None)
def _colour_runs(dn):
    """A gradients-only fused step on the small scene, twice: color_grad_out written by the per-Gaussian kernel (no event) and by the
    early extraction kernel (color_ready_event given)."""
    from igs_amd.refine import GaussianParams, Refiner, render
    from igs_amd.scenes import activate, perturbed_copy
    dev = torch.device("cuda:0")
    raw, cams_cpu, bg_cpu = X.color_scene()
    cam, bg = cams_cpu[0].to(dev), bg_cpu.to(dev)
    gt_raw = {k: v.to(dev) for k, v in perturbed_copy(raw).items()}
    with torch.no_grad():
        gt = render(activate(gt_raw), cam, bg)["images_pred"].clone()
    pa = GaussianParams(raw, dev)
    r = Refiner(pa, [cam], [gt], bg, loss="l1", lambda_depth_normal=0.05 if dn else 0.0, fused=True)
    P = pa.P
    late, early = Guard(dev, 3 * P), Guard(dev, 3 * P)
    pk = r._fused_step(cam, gt, grads_only=True, color_out=late.v)
    torch.cuda.synchronize(dev)
    color, radii = pk["images_pred"].cpu().numpy().copy(), pk["radii"].cpu().numpy().copy()
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))               # (creates the hipEvent_t the library records)
    r._fused_step(cam, gt, grads_only=True, color_out=early.v, color_event=ev)
    torch.cuda.synchronize(dev)
    late.check("late writer")
    early.check("early writer")
    from igs_amd import rasterizer as R
    return dict(raw=raw, cam=cams_cpu[0], bg=bg_cpu, gt=gt.cpu().numpy(), color=color, radii=radii, late=late.v.cpu().view(P, 3),
                early=early.v.cpu().view(P, 3), instance=R.last_backward_instance())


@pytest.mark.parametrize("mode", ["colour_l1", "depth_normal"])
def test_both_writers_of_color_grad_out_return_the_same_bits(dev, mode):
    """The accumulator rows are read at the compact stride (colour-only instance) and at the full stride (depth-normal regulariser)."""
    run = _colour_runs(mode == "depth_normal")
    assert run["instance"]["depth"] == (mode == "depth_normal")
    assert not torch.isnan(run["late"]).any() and not torch.isnan(run["early"]).any()
    assert torch.equal(_bits(run["late"]), _bits(run["early"]))
    assert float(run["late"].abs().max()) > 0


@pytest.mark.parametrize("mode", ["colour_l1", "depth_normal"])
def test_color_grad_out_against_the_oracle(dev, mode):
    """color_grad_out = the oracle's float64 dL/dcolour of the same step (upstream gradient sign(colour - gt) / (3 H W) from the image
    the step rendered; colour does not depend on the regulariser's depth / normal gradients), channels the SH evaluation clamped and
    Gaussians the view does not see zeroed -- those exact +0.0 -- under the every-element certificate at certify_grads' bars.  Left
    out: channels whose float64 colour before the clamp is within 1e-5 of zero (test_exchange_host.py caps them at 0.5 %)."""
    import certificate as cert
    from igs_amd.scenes import activate
    run = _colour_runs(mode == "depth_normal")
    raw, cam = run["raw"], run["cam"]
    H, W = cam.height, cam.width
    g = {k: None for k in cert.KEYS}
    g["color"] = (np.sign(run["color"] - run["gt"]) / (3.0 * H * W)).astype(np.float32)
    ob = cert.oracle_all(activate(raw), cam, run["bg"], g, samples=12, exp_samples=2)
    seen = ob["out"]["radii"] > 0
    assert ((run["radii"] > 0) == seen).all()
    clamped = ob["state"].intermediates()["clamped"].astype(bool)
    near = (np.abs(X.preclamp_colors(raw, cam).numpy()) < X.NEAR_CLAMP) & seen[:, None]
    assert near.sum() <= X.NEAR_CLAMP_CAP * 3 * seen.sum()
    zero = (clamped | ~seen[:, None]) & ~near
    A = run["late"].numpy().copy()
    assert (A.view(np.int32)[zero] == 0).all(), "unseen rows and clamped channels are exact +0.0"
    assert (A[~zero & ~near] != 0).mean() > 0.9

    def masked(G):
        G = np.array(G, dtype=np.float64).reshape(-1, 3)
        G[clamped | ~seen[:, None]] = 0.0
        return G
    G32, G64 = masked(ob["g32"]["colors"]), masked(ob["g64"]["colors"])
    A[near] = G64[near]
    empty = np.zeros((0,))
    ob_c = dict(g32={n: (G32 if n == "colors" else empty) for n in cert.GNAMES}, g64={n: (G64 if n == "colors" else empty) for n in cert.GNAMES},
                shift={"colors": ob["shift"]["colors"]})
    gout = [A if n == "colors" else empty for n in cert.GNAMES]
    st = cert.certify(gout, ob_c, "color_grad_out, %s" % mode, max_allowance_frac=0.05, oracle_factor=2.0, allowance_floor=50)
    assert st["colors"][0] == A.size
    rel = np.abs(A - G64)[~zero] / (cert.REL * np.abs(G64[~zero]) + cert.FLOOR * np.abs(G64).max())
    print("color_grad_out %s: worst |err| / (1e-3 |f64| + 1e-5 max|f64|) %.4f; %d channels left out near the clamp" % (mode, rel.max(), near.sum()))


# ---------------------------------------------------------------- refusals
def test_sizes_outside_the_contract_are_refused_before_any_launch(dev):
    L = _lib()
    betas, eps = X.adam_constants()
    buf = torch.full((4096,), NAN, device=dev)
    gd = torch.zeros((4096,), device=dev)
    arr = (C.c_float * 195)(*([1.0] * 195))
    cp = C.cast(arr, C.c_void_p)
    st = _stream(dev)

    def calls(P, D, M, V, null=False):
        b, g_, c_ = (None, None, None) if null else (buf.data_ptr(), gd.data_ptr(), cp)
        return (L.igs_sh_grad_from_view_colors(st, P, D, M, V, g_, c_, g_, 0.0, b),
                L.igs_adam_sh_from_view_colors(st, P, D, M, V, g_, c_, g_, 0.0, b, b, b, 1e-3, betas[0], betas[1], eps, 0.1, 0.03),
                L.igs_adam_exchange_step(st, P, D, M, V, c_, g_, 0.0, b, b, b, g_, 0, 6, 30, 14, 16, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3, betas[0], betas[1],
                                         eps, 0.1, 0.03))
    for P, D, M, V in ((2, 4, 16, 1), (2, 3, 17, 1), (2, 3, 16, 65), (-1, 3, 16, 1), (2, -1, 16, 1), (2, 3, -1, 1), (2, 3, 16, -1)):
        assert calls(P, D, M, V) == (E_INVALID,) * 3, (P, D, M, V)
    assert calls(0, 3, 16, 3, null=True) == (0, 0, 0)
    torch.cuda.synchronize(dev)
    assert torch.isnan(buf).all()
