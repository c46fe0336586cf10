"""CPU checks of tests/exchange_restatement.py, the float64 restatement the MI355X tests of the N > 1 colour exchange are held to
(tests/test_gpu_exchange_edges.py): the restatement against autograd, the derived bound against a float32 evaluation and against
three wrong variants, every GPU case against the branch its id names, the clamp cases' activity and the exclusion cap of the
colour-gradient scene.  No GPU is used."""
import numpy as np
import pytest
import torch

import exchange_restatement as X
from oracle import torch_oracle as TO

ALL_SH_CASES = X.GRAD_CASES + X.ADAM_CASES + X.EXCHANGE_CASES


def _steps_of(c):
    return range(1) if c in X.GRAD_CASES else range(X.STEPS)


def _ratio(got, ref, allow):
    """Largest |got - ref| / allow; where the allowance is an exact zero the result has to be an exact zero."""
    err = (got.double() - ref).abs()
    zero = allow == 0
    assert (err[zero] == 0).all()
    return float((err[~zero] / allow[~zero]).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("c", [X.GRAD_CASES[i] for i in (0, 2, 4, 5, 6, 8, 11)], ids=lambda c: c.id)
def test_rebuild_sh_is_the_autograd_gradient_of_the_colour_sum(c):
    """d/dsh of sum_v <g_v, sum_k b_k(dir_v) sh_k> (no clamp) in float64 = rebuild_sh(clamp = 0), to 1e-12 relative."""
    means, campos, gc = X.build_inputs(c)
    used = min((c.D + 1) ** 2, c.M)
    sh = torch.zeros((c.P, c.M, 3), dtype=torch.float64, requires_grad=True)
    loss = torch.zeros((), dtype=torch.float64)
    for v in range(c.V):
        d = means.double() - campos[v].double()
        b = TO.sh_basis(c.D, d / d.norm(dim=1, keepdim=True))[:, :used]
        colour = (b[:, :, None] * sh[:, :used]).sum(1)
        loss = loss + (gc[v].double() * colour).sum()
    (want,) = torch.autograd.grad(loss, sh)
    got = X.rebuild_sh(c.D, c.M, means, campos, gc, 0.0)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(want.abs().max()) > 0
    assert (got[:, used:] == 0).all() and not torch.signbit(got[:, used:]).any()


def test_the_bound_holds_for_a_float32_evaluation_of_every_gpu_case():
    worst = {}
    for c in ALL_SH_CASES:
        for step in _steps_of(c):
            means, campos, gc = X.build_inputs(c, step)
            ref = X.rebuild_sh(c.D, c.M, means, campos, gc, c.clamp)
            r = _ratio(X.rebuild_f32(c.D, c.M, means, campos, gc, c.clamp), ref, X.rebuild_allowance(c.D, c.M, means, campos, gc))
            worst[c.id] = max(worst.get(c.id, 0.0), r)
    print("float32 evaluation, worst |err| / allowance per case: " + ", ".join("%s %.3f" % kv for kv in worst.items()))
    print("worst of all: %.3f" % max(worst.values()))
    assert max(worst.values()) <= 1.0, worst
    assert max(worst.values()) > 0.01          # (a bound a hundred times too wide would have no teeth)


@pytest.mark.parametrize("variant", ["flip_c3", "unnormalised", "clamp_after_sum"])
def test_the_bound_rejects_a_wrong_evaluation(variant):
    cases = [c for c in X.GRAD_CASES if c.V > 0 and ((variant == "flip_c3" and c.D == 3 and c.M == 16)
                                                    or (variant == "unnormalised" and c.D > 0 and c.M > 1)
                                                    or (variant == "clamp_after_sum" and c.clamp > 0 and c.V > 1))]
    assert cases
    for c in cases:
        means, campos, gc = X.build_inputs(c)
        ref = X.rebuild_sh(c.D, c.M, means, campos, gc, c.clamp)
        allow = X.rebuild_allowance(c.D, c.M, means, campos, gc)
        err = (X.rebuild_f32(c.D, c.M, means, campos, gc, c.clamp, variant=variant).double() - ref).abs()
        nz = allow > 0
        r = float((err[nz] / allow[nz]).max())
        print("%s on %s: worst |err| / allowance %.3g" % (variant, c.id, r))
        assert r > 1.0, (variant, c.id, r)


def _features(c):
    """The branch names a case stands for, from the restated launch geometry (not from its id)."""
    f = set()
    used = (c.D + 1) ** 2
    if c.M and c.M < used:
        f.add("M_below")
    if c.M > used:
        f.add("M_above")
    if c.V in (0, 64):
        f.add("V%d" % c.V)
    if c in X.GRAD_CASES:
        f.add(X.branches(c.P, c.M, 0, 4 * c.off).store + "_store")
        return f
    if c in X.ADAM_CASES:
        b = X.branches(c.P, c.M, c.off, 0)
    else:
        off, _ = X.store_offsets(c.P) if c.layout == "store" else X.gap_offsets(c.P, c.M)
        b = X.branches(c.P, c.M, off["shs"], 0)
    f.add(b.sweep)
    if (3 * c.M) % 4 != 0:
        f.add("F_not_multiple_of_4")
    if b.second_half != "-":
        f.add({"none": "no_second_half", "partial": "partial_second_half", "more": "more"}[b.second_half])
    return f


NAMED = ("M_below", "M_above", "V0", "V64", "float4_store", "scalar_store", "vector", "scalar", "none", "F_not_multiple_of_4",
         "no_second_half", "partial_second_half", "more")


def test_every_case_lands_in_the_branch_its_id_names():
    seen = set()
    for c in ALL_SH_CASES:
        f = _features(c)
        tokens = c.id.split("-")
        for name in NAMED:          # whatever the id names is what the geometry gives
            if name in tokens:
                assert name in f, (c.id, name, f)
        kinds = ("float4_store", "scalar_store") if c in X.GRAD_CASES else ("vector", "scalar", "none")
        assert [t for t in tokens if t in kinds] == [k for k in kinds if k in f], (c.id, f)      # every id names its store / sweep
        seen |= f
    for need in ("scalar", "vector", "scalar_store", "float4_store", "no_second_half", "partial_second_half", "F_not_multiple_of_4",
                 "M_below", "M_above", "V0", "V64"):
        assert need in seen, need
    # the workgroup counts and last-workgroup sizes the ids rely on
    assert X.branches(129, 16, 0, 0)[:2] == (2, 1) and X.branches(128, 16, 0, 0)[:2] == (1, 128) and X.branches(1031, 16, 0, 0)[:2] == (9, 7)
    assert X.branches(143, 16, 0, 0).second_half == "partial" and X.branches(143, 16, 1, 0).sweep == "scalar"
    # the store's own layout: the SH span starts at 11 P floats, off the 16-byte grid unless P is a multiple of 4
    for P in (128, 129, 143, 1031):
        off, total = X.store_offsets(P)
        assert off["shs"] == 11 * P and total == 59 * P
        assert (X.branches(P, 16, off["shs"], 0).sweep == "vector") == (P % 4 == 0)
    off, total = X.gap_offsets(143, 16)
    spans = sorted((o, o + k * 143) for o, k in ((off["xyz"], 3), (off["rotation"], 4), (off["opacity"], 1), (off["scaling"], 3), (off["shs"], 48)))
    assert spans[0][0] >= 5 and all(b[0] - a[1] >= 5 for a, b in zip(spans, spans[1:])) and total - spans[-1][1] >= 5
    assert off["shs"] % 4 == 0


def test_the_clamp_cases_clamp_and_the_unseen_pattern_is_there():
    for c in ALL_SH_CASES:
        means, campos, gc = X.build_inputs(c)
        if c.V:
            assert (gc[:, 2::3] == 0).all()
            if c.P >= 2:
                assert (gc[0, 0] != 0).all()
        if c.V > 1 and c.P >= 5:
            assert (gc[1, 4] == 0).all() and (gc[0, 4] != 0).any()
        if c.clamp > 0 and c.M:
            ref = X.rebuild_sh(c.D, c.M, means, campos, gc, c.clamp)
            one = X.rebuild_sh(c.D, c.M, means, campos[:1], gc[:1], c.clamp)
            assert (one.abs() == c.clamp).any(), c.id                      # some per-view term sits at +-clamp
            free = X.rebuild_sh(c.D, c.M, means, campos, gc, 0.0)
            assert float((ref - free).abs().max()) > 1.0, c.id              # and the clamp changes the sum


def test_adam_allowance_covers_a_float32_gradient_and_equals_the_bars_without_one():
    """Float64 Adam fed the float32-evaluated gradients stays inside adam_allowance of float64 Adam on the float64 gradients; with
    check_adam's bars alone it would not on every element (the reason the propagated part exists) -- printed, not asserted."""
    from test_gpu_loss_optim_edges import ADAM_BARS
    c = X.ADAM_CASES[3]
    means, campos, _ = X.build_inputs(c)
    grads = [X.view_gradients(c, s) for s in range(X.STEPS)]
    n = c.P * c.M * 3
    p0, m0, v0 = X.build_state(c, n)
    R = X.sh_reference(c, means, campos, grads, p0, m0, v0)
    betas, eps = X.adam_constants()
    p, m, v = p0.double(), m0.double(), v0.double()
    for s, gc in enumerate(grads):
        g32 = X.rebuild_f32(c.D, c.M, means, campos, gc, c.clamp).reshape(-1).double()
        p, m, v = X.adam_formula(p, m, v, g32, X.LR_SH, X.T0 + 1 + s, betas, eps)
    for name, got, ref, allow in (("param", p, R["p"], R["allow_p"]), ("exp_avg", m, R["m"], R["allow_m"]), ("exp_avg_sq", v, R["v"], R["allow_v"])):
        r = _ratio(got, ref, allow)
        rtol, atol = ADAM_BARS[name]
        plain = rtol * ref.abs() + atol * (X.LR_SH if name == "param" else float(ref.abs().max()))
        assert (allow >= plain * (1.0 - 1e-9)).all() and torch.isfinite(allow).all()
        print("%s: worst |err| / allowance %.3g; the propagated part is at most %.3g x the plain bars" % (name, r, float(((allow - plain) / plain).max())))
        assert r <= 1.0


def test_the_colour_scene_meets_its_exclusion_cap_and_has_clamped_channels():
    """color_grad_out against the oracle may leave out channels whose float64 colour before the clamp is within 1e-5 of zero (the
    float32 decision may fall either way): at most 0.5 % of the channels of seen Gaussians, on the scene the GPU test uses."""
    from oracle import c_oracle as co
    from igs_amd.scenes import activate
    raw, cams, bg = X.color_scene()
    cam = cams[0]
    a = activate(raw)
    with co.thread_precision("float64"):
        f64 = lambda t: np.asarray(t.detach().cpu().numpy(), np.float64)
        nr, oo, st = co.rasterize_forward(f64(bg), f64(a["means3D"]), None, f64(a["opacities"]), f64(a["scales"]), f64(a["rotations"]), 1.0, None,
                                          f64(cam.world_view_transform), f64(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, 0.0,
                                          cam.height, cam.width, f64(a["shs"]), 3, f64(cam.camera_center))
        clamped = st.intermediates()["clamped"].astype(bool)
    seen = oo["radii"] > 0
    pre = X.preclamp_colors(raw, cam).numpy()
    near = (np.abs(pre) < X.NEAR_CLAMP) & seen[:, None]
    frac = near.sum() / max(3 * seen.sum(), 1)
    print("seen Gaussians %d of %d; clamped channels among them %d; within %g of the clamp %d (%.4f %%)"
          % (seen.sum(), seen.size, clamped[seen].sum(), X.NEAR_CLAMP, near.sum(), 100.0 * frac))
    assert seen.sum() > 1000 and (~seen).sum() > 10
    assert frac <= X.NEAR_CLAMP_CAP
    assert clamped[seen].sum() > 50
    assert (clamped[seen] == (pre[seen] < 0))[~near[seen]].all()          # the oracle's decision is the restated colour's sign
