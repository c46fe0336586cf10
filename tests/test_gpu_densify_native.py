"""The native densify-and-prune plan on the GPU (densify.hip: igs_densify_plan through igs_amd.densify.plan_native): the decision
against the PyTorch plan and the float64 restatement of tests/densify_plan_restatement.py, the children against the restatement
with the test's own normals, every branch of the selection, the whole event on a GaussianParams store and the refine loop."""
import math

import numpy as np
import pytest
import torch

import densify_plan_restatement as DR
from igs_amd import densify as dn
from igs_amd.scenes import cfg1_scene, activate

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # largest relative error of one float32 rounding


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Stats:
    """grad_accum / denom of a DensifyState without the object (CPU tensors)."""

    def __init__(self, grad_accum, denom):
        self.grad_accum, self.denom = grad_accum, denom


def _cfg(max_num=10 ** 7, world=True, **kw):
    # split limit 0.05 * 2 = 0.1, world limit 0.1 * 2 = 0.2 (a child of a Gaussian with a scale above 0.32 is pruned for its size)
    return dn.DensifyConfig(grad_threshold=1.5e-4, min_opacity=0.005, max_num=max_num, percent_dense=0.05, extent=2.0,
                            max_screen_size=20 if world else None, **kw)


def _inputs(P, seed, cfg, grads=None):
    """Raw leaves (quaternions NOT normalised, |xyz_c| in [1, 3], scales log-uniform in [0.005, 0.4]), statistics with denom in
    {0, 1, 2} -- x/0 and, on every fifth of those rows, 0/0 -- or the given gradients over denom = 1, and normals; all moved off the
    thresholds by with_margin, and asserted to classify identically in float64 and float32."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(P, 3, generator=g) < 0.5, -1.0, 1.0)
    t = dict(xyz=(1.0 + 2.0 * torch.rand(P, 3, generator=g)) * sign,
             rotation=torch.randn(P, 4, generator=g) * (0.1 + 3.0 * torch.rand(P, 1, generator=g)),
             opacity=torch.randn(P, 1, generator=g) * 3.0,
             scaling=math.log(0.005) + torch.rand(P, 3, generator=g) * (math.log(0.4) - math.log(0.005)))
    if grads is None:
        accum = torch.rand(P, generator=g) * 6e-4
        denom = torch.randint(0, 3, (P,), generator=g).float()
        accum[(denom == 0) & (torch.arange(P) % 5 == 0)] = 0.0
    else:
        accum, denom = grads.clone().float(), torch.ones(P)
    normals = torch.randn(P, 2, 3, generator=g)
    t, accum = DR.with_margin(t, accum, denom, cfg)
    assert DR.classes_agree(t, accum, denom, cfg)
    return t, Stats(accum, denom), normals


def _distinct_grads(P, seed, n_cand):
    """P distinct gradients, n_cand of them at or above the threshold 1.5e-4, in random order."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.cat([torch.linspace(2e-4, 9e-4, n_cand), torch.linspace(1e-6, 1e-4, P - n_cand)])
    assert vals.unique().numel() == P
    return vals[torch.randperm(P, generator=g)]


def _native(dev, t, S, cfg, normals):
    st = dn.DensifyState(t["xyz"].shape[0], dev)
    st.grad_accum.copy_(S.grad_accum)
    st.denom.copy_(S.denom)
    d = {k: v.to(dev) for k, v in t.items()}
    pl = dn.plan_native(d["xyz"], d["rotation"], d["opacity"], d["scaling"], st, cfg, normals=normals.to(dev))
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in pl.items()}, st, d


def _torch_plan(dev, d, st, cfg):
    pl = dn.plan(d["xyz"], d["rotation"], d["opacity"], d["scaling"], st, cfg, torch.Generator(device=dev).manual_seed(5))
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in pl.items()}


def _same_decision(a, b):
    for k in ("src", "fresh", "ovr"):
        assert a[k].dtype == np.int32 and np.array_equal(a[k], b[k]), k
    for k in ("n_clone", "n_split", "n_pruned"):
        assert a[k] == b[k], (k, a[k], b[k])


def _child_bounds(t, re_):
    """Error bounds of the children against the float64 restatement, from the kernel's operation chain (u = 2^-24):
      position  p_c = sum_j R_cj v_j + xyz_c,  v_j = z_j * expf(ls_j):  expf 1 ulp = 2u, the product u -> v_j relative 3u; each R_cj v_j
        product u; the three additions u each on partial sums bounded by |xyz_c| + sum_j |R_cj| |v_j| =: m_c -> 7u m_c.  R itself:
        q / |q| relative 2.5u per component (four squares, three additions, sqrt, division), a product of two 5.5u, so an entry
        2 (a b +- c d) or 1 - 2 (a^2 + b^2) carries an ABSOLUTE error of at most 12u (|a b| + |c d| <= 1/2) -> 12u sum_j |v_j|.
        The test's inputs keep sum_j |v_j| <= 4 m_c (|xyz_c| >= 1, scales <= 0.4; asserted), so the total is below
        (7 + 48) u m_c, held to 64 u m_c.  A contracted multiply-add only removes roundings.
      log-scale  logf(expf(ls) / 1.6f): the argument is relative 2u (expf) + u (division) + 0.25u (1.6f against 1.6) = 3.25u, which
        is its absolute effect on the logarithm, plus logf's 1 ulp = 2u |value| -> held to 8u max(1, |value|)."""
    R, v = re_["child_R"], re_["child_v"]
    m = np.abs(t["xyz"].double().numpy()[re_["child_src"]]) + (np.abs(R) * np.abs(v)[:, None, :]).sum(axis=2)
    assert (np.abs(v).sum(axis=1, keepdims=True) <= 4.0 * m).all()
    return 64.0 * U * m, 8.0 * U * np.maximum(1.0, np.abs(re_["ovr_scale"]))


def _plan_lines_float32(t, normals, idx_split):
    """The float32 lines of densify.plan that make the children, on the CPU, with torch.normal(0, std) written as z * std."""
    idx = torch.from_numpy(idx_split).long()
    scaling = torch.exp(t["scaling"])
    stds = scaling[idx].repeat(2, 1)
    samples = torch.cat([normals[idx, 0], normals[idx, 1]]) * stds
    rots = dn.build_rotation(t["rotation"][idx]).repeat(2, 1, 1)
    ovr_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][idx].repeat(2, 1)
    ovr_scale = torch.log(scaling[idx].repeat(2, 1) / (0.8 * 2))
    return ovr_xyz.double().numpy(), ovr_scale.double().numpy()


def _check(dev, t, S, cfg, normals, against_plan=True):
    """plan_native == the restatement (== densify.plan) in the decision; the children inside their bounds.  Returns the native plan."""
    pn, st, d = _native(dev, t, S, cfg, normals)
    re_ = DR.restate_cfg(t, S, cfg, normals)
    _same_decision(pn, re_)
    # (densify.plan with the world-size prune on indexes an empty ovr_scale when nothing splits -- an IndexError on the CPU, an
    #  out-of-range gather on the GPU -- so that one combination is held to the restatement alone)
    if against_plan and not (cfg.max_screen_size and re_["n_split"] == 0):
        _same_decision(pn, _torch_plan(dev, d, st, cfg))
    n_s = pn["n_split"]
    assert pn["ovr_xyz"].shape == (2 * n_s, 3) and pn["ovr_scale"].shape == (2 * n_s, 3)
    assert pn["src"].size == t["xyz"].shape[0] + pn["n_clone"] + n_s - pn["n_pruned"]
    if n_s:
        bx, bs = _child_bounds(t, re_)
        assert (np.abs(pn["ovr_xyz"] - re_["ovr_xyz"]) <= bx).all(), float((np.abs(pn["ovr_xyz"] - re_["ovr_xyz"]) / bx).max())
        assert (np.abs(pn["ovr_scale"] - re_["ovr_scale"]) <= bs).all(), float((np.abs(pn["ovr_scale"] - re_["ovr_scale"]) / bs).max())
        px, ps = _plan_lines_float32(t, normals, re_["child_src"][:n_s])
        assert (np.abs(px - re_["ovr_xyz"]) <= bx).all() and (np.abs(ps - re_["ovr_scale"]) <= bs).all()
    return pn


# ---------------------------------------------------------------- the decision against plan and the restatement
@pytest.mark.parametrize("world", [True, False])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 4000, 70000])
def test_decision_and_children(dev, P, world):
    """One thread, the block edges, several blocks, and more blocks (274) than one wave of the scan block has lanes; x/0 and 0/0 rows,
    quaternions that are not normalised, the world-size prune on and off."""
    cfg = _cfg(world=world)
    t, S, normals = _inputs(P, 100 + P, cfg)
    pn = _check(dev, t, S, cfg, normals)
    if P >= 255:
        assert pn["n_clone"] > 0 and pn["n_split"] > 0 and pn["n_pruned"] > 0
        g = DR.gradient(S.grad_accum, S.denom)
        assert np.isinf(g).any() and ((S.denom == 0) & (S.grad_accum == 0)).any()
        assert int((pn["ovr"] >= 0).sum()) < 2 * pn["n_split"] if world else True          # some children go for their size


def test_single_gaussian_classes(dev):
    """P = 1 in each class: kept, pruned, cloned, split."""
    cfg = _cfg(world=False)
    for accum, ls, opa, want in ((0.0, -4.0, 0.0, (1, 0, 0, 0)), (0.0, -4.0, -9.0, (0, 0, 0, 1)), (1.0, -4.0, 0.0, (2, 1, 0, 0)),
                                 (1.0, -1.0, 0.0, (2, 0, 1, 0)), (1.0, -1.0, -9.0, (0, 0, 1, 2))):
        t = dict(xyz=torch.tensor([[1.0, -2.0, 1.5]]), rotation=torch.tensor([[0.3, -1.0, 2.0, 0.5]]), opacity=torch.tensor([[opa]]),
                 scaling=torch.full((1, 3), ls))
        S = Stats(torch.tensor([accum]), torch.tensor([1.0]))
        pn = _check(dev, t, S, cfg, torch.tensor([[[0.5, -1.0, 0.25], [-0.5, 1.5, 2.0]]]))
        assert (pn["src"].size, pn["n_clone"], pn["n_split"], pn["n_pruned"]) == want


# ---------------------------------------------------------------- branches
def test_no_candidate_prunes_only(dev):
    cfg = _cfg(world=True)
    t, S, normals = _inputs(1000, 7, cfg)
    S.grad_accum.zero_()
    pn = _check(dev, t, S, cfg, normals)
    assert pn["n_clone"] == 0 and pn["n_split"] == 0 and 0 < pn["n_pruned"] == 1000 - pn["src"].size
    assert not pn["fresh"].any() and (pn["ovr"] == -1).all() and (np.diff(pn["src"]) > 0).all()


def test_every_gaussian_a_candidate(dev):
    cfg = _cfg(world=False)
    t, S, normals = _inputs(1000, 8, cfg, grads=torch.linspace(2e-4, 9e-4, 1000))
    pn = _check(dev, t, S, cfg, normals)
    assert pn["n_clone"] + pn["n_split"] == 1000 and pn["n_clone"] > 0 and pn["n_split"] > 0


def test_everything_pruned_leaves_an_empty_store(dev):
    from igs_amd.refine import GaussianParams
    cfg = _cfg(world=False)
    t, S, normals = _inputs(600, 9, cfg)
    t["opacity"].fill_(-20.0)
    pn = _check(dev, t, S, cfg, normals)
    assert pn["src"].size == 0 and pn["n_pruned"] == 600 + pn["n_clone"] + pn["n_split"] and pn["n_split"] > 0
    raw, _, _ = cfg1_scene(P=600, size=32)
    raw["opacity"].fill_(-20.0)
    params = GaussianParams(raw, dev)
    st = dn.DensifyState(600, dev)
    st.grad_accum.copy_(S.grad_accum)
    st.denom.copy_(S.denom)
    pl = dn.densify_and_prune(params, st, _cfg(world=False, native=True), torch.Generator(device=dev).manual_seed(2))
    torch.cuda.synchronize()
    assert pl["src"].numel() == 0 and params.P == 0 and params.flat.numel() == 0 and st.denom.numel() == 0


N_CAND = 300


@pytest.mark.parametrize("add", [-5, 0, N_CAND - 1, N_CAND, N_CAND + 1, 37])
def test_max_points_bound_with_distinct_gradients(dev, add):
    """max_num_add negative, 0, one below / at / one above the candidate count, and well inside: equality with plan and the restatement."""
    P = 3000
    cfg = _cfg(max_num=P + add, world=True)
    t, S, normals = _inputs(P, 11, cfg, grads=_distinct_grads(P, 12, N_CAND))
    assert int((DR.gradient(S.grad_accum, S.denom) >= cfg.grad_threshold).sum()) == N_CAND
    pn = _check(dev, t, S, cfg, normals)
    assert pn["n_clone"] + pn["n_split"] == (N_CAND if add >= N_CAND else max(add, 0))


def test_control_max_off_ignores_the_bound(dev):
    P = 3000
    cfg = _cfg(max_num=P + 10, world=False, control_max=False)
    t, S, normals = _inputs(P, 11, cfg, grads=_distinct_grads(P, 12, N_CAND))
    pn = _check(dev, t, S, cfg, normals)
    assert pn["n_clone"] + pn["n_split"] == N_CAND


@pytest.mark.parametrize("tie", ["finite", "inf"])
def test_equal_gradients_at_the_cut_go_to_the_lowest_index(dev, tie):
    """40 candidates above a block of 100 equal gradients spread over several blocks of the grid, 100 candidates below it; 70 may be
    added: the 40, then the 30 equal ones with the lowest indices.  (torch.topk leaves this choice open, so plan is not compared.)"""
    P = 3000
    g = torch.Generator().manual_seed(21)
    perm = torch.randperm(P, generator=g)
    grads = torch.linspace(1e-6, 1e-4, P)
    top, eq, low = perm[:40], perm[40:140], perm[140:240]
    if tie == "finite":
        grads[top] = torch.linspace(6e-4, 9e-4, 40)
        grads[eq] = 5e-4
    grads[low] = torch.linspace(2e-4, 4e-4, 100)
    cfg = _cfg(max_num=P + 70, world=False)
    t, S, normals = _inputs(P, 22, cfg, grads=grads)
    if tie == "inf":                      # the equal block is x/0 = +inf and lies ABOVE everything else: the 70 lowest-index ones stay
        S.denom[eq] = 0.0
        S.grad_accum[eq] = 1e-4
        assert DR.classes_agree(t, S.grad_accum, S.denom, cfg)
    pn = _check(dev, t, S, cfg, normals, against_plan=False)
    eq_sorted = np.sort(eq.numpy())
    want = np.sort(np.concatenate([top.numpy(), eq_sorted[:30]])) if tie == "finite" else eq_sorted[:70]
    gv = DR.gradient(S.grad_accum, S.denom)
    got = np.nonzero(DR.select(gv, cfg.grad_threshold, 70, True))[0]
    assert np.array_equal(got, want)              # the restatement, which _check held the kernel's rows equal to, follows the rule
    assert pn["n_clone"] + pn["n_split"] == 70
    assert len(set((eq_sorted // 256).tolist())) > 4


def test_two_calls_give_identical_bits(dev):
    cfg = _cfg(max_num=20000 + 500, world=True)
    t, S, normals = _inputs(20000, 31, cfg)
    a = _check(dev, t, S, cfg, normals, against_plan=False)      # (the cut lies among the +inf gradients: plan's choice there is torch's)
    b, _, _ = _native(dev, t, S, cfg, normals)
    assert a["n_split"] > 0 and a["n_clone"] + a["n_split"] == 500
    for k in ("src", "fresh", "ovr", "ovr_xyz", "ovr_scale"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["n_clone"], a["n_split"], a["n_pruned"]) == (b["n_clone"], b["n_split"], b["n_pruned"])


def test_draws_its_own_normals_and_refuses_other_dtypes(dev):
    cfg = _cfg(world=False)
    t, S, normals = _inputs(2000, 41, cfg)
    st = dn.DensifyState(2000, dev)
    st.grad_accum.copy_(S.grad_accum)
    st.denom.copy_(S.denom)
    d = {k: v.to(dev) for k, v in t.items()}
    pl = dn.plan_native(d["xyz"], d["rotation"], d["opacity"], d["scaling"], st, cfg, torch.Generator(device=dev).manual_seed(3))
    z = torch.randn((2000, 2, 3), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    got = {k: (v.cpu().numpy().copy() if torch.is_tensor(v) else v) for k, v in pl.items()}
    assert st.plan_bufs is not None and st.plan_bufs.P == 2000
    re_ = DR.restate_cfg(t, S, cfg, z.cpu())
    _same_decision(got, re_)
    bx, bs = _child_bounds(t, re_)
    assert (np.abs(got["ovr_xyz"] - re_["ovr_xyz"]) <= bx).all() and (np.abs(got["ovr_scale"] - re_["ovr_scale"]) <= bs).all()
    with pytest.raises(NotImplementedError):
        dn.plan_native(d["xyz"].double(), d["rotation"], d["opacity"], d["scaling"], st, cfg)


# ---------------------------------------------------------------- the whole event and the refine loop
@pytest.mark.parametrize("max_num", [150000, 4300])
def test_event_on_a_store_with_moments(dev, max_num):
    """densify_and_prune with the native plan on the store of test_densify_and_prune_matches_reference_style_surgery: every row of
    the new store is bitwise its source row in parameters and moments, fresh rows have zero moments, children carry ovr_xyz /
    ovr_scale, the statistics are reset to the new size."""
    from igs_amd.refine import GaussianParams
    raw, _, _ = cfg1_scene(P=4000, size=64)
    params = GaussianParams(raw, dev)
    g = torch.Generator().manual_seed(3)
    params.exp_avg.copy_(torch.randn(params.exp_avg.shape, generator=g).to(dev))
    params.exp_avg_sq.copy_(torch.rand(params.exp_avg_sq.shape, generator=g).to(dev))
    P = params.P
    st = dn.DensifyState(P, dev)
    st.grad_accum.copy_((torch.rand(P, generator=g) * 6e-4).to(dev))
    st.denom.copy_(torch.randint(0, 3, (P,), generator=g).float().to(dev))
    cfg = dn.DensifyConfig(grad_threshold=0.00015, min_opacity=0.005, max_num=max_num, percent_dense=0.01, extent=5.0, native=True)

    def groups(p):
        return {k: [buf[p.spans[k][0]:p.spans[k][0] + p.spans[k][1]].view(p.leaves[k].shape).clone() for buf in (p.flat, p.exp_avg, p.exp_avg_sq)]
                for k in p.leaves}
    old = groups(params)
    pl = dn.densify_and_prune(params, st, cfg, torch.Generator(device=dev).manual_seed(11))
    src, fresh, child = pl["src"].long(), pl["fresh"].bool(), pl["ovr"] >= 0
    ovr = pl["ovr"].long()
    assert pl["n_clone"] > 0 and pl["n_split"] > 0 and pl["n_pruned"] > 0
    assert params.P == src.numel() == P + pl["n_clone"] + pl["n_split"] - pl["n_pruned"] and params.P != P
    if max_num == 4300:
        assert pl["n_clone"] + pl["n_split"] == 300
    assert bool(fresh[child].all()) and int(child.sum()) > 0 and int((fresh & ~child).sum()) > 0
    new = groups(params)
    for k in new:
        want_p = old[k][0][src].clone()
        if k == "xyz":
            want_p[child] = pl["ovr_xyz"][ovr[child]]
        if k == "scaling":
            want_p[child] = pl["ovr_scale"][ovr[child]]
        assert torch.equal(new[k][0], want_p), k
        for j in (1, 2):
            want_m = old[k][j][src].clone()
            want_m[fresh] = 0.0
            assert torch.equal(new[k][j], want_m), (k, j)
    assert st.denom.numel() == params.P and float(st.denom.sum()) == 0.0 and float(st.grad_accum.sum()) == 0.0
    assert st.max_radii.numel() == params.P and st.plan_bufs is None


@pytest.fixture(scope="module")
def loop_scene(dev):
    from igs_amd.refine import render
    from igs_amd.scenes import perturbed_copy
    raw, cams, bg = cfg1_scene(P=3000, size=128)
    cams = [cams[0].to(dev)]
    bg = bg.to(dev)
    gt_raw = {k: v.to(dev) for k, v in perturbed_copy(raw, sigma=0.05).items()}
    with torch.no_grad():
        gts = [render(activate(gt_raw), cams[0], bg)["images_pred"].clone()]
    return raw, cams, gts, bg


def test_refine_loop_native_against_the_pytorch_plan(dev, loop_scene):
    """The loop of test_refine_loop_with_densification twice, once with the native plan: up to the first event both runs are the
    same computation, and the event's counts do not depend on the split draws, so the first log entry is identical; the native run
    improves the PSNR by that test's margin."""
    from igs_amd.refine import GaussianParams, Refiner, render, psnr
    raw, cams, gts, bg = loop_scene
    logs = {}
    for native in (False, True):
        params = GaussianParams(raw, dev)
        cfg = dn.DensifyConfig(until_iter=30, from_iter=0, interval=10, grad_threshold=2e-5, min_opacity=0.005, max_num=3400,
                               percent_dense=0.01, extent=5.0, native=native)
        ref = Refiner(params, cams, gts, bg, loss="l1_ssim", densify=cfg)
        with torch.no_grad():
            p0 = float(psnr(render(params.activated(), cams[0], bg)["images_pred"], gts[0]))
        for it in range(40 if native else 11):
            ref.step(view=0)
        logs[native] = ref.densify_log
        if native:
            assert [e[0] for e in ref.densify_log] == [10, 20] and params.step_count == 40 - 2
            with torch.no_grad():
                p1 = float(psnr(render(params.activated(), cams[0], bg)["images_pred"], gts[0]))
            assert p1 > p0 + 0.5, (p0, p1)
    assert logs[False][0] == logs[True][0] and logs[True][0][1] + logs[True][0][2] > 0


def test_a_native_rebuild_adds_no_attribute(dev, loop_scene):
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = loop_scene
    p = GaussianParams(raw, dev)
    r = Refiner(p, cams, gts, bg, densify=dn.DensifyConfig(from_iter=0, interval=2, until_iter=10, native=True))
    before = set(vars(r)), set(vars(p))
    r.step()
    state_before = set(vars(r.densify_state))
    for _ in range(3):
        r.step()
    torch.cuda.synchronize()
    assert [e[0] for e in r.densify_log] == [2]
    assert (set(vars(r)), set(vars(p))) == before and set(vars(r.densify_state)) == state_before
