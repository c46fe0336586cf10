"""Masked refinement on the GPU: igs_refine_step_masked, the partitioned GaussianParams, the Refiner's modes and run_stream against
the semantics of the reference's load_fromstream(refine_item) / convert2stream."""
import pytest
import torch
import torch.nn as nn

from igs_amd.scenes import cfg1_scene, activate

pytestmark = pytest.mark.gpu

P0 = 3000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _scene(dev, P=P0, size=128):
    from igs_amd.refine import render
    from igs_amd.scenes import perturbed_copy
    raw, cams, bg = cfg1_scene(P=P, size=size)
    cams = [cams[0].to(dev)]
    bgd = bg.to(dev)
    gt_raw = {k: v.to(dev) for k, v in perturbed_copy(raw, sigma=0.03).items()}
    with torch.no_grad():
        gts = [render(activate(gt_raw), cams[0], bgd)["images_pred"].clone()]
    return raw, cams, gts, bgd


def _index_mask(P, frac=0.3, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(P, generator=g)[: int(frac * P)]


def _store_rows(p, name):
    """Group `name` of the store as [P, k] rows (params, exp_avg, exp_avg_sq)."""
    o, n = p.spans[name]
    k = n // p.P
    return [t[o:o + n].view(p.P, k) for t in (p.flat, p.exp_avg, p.exp_avg_sq)]


class MaskedCallerModel:
    """A caller-side restatement of GaussianModel.load_fromstream(use_mask=True) (gaussian_model.py:265-348, 88-127): the outbox
    tensors (Gaussians outside the mask) are detached, the dynamic ones nn.Parameters; the getters concatenate outbox first; Adam
    (eps 1e-15) gets the groups refine_item leaves."""

    def __init__(self, raw, trainable, device, lrs, refine_item):
        out_idx, dyn_idx = torch.nonzero(~trainable).flatten(), torch.nonzero(trainable).flatten()
        self.out = {k: v[out_idx].detach().clone().to(device) for k, v in raw.items()}
        self.dyn = {k: nn.Parameter(v[dyn_idx].detach().clone().to(device).contiguous()) for k, v in raw.items()}
        skip = dict(shs=refine_item.get("no_shs"), opacity=refine_item.get("no_opacity"), scaling=refine_item.get("no_scaling"))
        groups = [{"params": [self.dyn[n]], "lr": lrs[n], "name": n} for n in ("xyz", "rotation", "shs", "opacity", "scaling") if not skip.get(n)]
        self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)

    def _cat(self, k):
        return torch.cat([self.out[k], self.dyn[k]], dim=0)

    get_xyz = property(lambda self: self._cat("xyz"))
    get_features = property(lambda self: self._cat("shs"))
    get_opacity = property(lambda self: torch.sigmoid(self._cat("opacity")))
    get_scaling = property(lambda self: torch.exp(self._cat("scaling")))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._cat("rotation")))


def _run_restatement(raw, trainable, cams, gts, bg, loss, refine_item, steps, dev):
    from igs_amd.refine import DEFAULT_LRS
    from tools.dropin_loop import refine_iteration, make_losses
    gs = MaskedCallerModel(raw, trainable, dev, DEFAULT_LRS, refine_item)
    lf = make_losses("igs")
    for _ in range(steps):
        refine_iteration(gs, cams[0], gts[0], bg, loss=loss, losses=lf)
    return {k: gs._cat(k).detach() for k in raw}


def _assert_close_to_restatement(got, want, steps, where):
    from igs_amd.refine import DEFAULT_LRS
    for k in want:
        d = (got[k].reshape(want[k].shape) - want[k]).abs()
        if d.numel() == 0:
            continue
        lr = DEFAULT_LRS[k]
        q = float(torch.quantile(d.flatten()[:100000].float(), 0.98))
        assert q < 0.02 * lr * steps, (where, k, q)
        assert float(d.max()) <= 2.05 * lr * steps, (where, k, float(d.max()))


def _leaves(p):
    return {k: v.detach().clone() for k, v in p.leaves.items()}


@pytest.mark.parametrize("loss", ["l1", "l1_ssim"])
def test_trivial_mask_is_igs_refine_step_bit_for_bit(dev, loss, monkeypatch):
    """igs_refine_step_masked with m = NULL and with {0, 0} leaves parameters, moments and images bit-identical to igs_refine_step."""
    import ctypes as C
    from igs_amd import _cabi
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = _scene(dev)
    L = _cabi.lib()

    def run(entry):
        p = GaussianParams(raw, dev)
        r = Refiner(p, cams, gts, bg, loss=loss)
        if entry is not None:
            monkeypatch.setattr(L, "igs_refine_step", entry)
        for _ in range(4):
            pkg = r.step(view=0)
        monkeypatch.undo()
        torch.cuda.synchronize()
        return p.flat.clone(), p.exp_avg.clone(), p.exp_avg_sq.clone(), pkg["images_pred"].clone()

    masked = L.igs_refine_step_masked
    base = run(None)
    null = run(lambda a: masked(a, None))
    zero = run(lambda a: masked(a, C.byref(_cabi.RefineMaskArgs(0, 0))))
    for got in (null, zero):
        for x, y in zip(base, got):
            assert torch.equal(x, y)


@pytest.mark.parametrize("loss", ["l1", "l1_ssim"])
def test_first_masked_step_equals_the_unmasked_step_on_trainable_rows(dev, loss):
    """One step of a masked store against one step of an unmasked store in the same (partitioned) order: trainable rows of parameters and
    moments bit-identical (the blend backward's per-Gaussian sums are double rows, exact for these addends, so the frozen splats' missing
    moments change nothing else), frozen rows at their start values, images identical."""
    from igs_amd.refine import GaussianParams, Refiner, GROUPS
    raw, cams, gts, bg = _scene(dev)
    mask = _index_mask(P0)
    pm = GaussianParams(raw, dev, refine_item=dict(use_mask=True), mask=mask)
    F = pm.trainable_from
    assert 0 < F < P0 and pm.mask_num == len(mask)
    part = {k: v[pm.order.cpu()] for k, v in raw.items()}
    pu = GaussianParams(part, dev)
    assert torch.equal(pm.flat, pu.flat)
    start = pm.flat.clone()
    km = Refiner(pm, cams, gts, bg, loss=loss).step(view=0)
    ku = Refiner(pu, cams, gts, bg, loss=loss).step(view=0)
    torch.cuda.synchronize()
    assert torch.equal(km["images_pred"], ku["images_pred"])
    for name, _ in GROUPS:
        rm, ru = _store_rows(pm, name), _store_rows(pu, name)
        o, n = pm.spans[name]
        k = n // P0
        for a, b in zip(rm, ru):
            assert torch.equal(a[F:], b[F:]), name
        assert torch.equal(rm[0][:F], start[o:o + n].view(P0, k)[:F]), name
        assert not rm[1][:F].any() and not rm[2][:F].any(), name
        assert rm[1][F:].abs().sum() > 0, name          # (the trainable rows did move)


@pytest.mark.parametrize("loss", ["l1", "l1_ssim"])
@pytest.mark.parametrize("item", [{}, dict(no_shs=True), dict(no_opacity=True, no_scaling=True)], ids=["all", "no_shs", "no_opac_scale"])
def test_masked_refiner_follows_the_reference_semantics(dev, loss, item):
    """4 steps of the masked fused step against the caller-side restatement of load_fromstream(use_mask=True) driven through the drop-in
    rasterizer: trainable values within the bars of test_unchanged_caller_loop_equals_the_fused_step, frozen ones bit-identical."""
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = _scene(dev)
    mask = _index_mask(P0)
    steps = 4
    ri = dict(item, use_mask=True)
    p = GaussianParams(raw, dev, refine_item=ri, mask=mask)
    r = Refiner(p, cams, gts, bg, loss=loss)
    for _ in range(steps):
        r.step(view=0)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in p.original_order().items()}
    trainable = torch.zeros(P0, dtype=torch.bool)
    trainable[mask] = True
    want_part = _run_restatement(raw, trainable, cams, gts, bg, loss, ri, steps, dev)
    inv = torch.empty_like(p.order.cpu())
    inv[p.order.cpu()] = torch.arange(P0)
    want = {k: v.cpu()[inv] for k, v in want_part.items()}          # restatement rows: outbox first, dynamic last = the store's order
    frozen_groups = set(p.frozen_groups)
    for k in raw:
        g, s0 = got[k].reshape(raw[k].shape), raw[k]
        assert torch.equal(g[~trainable], s0[~trainable]), k
        if k in frozen_groups:
            assert torch.equal(g, s0), k
            continue
        assert torch.isfinite(g).all(), k
    _assert_close_to_restatement({k: got[k][trainable] for k in raw}, {k: want[k][trainable] for k in raw}, steps, (loss, item))


def test_frozen_sh_without_a_mask(dev):
    """no_shs alone: the SH span and its moments stay as they were; the other groups follow the restatement."""
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = _scene(dev)
    steps = 4
    p = GaussianParams(raw, dev, refine_item=dict(no_shs=True))
    assert p.trainable_from == 0 and p.frozen_groups == ("shs",)
    rows0 = [t.clone() for t in _store_rows(p, "shs")]
    r = Refiner(p, cams, gts, bg, loss="l1")
    for _ in range(steps):
        r.step(view=0)
    torch.cuda.synchronize()
    for a, b in zip(_store_rows(p, "shs"), rows0):
        assert torch.equal(a, b)
    want = _run_restatement(raw, torch.ones(P0, dtype=torch.bool), cams, gts, bg, "l1", dict(no_shs=True), steps, dev)
    got = _leaves(p)
    assert float((got["xyz"] - raw["xyz"].to(dev)).abs().max()) > 0
    _assert_close_to_restatement(got, want, steps, "no_shs")


@pytest.mark.parametrize("case", ["depth_normal", "clamp"])
def test_other_losses_and_the_clamp_under_a_mask(dev, case):
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = _scene(dev)
    mask = _index_mask(P0)
    p = GaussianParams(raw, dev, refine_item=dict(use_mask=True, no_opacity=(case == "clamp")), mask=mask)
    F = p.trainable_from
    start = p.flat.clone()
    if case == "depth_normal":
        r = Refiner(p, cams, gts, bg, loss="l1_ssim", lambda_depth_normal=0.05)
    else:
        r = Refiner(p, cams, gts, bg, loss="l1")
        r.clamp = True
    for _ in range(4):
        pkg = r.step(view=0)
    torch.cuda.synchronize()
    assert torch.isfinite(pkg["loss"]).all()
    for name in ("xyz", "rotation", "shs", "opacity", "scaling"):
        o, n = p.spans[name]
        k = n // p.P
        rows = _store_rows(p, name)
        assert torch.equal(rows[0][:F], start[o:o + n].view(p.P, k)[:F]), name
        assert not rows[1][:F].any() and not rows[2][:F].any(), name
        assert all(torch.isfinite(t).all() for t in rows), name
    if case == "clamp":
        o, n = p.spans["opacity"]
        assert torch.equal(p.flat[o:o + n], start[o:o + n]) and not p.exp_avg[o:o + n].any()
    o, n = p.spans["xyz"]
    assert p.exp_avg[o + 3 * F:o + n].abs().sum() > 0


def test_run_stream_with_the_dynamic_mask(dev):
    from igs_amd.stream import run_stream, SyntheticStream
    from igs_amd.scenes import sear_steak_like_scene
    raw, cams, bg = sear_steak_like_scene(P=6000, n_cams=3, width=160, height=120, focal=90.0)
    d = torch.device(dev)
    cams_d = [c.to(d) for c in cams]
    src = SyntheticStream(raw, cams_d, bg.to(d), d)
    dyn = src.dynamic.cpu()
    assert 0 < int(dyn.sum()) < dyn.numel()
    states = []
    recs = run_stream(raw, cams, bg, frames=3, refine_iterations=10, device="cuda:0", loss="l1_ssim", source=src, mask="dynamic",
                      states=states)
    assert len(recs) == len(states) == 3
    for rec, st in zip(recs, states):
        assert rec["mask_num"] == int(dyn.sum())
        assert rec["psnr_after"] >= rec["psnr_before"], rec
        for k in raw:
            assert torch.equal(st[k].cpu().reshape(raw[k].shape)[~dyn], raw[k][~dyn]), (rec["frame"], k)
        assert not torch.equal(st["xyz"].cpu()[dyn], raw["xyz"][dyn])


@pytest.mark.parametrize("mode", ["autograd", "direct", "native"])
def test_unfused_paths_agree_with_the_fused_masked_step(dev, mode):
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = _scene(dev)
    mask = _index_mask(P0)
    steps = 4
    ri = dict(use_mask=True, no_scaling=True)
    pf = GaussianParams(raw, dev, refine_item=ri, mask=mask)
    rf = Refiner(pf, cams, gts, bg, loss="l1")
    pu = GaussianParams(raw, dev, refine_item=ri, mask=mask)
    if mode == "native":
        ru = Refiner(pu, cams, gts, bg, loss="l1", fused=False)
    else:
        ru = Refiner(pu, cams, gts, bg, loss="l1", native=False)
        ru.direct_adam = mode == "direct"
    start = pu.flat.clone()
    for _ in range(steps):
        rf.step(view=0)
        ru.step(view=0)
    torch.cuda.synchronize()
    assert ru._mode() == {"autograd": "autograd", "direct": "direct", "native": "exchange"}[mode]
    F = pu.trainable_from
    for name in ("xyz", "rotation", "shs", "opacity", "scaling"):
        o, n = pu.spans[name]
        k = n // pu.P
        assert torch.equal(_store_rows(pu, name)[0][:F], start[o:o + n].view(pu.P, k)[:F]), name
    o, n = pu.spans["scaling"]
    assert torch.equal(pu.flat[o:o + n], start[o:o + n])
    got, want = _leaves(pu), _leaves(pf)
    _assert_close_to_restatement({k: v[F:] for k, v in got.items()}, {k: v[F:] for k, v in want.items()}, steps, mode)


@pytest.fixture(scope="module")
def small_scene(dev):
    return _scene(dev)


def _attribute_cases():
    from igs_amd.densify import DensifyConfig
    return {
        "fused_l1": (dict(loss="l1"), {}, "fused"),
        "fused_l1_ssim_depth_normal": (dict(loss="l1_ssim", lambda_depth_normal=0.05), {}, "fused"),
        "native": (dict(fused=False), {}, "exchange"),
        "autograd": (dict(native=False), {}, "autograd"),
        "direct": (dict(native=False, direct_adam=True), {}, "direct"),
        "masked": ({}, dict(refine_item=dict(use_mask=True, no_scaling=True), mask=_index_mask(P0)), "fused"),
        "densify": (dict(densify=DensifyConfig(from_iter=0, interval=2, until_iter=10)), {}, "densify"),
    }


@pytest.mark.parametrize("case", ["fused_l1", "fused_l1_ssim_depth_normal", "native", "autograd", "direct", "masked", "densify"])
def test_a_step_adds_no_attribute(small_scene, dev, case):
    """Everything a Refiner and its GaussianParams can carry is declared at construction: 4 steps in every mode (the densify case
    rebuilds the store through _bind in its third) leave the attribute sets of both objects as they were."""
    from igs_amd.refine import GaussianParams, Refiner
    raw, cams, gts, bg = small_scene
    refiner_kw, store_kw, mode = _attribute_cases()[case]
    p = GaussianParams(raw, dev, **store_kw)
    r = Refiner(p, cams, gts, bg, **refiner_kw)
    before = set(vars(r)), set(vars(p))
    for _ in range(4):
        r.step()
    torch.cuda.synchronize()
    assert r._mode() == mode
    assert (set(vars(r)), set(vars(p))) == before
    if case == "densify":
        assert [e[0] for e in r.densify_log] == [2]          # (the rebuild did happen, at iteration 2)
