"""Masked refinement (refine_item / mask of GaussianModel.load_fromstream), host side: parsing, the partitioned store, the order it
keeps, the C ABI of igs_refine_step_masked and the refusals.  No GPU needed."""
import ctypes as C
import types

import pytest
import torch


def _raw(P=40, seed=3):
    from igs_amd.scenes import cfg1_scene
    raw, _, _ = cfg1_scene(P=P, seed=seed, size=16)
    return raw


def test_refine_item_parsing_dict_attribute_and_missing_keys():
    from igs_amd.refine import parse_refine_item, REFINE_ITEM_KEYS
    assert parse_refine_item(None) == dict.fromkeys(REFINE_ITEM_KEYS, False)
    assert parse_refine_item({}) == dict.fromkeys(REFINE_ITEM_KEYS, False)
    d = parse_refine_item(dict(no_shs=True, use_mask=1))
    assert d["no_shs"] and d["use_mask"] and not d["no_opacity"] and not d["no_scaling"]
    # attribute access (an OmegaConf node behaves like this); missing attributes and None mean False
    node = types.SimpleNamespace(no_opacity=True, no_scaling=None)
    a = parse_refine_item(node)
    assert a["no_opacity"] and not a["no_scaling"] and not a["no_shs"] and not a["use_mask"]
    # the same flags through both forms
    assert parse_refine_item(types.SimpleNamespace(no_shs=True, use_mask=True)) == parse_refine_item(dict(no_shs=True, use_mask=True))


@pytest.mark.parametrize("key", ["use_new_shs", "tracking"])
def test_refine_item_unsupported_flags_raise(key):
    from igs_amd.refine import parse_refine_item, GaussianParams
    with pytest.raises(NotImplementedError, match=key):
        parse_refine_item({key: True})
    with pytest.raises(NotImplementedError, match=key):
        parse_refine_item(types.SimpleNamespace(**{key: True}))
    with pytest.raises(NotImplementedError, match=key):
        GaussianParams(_raw(), torch.device("cpu"), refine_item={key: True})
    parse_refine_item({key: False})          # (False is fine)


def test_index_and_bool_masks_give_the_same_partition():
    from igs_amd.refine import GaussianParams, normalize_mask
    P = 40
    raw = _raw(P)
    idx = torch.tensor([31, 2, 5, 17, 5, 39, 0])                  # unsorted, one duplicate (the index form selects a set)
    b = torch.zeros(P, dtype=torch.bool)
    b[idx] = True
    assert torch.equal(normalize_mask(idx, P), b)
    pi = GaussianParams(raw, torch.device("cpu"), refine_item=dict(use_mask=True), mask=idx)
    pb = GaussianParams(raw, torch.device("cpu"), refine_item=dict(use_mask=True), mask=b)
    assert pi.trainable_from == pb.trainable_from == P - 6 and pi.mask_num == pb.mask_num == 6
    assert torch.equal(pi.order, pb.order) and torch.equal(pi.flat, pb.flat)
    # frozen Gaussians first, trainable ones last, each part in its original order
    assert sorted(pi.order[pi.trainable_from:].tolist()) == pi.order[pi.trainable_from:].tolist() == sorted(set(idx.tolist()))
    assert pi.order[:pi.trainable_from].tolist() == [i for i in range(P) if not b[i]]
    assert torch.equal(pi.leaves["xyz"].detach(), raw["xyz"][pi.order])
    with pytest.raises(ValueError):
        normalize_mask(torch.tensor([P]), P)
    with pytest.raises(ValueError):
        normalize_mask(torch.ones(P - 1, dtype=torch.bool), P)
    with pytest.raises(ValueError, match="needs a mask"):
        GaussianParams(raw, torch.device("cpu"), refine_item=dict(use_mask=True))


def test_store_exposes_partition_and_frozen_groups():
    from igs_amd.refine import GaussianParams, GROUPS
    P = 40
    raw = _raw(P)
    p = GaussianParams(raw, torch.device("cpu"), refine_item=dict(use_mask=True, no_shs=True, no_scaling=True), mask=torch.arange(10))
    assert p.trainable_from == 30 and p.mask_num == 10 and p.partial
    assert set(p.frozen_groups) == {"shs", "scaling"} and p.frozen_group_bits == 4 | 16
    spans = {n: (o, c) for n, o, c in p.trainable_spans()}
    assert set(spans) == {"xyz", "rotation", "opacity"}
    k = dict(GROUPS)
    for n, (o, c) in spans.items():
        assert o == p.spans[n][0] + k[n] * 30 and c == k[n] * 10
    q = GaussianParams(raw, torch.device("cpu"))
    assert q.trainable_from == 0 and q.mask_num == P and not q.partial and q.frozen_groups == ()
    assert [(n, o, c) for n, o, c in q.trainable_spans()] == [(n, q.spans[n][0], q.spans[n][1]) for n, _ in GROUPS]
    # a mask without refine_item means use_mask; refine_item without use_mask ignores a mask (as load_fromstream does)
    assert GaussianParams(raw, torch.device("cpu"), mask=torch.arange(10)).trainable_from == 30
    assert GaussianParams(raw, torch.device("cpu"), refine_item=dict(no_shs=True), mask=torch.arange(10)).trainable_from == 0


def test_original_order_undoes_partition_and_per_part_sorts():
    """The order bookkeeping of a masked store: partition, then a permutation inside each part (what spatial_sort does with the Morton
    order of each part), twice; the inverse gives every row back in the original order."""
    from igs_amd.refine import GaussianParams, partition_order, compose_order, inverse_order
    P = 50
    raw = _raw(P, seed=5)
    gen = torch.Generator().manual_seed(11)
    trainable = torch.rand(P, generator=gen) < 0.3
    F = int((~trainable).sum())
    order = compose_order(None, partition_order(trainable))
    assert (~trainable[order[:F]]).all() and trainable[order[F:]].all()
    rows = raw["xyz"][order]
    for _ in range(2):
        perm = torch.cat([torch.randperm(F, generator=gen), F + torch.randperm(P - F, generator=gen)])
        rows = rows[perm]
        order = compose_order(order, perm)
        assert (~trainable[order[:F]]).all() and trainable[order[F:]].all()       # the parts stay where they are
    assert torch.equal(rows, raw["xyz"][order])
    assert torch.equal(rows[inverse_order(order)], raw["xyz"])
    # the store applies the same bookkeeping: original_order() after the partition alone
    p = GaussianParams(raw, torch.device("cpu"), mask=trainable)
    back = p.original_order()
    for k in raw:
        assert torch.equal(back[k].reshape(raw[k].shape), raw[k])


def test_masked_entry_point_exports_and_struct_size():
    from igs_amd import _cabi
    L = _cabi.lib()
    for n in ("igs_refine_step_masked", "igs_refine_mask_args_size"):
        assert n in _cabi.EXPORTS and hasattr(L, n)
    assert L.igs_refine_mask_args_size() == C.sizeof(_cabi.RefineMaskArgs) == 8
    assert L.igs_rast_version() == _cabi.VERSION == 4


def test_masked_entry_point_validates_before_it_launches():
    """Every refusal of igs_refine_step_masked returns IGS_RAST_E_INVALID before any HIP call: the step arguments below point at
    addresses that are never dereferenced."""
    from igs_amd import _cabi
    L = _cabi.lib()
    INVALID = -1

    def args(**kw):
        a = _cabi.RefineStepArgs()
        a.P, a.D, a.M, a.width, a.height, a.step = 100, 3, 16, 64, 48, 1
        a.param, a.exp_avg, a.exp_avg_sq, a.gt = 0x1000, 0x2000, 0x3000, 0x4000
        a.out_images, a.radii, a.workspace, a.background = 0x5000, 0x6000, 0x7000, 0x8000
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(a, first, groups):
        m = _cabi.RefineMaskArgs(first, groups)
        return L.igs_refine_step_masked(C.byref(a), C.byref(m))

    G = _cabi
    assert call(args(), -1, 0) == INVALID
    assert "first_trainable" in _cabi.last_error()
    assert call(args(), 101, 0) == INVALID
    assert call(args(), 0, 32) == INVALID                                          # unknown group bit
    assert "unknown group" in _cabi.last_error()
    assert call(args(), 0, 1 << 31) == INVALID
    assert call(args(), 10, G.GROUP_XYZ) == INVALID                               # xyz is always trained
    assert call(args(), 0, G.GROUP_ROT | G.GROUP_SH) == INVALID                   # ... and rotation
    assert "always trained" in _cabi.last_error()
    assert call(args(grad_out=0x9000), 10, 0) == INVALID                           # multi-GPU exchange with a mask
    assert call(args(color_grad_out=0x9000), 0, G.GROUP_SH) == INVALID
    assert "multi-GPU" in _cabi.last_error()
    assert call(args(dL_dmean2D=0x9000), 10, 0) == INVALID                         # densification with a mask
    assert call(args(dL_dmean2D=0x9000), 0, G.GROUP_OPACITY) == INVALID
    assert "densification" in _cabi.last_error()
    assert L.igs_refine_step_masked(None, None) == INVALID


def test_refiner_refuses_densify_and_multi_gpu_with_a_mask():
    from igs_amd.refine import GaussianParams, Refiner
    from igs_amd.densify import DensifyConfig
    P = 40
    raw = _raw(P)
    cams, gts, bg = [None], [torch.zeros(3, 4, 4)], torch.zeros(3)
    for kw in (dict(mask=torch.arange(8)), dict(refine_item=dict(no_shs=True))):
        p = GaussianParams(raw, torch.device("cpu"), **kw)
        with pytest.raises(NotImplementedError, match="densify"):
            Refiner(p, cams, gts, bg, densify=DensifyConfig())
        with pytest.raises(NotImplementedError, match="world_size > 1"):
            Refiner(p, cams, gts, bg, world_size=2)
    Refiner(GaussianParams(raw, torch.device("cpu")), cams, gts, bg, world_size=2)      # (no mask: unchanged)


REFINER_OPTIONS = dict(require_geometry=True, clamp=False, want_viewspace_grad=None, exchange="colors", overlap_exchange=True,
                       direct_adam=False, fused_activations=False, loss_scale=1.0, cache_gt_stats=True, ssim_fn=None, depth_normal_fn=None)


def _cpu_refiner(**kw):
    from igs_amd.refine import GaussianParams, Refiner
    p = GaussianParams(_raw(8), torch.device("cpu"))
    if kw.get("adam_fn") == "injected":
        kw["adam_fn"] = lambda: None
    return Refiner(p, [None], [torch.zeros(3, 4, 4)], torch.zeros(3), **kw)


def test_refiner_constructor_owns_every_option():
    """Every option the step code reads is a keyword-only argument of Refiner.__init__ and a plain attribute of the fresh object, with
    the default the step code used to assume; `want_viewspace_grad=None` resolves to `densify is not None`."""
    import inspect
    from igs_amd.refine import Refiner
    from igs_amd.densify import DensifyConfig
    sig = inspect.signature(Refiner.__init__).parameters
    r = _cpu_refiner()
    for name, default in REFINER_OPTIONS.items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
        assert name in vars(r), name
        assert vars(r)[name] == (False if name == "want_viewspace_grad" else default), name
    assert _cpu_refiner(densify=DensifyConfig()).want_viewspace_grad is True
    assert _cpu_refiner(densify=DensifyConfig(), want_viewspace_grad=False).want_viewspace_grad is False
    assert list(sig)[:17] == ["self", "params", "cams", "gt_images", "bg", "loss", "lambda_l1", "world_size", "rank", "seed", "render_fn",
                              "adam_fn", "native", "fused", "densify", "densify_seed", "lambda_depth_normal"]      # (positional order unmoved)
    other = dict(require_geometry=False, clamp=True, want_viewspace_grad=True, exchange="gradients", overlap_exchange=False, direct_adam=True,
                 fused_activations=True, loss_scale=3.0, cache_gt_stats=False, ssim_fn=len, depth_normal_fn=max)
    assert set(other) == set(REFINER_OPTIONS)
    r = _cpu_refiner(**other)
    assert all(vars(r)[k] is v or vars(r)[k] == v for k, v in other.items())


def _fake_render(act, cam, bg):
    raise AssertionError("not called")


MODE_TABLE = [
    (dict(), "fused"),
    (dict(loss="l1_ssim"), "fused"),
    (dict(lambda_depth_normal=0.05), "fused"),
    (dict(world_size=2), "exchange"),
    (dict(adam_fn="injected"), "exchange"),
    (dict(fused=False), "exchange"),
    (dict(fused=False, lambda_depth_normal=0.05), "autograd"),
    (dict(native=False), "autograd"),
    (dict(native=False, direct_adam=True), "autograd"),          # (a CPU store; on a CUDA store: "direct")
    (dict(render_fn=_fake_render), "autograd"),
    (dict(densify=True), "densify"),
    (dict(densify=True, fused=False), "densify"),
    (dict(densify=True, world_size=2), "densify"),
    (dict(densify=True, adam_fn="injected"), NotImplementedError),
    (dict(densify=True, native=False), NotImplementedError),
]


@pytest.mark.parametrize("kw,want", MODE_TABLE, ids=[",".join("%s=%s" % (k, getattr(v, "__name__", v)) for k, v in kw.items()) or "defaults"
                                                     for kw, _ in MODE_TABLE])
def test_refiner_mode_table(kw, want):
    """`_mode()` for every way a Refiner is set up (taken from the class before its options moved into the constructor)."""
    from igs_amd.densify import DensifyConfig
    kw = dict(kw)
    if kw.get("densify"):
        kw["densify"] = DensifyConfig()
    r = _cpu_refiner(**kw)
    if want is NotImplementedError:
        with pytest.raises(NotImplementedError):
            r._mode()
    else:
        assert r._mode() == want
