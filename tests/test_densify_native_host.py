"""The native densify-and-prune plan without a GPU: the C ABI declares, binds and exports igs_densify_plan, it refuses bad arguments
before any HIP call, plan_native has no CPU path, and the float64 restatement the GPU tests use (tests/densify_plan_restatement.py)
reproduces the pinned PyTorch plan on the scene of tests/test_densify_plan.py."""
import os
import re

import numpy as np
import pytest
import torch

import densify_plan_restatement as DR
from igs_amd import densify as dn
from igs_amd.scenes import cfg1_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_params(name):
    hdr = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "%s is not declared in include/igs_rast.h" % name
    return [p for p in m.group(1).split(",") if p.strip()]


def test_header_binding_and_library_agree():
    from igs_amd import _cabi
    assert len(_declared_params("igs_densify_plan_scratch_bytes")) == 1 == len(_cabi.SIGNATURES["igs_densify_plan_scratch_bytes"][1])
    assert len(_declared_params("igs_densify_plan")) == 22 == len(_cabi.SIGNATURES["igs_densify_plan"][1])
    L = _cabi.lib()
    assert hasattr(L, "igs_densify_plan") and hasattr(L, "igs_densify_plan_scratch_bytes")
    assert L.igs_rast_version() == 4
    # capacity: scratch grows with P, is refused outside the range
    assert L.igs_densify_plan_scratch_bytes(-1) == 0 and L.igs_densify_plan_scratch_bytes((1 << 28) + 1) == 0
    assert L.igs_densify_plan_scratch_bytes(200000) >= 200000 * 5
    assert "densify.hip" in __import__("igs_amd.build", fromlist=["SOURCES"]).SOURCES


def test_bad_arguments_are_refused_before_any_hip_call():
    from igs_amd import _cabi
    L = _cabi.lib()
    p = 4096                                                     # never dereferenced: every call below returns before a launch
    ptrs = [p] * 7
    outs = [p] * 7
    assert L.igs_densify_plan(None, -1, *ptrs, 1e-4, 0.005, 0.05, 0.0, 10, 1, *outs) == -1 and "P out of range" in _cabi.last_error()
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert L.igs_densify_plan(None, 5, *ptrs, thr, 0.005, 0.05, 0.0, 10, 1, *outs) == -1 and "grad_threshold" in _cabi.last_error()
    for k in range(14):
        if k == 6:
            continue                                             # normals may be NULL
        a = ptrs + outs
        a[k] = None
        assert L.igs_densify_plan(None, 5, *a[:7], 1e-4, 0.005, 0.05, 0.0, 10, 1, *a[7:]) == -1 and "NULL" in _cabi.last_error(), k
    assert L.igs_densify_plan(None, 0, *([None] * 7), 1e-4, 0.005, 0.05, 0.0, 10, 1, *([None] * 7)) == 0      # P == 0: nothing to do


def test_config_default_keeps_the_pytorch_plan():
    assert dn.DensifyConfig().native is False
    assert dn.DensifyConfig(native=True).native is True
    assert dn.DensifyState(4, torch.device("cpu")).plan_bufs is None


def test_plan_native_has_no_cpu_path():
    raw, _, _ = cfg1_scene(P=64, size=32)
    st = dn.DensifyState(64, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        dn.plan_native(raw["xyz"], raw["rotation"], raw["opacity"], raw["scaling"], st, dn.DensifyConfig())


def _pinned(max_num, denom_low):
    """Scene, statistics and configuration of tests/test_densify_plan.py::test_plan_equals_reference_sequence_on_cpu
    (denom_low = 0); denom_low = 1 draws the denominators from {1, 2} instead of {0, 1, 2}."""
    raw, _, _ = cfg1_scene(P=3000, size=32)
    g = torch.Generator().manual_seed(1)

    class S:
        grad_accum = torch.rand(3000, generator=g) * 6e-4
        denom = torch.randint(denom_low, 3, (3000,), generator=g).float()
    cfg = dn.DensifyConfig(grad_threshold=0.00015, min_opacity=0.005, max_num=max_num, percent_dense=0.01, extent=5.0)
    pl = dn.plan(raw["xyz"], raw["rotation"], raw["opacity"], raw["scaling"], S, cfg, torch.Generator().manual_seed(4))
    assert pl["n_clone"] > 0 and pl["n_split"] > 0
    return raw, S, cfg, pl


def _assert_same_decision(pl, re_):
    for k in ("src", "fresh", "ovr"):
        assert np.array_equal(pl[k].numpy(), re_[k]), k
    assert (pl["n_clone"], pl["n_split"], pl["n_pruned"]) == (re_["n_clone"], re_["n_split"], re_["n_pruned"])
    assert np.allclose(pl["ovr_scale"].numpy(), re_["ovr_scale"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("max_num", [100000, 3200])
def test_restatement_reproduces_the_pinned_plan(max_num):
    """Same inputs as tests/test_densify_plan.py::test_plan_equals_reference_sequence_on_cpu: src / fresh / ovr and the counts of the
    float64 restatement equal those of densify.plan (whose draws do not enter the selection: the world-size prune is off).

    max_num = 3200 admits 200 candidates, and the pinned statistics hold about a thousand x/0 = +inf gradients (every third denom
    is 0): the cut falls INSIDE that block of equal values, where torch.topk's choice is unspecified (its CPU kernel does not take
    the lowest indices) and the restatement's lowest-index rule picks other rows by design.  There the restatement is given the rows
    torch.topk admits -- the same call on the same input as inside plan -- and everything else (classes, children's rows, prune,
    order, counts) must still be equal; the select itself is compared with plan in the next test, on statistics without ties."""
    raw, S, cfg, pl = _pinned(max_num, 0)
    g = DR.gradient(S.grad_accum, S.denom)
    k = max_num - 3000
    candidates = None
    if int((g >= cfg.grad_threshold).sum()) > k:
        cut = np.sort(g)[::-1][k - 1]
        assert np.isinf(cut) and int((g == cut).sum()) > k                 # the tie block straddles the cut
        idx = torch.topk(torch.from_numpy(g).view(-1, 1), k, dim=0).indices.view(-1)
        candidates = np.zeros(3000, dtype=bool)
        candidates[idx.numpy()] = True
        lowest = DR.select(g, cfg.grad_threshold, k, True)
        assert int(lowest.sum()) == k and bool(np.isinf(g[lowest]).all())
        assert np.array_equal(np.nonzero(lowest)[0], np.nonzero(np.isinf(g))[0][:k])          # the lowest-index rule
    else:
        assert max_num == 100000
    _assert_same_decision(pl, DR.restate_cfg(raw, S, cfg, np.zeros((3000, 2, 3)), candidates))


@pytest.mark.parametrize("max_num", [100000, 3200])
def test_restatement_select_equals_topk_without_ties(max_num):
    """The same scene with denominators >= 1: the gradients at the cut are distinct, torch.topk is determined, and the restatement's
    own select gives plan's decision exactly, in the unbounded and in the bounded branch."""
    raw, S, cfg, pl = _pinned(max_num, 1)
    g = DR.gradient(S.grad_accum, S.denom)
    cands = np.sort(g[g >= cfg.grad_threshold])[::-1]
    assert cands.size > 200 and cands[199] > cands[200]
    if max_num == 3200:
        assert pl["n_clone"] + pl["n_split"] == 200
    _assert_same_decision(pl, DR.restate_cfg(raw, S, cfg, np.zeros((3000, 2, 3))))
