"""The swin window attention (igs_amd/csrc/wattn.hip, igs_amd/attention.py) without a GPU: the float64 restatement against the
reference-produced golden file and against its own second statement, exports and argument counts, the refusals of the C ABI before any
HIP call, the scratch bound, the residency and the instruction mix of the built gfx950 kernels, the derived error bounds on a torch
emulation of the half pipeline and on three wrong variants, and the Python layer."""
import inspect
import os
import re
import shutil
import sys
import types

import numpy as np
import pytest
import torch

import window_attention_restatement as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_window_attn_fwd", "igs_window_attn_bwd", "igs_window_attn_bwd_scratch_bytes")
INVALID = -1
F32, F16 = 0, 1
GOLDEN_CASES = ((4, 10, 2), (6, 9, 3))


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_swin.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_restatement_equals_the_reference_golden(golden, case):
    h, w, K = case
    tag = "h%d_w%d_K%d_" % case
    q, k, v, dout = (golden[tag + n] for n in ("q", "k", "v", "dout"))
    assert q.dtype == torch.float64 and q.shape == (1, h * w, 16)
    plain = WR.restate(q, k, v, h, w, K, False)
    shifted = WR.restate(q, k, v, h, w, K, True)
    assert (plain["o"] - golden[tag + "out"]).abs().max() <= 1e-12
    assert (shifted["o"] - golden[tag + "out_shift"]).abs().max() <= 1e-12
    assert (golden[tag + "out"] - golden[tag + "out_shift"]).abs().max() > 1e-3          # (the shifted case is another function)
    assert torch.equal(shifted["mask"], golden[tag + "mask"])                            # the reference's own mask, bit for bit
    for a, n in zip(WR.gradients(q, k, v, h, w, K, True, dout), ("dq", "dk", "dv")):
        assert (a - golden[tag + n]).abs().max() <= 1e-12, n
    e = WR.explicit_gradients(shifted, dout)
    for n in ("dq", "dk", "dv"):
        assert (e[n] - golden[tag + n]).abs().max() <= 1e-12, n


@pytest.mark.parametrize("case", [(10, 14, 2), (24, 22, 2), (16, 16, 4), (6, 9, 3), (8, 8, 1)])
@pytest.mark.parametrize("shift", [False, True])
def test_gather_form_equals_roll_and_split_form(case, shift):
    h, w, K = case
    q, k, v, dout = WR.random_inputs(2, h, w, torch.float64, "cpu", seed=h * w + K, with_dout=True, C=24)
    r = WR.restate(q, k, v, h, w, K, shift)
    assert (r["o"] - WR.restate_roll(q, k, v, h, w, K, shift)).abs().max() <= 1e-12
    if shift:
        assert torch.equal(r["mask"], WR.paint_mask(h, w, K))
    ga = WR.gradients(q, k, v, h, w, K, shift, dout)
    ge = WR.explicit_gradients(r, dout)
    for a, n in zip(ga, ("dq", "dk", "dv")):
        assert (a - ge[n]).abs().max() <= 1e-12 * (1 + a.abs().max()), n
    tok, _ = WR.token_map(h, w, K, shift)
    assert sorted(tok.reshape(-1).tolist()) == list(range(h * w))                        # every token is in exactly one window


def test_full_attention_is_one_window():
    q, k, v = WR.random_inputs(2, 5, 7, torch.float64, "cpu", seed=2, C=16)
    ref = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(1, 2)) / 4.0, 2), v)
    assert (WR.restated_full(q, k, v) - ref).abs().max() <= 1e-13


# ---------------------------------------------------------------- exports and ABI
def test_exports_and_argument_counts():
    from igs_amd import _cabi, build
    L = _cabi.lib()
    hdr = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert m, n
        assert len(_cabi.SIGNATURES[n][1]) == len(m.group(1).split(",")), n
    assert "wattn.hip" in build.SOURCES
    m = _cabi.ext()
    assert hasattr(m._window, "window_attn_fwd") and hasattr(m._window, "window_attn_bwd")      # (a private submodule of _C)


def _fwd(L, B=1, h=16, w=16, K=2, shift=0, D=128, dt=F32, q=None, strides=None, kv=None, out=None, ostrides=None, scale=0.088):
    s = strides or (h * w * D, D)
    return L.igs_window_attn_fwd(None, B, h, w, K, shift, D, dt, q, *s, kv, h * w * D, D, kv, h * w * D, D, scale, out, *(ostrides or (h * w * D, D)), None)


def _bwd(L, B=1, h=16, w=16, K=2, shift=0, D=128, dt=F32, strides=None, dq=None, ostrides=None, scale=0.088, rest=None):
    s = strides or (h * w * D, D)
    c = (h * w * D, D)
    return L.igs_window_attn_bwd(None, B, h, w, K, shift, D, dt, rest, *s, rest, *c, rest, *c, rest, *c, rest, rest, *c, scale, dq, *(ostrides or c),
                                 None, *c, None, *c, rest)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """NULL device pointers throughout and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    L = _cabi.lib()
    fake = 0x1000                                                # a non-NULL, 16-byte aligned address that is never dereferenced
    for call in (_fwd, _bwd):
        for kw, word in ((dict(D=64), "D must be 128"), (dict(dt=7), "dtype"), (dict(B=-1), "B out of range"), (dict(B=70000), "B out of range"),
                         (dict(h=0), "h, w out of range"), (dict(w=-4), "h, w out of range"), (dict(h=8192, w=4096, K=1), "h * w"),
                         (dict(B=5, h=2048, w=2048, K=1), "B * h * w"), (dict(K=0), "K out of range"), (dict(K=3), "multiples of K"),
                         (dict(h=16, w=18, K=4), "multiples of K"), (dict(h=16, w=4, K=4, shift=1), "at least 2 x 2"),
                         (dict(h=2, w=16, K=2, shift=1), "at least 2 x 2"),
                         (dict(strides=(256 * 128, 130)), "16 bytes"), (dict(strides=(256 * 128, -128)), "negative"),
                         (dict(dt=F16, strides=(256 * 128 + 4, 128)), "16 bytes")):
            assert call(L, **kw) == INVALID, (call.__name__, kw)
            assert word in _cabi.last_error() and "igs_window_attn" + call.__name__ in _cabi.last_error(), (kw, _cabi.last_error())
    assert _fwd(L, h=16, w=4, K=4) == INVALID and "NULL" in _cabi.last_error()              # unshifted 4 x 1 windows are in order: only NULL q
    assert _fwd(L) == INVALID and "NULL" in _cabi.last_error()
    assert _fwd(L, q=fake) == INVALID and "NULL" in _cabi.last_error()                      # ... and NULL k, v, out
    assert _bwd(L, dq=fake) == INVALID and "NULL" in _cabi.last_error()
    # a base pointer off the 16-byte grid, a scale that is not finite, an output whose rows alias (stride 0 or below D)
    assert _fwd(L, q=fake + 4, kv=fake, out=fake) == INVALID and "16-byte aligned" in _cabi.last_error()
    assert _fwd(L, q=fake, kv=fake, out=fake + 8) == INVALID and "16-byte aligned" in _cabi.last_error()
    assert _bwd(L, dq=fake + 4, rest=fake) == INVALID and "16-byte aligned" in _cabi.last_error()
    for bad in (float("inf"), float("nan")):
        assert _fwd(L, q=fake, kv=fake, out=fake, scale=bad) == INVALID and "finite" in _cabi.last_error()
        assert _bwd(L, dq=fake, rest=fake, scale=bad) == INVALID and "finite" in _cabi.last_error()
    for so in ((256 * 128, 0), (256 * 128, 64)):
        assert _fwd(L, q=fake, kv=fake, out=fake, ostrides=so) == INVALID and "overlap" in _cabi.last_error(), so
        assert _bwd(L, dq=fake, rest=fake, ostrides=so) == INVALID and "overlap" in _cabi.last_error(), so
    assert _fwd(L, B=2, q=fake, kv=fake, out=fake, ostrides=(0, 128)) == INVALID and "overlap" in _cabi.last_error()
    assert _fwd(L, B=0) == 0 and _bwd(L, B=0) == 0                                          # nothing to do
    assert _bwd(L) == 0                                                                     # no gradient wanted: nothing to do
    assert L.igs_window_attn_bwd_scratch_bytes(1, 16, 16, 2, 64, F32) == 0
    assert L.igs_window_attn_bwd_scratch_bytes(1, 16, 16, 3, 128, F32) == 0


def test_the_other_attention_still_refuses_every_head_size_but_64():
    from igs_amd import _cabi
    L = _cabi.lib()
    s = (8 * 128 * 128, 128 * 128, 128)
    assert L.igs_attn_fwd(None, 1, 8, 128, 128, 128, F32, None, *s, None, *s, None, *s, 0.1, None, *s, None) == INVALID
    assert "D must be 64" in _cabi.last_error()
    assert L.igs_attn_bwd_scratch_bytes(1, 8, 128, 128, 128, F32) == 0


def test_scratch_stays_under_the_stated_bound():
    from igs_amd import _cabi
    L = _cabi.lib()
    for B, h, w, K in ((8, 64, 64, 2), (4, 64, 64, 2), (1, 1, 1, 1), (2, 6, 9, 3), (3, 24, 22, 2), (1, 4096, 4096, 1)):
        for dt in (F32, F16):
            n = L.igs_window_attn_bwd_scratch_bytes(B, h, w, K, 128, dt)
            assert 4 * B * h * w <= n <= 4 * B * h * w + 4 * h * w + 512, (B, h, w, K, n)


# ---------------------------------------------------------------- the built code objects
@pytest.fixture(scope="module")
def wattn_kernels():
    """{symbol: (metadata, instructions)} of every wattn_* kernel of libigs_rast.so."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from igs_amd import build
    build.build()
    import audit_barriers as A
    from test_geom_bwd_resources import kernel_metadata
    tmp, cos = A.code_objects(build.LIB)
    try:
        found = {}
        for co in cos:
            md = kernel_metadata(co)
            for name, insns in A.parse(co).items():
                if re.match(r"^_Z\d+wattn_\w+", name) and name in md:
                    found[name] = (md[name], insns)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def _is_half(name):
    assert ("IDF16_E" in name) != ("IfE" in name), name
    return "IDF16_E" in name


def test_wattn_kernels_have_no_scratch_and_fit_the_lds(wattn_kernels):
    kinds = sorted(re.match(r"^_Z\d+(wattn_[a-z_]+?)_kernel", n).group(1) for n in wattn_kernels)
    assert kinds == sorted(2 * ["wattn_fwd", "wattn_delta", "wattn_dkdv", "wattn_dq"]), kinds  # a float and a half instance of each
    for name, (md, _) in wattn_kernels.items():
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0 and int(md.get(".sgpr_spill_count", 0)) == 0, (name, "spills")
        assert int(md[".group_segment_fixed_size"]) <= 160 * 1024, (name, "LDS")               # (no kernel asks for dynamic LDS)
        print(name, "vgpr", md[".vgpr_count"], "agpr", md.get(".agpr_count"), "lds", md[".group_segment_fixed_size"])


def test_wattn_kernels_use_the_matrix_cores_of_their_dtype(wattn_kernels):
    for name, (_, insns) in wattn_kernels.items():
        mn = [m for _, m, _, _ in insns]
        f16_mfma = [m for m in mn if re.match(r"^v_mfma_f32_\w+_f16", m)]
        f32_mfma = [m for m in mn if re.match(r"^v_mfma_f32_\w+_f32", m)]
        matrix = "wattn_delta" not in name                        # (the row sums of d O * O are no matrix product)
        if _is_half(name):
            assert not matrix or f16_mfma, (name, "no v_mfma_f32_*_f16")
            assert not f32_mfma, name
            assert all(m.startswith("v_mfma_f32_32x32x16_f16") for m in f16_mfma), (name, set(f16_mfma))
        else:
            assert not matrix or f32_mfma, (name, "no v_mfma_f32_*_f32")
            assert all(m.startswith("v_mfma_f32_32x32x2_f32") for m in f32_mfma), (name, set(f32_mfma))
            assert not [m for m in mn if re.match(r"^v_mfma_\w+_(f16|bf16)", m)], (name, "a half matrix instruction in a float instance")
            assert not [m for m in mn if re.match(r"^v_cvt\w*f16", m)], (name, "a conversion to or from half in a float instance")
            assert not [m for m in mn if "f16" in m or "bf16" in m], (name, "a half instruction in a float instance")


# ---------------------------------------------------------------- the bounds
@pytest.mark.parametrize("case", [(10, 14, 2), (24, 22, 2), (32, 24, 2)])
def test_half_bound_accepts_the_half_pipeline_and_rejects_the_three_wrong_variants(case):
    """The float16 bound on the CPU emulation of the kernel's arithmetic, shifted: inside for the right pipeline, outside somewhere for the
    mask ignored, the roll's sign flipped and h / w swapped in the window arithmetic.  (Non-square maps: on a square one the swap is the
    identity.)"""
    h, w, K = case
    q, k, v = WR.random_inputs(2, h, w, torch.float16, "cpu", seed=h * w)
    r = WR.restate(q.double(), k.double(), v.double(), h, w, K, True)
    bound = WR.forward_bound(r, torch.float16, True)
    ratio = {var: ((WR.half_pipeline(q, k, v, h, w, K, True, var) - r["o"]).abs() / bound).max().item()
             for var in ("right", "no_mask", "roll_sign", "hw_swapped")}
    print(case, "max |err| / bound:", ratio, "max |scaled score| %.1f" % (r["s"] - r["mask"]).abs().max().item())
    assert ratio["right"] <= 1.0, ratio
    assert ratio["no_mask"] > 1.0 and ratio["roll_sign"] > 1.0 and ratio["hw_swapped"] > 1.0, ratio
    plain = WR.restate(q.double(), k.double(), v.double(), h, w, K, False)
    assert ((WR.half_pipeline(q, k, v, h, w, K, False) - plain["o"]).abs() <= WR.forward_bound(plain, torch.float16, False)).all()


def test_float_bound_accepts_pytorch_float32_and_is_tighter_than_half():
    h, w, K = 24, 22, 2
    q, k, v = WR.random_inputs(1, h, w, torch.float32, "cpu", seed=7)
    r = WR.restate(q.double(), k.double(), v.double(), h, w, K, True)
    b32, b16 = WR.forward_bound(r, torch.float32, True), WR.forward_bound(r, torch.float16, True)
    o32 = WR.restate(q, k, v, h, w, K, True)["o"]
    assert ((o32.double() - r["o"]).abs() <= b32).all()
    assert (b32 < b16).all()


# ---------------------------------------------------------------- the Python layer
def test_window_attention_refusals_on_the_cpu():
    from igs_amd import attention as AT
    q, k, v = WR.random_inputs(1, 8, 8, torch.float32, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        AT.window_attention(q, k, v, 8, 8, 2, True)
    with pytest.raises(RuntimeError, match="GPU"):
        AT.single_head_full_attention(q, k, v)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError):
            AT.window_attention(q.to(dt), k.to(dt), v.to(dt), 8, 8)
    with pytest.raises(NotImplementedError):
        AT.window_attention(q, k.half(), v, 8, 8)
    with pytest.raises(NotImplementedError, match="channel count"):
        AT.window_attention(q[..., :64], k[..., :64], v[..., :64], 8, 8)
    with pytest.raises(ValueError):
        AT.window_attention(q[0], k[0], v[0], 8, 8)
    with pytest.raises(ValueError):
        AT.window_attention(q, k, v[:, :32], 8, 8)
    with pytest.raises(ValueError, match="token count"):
        AT.window_attention(q, k, v, 8, 9)
    with pytest.raises(ValueError, match="split"):
        AT.window_attention(q, k, v, 8, 8, 3)
    with pytest.raises(ValueError, match="2 x 2"):
        AT.window_attention(q, k, v, 8, 8, 8, True)


def test_drop_in_signatures_and_the_attn_mask_rule():
    from igs_amd import attention as AT
    assert list(inspect.signature(AT.single_head_split_window_attention).parameters) == ["q", "k", "v", "num_splits", "with_shift", "h", "w", "attn_mask"]
    d = {n: p.default for n, p in inspect.signature(AT.single_head_split_window_attention).parameters.items()}
    assert (d["num_splits"], d["with_shift"], d["h"], d["w"], d["attn_mask"]) == (1, False, None, None, None)
    assert list(inspect.signature(AT.single_head_full_attention).parameters) == ["q", "k", "v"]
    assert list(inspect.signature(AT.window_attention).parameters) == ["q", "k", "v", "h", "w", "num_splits", "with_shift", "scale"]
    q, k, v = WR.random_inputs(1, 8, 8, torch.float32, "cpu")
    with pytest.raises(ValueError, match="h and w"):
        AT.single_head_split_window_attention(q, k, v, num_splits=2)
    with pytest.raises(ValueError, match="attn_mask"):
        AT.single_head_split_window_attention(q, k, v, num_splits=2, with_shift=True, h=8, w=8)
    with pytest.raises(ValueError, match="attn_mask must have shape"):
        AT.single_head_split_window_attention(q, k, v, num_splits=2, with_shift=True, h=8, w=8, attn_mask=torch.zeros(4, 16, 15))
    with pytest.raises(RuntimeError, match="GPU"):               # a mask of the right shape: only the device is wrong
        AT.single_head_split_window_attention(q, k, v, num_splits=2, with_shift=True, h=8, w=8, attn_mask=torch.zeros(4, 16, 16))
    assert "NOT READ" in AT.single_head_split_window_attention.__doc__


def test_use_native_window_attention_patches_a_namespace():
    from igs_amd import attention as AT
    ns = types.SimpleNamespace(single_head_full_attention=WR.restated_full, single_head_split_window_attention=WR.restated_split, other=1)
    assert AT.use_native_window_attention(ns) == 2
    assert ns.single_head_full_attention is AT.single_head_full_attention
    assert ns.single_head_split_window_attention is AT.single_head_split_window_attention and ns.other == 1
    half = types.SimpleNamespace(single_head_full_attention=WR.restated_full)
    assert AT.use_native_window_attention(half) == 1 and not hasattr(half, "single_head_split_window_attention")
    assert AT.use_native_window_attention(types.SimpleNamespace()) == 0
