"""The fused attention (igs_amd/csrc/attn.hip, igs_amd/attention.py) without a GPU: exports and argument counts, the refusals of the C ABI
before any HIP call, the scratch bound, the residency and the instruction mix of the built gfx950 kernels, the float64 restatement against
PyTorch's own attention, and the refusals of the Python layer."""
import os
import re
import shutil
import sys

import pytest
import torch
import torch.nn.functional as F

import attention_restatement as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_attn_fwd", "igs_attn_bwd", "igs_attn_bwd_scratch_bytes")
INVALID = -1
F32, F16 = 0, 1


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
    assert "attn.hip" in build.SOURCES
    m = _cabi.ext()
    assert hasattr(m, "attn_fwd") and hasattr(m, "attn_bwd")


def _fwd(L, B=1, H=8, Aq=128, Ak=128, D=64, dt=F32, q=None, strides=None, kv=None, out=None, ostrides=None, scale=0.125):
    s = strides or (H * Aq * D, Aq * D, D)
    sk = (H * Ak * D, Ak * D, D)
    so = ostrides or (H * Aq * D, Aq * D, D)
    return L.igs_attn_fwd(None, B, H, Aq, Ak, D, dt, q, *s, kv, *sk, kv, *sk, scale, out, *so, None)


def _bwd(L, B=1, H=8, Aq=128, Ak=128, D=64, dt=F32, strides=None, dq=None, ostrides=None, scale=0.125, rest=None):
    s = strides or (H * Aq * D, Aq * D, D)
    sk = (H * Ak * D, Ak * D, D)
    so = (H * Aq * D, Aq * D, D)
    return L.igs_attn_bwd(None, B, H, Aq, Ak, D, dt, rest, *s, rest, *sk, rest, *sk, rest, *so, rest, rest, *so, scale, dq, *(ostrides or so),
                          None, *sk, None, *sk, rest)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """NULL device pointers throughout and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    L = _cabi.lib()
    fake = 0x1000                                                # a non-NULL, 16-byte aligned address that is never dereferenced
    for call in (_fwd, _bwd):
        for kw, word in ((dict(D=32), "D must be 64"), (dict(Ak=0), "Ak out of range"), (dict(Aq=0), "Aq out of range"),
                         (dict(dt=7), "dtype"), (dict(H=0), "H out of range"), (dict(B=-1), "B out of range"),
                         (dict(strides=(8 * 128 * 64, 128 * 64, 66)), "16 bytes"), (dict(strides=(8 * 128 * 64, -64, 64)), "negative"),
                         (dict(dt=F16, strides=(8 * 128 * 64, 128 * 64 + 4, 64)), "16 bytes")):
            assert call(L, **kw) == INVALID, (call.__name__, kw)
            assert word in _cabi.last_error() and call.__name__.strip("_") in _cabi.last_error(), (kw, _cabi.last_error())
    assert _fwd(L) == INVALID and "NULL" in _cabi.last_error()                              # NULL q with everything else in order
    assert _fwd(L, q=fake) == INVALID and "NULL" in _cabi.last_error()                      # ... and NULL k, v, out
    assert _bwd(L, dq=fake) == INVALID and "NULL" in _cabi.last_error()
    # a base pointer off the 16-byte grid, a scale that is not finite, an output whose rows alias (stride 0 or below D)
    assert _fwd(L, q=fake + 4, kv=fake, out=fake) == INVALID and "16-byte aligned" in _cabi.last_error()
    assert _fwd(L, q=fake, kv=fake, out=fake + 8) == INVALID and "16-byte aligned" in _cabi.last_error()
    assert _bwd(L, dq=fake + 4, rest=fake) == INVALID and "16-byte aligned" in _cabi.last_error()
    for bad in (float("inf"), float("nan")):
        assert _fwd(L, q=fake, kv=fake, out=fake, scale=bad) == INVALID and "finite" in _cabi.last_error()
        assert _bwd(L, dq=fake, rest=fake, scale=bad) == INVALID and "finite" in _cabi.last_error()
    for so in ((8 * 128 * 64, 128 * 64, 0), (8 * 128 * 64, 0, 64), (8 * 128 * 64, 128 * 64, 32)):
        assert _fwd(L, q=fake, kv=fake, out=fake, ostrides=so) == INVALID and "overlap" in _cabi.last_error(), so
        assert _bwd(L, dq=fake, rest=fake, ostrides=so) == INVALID and "overlap" in _cabi.last_error(), so
    assert _fwd(L, B=2, q=fake, kv=fake, out=fake, ostrides=(0, 128 * 64, 64)) == INVALID and "overlap" in _cabi.last_error()
    assert _fwd(L, B=0) == 0 and _bwd(L, B=0) == 0                                          # nothing to do
    assert _bwd(L) == 0                                                                     # no gradient wanted: nothing to do
    assert L.igs_attn_bwd_scratch_bytes(1, 8, 128, 128, 32, F32) == 0


def test_scratch_stays_under_the_stated_bound():
    from igs_amd import _cabi
    L = _cabi.lib()
    for B, H, Aq, Ak in ((5, 8, 8192, 8192), (1, 8, 8192, 8192), (1, 1, 1, 1), (2, 3, 1000, 257)):
        for dt in (F32, F16):
            n = L.igs_attn_bwd_scratch_bytes(B, H, Aq, Ak, 64, dt)
            assert 4 * B * H * Aq <= n <= 4 * B * H * Aq * (64 + 2) + 8 * B * H * Ak * 64 + 4096, (B, H, Aq, Ak, n)
            assert n <= 4 * B * H * Aq + 512                       # (what the header promises: nothing of size A x A, no per-tile partials)


# ---------------------------------------------------------------- the built code objects
@pytest.fixture(scope="module")
def attn_kernels():
    """{symbol: (metadata, instructions)} of every attn_* kernel of libigs_rast.so."""
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
                if re.match(r"^_Z\d+attn_\w+", name) and name in md:
                    found[name] = (md[name], insns)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def _is_half(name):
    assert ("IDF16_E" in name) != ("IfE" in name), name
    return "IDF16_E" in name


def test_attn_kernels_have_no_scratch_and_fit_the_lds(attn_kernels):
    kinds = sorted(re.match(r"^_Z\d+(attn_[a-z_]+?)_kernel", n).group(1) for n in attn_kernels)
    assert kinds == sorted(2 * ["attn_fwd", "attn_delta", "attn_dkdv", "attn_dq"]), kinds      # a float and a half instance of each
    for name, (md, _) in attn_kernels.items():
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md[".group_segment_fixed_size"]) <= 160 * 1024, (name, "LDS")               # (no kernel asks for dynamic LDS)
        print(name, "vgpr", md[".vgpr_count"], "agpr", md.get(".agpr_count"), "lds", md[".group_segment_fixed_size"])


def test_attn_kernels_use_the_matrix_cores_of_their_dtype(attn_kernels):
    for name, (_, insns) in attn_kernels.items():
        mn = [m for _, m, _, _ in insns]
        f16_mfma = [m for m in mn if re.match(r"^v_mfma_f32_\w+_f16", m)]
        f32_mfma = [m for m in mn if re.match(r"^v_mfma_f32_\w+_f32", m)]
        matrix = "attn_delta" not in name                         # (the row sums of d O * O are no matrix product)
        if _is_half(name):
            assert not matrix or f16_mfma, (name, "no v_mfma_f32_*_f16")
            assert not f32_mfma, name
        else:
            assert not matrix or f32_mfma, (name, "no v_mfma_f32_*_f32")
            assert not [m for m in mn if re.match(r"^v_mfma_\w+_(f16|bf16)", m)], (name, "a half matrix instruction in a float instance")
            assert not [m for m in mn if re.match(r"^v_cvt\w*f16", m)], (name, "a conversion to or from half in a float instance")
            assert not [m for m in mn if "f16" in m or "bf16" in m], (name, "a half instruction in a float instance")


# ---------------------------------------------------------------- the restatement
def test_restatement_equals_pytorch_attention_in_float64():
    q, k, v, g = AR.random_inputs(2, 3, 77, 130, torch.float64, "cpu", seed=3, with_dout=True)
    r = AR.restate(q, k, v, 0.125)
    ref = F.scaled_dot_product_attention(q, k, v, scale=0.125)
    assert (r["o"] - ref).abs().max() <= 1e-13 * (1 + ref.abs().max())
    assert (r["lse"] - torch.logsumexp(torch.matmul(q, k.transpose(-1, -2)) * 0.125, -1)).abs().max() <= 1e-12
    # the two statements of the backward agree, and agree with autograd through PyTorch's attention
    ga = AR.gradients(q, k, v, 0.125, g)
    ge = AR.explicit_gradients(q, k, v, 0.125, g)
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    gp = torch.autograd.grad(F.scaled_dot_product_attention(qq, kk, vv, scale=0.125), (qq, kk, vv), g)
    for a, e, p in zip(ga, (ge["dq"], ge["dk"], ge["dv"]), gp):
        assert (a - e).abs().max() <= 1e-12 * (1 + a.abs().max()) and (a - p).abs().max() <= 1e-12 * (1 + a.abs().max())


def test_half_bound_accepts_the_half_pipeline_and_rejects_both_wrong_variants():
    """The float16 bound on the CPU emulation of the kernel's arithmetic: inside for the right pipeline, outside somewhere for the softmax
    scale 1 / D and for scores rounded to half before the softmax."""
    for Aq, Ak in ((257, 1000), (1024, 1024)):
        q, k, v = AR.random_inputs(1, 1, Aq, Ak, torch.float16, "cpu", seed=Aq)
        q64, k64, v64 = q.double(), k.double(), v.double()
        r = AR.restate(q64, k64, v64, 0.125)
        bound = AR.forward_bound(q64, k64, v64, 0.125, torch.float16, r)
        ratio = {var: ((AR.half_pipeline(q, k, v, 0.125, var) - r["o"]).abs() / bound).max().item() for var in ("right", "scale_1_over_D", "half_scores")}
        print((Aq, Ak), "max |err| / bound:", ratio, "max |scaled score| %.1f" % r["s"].abs().max().item())
        assert ratio["right"] <= 1.0 and ratio["scale_1_over_D"] > 1.0 and ratio["half_scores"] > 1.0, ratio


# ---------------------------------------------------------------- the Python layer
def test_sdpa_refusals_on_the_cpu():
    from igs_amd import attention as AT
    q, k, v = AR.random_inputs(1, 2, 16, 16, torch.float32, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        AT.sdpa(q, k, v)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(NotImplementedError):
            AT.sdpa(q.to(dt), k.to(dt), v.to(dt))
    with pytest.raises(NotImplementedError):
        AT.sdpa(q, k.half(), v)
    with pytest.raises(NotImplementedError, match="head size"):
        AT.sdpa(q[..., :32], k[..., :32], v[..., :32])
    with pytest.raises(ValueError):
        AT.sdpa(q[0], k[0], v[0])
    with pytest.raises(ValueError):
        AT.sdpa(q, k, v[:, :, :8])
    with pytest.raises(ValueError):
        AT.sdpa(q, k[:, :1], v[:, :1])
    with pytest.raises(ValueError):
        AT.sdpa(q, k, v, layout="abhd")


def test_processor_refusals_and_cpu_tensors():
    from igs_amd import attention as AT
    proc = AT.AnchorAttnProcessor()
    x = torch.randn(2, 16, 512)
    with pytest.raises(RuntimeError, match="GPU"):
        proc(AR.AttentionStandIn(), x)
    with pytest.raises(NotImplementedError, match="mask"):
        proc(AR.AttentionStandIn(), x, attention_mask=torch.zeros(2, 1, 16))
    with pytest.raises(NotImplementedError, match="4-D"):
        proc(AR.AttentionStandIn(), x.view(2, 512, 4, 4))
    m = AR.AttentionStandIn()
    m.norm_cross = torch.nn.LayerNorm(512)
    with pytest.raises(NotImplementedError, match="norm_cross"):
        proc(m, x, encoder_hidden_states=x)
    for name, value in (("group_norm", torch.nn.GroupNorm(4, 512)), ("spatial_norm", torch.nn.Identity()), ("residual_connection", True),
                        ("rescale_output_factor", 2.0)):
        m = AR.AttentionStandIn()
        setattr(m, name, value)
        with pytest.raises(NotImplementedError, match=name):
            proc(m, x)
    m = AR.AttentionStandIn(dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        proc(m.train(), x)
    with pytest.raises(RuntimeError, match="GPU"):                 # in eval mode the dropout is the identity: only the device is wrong
        proc(m.eval(), x)


def test_use_native_attention_installs_the_processor():
    from igs_amd import attention as AT
    net = torch.nn.Sequential(AR.AttentionStandIn(), torch.nn.Linear(4, 4), torch.nn.Sequential(AR.AttentionStandIn(seed=1)))
    assert AT.use_native_attention(net) == 2
    assert isinstance(net[0].processor, AT.AnchorAttnProcessor) and isinstance(net[2][0].processor, AT.AnchorAttnProcessor)
    assert AT.use_native_attention(torch.nn.Linear(4, 4)) == 0
