"""The transformers' LayerNorm and GEGLU (igs_amd/csrc/tokens.hip, igs_amd/tokens.py) without a GPU: the float64 restatement and the
stand-in modules against the reference-produced golden file, exports and argument counts, the refusals of the C ABI before any HIP call and
of the Python layer, the registers and scratch of the built gfx950 kernels, the derived allowances on a float32 emulation of the kernels'
arithmetic, on CPU PyTorch float32 and on three wrong variants per operation, and the two installers on the stand-ins."""
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import token_ops_restatement as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_layer_norm_fwd", "igs_layer_norm_bwd_scratch_bytes", "igs_layer_norm_bwd", "igs_geglu_fwd", "igs_geglu_bwd")
INVALID = -1
F32, F16 = 0, 1
B, H, W, K, DIM = 2, 4, 6, 2, 16                                     # the golden cases (tests/golden/make_token_ops_golden.py)


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_token_ops.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _replay(golden, tag, module, call):
    """The stand-in with the stored parameters on the stored inputs: output and every gradient within 1e-12 of the reference's."""
    module = module.double()
    params = {k[len(tag + "param."):]: v for k, v in golden.items() if k.startswith(tag + "param.")}
    assert sorted(params) == sorted(module.state_dict().keys()), (tag, sorted(params))
    module.load_state_dict(params)
    inputs = {k[len(tag + "in."):]: v.clone().requires_grad_(True) for k, v in golden.items() if k.startswith(tag + "in.")}
    out = call(module, inputs)
    assert out.dtype == torch.float64 and (out - golden[tag + "out"]).abs().max() <= 1e-12, tag
    named = dict(module.named_parameters())
    grads = torch.autograd.grad(out, list(inputs.values()) + list(named.values()), golden[tag + "gout"])
    for name, g in zip(list(inputs), grads):
        assert (g - golden[tag + "grad_in." + name]).abs().max() <= 1e-12, (tag, name)
    for name, g in zip(list(named), grads[len(inputs):]):
        assert (g - golden[tag + "grad_param." + name]).abs().max() <= 1e-12, (tag, name)
    return out


@pytest.mark.parametrize("ffn", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
def test_stand_in_layer_equals_the_reference_layer(golden, ffn, shift):
    tag = "layer_ffn%d_shift%d." % (ffn, shift)
    assert golden[tag + "in.source"].shape == (B, H * W, DIM) and golden[tag + "in.source"].dtype == torch.float64
    mask = torch.zeros(K * K, (H // K) * (W // K), (H // K) * (W // K), dtype=torch.float64)      # (its values are regenerated)
    _replay(golden, tag, TR.TransformerLayer(d_model=DIM, no_ffn=not ffn),
            lambda m, i: m(i["source"], i["target"], height=H, width=W, shifted_window_attn_mask=mask, with_shift=bool(shift), attn_num_splits=K))


def test_stand_in_block_equals_the_reference_block(golden):
    assert golden["block.in.hidden_states"].shape == (2, 10, DIM)
    _replay(golden, "block.", TR.BasicTransformerBlock(DIM, TR.LinearAttention(DIM)), lambda m, i: m(i["hidden_states"]))


def test_restated_operations_equal_pytorch_float64_and_the_golden_tails(golden):
    g = torch.Generator().manual_seed(3)
    x, res, dout = (torch.randn(7, 12, generator=g, dtype=torch.float64) * 3 + 1 for _ in range(3))
    w, b = (torch.randn(12, generator=g, dtype=torch.float64) for _ in range(2))
    assert (TR.layer_norm_restate(x, w, b, 1e-5, res) - (res + F.layer_norm(x, (12,), w, b, 1e-5))).abs().max() <= 1e-12
    assert (TR.layer_norm_restate(x, None, None, 1e-5) - F.layer_norm(x, (12,), None, None, 1e-5)).abs().max() <= 1e-12
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    want = torch.autograd.grad(F.layer_norm(leaves[0], (12,), leaves[1], leaves[2], 1e-5), leaves, dout)
    for got, ref in zip(TR.layer_norm_backward_restate(x, w, 1e-5, dout), want):
        assert (got - ref).abs().max() <= 1e-12
    p = torch.randn(5, 16, generator=g, dtype=torch.float64) * 2
    h, gate = p.chunk(2, dim=-1)
    assert (TR.geglu_restate(p) - h * F.gelu(gate)).abs().max() <= 1e-12
    leaf = p.clone().requires_grad_(True)
    hh, gg = leaf.chunk(2, dim=-1)
    (dp,) = torch.autograd.grad(hh * F.gelu(gg), leaf, dout[:5, :8])
    assert (TR.geglu_backward_restate(p, dout[:5, :8]) - dp).abs().max() <= 1e-12
    # the tail of the golden no-FFN layer is source + LN1(.): the restated LayerNorm with a residual, on the reference's own numbers
    tag = "layer_ffn0_shift1."
    layer = TR.TransformerLayer(d_model=DIM, no_ffn=True).double()
    layer.load_state_dict({k[len(tag + "param."):]: v for k, v in golden.items() if k.startswith(tag + "param.")})
    src, tgt = golden[tag + "in.source"], golden[tag + "in.target"]
    with torch.no_grad():
        msg = layer.merge(TR.single_head_split_window_attention(layer.q_proj(src), layer.k_proj(tgt), layer.v_proj(tgt), num_splits=K, with_shift=True,
                                                                h=H, w=W))
        tail = TR.layer_norm_restate(msg.view(-1, DIM), layer.norm1.weight, layer.norm1.bias, layer.norm1.eps, src.view(-1, DIM))
    assert (tail.view_as(src) - golden[tag + "out"]).abs().max() <= 1e-12


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
    assert "tokens.hip" in build.SOURCES
    m = _cabi.ext()
    for f in ("layer_norm_fwd", "layer_norm_bwd", "geglu_fwd", "geglu_bwd"):
        assert hasattr(m._tokens, f), f                                                          # (a private submodule of _C)
    from igs_amd import tokens as TK
    assert re.search(r"#define IGS_LN_MAX_C %d\b" % TK.LN_MAX_C, hdr) and TK.LN_MAX_C >= 1024
    assert re.search(r"#define IGS_GEGLU_MAX_D %d\b" % TK.GEGLU_MAX_D, hdr) and TK.GEGLU_MAX_D == 8192


X, RES, OUT, WGT, BIAS, DOUT, DX, DW, DB, SCR = 0x1000000, 0x3000000, 0x5000000, 0x7000000, 0x7100000, 0x9000000, 0xB000000, 0xD000000, 0xD100000, 0xF000000


def _fwd(L, N=3, C=512, xdt=F32, x=X, xs=None, rdt=F32, res=None, rs=None, w=WGT, b=BIAS, eps=1e-5, odt=F32, out=OUT, os_=None):
    return L.igs_layer_norm_fwd(None, N, C, xdt, x, C if xs is None else xs, rdt, res, C if rs is None else rs, w, b, eps, odt, out, C if os_ is None else os_)


def _bwd(L, N=3, C=512, xdt=F32, x=X, xs=None, w=WGT, eps=1e-5, gdt=F32, g=DOUT, gs=None, ddt=F32, dx=DX, dxs=None, dw=DW, db=DB, scr=SCR):
    return L.igs_layer_norm_bwd(None, N, C, xdt, x, C if xs is None else xs, w, eps, gdt, g, C if gs is None else gs, ddt, dx, C if dxs is None else dxs,
                                dw, db, scr)


def _gf(L, N=3, D=8, dt=F32, p=X, ps=None, out=OUT):
    return L.igs_geglu_fwd(None, N, D, dt, p, 2 * D if ps is None else ps, out)


def _gb(L, N=3, D=8, dt=F32, p=X, ps=None, dout=DOUT, dp=DX):
    return L.igs_geglu_bwd(None, N, D, dt, p, 2 * D if ps is None else ps, dout, dp)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    from igs_amd import tokens as TK
    L = _cabi.lib()

    def refused(call, name, cases):
        for kw, word in cases:
            assert call(L, **kw) == INVALID, (name, kw)
            assert word in _cabi.last_error() and name in _cabi.last_error(), (kw, _cabi.last_error())

    sizes = [(dict(C=0), "C out of range"), (dict(C=-3), "C out of range"), (dict(C=TK.LN_MAX_C + 1), "C out of range"), (dict(N=-1), "N out of range"),
             (dict(N=(1 << 24) + 1), "N out of range")]
    eps = [(dict(eps=-1e-5), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps")]
    refused(_fwd, "igs_layer_norm_fwd", sizes + eps + [
        (dict(xdt=2), "dtype"), (dict(odt=-1), "dtype"), (dict(res=RES, rdt=7), "dtype"),
        (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(b=None), "weight and bias go together"), (dict(w=None), "weight and bias go together"),
        (dict(x=X + 2), "aligned to its element size"), (dict(xdt=F16, x=X + 1), "aligned to its element size"), (dict(out=OUT + 1), "aligned"),
        (dict(res=RES + 3), "aligned"), (dict(w=WGT + 2), "aligned"), (dict(b=BIAS + 1), "aligned"),
        (dict(xs=511), "row stride"), (dict(os_=100), "row stride"), (dict(res=RES, rs=0), "row stride"), (dict(xs=-512), "row stride"),
        (dict(xs=(1 << 31) + 4), "row stride"),
        (dict(out=X), "out overlaps x"), (dict(out=X + 512 * 4), "out overlaps x"), (dict(x=X, xs=1024, out=X + 2048, os_=1024), "out overlaps x"),
        (dict(res=RES, out=RES + 16), "without being res"), (dict(res=RES, out=RES, os_=1024), "without being res"),
        (dict(res=RES, rdt=F16, out=RES), "without being res"), (dict(out=WGT - 4 * 512 * 3 + 8), "overlaps weight or bias"),
        (dict(out=BIAS), "overlaps weight or bias")])
    assert _fwd(L, N=0) == 0 and _fwd(L, N=0, x=None, out=None) == 0                            # nothing to do
    assert _fwd(L, N=0, C=0) == INVALID and _fwd(L, N=0, eps=-1.0) == INVALID                   # ... but the arguments are still checked
    refused(_bwd, "igs_layer_norm_bwd", sizes + eps + [
        (dict(xdt=3), "dtype"), (dict(gdt=2), "dtype"), (dict(ddt=-1), "dtype"), (dict(x=None), "NULL"), (dict(g=None), "NULL"),
        (dict(scr=None), "scratch is required"), (dict(dx=None, dw=None, scr=None), "scratch is required"),
        (dict(x=X + 1), "aligned"), (dict(g=DOUT + 2), "aligned"), (dict(ddt=F16, dx=DX + 1), "aligned"), (dict(dw=DW + 2), "aligned"),
        (dict(db=DB + 1), "aligned"), (dict(w=WGT + 1), "aligned"),
        (dict(xs=10), "row stride"), (dict(gs=511), "row stride"), (dict(dxs=0), "row stride"),
        (dict(dx=X), "overlaps x, dout or weight"), (dict(dx=DOUT + 64), "overlaps x, dout or weight"), (dict(dw=WGT), "overlaps x, dout or weight"),
        (dict(db=X + 40), "overlaps x, dout or weight"), (dict(scr=DOUT), "overlaps x, dout or weight"),
        (dict(dw=DX + 16), "overlap one another"), (dict(db=DW + 4), "overlap one another"), (dict(scr=DX + 256), "overlap one another"),
        (dict(scr=DB - 64), "overlap one another")])
    assert _bwd(L, N=0) == 0 and _bwd(L, dx=None, dw=None, db=None, x=None, g=None) == 0        # nothing to do
    assert _bwd(L, N=0, C=0) == INVALID
    assert L.igs_layer_norm_bwd_scratch_bytes(8192, 512) > 0 and L.igs_layer_norm_bwd_scratch_bytes(1, 4) > 0
    for n, c in ((-1, 512), ((1 << 24) + 1, 512), (8, 0), (8, TK.LN_MAX_C + 1)):
        assert L.igs_layer_norm_bwd_scratch_bytes(n, c) == 0, (n, c)
    geglu = [(dict(D=0), "D out of range"), (dict(D=8193), "D out of range"), (dict(N=-1), "N out of range"), (dict(N=(1 << 27) + 1), "N out of range"),
             (dict(N=1 << 62, D=8192), "N out of range"), (dict(N=(1 << 63) - 1, D=2), "N out of range"),      # (N * D would wrap)
             (dict(N=1 << 20, D=2048), "N out of range"), (dict(dt=2), "dtype"), (dict(dt=-1), "dtype"), (dict(p=None), "NULL"),
             (dict(ps=15), "row stride"), (dict(ps=0), "row stride"), (dict(ps=(1 << 31) + 2), "row stride"), (dict(p=X + 2), "aligned"),
             (dict(dt=F16, p=X + 1), "aligned")]
    refused(_gf, "igs_geglu_fwd", geglu + [(dict(out=None), "NULL"), (dict(out=OUT + 1), "aligned"), (dict(out=X + 8), "out overlaps p"),
                                           (dict(p=X, ps=64, out=X + 64), "out overlaps p")])
    refused(_gb, "igs_geglu_bwd", geglu + [(dict(dout=None), "NULL"), (dict(dp=None), "NULL"), (dict(dout=DOUT + 2), "aligned"), (dict(dp=DX + 1), "aligned"),
                                           (dict(dp=X + 4), "dp overlaps p or dout"), (dict(dp=DOUT - 8), "dp overlaps p or dout")])
    assert _gf(L, N=0) == 0 and _gb(L, N=0) == 0 and _gf(L, N=0, p=None, out=None) == 0
    assert _gf(L, N=0, D=0) == INVALID


# ---------------------------------------------------------------- the built code objects
@pytest.fixture(scope="module")
def token_kernels():
    """{symbol: metadata} of every kernel of tokens.hip in libigs_rast.so."""
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
            for name, md in kernel_metadata(co).items():
                if re.match(r"^_ZL?\d+(ln_\w+_kernel|geglu_\w+_kernel|param_reduce_kernel)", name):      # (param_reduce.h: static, one copy per file)
                    found[name] = md
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_kernels_have_no_scratch_no_spills_and_the_budgeted_registers(token_kernels):
    """every kernel without scratch or spills; the shapes of the two shipped widths (16 lanes x 2 groups for C = 128,
    64 x 2 for C = 512), every forward and every GEGLU kernel at 8 waves per SIMD (<= 64 registers); the other backward shapes at 4 (<= 128)."""
    k = token_kernels
    assert len([n for n in k if "ln_fwd_kernel" in n]) == 10 and len([n for n in k if "ln_bwd_kernel" in n]) == 10, sorted(k)
    assert len([n for n in k if "geglu_fwd_kernel" in n]) == 4 and len([n for n in k if "geglu_bwd_kernel" in n]) == 4
    assert len([n for n in k if "param_reduce_kernel" in n]) == 1
    for name, md in k.items():
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0 and int(md.get(".sgpr_spill_count", 0)) == 0, (name, "spills")
        regs = (int(md[".vgpr_count"]) + int(md.get(".agpr_count", 0)) + 7) // 8 * 8
        print(name, "vgpr", md[".vgpr_count"], "lds", md[".group_segment_fixed_size"])
        assert regs <= 256, (name, regs)
        shape = re.search(r"ILi(\d+)ELi(\d+)ELb([01])E", name)
        if "geglu" in name or "reduce" in name:
            assert regs <= 64, (name, regs)
        elif shape.group(3) == "1" and (shape.group(1), shape.group(2)) in (("16", "2"), ("64", "2")):
            assert regs <= 64, (name, regs)
        elif "ln_fwd" in name:
            assert regs <= 64, (name, regs)
        else:
            assert regs <= 128, (name, regs)
        assert int(md[".max_flat_workgroup_size"]) in (256, 1024), name


# ---------------------------------------------------------------- the allowances
def _ln_ratio(y, x, w=None, b=None, eps=1e-5):
    ref = TR.layer_norm_restate(x.double(), None if w is None else w.double(), None if b is None else b.double(), eps)
    return ((y.double() - ref).abs() / TR.layer_norm_forward_bound(x, w, b, eps)).max().item()


@pytest.mark.parametrize("C", [4, 12, 128, 132, 512, 1024] + [64, 68, 256, 260, 516] + [1, 63, 65, 129, 257, 513, 1023])   # (every width of LN_CASES)
def test_layer_norm_allowance_accepts_the_kernel_arithmetic_and_pytorch_float32(C):
    """On the GPU tests' inputs (every pair of mean and std): the float32 emulation of the kernel's arithmetic and PyTorch's own float32
    layer_norm on the CPU, forward and backward, stay inside the allowance."""
    x = TR.row_inputs(9, C, torch.float32, "cpu", seed=3)
    w, b = TR.affine_inputs(C, "cpu", seed=C)
    r_emul = _ln_ratio(TR.layer_norm_emulate(x), x)
    r_torch = _ln_ratio(F.layer_norm(x, (C,), w, b, 1e-5), x, w, b)
    g = torch.randn(9, C, generator=torch.Generator().manual_seed(C))
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    got = torch.autograd.grad(F.layer_norm(leaves[0], (C,), leaves[1], leaves[2], 1e-5), leaves, g)
    want = TR.layer_norm_backward_restate(x.double(), w.double(), 1e-5, g.double())
    bounds = TR.layer_norm_backward_bounds(x, w, 1e-5, g)
    r_bwd = [((a.double() - r).abs() / bounds[k]).max().item() for a, r, k in zip(got, want, ("dx", "dweight", "dbias"))]
    print(C, "max |err| / allowance: emulation %.3f, F.layer_norm float32 %.3f, its backward %s" % (r_emul, r_torch, ["%.3f" % r for r in r_bwd]))
    assert r_emul <= 1.0 and r_torch <= 1.0 and max(r_bwd) <= 1.0, (r_emul, r_torch, r_bwd)
    const = torch.full((1, C), 100.37, dtype=torch.float32)
    assert (TR.layer_norm_emulate(const) == 0).all()                                          # a constant row: exactly zero, so exactly bias


def test_layer_norm_allowance_rejects_three_wrong_variants():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4, 128, generator=g, dtype=torch.float64) + 1e3).float()                # mean 1e3, std 1: E[x^2] - mean^2 cancels
    r = {"right": _ln_ratio(TR.layer_norm_emulate(x), x), "one_pass": _ln_ratio(TR.layer_norm_emulate(x, variant="one_pass"), x)}
    y = torch.randn(16, 4, generator=g, dtype=torch.float64).float()                         # C = 4: C - 1 instead of C is 13 % of rstd
    r["unbiased"] = _ln_ratio(TR.layer_norm_emulate(y, variant="unbiased"), y)
    assert _ln_ratio(TR.layer_norm_emulate(y), y) <= 1.0
    z = (torch.randn(4, 128, generator=g, dtype=torch.float64) * 1e-3).float()               # std 1e-3: var = 1e-6 against eps = 1e-5
    r["no_eps"] = _ln_ratio(TR.layer_norm_emulate(z, variant="no_eps"), z)
    assert _ln_ratio(TR.layer_norm_emulate(z), z) <= 1.0
    print("max |err| / allowance:", r)
    assert r["right"] <= 1.0, r
    assert r["one_pass"] > 1.0 and r["unbiased"] > 1.0 and r["no_eps"] > 1.0, r


def _geglu_ratio(y, p):
    return ((y.double() - TR.geglu_restate(p.double())).abs() / TR.geglu_forward_allowance(p)).max().item()


@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_geglu_allowance_accepts_float32_and_rejects_three_wrong_variants(scale):
    p = TR.geglu_inputs(67, 48, torch.float32, "cpu", seed=int(scale), scale=scale)
    h, gate = p.chunk(2, dim=-1)
    r = {v: _geglu_ratio(TR.geglu_emulate(p, v), p) for v in ("right", "tanh", "sigmoid", "swapped")}
    r["torch"] = _geglu_ratio(h * F.gelu(gate), p)
    dout = torch.randn(67, 48, generator=torch.Generator().manual_seed(9))
    leaf = p.clone().requires_grad_(True)
    hh, gg = leaf.chunk(2, dim=-1)
    (dp,) = torch.autograd.grad(hh * F.gelu(gg), leaf, dout)
    r["torch_bwd"] = ((dp.double() - TR.geglu_backward_restate(p.double(), dout.double())).abs() / TR.geglu_backward_allowance(p, dout)).max().item()
    print("scale", scale, "max |err| / allowance:", {k: round(v, 3) for k, v in r.items()})
    assert r["right"] <= 1.0 and r["torch"] <= 1.0 and r["torch_bwd"] <= 1.0, r
    assert r["tanh"] > 1.0 and r["sigmoid"] > 1.0 and r["swapped"] > 1.0, r


# ---------------------------------------------------------------- the Python layer
def test_python_refusals_on_the_cpu():
    from igs_amd import tokens as TK
    x, w, b = torch.randn(2, 5, 16), torch.ones(16), torch.zeros(16)
    for call in (lambda t: TK.layer_norm(t, w, b), lambda t: TK.layer_norm(t, None, None, residual=t.clone()), lambda t: TK.geglu(t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x)
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(NotImplementedError):
                call(x.to(dt))
    with pytest.raises(NotImplementedError):
        TK.layer_norm(x, w.double(), b.double())
    with pytest.raises(NotImplementedError):
        TK.layer_norm(x, w, b, residual=x.to(torch.bfloat16))
    with pytest.raises(NotImplementedError):
        TK.layer_norm(x, w, b, out_dtype=torch.bfloat16)
    for bad in (lambda: TK.layer_norm(x, w[:8], b[:8]), lambda: TK.layer_norm(x, w, None), lambda: TK.layer_norm(x, w, b, residual=x[:1]),
                lambda: TK.layer_norm(torch.tensor(1.0), None, None), lambda: TK.layer_norm(torch.randn(2, TK.LN_MAX_C + 4), None, None),
                lambda: TK.geglu(torch.randn(3, 7)), lambda: TK.geglu(torch.tensor(1.0)), lambda: TK.geglu(torch.randn(2, 2 * TK.GEGLU_MAX_D + 2))):
        with pytest.raises(ValueError):
            bad()


def test_use_native_block_ops_binds_three_modules_per_block_and_keeps_the_state_dict():
    from igs_amd import tokens as TK
    model = nn.Sequential(TR.make_block(32, TR.LinearAttention(32), seed=1), nn.GroupNorm(4, 32), TR.make_block(32, TR.LinearAttention(32), seed=2))
    keys = list(model.state_dict().keys())
    classes = [type(m) for m in model.modules()]
    ln_forward, geglu_forward = nn.LayerNorm.forward, TR.Geglu.forward
    assert TK.use_native_block_ops(model) == 6
    assert list(model.state_dict().keys()) == keys and [type(m) for m in model.modules()] == classes
    assert nn.LayerNorm.forward is ln_forward and TR.Geglu.forward is geglu_forward             # (the classes are untouched)
    bound = [m for m in model.modules() if "forward" in vars(m)]
    assert len(bound) == 6 and all(isinstance(m, (nn.LayerNorm, TR.Geglu)) for m in bound)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                   # the bound forward runs the native path: no fallback
        model[0](torch.randn(1, 4, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model[0].ff.net[0](torch.randn(1, 4, 32))
    assert TK.use_native_block_ops(nn.Linear(3, 3)) == 0


def _unsupported_blocks():
    ada = TR.make_block(32, TR.LinearAttention(32))
    ada.use_ada_layer_norm_zero = True
    mixed = TR.make_block(32, TR.LinearAttention(32))
    mixed.norm3 = nn.LayerNorm(32, elementwise_affine=False)
    cross = TR.make_block(32, TR.LinearAttention(32))
    cross.norm2, cross.attn2 = nn.LayerNorm(32), TR.LinearAttention(32)
    batch = TR.make_block(32, TR.LinearAttention(32))
    batch.norm1 = nn.GroupNorm(4, 32)
    return {"ada": ada, "mixed affine": mixed, "cross attention": cross, "gelu": TR.make_block(32, TR.LinearAttention(32), activation_fn="gelu"),
            "gelu-approximate": TR.make_block(32, TR.LinearAttention(32), activation_fn="gelu-approximate"), "another norm": batch}


@pytest.mark.parametrize("what", ["ada", "mixed affine", "cross attention", "gelu", "gelu-approximate", "another norm"])
def test_use_native_block_ops_refuses_before_any_binding(what):
    from igs_amd import tokens as TK
    model = nn.Sequential(TR.make_block(32, TR.LinearAttention(32)), _unsupported_blocks()[what])        # a good block first: it must stay unbound
    with pytest.raises(NotImplementedError):
        TK.use_native_block_ops(model)
    assert not any("forward" in vars(m) for m in model.modules())
    with torch.no_grad():
        assert model[0](torch.randn(1, 4, 32)).shape == (1, 4, 32)                               # still the PyTorch module it was
    plain = TR.make_block(32, TR.LinearAttention(32), norm_elementwise_affine=False)             # both norms without parameters: provided
    assert TK.use_native_block_ops(plain) == 3


def test_use_native_transformer_layers_binds_and_looks_the_attention_up_at_call_time(monkeypatch):
    from igs_amd import tokens as TK
    model = nn.ModuleList([TR.make_layer(16, no_ffn=True, seed=1), TR.make_layer(16, no_ffn=False, seed=2)])
    keys, classes = list(model.state_dict().keys()), [type(m) for m in model.modules()]
    ref_forward = TR.TransformerLayer.forward
    assert TK.use_native_transformer_layers(model) == 2
    assert list(model.state_dict().keys()) == keys and [type(m) for m in model.modules()] == classes
    assert TR.TransformerLayer.forward is ref_forward and all("forward" in vars(m) for m in model)
    seen = []

    def split(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None):
        seen.append(("split", num_splits, with_shift, h, w))
        return v

    def full(q, k, v):
        seen.append(("full",))
        return v

    monkeypatch.setattr(TR, "single_head_split_window_attention", split)                         # patched AFTER the binding
    monkeypatch.setattr(TR, "single_head_full_attention", full)
    x = torch.randn(2, 24, 16)
    for layer in model:
        with pytest.raises(RuntimeError, match="no CPU fallback"):                               # ... and then the native tail: no fallback
            layer(x, x, height=4, width=6, with_shift=True, attn_num_splits=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(x, x, height=4, width=6, attn_num_splits=1)
    assert seen == [("split", 2, True, 4, 6), ("full",)] * 2
    with pytest.raises(NotImplementedError, match="attn_type"):
        model[0](x, x, height=4, width=6, attn_type="self_swin2d_cross_1d", attn_num_splits=2)
    assert len(seen) == 4                                                                        # (refused before anything ran)
    assert TK.use_native_transformer_layers(nn.Linear(3, 3)) == 0


def test_use_native_transformer_layers_refuses_before_any_binding():
    from igs_amd import tokens as TK
    heads = TR.make_layer(16)
    heads.nhead = 2
    other = TR.make_layer(16)
    other.norm2 = nn.BatchNorm1d(16)
    for bad in (heads, other):
        model = nn.ModuleList([TR.make_layer(16, no_ffn=True), bad])
        with pytest.raises(NotImplementedError):
            TK.use_native_transformer_layers(model)
        assert not any("forward" in vars(m) for m in model.modules())
