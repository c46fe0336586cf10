"""The two ends of Transformer1D (igs_amd/csrc/gnorm.hip, igs_amd/tokens.py) without a GPU: the float64 restatement and the stand-in
module against PyTorch and the reference-produced golden file, exports and argument counts, the refusals of the C ABI before any HIP call
and of the Python layer, the binder on the stand-in, the registers and scratch of the built gfx950 kernels, and the derived allowances on a
float32 emulation of the kernels' arithmetic, on CPU PyTorch float32 and on four wrong variants."""
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
import transformer_ends_restatement as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_group_norm_tokens_fwd", "igs_group_norm_tokens_bwd_scratch_bytes", "igs_group_norm_tokens_bwd", "igs_tokens_add_residual")
INVALID = -1
F32, F16 = 0, 1
EPS = 1e-6
CASES = [dict(in_channels=12, norm_num_groups=3, A=7, num_layers=0), dict(in_channels=16, norm_num_groups=4, A=10, num_layers=1)]      # the golden file's


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_transformer_ends.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def test_restated_operations_equal_pytorch_float64():
    g = torch.Generator().manual_seed(3)
    B, C, G, A = 2, 12, 3, 7
    x = torch.randn(B, C, A, generator=g, dtype=torch.float64) * 3 + 1
    dout = torch.randn(B, A, C, generator=g, dtype=torch.float64)
    w, b = (torch.randn(C, generator=g, dtype=torch.float64) for _ in range(2))
    assert (ER.group_norm_tokens_restate(x, G, w, b, EPS) - F.group_norm(x, G, w, b, EPS).permute(0, 2, 1)).abs().max() <= 1e-12
    assert (ER.group_norm_tokens_restate(x, G, None, None, EPS) - F.group_norm(x, G, None, None, EPS).permute(0, 2, 1)).abs().max() <= 1e-12
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    want = torch.autograd.grad(F.group_norm(leaves[0], G, leaves[1], leaves[2], EPS).permute(0, 2, 1), leaves, dout)
    for got, ref in zip(ER.group_norm_tokens_backward_restate(x, G, w, EPS, dout), want):
        assert (got - ref).abs().max() <= 1e-11
    stats = ER.group_norm_stats_restate(x, G, EPS)
    xg = x.reshape(B, G, -1)
    assert stats.shape == (B, G, 2) and (stats[..., 0] - xg.mean(-1)).abs().max() <= 1e-12
    assert (stats[..., 1] - (xg.var(-1, unbiased=False) + EPS).rsqrt()).abs().max() <= 1e-12
    assert torch.equal(ER.add_residual_restate(dout, x), dout + x.permute(0, 2, 1))


@pytest.mark.parametrize("i", [0, 1])
def test_stand_in_transformer_and_the_restated_ends_equal_the_reference(golden, i):
    case, tag = CASES[i], "case%d." % i
    model = ER.Transformer1D(case["in_channels"], case["norm_num_groups"], 16, case["num_layers"]).double()
    params = {k[len(tag + "param."):]: v for k, v in golden.items() if k.startswith(tag + "param.")}
    assert sorted(params) == sorted(model.state_dict().keys()), sorted(params)
    model.load_state_dict(params)
    x = golden[tag + "in.hidden_states"].clone().requires_grad_(True)
    assert x.shape == (2, case["in_channels"], case["A"]) and x.dtype == torch.float64
    out = model(x)
    assert (out - golden[tag + "out"]).abs().max() <= 1e-12
    named = dict(model.named_parameters())
    grads = torch.autograd.grad(out, [x] + list(named.values()), golden[tag + "gout"])
    assert (grads[0] - golden[tag + "grad_in.hidden_states"]).abs().max() <= 1e-12
    for name, g in zip(named, grads[1:]):
        assert (g - golden[tag + "grad_param." + name]).abs().max() <= 1e-12, name
    # ... and the restated ends around the same projections and blocks, on the reference's own numbers
    with torch.no_grad():
        tokens = model.proj_in(ER.group_norm_tokens_restate(x.detach(), case["norm_num_groups"], model.norm.weight, model.norm.bias, model.norm.eps))
        for block in model.transformer_blocks:
            tokens = block(tokens)
        ends = ER.add_residual_restate(model.proj_out(tokens), x.detach()).permute(0, 2, 1)
    assert (ends - golden[tag + "out"]).abs().max() <= 1e-12


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
    assert "gnorm.hip" in build.SOURCES
    m = _cabi.ext()
    for f in ("group_norm_tokens_fwd", "group_norm_tokens_bwd", "tokens_add_residual"):
        assert hasattr(m._gnorm, f), f                                                           # (a private submodule of _C)
    from igs_amd import tokens as TK
    assert re.search(r"#define IGS_GN_MAX_C %d\b" % TK.GN_MAX_C, hdr) and TK.GN_MAX_C == 1024
    assert re.search(r"#define IGS_GN_MAX_TOKENS \(1LL << 24\)", hdr) and TK.GN_MAX_TOKENS == 1 << 24
    assert re.search(r"#define IGS_GN_MAX_GROUP_ELEMS \(1LL << 30\)", hdr) and TK.GN_MAX_GROUP_ELEMS == 1 << 30


X, OUT, WGT, BIAS, STATS, DOUT, DX, DW, DB, SCR, TOK = (0x10000000, 0x30000000, 0x50000000, 0x50100000, 0x50200000, 0x70000000, 0x90000000,
                                                        0xB0000000, 0xB0100000, 0xD0000000, 0xF0000000)
B0, C0, G0, A0 = 2, 128, 32, 96


def _fwd(L, B=B0, C=C0, G=G0, A=A0, xdt=F32, x=X, bs=None, cs=None, w=WGT, b=BIAS, eps=EPS, odt=F32, out=OUT, os_=None, stats=STATS):
    cs = A if cs is None else cs
    return L.igs_group_norm_tokens_fwd(None, B, C, G, A, xdt, x, C * cs if bs is None else bs, cs, w, b, eps, odt, out, C if os_ is None else os_, stats)


def _bwd(L, B=B0, C=C0, G=G0, A=A0, xdt=F32, x=X, bs=None, cs=None, w=WGT, stats=STATS, gdt=F32, g=DOUT, gs=None, ddt=F32, dx=DX, dbs=None, dcs=None,
         dw=DW, db=DB, scr=SCR):
    cs, dcs = A if cs is None else cs, A if dcs is None else dcs
    return L.igs_group_norm_tokens_bwd(None, B, C, G, A, xdt, x, C * cs if bs is None else bs, cs, w, stats, gdt, g, C if gs is None else gs, ddt, dx,
                                       C * dcs if dbs is None else dbs, dcs, dw, db, scr)


def _add(L, B=B0, C=C0, A=A0, tdt=F32, tok=TOK, ts=None, rdt=F32, res=X, bs=None, cs=None, odt=F32, out=OUT, os_=None):
    cs = A if cs is None else cs
    return L.igs_tokens_add_residual(None, B, C, A, tdt, tok, C if ts is None else ts, rdt, res, C * cs if bs is None else bs, cs, odt, out,
                                     C if os_ is None else os_)


def test_every_invalid_argument_class_is_refused_before_any_hip_call():
    """Addresses that are never dereferenced and no GPU in the process: a check that came after a HIP call could not return these codes."""
    from igs_amd import _cabi
    from igs_amd import tokens as TK
    L = _cabi.lib()

    def refused(call, name, cases):
        for kw, word in cases:
            assert call(L, **kw) == INVALID, (name, kw)
            assert word in _cabi.last_error() and name in _cabi.last_error(), (kw, _cabi.last_error())

    every = [(dict(C=0), "C out of range"), (dict(C=-4), "C out of range"), (dict(C=TK.GN_MAX_C + 32), "C out of range"), (dict(A=0), "A out of range"),
             (dict(A=-5), "A out of range"), (dict(B=-1), "B out of range"), (dict(B=(1 << 24) // A0 + 1), "B out of range")]
    sizes = every + [(dict(A=(1 << 28) + 1), "A out of range"), (dict(B=1, A=(1 << 24) + 1), "B out of range")]      # 4 channels per group: 4 A > 2^30
    groups = [(dict(G=0), "G must be"), (dict(G=-2), "G must be"), (dict(G=5), "G must be"), (dict(G=256), "G must be")]
    span = C0 * A0 * B0 * 4                                                                              # bytes of a float32 [B, C, A] or [B, A, C]
    refused(_fwd, "igs_group_norm_tokens_fwd", sizes + groups + [
        (dict(eps=-1e-6), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"),
        (dict(xdt=2), "dtype"), (dict(odt=-1), "dtype"),
        (dict(x=None), "NULL"), (dict(out=None), "NULL"), (dict(stats=None), "NULL"),
        (dict(b=None), "weight and bias go together"), (dict(w=None), "weight and bias go together"),
        (dict(x=X + 2), "aligned to its element size"), (dict(xdt=F16, x=X + 1), "aligned"), (dict(out=OUT + 1), "aligned"), (dict(w=WGT + 2), "aligned"),
        (dict(b=BIAS + 1), "aligned"), (dict(stats=STATS + 2), "aligned"),
        (dict(cs=A0 - 1, bs=C0 * A0), "stride"), (dict(bs=C0 * A0 - 1), "stride"), (dict(cs=A0 + 4, bs=C0 * A0), "stride"), (dict(os_=C0 - 1), "stride"),
        (dict(cs=-A0), "stride"), (dict(os_=0), "stride"), (dict(os_=(1 << 31) + 4), "stride"), (dict(cs=(1 << 31) + 4, bs=1 << 40), "stride"),
        (dict(bs=(1 << 36) + 4), "stride"),
        (dict(out=X), "overlaps x, weight or bias"), (dict(out=X + span - 4), "overlaps x, weight or bias"), (dict(out=X - span + 4), "overlaps x, weight or bias"),
        (dict(stats=X + 64), "overlaps x, weight or bias"), (dict(stats=WGT + 4 * C0 - 4), "overlaps x, weight or bias"), (dict(out=BIAS - span + 4), "overlaps x"),
        (dict(x=X, cs=2 * A0, bs=2 * C0 * A0, out=X + span + 64), "overlaps x, weight or bias"),                 # (inside the strided x's span only)
        (dict(stats=OUT + 128), "overlap one another")])
    assert _fwd(L, B=0) == 0 and _fwd(L, B=0, x=None, out=None, stats=None) == 0                            # nothing to do
    assert _fwd(L, B=0, C=0) == INVALID and _fwd(L, B=0, eps=-1.0) == INVALID and _fwd(L, B=0, G=5) == INVALID      # ... the arguments are still checked
    refused(_bwd, "igs_group_norm_tokens_bwd", sizes + groups + [
        (dict(xdt=3), "dtype"), (dict(gdt=2), "dtype"), (dict(ddt=-1), "dtype"),
        (dict(x=None), "NULL"), (dict(g=None), "NULL"), (dict(stats=None), "NULL"), (dict(scr=None), "NULL"), (dict(dx=None, dw=None, scr=None), "NULL"),
        (dict(x=X + 1), "aligned"), (dict(g=DOUT + 2), "aligned"), (dict(ddt=F16, dx=DX + 1), "aligned"), (dict(dw=DW + 2), "aligned"),
        (dict(db=DB + 1), "aligned"), (dict(w=WGT + 1), "aligned"), (dict(stats=STATS + 1), "aligned"),
        (dict(cs=A0 - 1, bs=C0 * A0), "stride"), (dict(gs=C0 - 1), "stride"), (dict(dcs=A0 - 4, dbs=C0 * A0), "stride"), (dict(dbs=C0 * A0 - 1), "stride"),
        (dict(dx=X), "overlaps x, dout, weight or stats"), (dict(dx=DOUT + 64), "overlaps x, dout, weight or stats"), (dict(dw=WGT), "overlaps x, dout"),
        (dict(db=X + 40), "overlaps x, dout"), (dict(scr=DOUT), "overlaps x, dout"), (dict(dw=STATS + 8), "overlaps x, dout, weight or stats"),
        (dict(scr=STATS - 64), "overlaps x, dout, weight or stats"),
        (dict(dw=DX + 16), "overlap one another"), (dict(db=DW + 4), "overlap one another"), (dict(scr=DX + 256), "overlap one another"),
        (dict(scr=DB - 64), "overlap one another")])
    assert _bwd(L, B=0) == 0 and _bwd(L, dx=None, dw=None, db=None, x=None, g=None, scr=None) == 0          # nothing to do
    assert _bwd(L, B=0, C=0) == INVALID and _bwd(L, dx=None, dw=None, db=None, G=7) == INVALID
    assert L.igs_group_norm_tokens_bwd_scratch_bytes(1, 128, 32, 8192) > 0 and L.igs_group_norm_tokens_bwd_scratch_bytes(1, 4, 1, 1) > 0
    for b, c, g, a in ((-1, 128, 32, 64), (1, 0, 1, 64), (1, TK.GN_MAX_C + 4, 1, 64), (1, 128, 3, 64), (1, 128, 32, 0), (2, 128, 32, 1 << 24)):
        assert L.igs_group_norm_tokens_bwd_scratch_bytes(b, c, g, a) == 0, (b, c, g, a)
    refused(_add, "igs_tokens_add_residual", every + [
        (dict(C=1024, A=(1 << 20) + 1, B=1), "A out of range"), (dict(C=4, B=1, A=(1 << 24) + 1), "B out of range"),
        (dict(tdt=2), "dtype"), (dict(rdt=-1), "dtype"), (dict(odt=5), "dtype"), (dict(tok=None), "NULL"), (dict(res=None), "NULL"), (dict(out=None), "NULL"),
        (dict(tok=TOK + 2), "aligned"), (dict(rdt=F16, res=X + 1), "aligned"), (dict(out=OUT + 3), "aligned"),
        (dict(ts=C0 - 1), "stride"), (dict(cs=A0 - 1, bs=C0 * A0), "stride"), (dict(bs=C0 * A0 - 1), "stride"), (dict(os_=C0 - 2), "stride"),
        (dict(out=TOK), "out overlaps tok or res"), (dict(out=X + 16), "out overlaps tok or res"), (dict(out=TOK - span + 4), "out overlaps tok or res")])
    assert _add(L, B=0) == 0 and _add(L, B=0, tok=None, res=None, out=None) == 0 and _add(L, B=0, C=0) == INVALID


# ---------------------------------------------------------------- the built code objects
@pytest.fixture(scope="module")
def end_kernels():
    """{symbol: metadata} of every kernel of gnorm.hip in libigs_rast.so."""
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
                if re.match(r"^_ZL?\d+(gn_\w+_kernel|tok_\w+_kernel)", name):
                    found[name] = md
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_kernels_have_no_scratch_no_spills_and_the_budgeted_registers(end_kernels):
    """two instances (four-element and scalar access) of the statistics, the apply, the residual add, the backward's
    sums and its dx, one of the group sums; none with scratch or spills; every one at 8 waves per SIMD (<= 64 registers); the tile
    kernels with one 64 x 65 (+ 32) float tile of LDS."""
    k = end_kernels
    for stem, count in (("gn_stats_kernel", 2), ("gn_apply_kernel", 2), ("tok_add_residual_kernel", 2), ("gn_bwd_sums_kernel", 2), ("gn_bwd_dx_kernel", 2),
                        ("gn_bwd_group_kernel", 1)):
        assert len([n for n in k if stem in n]) == count, (stem, sorted(k))
    assert len(k) == 11, sorted(k)
    for name, md in k.items():
        assert int(md[".private_segment_fixed_size"]) == 0, (name, "scratch bytes per lane")
        assert int(md.get(".vgpr_spill_count", 0)) == 0 and int(md.get(".sgpr_spill_count", 0)) == 0, (name, "spills")
        regs = (int(md[".vgpr_count"]) + int(md.get(".agpr_count", 0)) + 7) // 8 * 8
        print(name, "vgpr", md[".vgpr_count"], "lds", md[".group_segment_fixed_size"])
        assert regs <= 64, (name, regs)
        tile = any(s in name for s in ("gn_apply", "tok_add", "gn_bwd_sums", "gn_bwd_dx"))
        assert int(md[".group_segment_fixed_size"]) == ((64 * 65 + 32) * 4 if tile else (192 if "gn_stats" in name else 0)), name
        assert int(md[".max_flat_workgroup_size"]) == (1024 if "gn_stats" in name else 64 if "gn_bwd_group" in name else 256), name


# ---------------------------------------------------------------- the allowances
# the shapes of the GPU tests that the CPU gets through quickly (tests/test_gpu_transformer_ends.py), eps as shipped
SHAPES = [(1, 4, 1, 1), (1, 4, 2, 1), (2, 6, 3, 63), (1, 8, 8, 33), (2, 12, 3, 7), (1, 128, 32, 65), (3, 128, 32, 257), (2, 132, 33, 67), (1, 256, 32, 130),
          (1, 1024, 32, 5)]


def _inputs(shape, seed):
    B, C, G, A = shape
    x = ER.group_inputs(B, C, G, A, torch.float32, "cpu", seed)
    w, b = TR.affine_inputs(C, "cpu", seed)
    g = torch.randn(B, A, C, generator=torch.Generator().manual_seed(seed + 1))
    return x, w, b, g


def _fwd_ratio(y, x, G, w=None, b=None):
    ref = ER.group_norm_tokens_restate(x.double(), G, None if w is None else w.double(), None if b is None else b.double(), EPS)
    return ((y.double() - ref).abs() / ER.group_norm_forward_bound(x, G, w, b, EPS)).max().item()


def _bwd_ratios(got, x, G, w, g):
    want = ER.group_norm_tokens_backward_restate(x.double(), G, w.double(), EPS, g.double())
    bounds = ER.group_norm_backward_bounds(x, G, w, EPS, g)
    return [((a.double() - r).abs() / bounds[k]).max().item() for a, r, k in zip(got, want, ("dx", "dweight", "dbias"))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-G%d-A%d" % s)
def test_allowance_accepts_the_kernel_arithmetic_and_pytorch_float32(shape):
    """On the GPU tests' inputs (every pair of standard deviation and mean): the float32 emulation of the kernels' arithmetic and PyTorch's
    own float32 group_norm on the CPU, forward and backward, stay inside the allowance."""
    B, C, G, A = shape
    x, w, b, g = _inputs(shape, 3 * A + C)
    r_emul = _fwd_ratio(ER.group_norm_emulate(x, G, w, b, EPS), x, G, w, b)
    r_torch = _fwd_ratio(F.group_norm(x, G, w, b, EPS).permute(0, 2, 1), x, G, w, b)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    r_bwd_torch = _bwd_ratios(torch.autograd.grad(F.group_norm(leaves[0], G, leaves[1], leaves[2], EPS).permute(0, 2, 1), leaves, g), x, G, w, g)
    r_bwd_emul = _bwd_ratios(ER.group_norm_backward_emulate(x, G, w, EPS, g), x, G, w, g)
    print(shape, "max |err| / allowance: emulation %.3f, F.group_norm float32 %.3f, backward emulation %s, autograd float32 %s"
          % (r_emul, r_torch, ["%.3f" % r for r in r_bwd_emul], ["%.3f" % r for r in r_bwd_torch]))
    assert r_emul <= 1.0 and r_torch <= 1.0 and max(r_bwd_emul) <= 1.0 and max(r_bwd_torch) <= 1.0
    const = torch.full((1, C, A), 100.37, dtype=torch.float32)
    assert torch.equal(ER.group_norm_emulate(const, G, w, b, EPS), b.view(1, 1, C).expand(1, A, C))      # a constant group: exactly bias


def test_allowance_rejects_four_wrong_variants():
    shape = (2, 12, 3, 7)
    B, C, G, A = shape
    x, w, b, g = _inputs(shape, 33)
    r = {v: _fwd_ratio(ER.group_norm_emulate(x, G, w, b, EPS, variant=v), x, G, w, b) for v in ("right", "unbiased", "shifted", "gamma_by_group")}
    r["no_s1"] = _bwd_ratios(ER.group_norm_backward_emulate(x, G, w, EPS, g, variant="no_s1"), x, G, w, g)[0]
    r["right_dx"] = _bwd_ratios(ER.group_norm_backward_emulate(x, G, w, EPS, g), x, G, w, g)[0]
    big = (3, 128, 32, 257)                                                                      # n = 1028: n - 1 for n is 5e-4 of rstd, far above u
    xb, wb, bb, _ = _inputs(big, 1)
    r["unbiased_n1028"] = _fwd_ratio(ER.group_norm_emulate(xb, 32, wb, bb, EPS, variant="unbiased"), xb, 32, wb, bb)
    print("max |err| / allowance:", {k: round(v, 3) for k, v in r.items()})
    assert r["right"] <= 1.0 and r["right_dx"] <= 1.0, r
    assert all(r[k] > 1.0 for k in ("unbiased", "unbiased_n1028", "shifted", "gamma_by_group", "no_s1")), r


# ---------------------------------------------------------------- the Python layer
def test_python_refusals_on_the_cpu():
    from igs_amd import tokens as TK
    x, w, b = torch.randn(2, 16, 5), torch.ones(16), torch.zeros(16)
    tok = torch.randn(2, 5, 16)
    for call in (lambda t: TK.group_norm_tokens(t, 4, w, b), lambda t: TK.group_norm_tokens(t, 4), lambda t: TK.add_residual_tokens(tok.to(t.dtype), t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x)
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(NotImplementedError):
                call(x.to(dt))
    with pytest.raises(NotImplementedError):
        TK.group_norm_tokens(x, 4, w.double(), b.double())
    with pytest.raises(NotImplementedError):
        TK.group_norm_tokens(x, 4, w, b, out_dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        TK.add_residual_tokens(tok.to(torch.bfloat16), x)
    for bad in (lambda: TK.group_norm_tokens(x, 3, w, b), lambda: TK.group_norm_tokens(x, 0), lambda: TK.group_norm_tokens(x, 4, w[:8], b[:8]),
                lambda: TK.group_norm_tokens(x, 4, w, None), lambda: TK.group_norm_tokens(x[0], 4), lambda: TK.group_norm_tokens(torch.randn(1, TK.GN_MAX_C + 4, 2), 1),
                lambda: TK.group_norm_tokens(torch.randn(2, 16, 0), 4), lambda: TK.add_residual_tokens(tok, x[:, :, :4]), lambda: TK.add_residual_tokens(tok, tok),
                lambda: TK.add_residual_tokens(tok[0], x[0])):
        with pytest.raises(ValueError):
            bad()


def _model():
    return nn.Sequential(ER.make_transformer(16, 4, 32, 1, seed=1), nn.GroupNorm(4, 16), ER.make_transformer(16, 2, 32, 2, seed=2))


def test_use_native_transformer_ends_counts_binds_and_keeps_the_state_dict():
    from igs_amd import tokens as TK
    model = _model()
    keys, classes = list(model.state_dict().keys()), [type(m) for m in model.modules()]
    ref_forward = ER.Transformer1D.forward
    assert TK.use_native_transformer_ends(model) == 2
    assert list(model.state_dict().keys()) == keys and [type(m) for m in model.modules()] == classes
    assert ER.Transformer1D.forward is ref_forward                                               # (the class is untouched)
    bound = [m for m in model.modules() if "forward" in vars(m)]
    assert len(bound) == 2 and all(isinstance(m, ER.Transformer1D) for m in bound)
    x = torch.randn(1, 16, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                   # the bound forward runs the native path: no fallback
        model[0](x)
    for name in ("attention_mask", "encoder_attention_mask"):
        with pytest.raises(NotImplementedError, match=name):
            model[0](x, **{name: torch.ones(1, 6)})
    assert TK.use_native_transformer_ends(nn.Linear(3, 3)) == 0
    # ... and composes with the block binder: three more bound modules per block, the same keys
    assert TK.use_native_block_ops(model) == 9
    assert list(model.state_dict().keys()) == keys and len([m for m in model.modules() if "forward" in vars(m)]) == 11


@pytest.mark.parametrize("what", ["layer norm", "no affine", "checkpointing"])
def test_use_native_transformer_ends_refuses_before_any_binding(what):
    from igs_amd import tokens as TK
    bad = ER.make_transformer(16, 4, 32, 1)
    if what == "layer norm":
        bad.norm = nn.LayerNorm(16)
    elif what == "no affine":
        bad.norm = nn.GroupNorm(4, 16, affine=False)
    else:
        bad.gradient_checkpointing = True
    model = nn.Sequential(ER.make_transformer(16, 4, 32, 1), bad)                                # a good one first: it must stay unbound
    with pytest.raises(NotImplementedError):
        TK.use_native_transformer_ends(model)
    assert not any("forward" in vars(m) for m in model.modules())
    with torch.no_grad():
        assert model[0](torch.randn(1, 16, 6)).shape == (1, 16, 6)                               # still the PyTorch module it was
