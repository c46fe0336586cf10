"""The swin window attention on the MI355X (igs_amd.attention.window_attention over wattn.hip) against the float64 restatement of
tests/window_attention_restatement.py.

Tolerances are derived (forward_bound / backward_bounds state the operation counts), never measured.  Every element is compared and the
worst error-to-bound ratio of every case is printed.  Float16 inputs are widened exactly before the float64 restatement sees them; the
restatement runs on the device in float64, once per case, for the forward and the backward together."""
import types

import pytest
import torch

import window_attention_restatement as WR

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float16, torch.float32]
# (h, w, K): window lengths 10 (below one 32-key sub-tile), 6 (nine windows, odd sides), 35 (crosses 32), 16, 64 (exactly one tile),
# 132 (crosses the 128-token ownership, ragged tail), 192 (full attention), 1024 (the shipped shape)
SHAPES = [(4, 10, 2), (6, 9, 3), (10, 14, 2), (16, 16, 4), (16, 16, 2), (24, 22, 2), (16, 12, 1), (64, 64, 2)]


def _shifts(K):
    return (False, True) if K > 1 else (False,)


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _native(q, k, v, h, w, K, shift, **kw):
    from igs_amd.attention import window_attention
    with torch.no_grad():
        return window_attention(q, k, v, h, w, K, shift, **kw)


def _native_grads(q, k, v, g, h, w, K, shift, need=(True, True, True)):
    from igs_amd.attention import window_attention
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), need)]
    out = window_attention(*leaves, h, w, K, shift)
    out.backward(g)
    return out.detach(), [t.grad for t in leaves]


def _ratio(x, ref, bound):
    err = (x.double() - ref).abs()
    assert torch.isfinite(x).all()
    return err, (err / bound.clamp_min(1e-300)).max().item()


def _check_forward(out, r, shift, label):
    assert out.dtype in DTYPES and out.shape == r["o"].shape and out.is_contiguous()
    err, worst = _ratio(out, r["o"], WR.forward_bound(r, out.dtype, shift))
    print("%s %s: forward max |err| / bound %.3f" % (label, _name(out.dtype), worst))
    assert worst <= 1.0, (label, worst, err.max().item())
    return worst


# ---------------------------------------------------------------- forward and backward, random inputs, every shape of the table
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_against_float64(dtype, shape):
    h, w, K = shape
    B = 2
    for shift in _shifts(K):
        label = "%s%s" % (shape, " shifted" if shift else "")
        q, k, v, g = WR.random_inputs(B, h, w, dtype, DEV, seed=1000 * h + 10 * w + K + shift, with_dout=True)
        out, grads = _native_grads(q, k, v, g, h, w, K, shift)
        assert torch.equal(out, _native(q, k, v, h, w, K, shift))                  # with and without lse: the same bits
        q64, k64, v64, g64 = (t.double() for t in (q, k, v, g))
        r = WR.restate(q64, k64, v64, h, w, K, shift)                              # once, for the forward and the backward
        _check_forward(out, r, shift, label)
        ref = WR.gradients(q64, k64, v64, h, w, K, shift, g64)
        bounds = WR.backward_bounds(r, g64, dtype, shift)
        worst = []
        for i, name in enumerate(("d q", "d k", "d v")):
            assert grads[i].dtype == dtype and grads[i].shape == q.shape and grads[i].is_contiguous()
            err, ratio = _ratio(grads[i], ref[i], bounds[i])
            worst.append(ratio)
            assert ratio <= 1.0, (label, name, ratio, err.max().item())
        print("%s %s: backward max |err| / bound: d q %.3f, d k %.3f, d v %.3f" % (label, _name(dtype), *worst))
        del r, ref, bounds


@pytest.mark.parametrize("dtype", DTYPES)
def test_drop_in_functions_match_window_attention(dtype):
    from igs_amd import attention as AT
    h, w, K = 16, 12, 2
    q, k, v = WR.random_inputs(2, h, w, dtype, DEV, seed=3)
    mask = torch.zeros(K * K, (h // K) * (w // K), (h // K) * (w // K), device=DEV)          # (the values are not read)
    with torch.no_grad():
        assert torch.equal(AT.single_head_split_window_attention(q, k, v, num_splits=K, with_shift=True, h=h, w=w, attn_mask=mask),
                           _native(q, k, v, h, w, K, True))
        assert torch.equal(AT.single_head_split_window_attention(q, k, v, num_splits=K, h=h, w=w), _native(q, k, v, h, w, K, False))
        full = AT.single_head_full_attention(q, k, v)
    assert torch.equal(full, _native(q, k, v, h, w, 1, False))
    r = WR.restate(q.double(), k.double(), v.double(), 1, h * w, 1, False)
    _check_forward(full, r, False, "single_head_full_attention")


# ---------------------------------------------------------------- views
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_qkv_slices_are_read_in_place_and_misaligned_views_are_copied(dtype):
    from igs_amd import attention as AT
    h, w, K, B = 24, 22, 2, 2
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, h * w, 384, generator=g)
    qkv[..., :256] *= 1.5
    qkv[..., 256:] += 0.3
    qkv = qkv.to(dtype).to(DEV)
    gout = torch.randn(B, h * w, 128, generator=g).to(dtype).to(DEV)
    q, k, v = (qkv[..., 128 * i:128 * (i + 1)] for i in range(3))                  # slices of one buffer
    assert all(AT._acceptable3(t) and not t.is_contiguous() for t in (q, k, v))    # read in place
    qc, kc, vc = (t.contiguous() for t in (q, k, v))
    for shift in (False, True):
        out, grads = _native_grads(q, k, v, gout, h, w, K, shift)
        out2, grads2 = _native_grads(qc, kc, vc, gout, h, w, K, shift)
        assert torch.equal(out, out2)                                              # the same arithmetic whatever the strides
        for a, b in zip(grads, grads2):
            assert torch.equal(a, b)
        _check_forward(out, WR.restate(qc.double(), kc.double(), vc.double(), h, w, K, shift), shift, "fused QKV slices")
        pad = lambda t: torch.cat([torch.zeros_like(t[..., :2]), t], -1)[..., 2:]  # the same values 4 or 8 bytes off alignment
        qm, km, vm = pad(qc), pad(kc), pad(vc)
        assert not AT._acceptable3(qm) and qm.stride(2) == 1
        assert torch.equal(_native(qm, km, vm, h, w, K, shift), out)               # the copy path
        wide = torch.stack([qc, qc], -1).reshape(B, h * w, 256)[..., ::2]          # stride 2 on d
        assert wide.stride(2) == 2
        assert torch.equal(_native(wide, kc, vc, h, w, K, shift), out)


# ---------------------------------------------------------------- the mask
def _regions(h, w, K, device):
    """[L] the region of every original token's rolled position"""
    tok, region = WR.token_map(h, w, K, True)
    return WR.scatter(region[None].to(device), tok)[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mask_acts(dtype):
    """(16, 16, 2) shifted, v the one-hot of the token's region, scores of the order of 0.1: without the mask every region of a window would
    get about its share of the weight; with it a query's own region channel is 1 and every other channel is e^-100 or nothing."""
    h, w, K, B = 16, 16, 2, 2
    g = torch.Generator().manual_seed(11)
    q = (0.3 * torch.randn(B, h * w, 128, generator=g)).to(dtype).to(DEV)
    k = (0.3 * torch.randn(B, h * w, 128, generator=g)).to(dtype).to(DEV)
    reg = _regions(h, w, K, DEV)
    assert sorted(reg.unique().tolist()) == list(range(9))
    v = torch.nn.functional.one_hot(reg, 128).to(dtype)[None].expand(B, -1, -1).contiguous()
    s = WR.restate(q.double(), k.double(), v.double(), h, w, K, True)
    assert 0.05 < (s["s"] - s["mask"]).abs().max().item() < 1.0
    out = _native(q, k, v, h, w, K, True).double()
    own = out.gather(2, reg[None, :, None].expand(B, -1, 1)).squeeze(2)
    other = out.clone()
    other.scatter_(2, reg[None, :, None].expand(B, -1, 1), 0.0)
    print("mask acts %s: max |own - 1| %.3e, max other %.3e" % (_name(dtype), (own - 1).abs().max().item(), other.max().item()))
    assert (own - 1).abs().max().item() <= 1e-6
    assert other.abs().max().item() < 1e-30
    plain = _native(q, k, v, h, w, K, False).double()                              # unshifted: windows of one region each
    assert ((plain.sum(-1) - 1).abs() <= 2e-3).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_mask_is_a_finite_addend(dtype):
    """Cross-region scores exceed same-region scores by 120 after scaling, so after the mask's -100 the masked keys still win by e^20: an
    implementation with -inf (or one that drops masked keys) returns the same-region mean instead."""
    h, w, K, B = 16, 16, 2, 2
    g = torch.Generator().manual_seed(13)
    reg = _regions(h, w, K, "cpu")
    alpha = (120.0 * 128 ** 0.5) ** 0.5
    hot = torch.nn.functional.one_hot(reg, 9).float()
    q = torch.cat([alpha * (1 - hot), 0.5 * torch.randn(h * w, 119, generator=g)], -1)
    k = torch.cat([alpha * hot, 0.5 * torch.randn(h * w, 119, generator=g)], -1)
    v = torch.randn(B, h * w, 128, generator=g) + 0.3
    q, k = (t[None].expand(B, -1, -1).contiguous().to(dtype).to(DEV) for t in (q, k))
    v = v.to(dtype).to(DEV)
    r = WR.restate(q.double(), k.double(), v.double(), h, w, K, True)
    masked = r["mask"] != 0
    assert masked.any() and (r["s"] - r["mask"])[:, masked].min().item() > 110.0           # unmasked scaled scores of the masked pairs
    weight = (r["p"] * masked.to(r["p"])).sum(-1)                                           # the weight a query gives to other regions
    multi = masked.any(-1)                                                                  # queries whose window holds another region
    assert weight[:, multi].min().item() > 0.99
    _check_forward(_native(q, k, v, h, w, K, True), r, True, "mask as an addend")


@pytest.mark.parametrize("shape", [(10, 14, 2), (24, 22, 2)])
def test_half_bound_rejects_the_wrong_variants_on_the_device(shape):
    """Not vacuous: the float16 bound that the native result meets rejects the mask ignored, the roll's sign flipped and h / w swapped."""
    h, w, K = shape
    q, k, v = WR.random_inputs(2, h, w, torch.float16, DEV, seed=h * w)
    r = WR.restate(q.double(), k.double(), v.double(), h, w, K, True)
    bound = WR.forward_bound(r, torch.float16, True)
    nat = ((_native(q, k, v, h, w, K, True).double() - r["o"]).abs() / bound).max().item()
    wrong = {var: ((WR.half_pipeline(q, k, v, h, w, K, True, var) - r["o"]).abs() / bound).max().item() for var in ("no_mask", "roll_sign", "hw_swapped")}
    print(shape, "max |err| / bound: native %.3f, wrong variants %s" % (nat, wrong))
    assert nat <= 1.0 and all(x > 1.0 for x in wrong.values())


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_keys_give_the_window_mean(dtype):
    h, w, K = 24, 22, 2
    q, k, v = WR.random_inputs(2, h, w, dtype, DEV, seed=4)
    tok, _ = WR.token_map(h, w, K, False)
    kw = WR.gather(k, tok)
    k = WR.scatter(kw[:, :, :1].expand_as(kw).contiguous(), tok)                  # one key per window and example
    out = _native(q, k, v, h, w, K, False)
    r = WR.restate(q.double(), k.double(), v.double(), h, w, K, False)
    _check_forward(out, r, False, "identical keys")
    mean = WR.scatter(r["vw"].mean(2, keepdim=True).expand_as(r["vw"]).contiguous(), tok)  # the second statement: the window's mean value
    assert ((out.double() - mean).abs() <= WR.forward_bound(r, dtype, False) + 1e-12 * mean.abs()).all()


# ---------------------------------------------------------------- backward
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_gradient_combinations_and_bitwise_repeat(dtype):
    h, w, K = 24, 22, 2
    q, k, v, g = WR.random_inputs(2, h, w, dtype, DEV, seed=12, with_dout=True)
    for shift in (False, True):
        _, full = _native_grads(q, k, v, g, h, w, K, shift)
        _, again = _native_grads(q, k, v, g, h, w, K, shift)
        for a, b in zip(full, again):
            assert torch.equal(a, b)                              # no float atomics: two runs agree bit for bit
        for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)):
            _, part = _native_grads(q, k, v, g, h, w, K, shift, need)
            for n, a, b in zip(need, part, full):
                assert (a is None) == (not n)
                if n:
                    assert torch.equal(a, b)
    from igs_amd.attention import window_attention
    leaves = [t.detach().clone().requires_grad_(False) for t in (q, k, v)]
    assert window_attention(*leaves, h, w, K, True).grad_fn is None                # no gradient wanted: nothing is saved


def test_gradients_reach_the_projection_weights_through_the_patched_namespace():
    from igs_amd import attention as AT
    h, w, K = 16, 16, 2
    ns = types.SimpleNamespace(single_head_full_attention=WR.restated_full, single_head_split_window_attention=WR.restated_split)
    ref_ns = types.SimpleNamespace(single_head_full_attention=WR.restated_full, single_head_split_window_attention=WR.restated_split)
    assert AT.use_native_window_attention(ns) == 2
    m = WR.TransformerLayerStandIn(ns, seed=3).to(DEV)
    m64 = WR.TransformerLayerStandIn(ref_ns, seed=3).to(DEV).double()
    g = torch.Generator().manual_seed(0)
    src, tgt, gout = (torch.randn(2, h * w, 128, generator=g).to(DEV) for _ in range(3))
    mask = torch.zeros(K * K, (h // K) * (w // K), (h // K) * (w // K), device=DEV)
    for splits, shift in ((K, True), (K, False), (1, False)):
        m.zero_grad()
        m64.zero_grad()
        y = m(src, tgt, h, w, splits, shift, mask if shift else None)
        y.backward(gout)
        y64 = m64(src.double(), tgt.double(), h, w, splits, shift, mask if shift else None)
        y64.backward(gout.double())
        assert (y.double() - y64).abs().max() <= 1e-4 * y64.abs().max()
        for name in ("q_proj", "k_proj", "v_proj", "merge"):
            a, b = getattr(m, name).weight.grad, getattr(m64, name).weight.grad
            assert a is not None and torch.isfinite(a).all() and a.abs().max() > 0
            print(splits, shift, name, "max |err| / max |grad| %.2e" % ((a.double() - b).abs().max() / b.abs().max()).item())
            assert (a.double() - b).abs().max() <= 1e-3 * b.abs().max()


# ---------------------------------------------------------------- memory
def test_peak_memory_is_the_output_and_the_log_sum_exp():
    """Float32, the shipped shape (64 x 64, K = 2, B = 8, shifted): no rolled copy, no split copy and nothing of size Lw x Lw (134 MB) is
    ever allocated.  Under no_grad the rise of max_memory_allocated is the output (+ 1 MiB of allocator rounding); with a gradient the
    forward adds lse [B, h w] float32."""
    from igs_amd.attention import window_attention
    B, h, w, K = 8, 64, 64, 2
    q, k, v = WR.random_inputs(B, h, w, torch.float32, DEV, seed=1)
    _native(q[:1], k[:1], v[:1], h, w, K, True)                   # (the module is loaded)
    out_bytes, lse_bytes, MiB = B * h * w * 128 * 4, B * h * w * 4, 1 << 20
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = _native(q, k, v, h, w, K, True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("no_grad: rise %d bytes, out %d" % (rise, out_bytes))
    assert rise <= out_bytes + MiB
    del out
    q.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = window_attention(q, k, v, h, w, K, True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("with a gradient: rise %d bytes, out %d, lse %d" % (rise, out_bytes, lse_bytes))
    assert rise <= out_bytes + lse_bytes + MiB
    assert out.grad_fn is not None
