"""The fused attention on the MI355X (igs_amd.attention over attn.hip) against the float64 restatement of tests/attention_restatement.py.

Tolerances are derived (forward_bound / backward_bounds state the operation counts), never measured.  Every element is compared and the
worst error-to-bound ratio of every case is printed.  Float16 inputs are widened exactly before the float64 restatement sees them.  The
float64 restatement of the large shapes is evaluated head by head (on the device, in float64)."""
import pytest
import torch

import attention_restatement as AR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 0.125
DTYPES = [torch.float16, torch.float32]
ODD = (1, 63, 65, 257, 1000)


def _sdpa(q, k, v, **kw):
    from igs_amd.attention import sdpa
    with torch.no_grad():
        return sdpa(q, k, v, **kw)


def _check_forward(out, q, k, v, scale, label):
    """out, q, k, v as [B, H, A, D]; returns the worst |err| / bound."""
    assert out.dtype == q.dtype and out.shape == q.shape
    assert torch.isfinite(out).all()
    worst = 0.0
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            q64, k64, v64 = q[b, h].double(), k[b, h].double(), v[b, h].double()
            r = AR.restate(q64, k64, v64, scale)
            bound = AR.forward_bound(q64, k64, v64, scale, q.dtype, r)
            err = (out[b, h].double() - r["o"]).abs()
            worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
            assert (err <= bound).all(), (label, b, h, (err / bound.clamp_min(1e-300)).max().item())
    print("%s %s: max |err| / bound %.3f" % (label, str(q.dtype).replace("torch.", ""), worst))
    return worst


# ---------------------------------------------------------------- forward, random inputs
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_shipped_shape(dtype):
    q, k, v = AR.random_inputs(2, 8, 8192, 8192, dtype, DEV, seed=1)
    out = _sdpa(q, k, v, scale=SCALE)
    assert out.is_contiguous()
    _check_forward(out, q, k, v, SCALE, "shipped B = 2")


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_odd_shapes(dtype):
    for Aq in ODD:
        for Ak in ODD:
            q, k, v = AR.random_inputs(1, 1, Aq, Ak, dtype, DEV, seed=Aq * 1009 + Ak)
            _check_forward(_sdpa(q, k, v), q, k, v, SCALE, "Aq %d Ak %d" % (Aq, Ak))       # (the default scale is 1 / sqrt(64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_token_major_views_and_fused_qkv_slices(dtype):
    from igs_amd import attention as AT
    B, H, A = 2, 8, 300
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, A, 3 * H * 64, generator=g)
    qkv[..., :2 * H * 64] *= 1.5
    qkv[..., 2 * H * 64:] += 0.3
    qkv = qkv.to(dtype).to(DEV)
    q, k, v = (qkv[..., i * H * 64:(i + 1) * H * 64].view(B, A, H, 64) for i in range(3))      # slices of one buffer, token-major
    assert all(AT._acceptable(t.permute(0, 2, 1, 3)) for t in (q, k, v))                       # read in place
    out = _sdpa(q, k, v, scale=SCALE, layout="bahd")
    assert out.shape == (B, A, H, 64) and out.is_contiguous()                                  # token-major: to_out reads it as [B, A, C]
    _check_forward(out.permute(0, 2, 1, 3), q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), SCALE, "fused QKV slices")
    qc, kc, vc = (t.contiguous() for t in (q, k, v))                                           # plain token-major tensors
    out2 = _sdpa(qc, kc, vc, scale=SCALE, layout="bahd")
    assert torch.equal(out, out2)                                                              # the same arithmetic whatever the strides
    out3 = _sdpa(qc.permute(0, 2, 1, 3).contiguous(), kc.permute(0, 2, 1, 3).contiguous(), vc.permute(0, 2, 1, 3).contiguous(), scale=SCALE)
    assert torch.equal(out3, out.permute(0, 2, 1, 3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_misaligned_and_strided_views_take_the_copy_path(dtype):
    from igs_amd import attention as AT
    q, k, v = AR.random_inputs(1, 2, 130, 77, dtype, DEV, seed=9)
    ref = _sdpa(q, k, v, scale=SCALE)
    pad = lambda t: torch.cat([torch.zeros_like(t[..., :2]), t], -1)[..., 2:]                  # the same values 4 or 8 bytes off alignment
    qm, km, vm = pad(q), pad(k), pad(v)
    assert not AT._acceptable(qm) and qm.stride(3) == 1
    assert torch.equal(_sdpa(qm, km, vm, scale=SCALE), ref)
    wide = lambda t: torch.stack([t, t], -1).reshape(*t.shape[:-1], 128)[..., ::2]             # stride 2 on d
    qs, ks, vs = wide(q), wide(k), wide(v)
    assert qs.stride(3) == 2 and not AT._acceptable(qs)
    assert torch.equal(_sdpa(qs, ks, vs, scale=SCALE), ref)
    _check_forward(ref, q, k, v, SCALE, "copy path")


def test_float32_error_stays_close_to_pytorch_float32():
    """The derived float32 bound is hundreds of times the real float32 error and would not catch a half-precision leak, so: the native
    error, as max over elements of |err| / sum_j p_ij |v_j|, is at most 4 x the same quantity of PyTorch's own float32 evaluation on the CPU
    (softmax(q k^T scale) v).  A tiled online-softmax float32 emulation gave 0.6-1.45 x at these shapes; a half operand anywhere > 100 x."""
    for Aq, Ak in ((257, 1000), (512, 8192)):
        q, k, v = AR.random_inputs(1, 2, Aq, Ak, torch.float32, "cpu", seed=Aq + Ak)
        r = AR.restate(q.double(), k.double(), v.double(), SCALE)
        den = torch.matmul(r["p"], v.double().abs())
        cpu = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * SCALE, -1), v)
        nat = _sdpa(q.to(DEV), k.to(DEV), v.to(DEV), scale=SCALE).cpu()
        e_cpu = ((cpu.double() - r["o"]).abs() / den).max().item()
        e_nat = ((nat.double() - r["o"]).abs() / den).max().item()
        print("(%d, %d): max |err| / sum p |v|: native %.3e, PyTorch float32 on the CPU %.3e, ratio %.2f" % (Aq, Ak, e_nat, e_cpu, e_nat / e_cpu))
        assert e_nat <= 4 * e_cpu


@pytest.mark.parametrize("shape", [(257, 1000), (1024, 1024)])
def test_half_bound_rejects_the_wrong_variants_on_the_device(shape):
    """Not vacuous: the float16 bound that the native result meets rejects the softmax scale 1 / D and scores rounded to half."""
    q, k, v = AR.random_inputs(1, 1, shape[0], shape[1], torch.float16, DEV, seed=shape[0])
    q64, k64, v64 = q.double(), k.double(), v.double()
    r = AR.restate(q64, k64, v64, SCALE)
    bound = AR.forward_bound(q64, k64, v64, SCALE, torch.float16, r)
    nat = ((_sdpa(q, k, v, scale=SCALE).double() - r["o"]).abs() / bound).max().item()
    wrong = {var: ((AR.half_pipeline(q, k, v, SCALE, var) - r["o"]).abs() / bound).max().item() for var in ("scale_1_over_D", "half_scores")}
    print(shape, "max |err| / bound: native %.3f, wrong variants %s" % (nat, wrong))
    assert nat <= 1.0 and wrong["scale_1_over_D"] > 1.0 and wrong["half_scores"] > 1.0


# ---------------------------------------------------------------- forward, by hand
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ak", [65, 1000])
def test_ragged_tail_keys_get_no_weight(dtype, Ak):
    """Every real score is <= -20, so a padding key with score 0 that took part in the softmax would take nearly all the weight."""
    g = torch.Generator().manual_seed(Ak)
    Aq = 70
    u = torch.randn(64, generator=g)
    u = u / u.norm()
    noise = torch.randn(Aq, 64, generator=g)
    noise = noise - (noise @ u)[:, None] * u
    q = ((8.0 + 2.0 * torch.rand(Aq, 1, generator=g)) * u + 0.5 * noise).to(dtype)
    k = (-(21.0 + 4.0 * torch.rand(Ak, 1, generator=g)) * u).to(dtype)
    v = (torch.randn(Ak, 64, generator=g) + 0.3).to(dtype)
    s = SCALE * q.double() @ k.double().T
    assert s.max() <= -20.0
    q, k, v = (t[None, None].to(DEV) for t in (q, k, v))
    _check_forward(_sdpa(q, k, v, scale=SCALE), q, k, v, SCALE, "ragged tail Ak %d" % Ak)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_key_returns_its_value_bit_for_bit(dtype):
    q, k, v = AR.random_inputs(2, 3, 70, 1, dtype, DEV, seed=2)
    out = _sdpa(q, k, v, scale=SCALE)
    assert torch.equal(out, v.expand(2, 3, 70, 64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_keys_give_the_mean_value(dtype):
    q, k, v = AR.random_inputs(1, 2, 100, 333, dtype, DEV, seed=4)
    k = k[:, :, :1].expand(1, 2, 333, 64).contiguous()
    out = _sdpa(q, k, v, scale=SCALE)
    _check_forward(out, q, k, v, SCALE, "identical keys")
    for h in range(2):                                            # the second statement: the mean of the values
        bound = AR.forward_bound(q[0, h].double(), k[0, h].double(), v[0, h].double(), SCALE, dtype)
        mean = v[0, h].double().mean(0, keepdim=True)
        assert ((out[0, h].double() - mean).abs() <= bound + 1e-12 * mean.abs()).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_of_plus_and_minus_sixty_stay_finite(dtype):
    g = torch.Generator().manual_seed(6)
    u = torch.zeros(64)
    u[3] = 1.0
    a = 480.0 ** 0.5                                              # scale a^2 = 60
    q = (a * u).repeat(40, 1)
    k = torch.cat([(a * u).repeat(50, 1), (-a * u).repeat(50, 1)])[torch.randperm(100, generator=g)]
    v = torch.randn(100, 64, generator=g) + 0.3
    q, k, v = (t.to(dtype)[None, None].to(DEV) for t in (q, k, v))
    out = _sdpa(q, k, v, scale=SCALE)
    assert torch.isfinite(out).all()
    _check_forward(out, q, k, v, SCALE, "scores +-60")
    out = _sdpa(-q, k, v, scale=SCALE)
    _check_forward(out, -q, k, v, SCALE, "scores -+60")


# ---------------------------------------------------------------- backward
def _native_grads(q, k, v, g, scale, need=(True, True, True), layout="bhad"):
    from igs_amd.attention import sdpa
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), need)]
    out = sdpa(*leaves, scale=scale, layout=layout)
    out.backward(g)
    return [t.grad for t in leaves]


def _check_backward(grads, q, k, v, g, scale, label):
    worst = [0.0, 0.0, 0.0]
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            a64 = [t[b, h].double() for t in (q, k, v, g)]
            r = AR.restate(a64[0], a64[1], a64[2], scale)
            ref = AR.gradients(a64[0], a64[1], a64[2], scale, a64[3])
            bounds = AR.backward_bounds(a64[0], a64[1], a64[2], scale, a64[3], q.dtype, r)
            for i, name in enumerate(("d q", "d k", "d v")):
                if grads[i] is None:
                    continue
                assert grads[i].dtype == q.dtype and torch.isfinite(grads[i]).all()
                err = (grads[i][b, h].double() - ref[i]).abs()
                ratio = (err / bounds[i].clamp_min(1e-300)).max().item()
                worst[i] = max(worst[i], ratio)
                assert (err <= bounds[i]).all(), (label, name, b, h, ratio, err.max().item())
            del r, ref, bounds
    print("%s %s: max |err| / bound: d q %.3f, d k %.3f, d v %.3f" % (label, str(q.dtype).replace("torch.", ""), *worst))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 2, 257, 1000), (2, 1, 65, 63), (1, 1, 1, 130), (1, 1, 200, 1)])
def test_backward_odd_shapes(dtype, shape):
    B, H, Aq, Ak = shape
    q, k, v, g = AR.random_inputs(B, H, Aq, Ak, dtype, DEV, seed=Aq + Ak, with_dout=True)
    grads = _native_grads(q, k, v, g, SCALE)
    assert grads[0].shape == q.shape and grads[1].shape == k.shape and grads[2].shape == v.shape
    _check_backward(grads, q, k, v, g, SCALE, "backward %s" % (shape,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_shipped_shape(dtype):
    q, k, v, g = AR.random_inputs(1, 8, 8192, 8192, dtype, DEV, seed=8, with_dout=True)
    grads = _native_grads(q, k, v, g, SCALE)
    _check_backward(grads, q, k, v, g, SCALE, "backward shipped B = 1")


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_null_gradient_combinations_and_bitwise_repeat(dtype):
    q, k, v, g = AR.random_inputs(2, 2, 300, 190, dtype, DEV, seed=12, with_dout=True)
    full = _native_grads(q, k, v, g, SCALE)
    again = _native_grads(q, k, v, g, SCALE)
    for a, b in zip(full, again):
        assert torch.equal(a, b)                                  # no float atomics: two runs agree bit for bit
    for need in ((True, False, False), (False, True, True), (False, False, True), (True, True, False)):
        part = _native_grads(q, k, v, g, SCALE, need)
        for n, a, b in zip(need, part, full):
            assert (a is None) == (not n)
            if n:
                assert torch.equal(a, b)
    # token-major leaves: the gradients come back in the leaves' layout with the same bits
    tm = [t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v, g)]
    gt = _native_grads(tm[0], tm[1], tm[2], tm[3], SCALE, layout="bahd")
    for a, b in zip(gt, full):
        assert a.is_contiguous() and torch.equal(a.permute(0, 2, 1, 3), b)


def test_gradients_reach_the_projection_weights_through_the_processor():
    from igs_amd import attention as AT
    torch.manual_seed(0)
    m = AR.AttentionStandIn(seed=3).to(DEV)
    assert AT.use_native_attention(m) == 1
    x = torch.randn(2, 300, 512, device=DEV)
    gout = torch.randn(2, 300, 512, device=DEV)
    y = m(x)
    assert y.shape == x.shape
    y.backward(gout)
    m64 = AR.AttentionStandIn(seed=3).to(DEV).double()
    y64 = m64.restated(x.double())
    y64.backward(gout.double())
    assert (y.double() - y64).abs().max() <= 1e-4 * y64.abs().max()
    for name in ("to_q", "to_k", "to_v"):
        a, b = getattr(m, name).weight.grad, getattr(m64, name).weight.grad
        assert a is not None and torch.isfinite(a).all() and a.abs().max() > 0
        print(name, "max |err| / max |grad| %.2e" % ((a.double() - b).abs().max() / b.abs().max()).item())
        assert (a.double() - b).abs().max() <= 1e-3 * b.abs().max()
    a, b = m.to_out[0].weight.grad, m64.to_out[0].weight.grad
    assert a is not None and (a.double() - b).abs().max() <= 1e-3 * b.abs().max()


# ---------------------------------------------------------------- memory
def test_peak_memory_is_the_output_and_the_log_sum_exp():
    """Float32, the shipped shape, B = 1: nothing of size A x A is ever allocated.  Under no_grad the rise of max_memory_allocated is the
    output (+ 1 MiB of allocator rounding); with a gradient the forward adds lse [B, H, Aq] float32."""
    from igs_amd.attention import sdpa
    B, H, A = 1, 8, 8192
    q, k, v = AR.random_inputs(B, H, A, A, torch.float32, DEV, seed=1)
    _sdpa(q[:, :, :128], k[:, :, :128], v[:, :, :128])            # (the module is loaded)
    out_bytes, MiB = B * H * A * 64 * 4, 1 << 20
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = _sdpa(q, k, v, scale=SCALE)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("no_grad: rise %d bytes, out %d" % (rise, out_bytes))
    assert rise <= out_bytes + MiB
    del out
    q.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = sdpa(q, k, v, scale=SCALE)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("with a gradient: rise %d bytes, out %d, lse %d" % (rise, out_bytes, 4 * B * H * A))
    assert rise <= out_bytes + 4 * B * H * A + MiB
    assert out.grad_fn is not None
