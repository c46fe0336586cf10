"""The batched SSIM / L1 of the AGM-Net training loss (igs_amd/csrc/ssim_batch.hip, igs_amd.losses.ssim on [N, C, H, W], l1_ssim) against
oracle/torch_losses.py in float64 on the same seeded inputs (the recipe of test_gpu_loss_optim_edges.ssim_case: uniform gt, plus
0.15 * normal, clamped to [0, 1.2]), every element compared.

Bars (the project's own for this arithmetic, test_gpu_loss_optim_edges.py / test_gpu_parity.py): every mean within 1e-6 + 1e-5 |want|;
every image's gradient under check_ssim_grad against that image's own largest element; the L1-only gradient exactly sign(pred - gt) * c.
The SSIM map is held to 4 * E32 + 1e-6, E32 = the worst error of the same restatement run in float32 on the CPU against float64 on the
same inputs, computed here (the factor covers the separable 11 + 11-tap blur in another summation order than the 121-tap window, and
explicit fma)."""
import functools
import os

import numpy as np
import pytest
import torch

from test_gpu_loss_optim_edges import _misaligned, check_ssim_grad
from test_gpu_parity import dev  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(2, 3, 1, 1), (2, 3, 1, 37), (2, 3, 37, 1), (5, 4, 11, 11),                  # below the window, single rows and columns
          (3, 3, 31, 32), (3, 3, 33, 33), (2, 1, 65, 97),                              # tile edges
          (2, 3, 40, 40), (1, 3, 256, 40), (2, 3, 257, 40),                            # 1 / 8 / 9 tile rows: rows per band 1 -> 2, a short last band
          (7, 1, 33, 20), (1, 5, 33, 20),                                              # plane counts that are no multiple of 3 or 8
          (1, 3, 45, 37)]                                                              # N = 1 with size_average=True


def _ext():
    from igs_amd import _cabi
    return _cabi.ext()


@functools.lru_cache(maxsize=None)
def batch_case(N, C, H, W, seed=0):
    """Seeded batch and its float64 reference: pred, gt (float32, CPU), per-image mean SSIM [N], SSIM map, rows d(mean_n)/d pred_n,
    per-image mean |pred - gt| [N], and E32 (see the module docstring).  Shared, never modified."""
    from oracle.torch_losses import ssim_map
    g = torch.Generator().manual_seed(7919 * H + W + 104729 * seed + 1299709 * N + 15485863 * C)
    gt = torch.rand((N, C, H, W), generator=g)
    pred = (gt + 0.15 * torch.randn((N, C, H, W), generator=g)).clamp(0, 1.2)
    x = pred.double().requires_grad_(True)
    m = ssim_map(x, gt.double())
    means = m.mean(dim=(1, 2, 3))
    means.sum().backward()                                  # the images are independent: row n is d(mean_n)/d pred_n
    l1 = (pred.double() - gt.double()).abs().mean(dim=(1, 2, 3))
    with torch.no_grad():
        e32 = float((ssim_map(pred, gt).double() - m).abs().max())
    return dict(pred=pred, gt=gt, means=means.detach().numpy(), map=m.detach().numpy(), grad=x.grad.numpy(), l1=l1.numpy(), e32=e32)


def check_means(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), what
    assert (np.abs(got - want) <= 1e-6 + 1e-5 * np.abs(want)).all(), (what, got, want)


def check_map(got, c, what):
    err = float(np.abs(np.asarray(got, np.float64) - c["map"]).max())
    bar = 4.0 * c["e32"] + 1e-6
    print("%s: map error %.3g, E32 %.3g, ratio to the bar %.3f" % (what, err, c["e32"], err / bar))
    assert err <= bar, (what, err, c["e32"])


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---- the kernels through the compiled module: every output of every instance ----------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_matches_float64(dev, shape):
    N, C, H, W = shape
    c = batch_case(*shape)
    a, b = c["pred"].to(dev), c["gt"].to(dev)
    E = _ext()
    means, l1m, grad, smap = E._loss.ssim_batch(a, b, 1.0, 0.0, True, True, True)
    assert means.shape == l1m.shape == (N + 1,) and grad.shape == smap.shape == shape
    check_means(means[:N].cpu(), c["means"], "ssim means %s" % (shape,))
    check_means(means[N].cpu(), c["means"].mean(), "batch mean")
    check_means(l1m[:N].cpu(), c["l1"], "l1 means")
    check_means(l1m[N].cpu(), c["l1"].mean(), "l1 batch mean")
    check_map(smap.cpu(), c, "%dx%dx%dx%d" % shape)
    for n in range(N):
        check_ssim_grad(grad[n].cpu().numpy(), c["grad"][n], "d mean_%d %s" % (n, shape))
    # the L1 term alone: exactly sign(pred - gt) * c, c = c_l1 / (C H W) in float32
    _, _, g1, none_map = E._loss.ssim_batch(a, b, 0.0, 0.7, True, False, False)
    assert none_map is None
    k = np.float32(0.7) / np.float32(C * H * W)
    assert (g1.cpu().numpy() == np.sign(c["pred"].numpy() - c["gt"].numpy()) * k).all()
    # both terms at once
    _, _, g2, _ = E._loss.ssim_batch(a, b, -0.2, 1.0, True, False, True)
    want = -0.2 * c["grad"] + np.sign(c["pred"].double().numpy() - c["gt"].double().numpy()) / (C * H * W)
    for n in range(N):
        check_ssim_grad(g2[n].cpu().numpy(), want[n], "combined gradient of image %d %s" % (n, shape))
    # forward only: no gradient, and the bits of the gradient instances (means, map, L1 means)
    for want_map in (True, False):
        m0, l0, g0, s0 = E._loss.ssim_batch(a, b, 1.0, 0.0, False, want_map, True)
        assert g0 is None and (s0 is None) == (not want_map)
        assert same_bits(m0, means) and same_bits(l0, l1m) and (not want_map or same_bits(s0, smap))
    m0, l0, _, _ = E._loss.ssim_batch(a, b, 1.0, 0.0, False, False, False)
    assert l0 is None and same_bits(m0, means)
    m0, l0, g0, s0 = E._loss.ssim_batch(a, b, 1.0, 0.0, False, True, False)      # the map without the L1 means: what ssim() asks for under no_grad
    assert l0 is None and g0 is None and same_bits(m0, means) and same_bits(s0, smap)


# ---- igs_amd.losses.ssim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 33, 33), (2, 1, 65, 97), (1, 3, 45, 37), (7, 1, 33, 20)], ids=lambda s: "x".join(map(str, s)))
def test_ssim_training_call(dev, shape):
    from igs_amd.losses import ssim
    N, C, H, W = shape
    c = batch_case(*shape)
    a, gt = c["pred"].to(dev).requires_grad_(True), c["gt"].to(dev)
    mean, smap = ssim(a, gt)
    assert mean.dim() == 0 and smap.shape == shape and mean.requires_grad and not smap.requires_grad
    check_means(mean.item(), c["means"].mean(), "mean")
    check_map(smap.cpu(), c, "ssim() %s" % (shape,))
    (0.2 * (1.0 - mean)).backward()                        # main.py:265 with the shipped lambda_ssim
    assert a.grad.shape == a.shape
    for n in range(N):
        check_ssim_grad(a.grad[n].cpu().numpy(), -0.2 / N * c["grad"][n], "image %d" % n)
    if N > 1:
        a2 = c["pred"].to(dev).requires_grad_(True)
        per = ssim(a2, gt, size_average=False)
        assert per.shape == (N,)
        check_means(per.detach().cpu(), c["means"], "per-image means")
        assert same_bits(per, _ext()._loss.ssim_batch(a2.detach(), gt, 1.0, 0.0, False, False, False)[0][:N])


def test_per_image_upstream_gradients_scale_the_rows_exactly(dev):
    from igs_amd.losses import ssim
    c = batch_case(3, 3, 33, 33)
    a, gt = c["pred"].to(dev).requires_grad_(True), c["gt"].to(dev)
    per = ssim(a, gt, size_average=False)
    per.backward(torch.tensor([1.0, 0.0, -2.5], device=dev))
    rows = _ext()._loss.ssim_batch(a.detach(), gt, 1.0, 0.0, True, False, False)[2]
    assert same_bits(a.grad[0], rows[0]) and bool((a.grad[1] == 0).all()) and same_bits(a.grad[2], rows[2] * -2.5)


def test_runs_positions_and_permutations_are_bit_equal(dev):
    from igs_amd.losses import ssim
    E = _ext()
    c = batch_case(5, 3, 33, 40)
    a, gt = c["pred"].to(dev), c["gt"].to(dev)
    first = E._loss.ssim_batch(a, gt, 1.0, 0.0, True, True, True)
    again = E._loss.ssim_batch(a, gt, 1.0, 0.0, True, True, True)
    assert all(same_bits(x, y) for x, y in zip(first, again))
    means, l1m, grad, smap = first
    for n in range(5):                                      # image n alone = image n at position n of the batch
        m1, l1, g1, s1 = E._loss.ssim_batch(a[n:n + 1], gt[n:n + 1], 1.0, 0.0, True, True, True)
        assert same_bits(m1[0], means[n]) and same_bits(m1[1], means[n]) and same_bits(l1[0], l1m[n])
        assert same_bits(g1[0], grad[n]) and same_bits(s1[0], smap[n])
        x = a[n:n + 1].clone().requires_grad_(True)
        mean, s = ssim(x, gt[n:n + 1])
        mean.backward()
        assert same_bits(mean, means[n]) and same_bits(s[0], smap[n]) and same_bits(x.grad[0], grad[n])
    # ... and at every other position: image 0 of this batch moved through a batch of 5
    for pos in range(1, 5):
        order = list(range(1, 5))
        order.insert(pos, 0)
        mp, lp, gp, sp = E._loss.ssim_batch(a[order], gt[order], 1.0, 0.0, True, True, True)
        assert same_bits(mp[pos], means[0]) and same_bits(lp[pos], l1m[0]) and same_bits(gp[pos], grad[0]) and same_bits(sp[pos], smap[0])
    perm = [3, 0, 4, 2, 1]
    mp, lp, gp, sp = E._loss.ssim_batch(a[perm], gt[perm], 1.0, 0.0, True, True, True)
    assert same_bits(mp[:5], means[perm]) and same_bits(lp[:5], l1m[perm]) and same_bits(gp, grad[perm]) and same_bits(sp, smap[perm])


def test_forward_only_keeps_nothing(dev):
    """no_grad and an img1 that needs no gradient: the bits of the gradient run, and neither a gradient buffer nor the derivative maps are
    allocated: the peak grows by the forward-only scratch and the outputs (512-byte allocator blocks)."""
    from igs_amd import _cabi
    from igs_amd.losses import ssim
    shape = (2, 3, 257, 40)
    N, C, H, W = shape
    c = batch_case(*shape)
    a, gt = c["pred"].to(dev), c["gt"].to(dev)
    mean_g, map_g = ssim(a.clone().requires_grad_(True), gt)
    up = lambda n: (n + 511) // 512 * 512
    sb = _cabi.lib().igs_ssim_batch_scratch_bytes
    scratch0, scratch1 = sb(W, H, N, C, 0), sb(W, H, N, C, 1)
    allowed = up(scratch0) + up(a.numel() * 4) + up((N + 1) * 4)
    assert allowed < scratch1 - scratch0                    # (the bound can tell: the derivative maps alone are larger)
    for mode in ("no_grad", "no requires_grad"):
        x = a.clone().requires_grad_(True) if mode == "no_grad" else a
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        if mode == "no_grad":
            with torch.no_grad():
                mean, smap = ssim(x, gt)
        else:
            mean, smap = ssim(x, gt)
        torch.cuda.synchronize(dev)
        grown = torch.cuda.max_memory_allocated(dev) - before
        assert not mean.requires_grad and same_bits(mean, mean_g) and same_bits(smap, map_g), mode
        assert grown <= allowed, (mode, grown, allowed)


def test_views_and_layouts_give_the_bits_of_a_contiguous_copy(dev):
    from igs_amd.losses import ssim
    c = batch_case(3, 3, 33, 33)
    a, gt = c["pred"].to(dev), c["gt"].to(dev)

    def run(x, y):
        x = x.detach().requires_grad_(True)
        mean, smap = ssim(x, y)
        mean.backward()
        assert x.grad.shape == x.shape
        return mean, smap, x.grad

    want = run(a, gt)
    big_a, big_g = torch.rand((6, 3, 33, 33), device=dev), torch.rand((6, 3, 33, 33), device=dev)
    big_a[::2], big_g[::2] = a, gt
    cases = {"misaligned": (_misaligned(a), _misaligned(gt)),
             "channels-last": (a.contiguous(memory_format=torch.channels_last), gt.contiguous(memory_format=torch.channels_last)),
             "sliced batch": (big_a[::2], big_g[::2])}
    assert not cases["channels-last"][0].is_contiguous() and not cases["sliced batch"][0].is_contiguous()
    for what, (x, y) in cases.items():
        got = run(x, y)
        assert all(same_bits(p, q) for p, q in zip(got, want)), what


def test_golden_results_of_the_reference(dev):
    from igs_amd.losses import ssim
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_ssim_batch.npz"))
    gt = torch.from_numpy(z["gt"]).to(dev)
    a = torch.from_numpy(z["x"]).to(dev).requires_grad_(True)
    mean, _ = ssim(a, gt)
    mean.backward()
    check_means(mean.item(), z["mean"], "golden mean")
    for n in range(3):
        check_ssim_grad(a.grad[n].cpu().numpy(), z["mean_grad"][n], "golden gradient of the mean, image %d" % n)
    b = torch.from_numpy(z["x"]).to(dev).requires_grad_(True)
    per = ssim(b, gt, size_average=False)
    per.backward(torch.from_numpy(z["per_image_w"]).to(dev))
    check_means(per.detach().cpu(), z["per_image"], "golden per-image means")
    for n in range(3):
        check_ssim_grad(b.grad[n].cpu().numpy(), z["per_image_grad"][n], "golden per-image gradient, image %d" % n)


# ---- igs_amd.losses.l1_ssim -----------------------------------------------------------------------------------------------------
def test_l1_ssim_matches_float64_and_the_separate_calls(dev):
    from igs_amd.losses import l1_loss, l1_ssim, ssim
    c = batch_case(4, 3, 33, 40)
    shape5 = (2, 2, 3, 33, 40)
    pred, gt = c["pred"].reshape(shape5).to(dev), c["gt"].reshape(shape5).to(dev)
    sign = np.sign(c["pred"].double().numpy() - c["gt"].double().numpy()) / c["pred"][0].numel()
    for lam_s, lam_1 in ((0.2, 1.0), (0.0, 1.0), (1.0, 0.0), (0.5, 2.5)):
        x = pred.clone().requires_grad_(True)
        out = l1_ssim(x, gt, lambda_ssim=lam_s, lambda_l1=lam_1)
        assert out._fields == ("loss", "l1", "ssim") and all(t.dim() == 0 for t in out)
        assert out.loss.requires_grad and not out.l1.requires_grad and not out.ssim.requires_grad
        out.loss.backward()
        want_l1, want_s = c["l1"].mean(), c["means"].mean()
        check_means(out.l1.item(), want_l1, "l1")
        check_means(out.ssim.item(), want_s, "ssim")
        check_means(out.loss.item(), lam_1 * want_l1 + lam_s * (1.0 - want_s), "loss")
        assert x.grad.shape == shape5
        got, want = x.grad.reshape(4, 3, 33, 40).cpu().numpy(), (lam_1 * sign - lam_s * c["grad"]) / 4
        if lam_s == 0.0:                                    # the L1 term alone: exactly sign * c, c = (lambda_l1 / N) / (C H W) in float32
            assert (got == np.sign(sign) * (np.float32(lam_1 / 4) / np.float32(3 * 33 * 40))).all()
        for n in range(4):
            check_ssim_grad(got[n], want[n], "l1_ssim gradient, image %d, lambdas %s" % (n, (lam_s, lam_1)))
        # the two separate native calls
        y = pred.clone().requires_grad_(True)
        y4 = y.reshape(4, 3, 33, 40)
        sep = lam_1 * l1_loss(y, gt) + lam_s * (1.0 - ssim(y4, gt.reshape(4, 3, 33, 40))[0])
        sep.backward()
        check_means(out.loss.item(), sep.item(), "against l1_loss + ssim")
        g_sep = y.grad.reshape(4, 3, 33, 40).cpu().numpy()
        for n in range(4):
            check_ssim_grad(got[n], g_sep[n], "against the gradient of l1_loss + ssim, image %d" % n)
    with torch.no_grad():
        quiet = l1_ssim(pred.clone().requires_grad_(True), gt)
    assert not quiet.loss.requires_grad
    check_means(quiet.loss.item(), c["l1"].mean() + 0.2 * (1.0 - c["means"].mean()), "loss under no_grad")


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_on_new_contents(dev):
    from igs_amd.losses import ssim
    c0, c1 = batch_case(2, 3, 40, 40), batch_case(2, 3, 40, 40, seed=1)
    a = c0["pred"].to(dev).requires_grad_(True)
    gt = c0["gt"].to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                           # warm-up off the default stream, as capture wants it
        for _ in range(2):
            mean, _ = ssim(a, gt)
            torch.autograd.grad(mean, a)
    torch.cuda.current_stream(dev).wait_stream(side)
    a = a.detach().requires_grad_(True)                     # (a leaf the warm-up's stream has not touched)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mean, smap = ssim(a, gt)
        (grad,) = torch.autograd.grad(mean, a)
    with torch.no_grad():
        a.copy_(c1["pred"].to(dev))
        gt.copy_(c1["gt"].to(dev))
    graph.replay()
    torch.cuda.synchronize(dev)
    x = c1["pred"].to(dev).requires_grad_(True)
    e_mean, e_map = ssim(x, c1["gt"].to(dev))
    (e_grad,) = torch.autograd.grad(e_mean, x)
    assert same_bits(mean, e_mean) and same_bits(smap, e_map) and same_bits(grad, e_grad)
    check_means(mean.item(), c1["means"].mean(), "replayed mean")


# ---- the C ABI on buffers embedded in poison ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_grad", [True, False])
def test_c_abi_writes_every_output_and_nothing_else(dev, with_grad):
    from igs_amd import _cabi
    L = _cabi.lib()
    N, C, H, W = shape = (2, 3, 33, 40)
    c = batch_case(*shape)
    n = N * C * H * W
    PAD = 4096                                              # floats of NaN on either side of every buffer
    nan = float("nan")

    def embedded(numel, fill=None):
        whole = torch.full((numel + 2 * PAD,), nan, device=dev)
        if fill is not None:
            whole[PAD:PAD + numel] = fill.reshape(-1).to(dev)
        return whole, whole[PAD:PAD + numel]

    scratch_bytes = L.igs_ssim_batch_scratch_bytes(W, H, N, C, int(with_grad))
    (wp, pred), (wg, gt) = embedded(n, c["pred"]), embedded(n, c["gt"])
    (wm, means), (wl, l1m), (wd, grad), (ws, smap) = embedded(N + 1), embedded(N + 1), embedded(n), embedded(n)
    wsc, scratch = embedded(scratch_bytes // 4 + 64)
    sp = (scratch.data_ptr() + 255) // 256 * 256
    rc = L.igs_ssim_batch_fwd_bwd(torch.cuda.current_stream(dev).cuda_stream, W, H, N, C, pred.data_ptr(), gt.data_ptr(), 1.0, 0.5, sp,
                                  means.data_ptr(), l1m.data_ptr(), grad.data_ptr() if with_grad else None, smap.data_ptr())
    assert rc == 0, _cabi.last_error()
    torch.cuda.synchronize(dev)
    outs = [("means", wm, means), ("l1 means", wl, l1m), ("map", ws, smap)] + ([("grad", wd, grad)] if with_grad else [])
    for what, whole, view in outs:
        assert bool(torch.isfinite(view).all()), what
        assert bool(torch.isnan(whole[:PAD]).all()) and bool(torch.isnan(whole[PAD + view.numel():]).all()), what
    if not with_grad:
        assert bool(torch.isnan(wd).all())
    assert bool(torch.isnan(wsc[:PAD]).all()) and bool(torch.isnan(wsc[PAD + scratch.numel():]).all())
    assert bool(torch.isnan(scratch.view(-1)[(sp - scratch.data_ptr()) // 4 + scratch_bytes // 4:]).all())      # nothing behind the stated size
    for whole, view, src in ((wp, pred, c["pred"]), (wg, gt, c["gt"])):
        assert bool((view.cpu() == src.reshape(-1)).all()) and bool(torch.isnan(whole[:PAD]).all()) and bool(torch.isnan(whole[PAD + n:]).all())
    check_means(means[:N].cpu(), c["means"], "means from poisoned surroundings")
    check_means(l1m[:N].cpu(), c["l1"], "l1 means from poisoned surroundings")
    check_map(smap.reshape(shape).cpu(), c, "poison")
    if with_grad:
        want = c["grad"] + 0.5 * np.sign(c["pred"].double().numpy() - c["gt"].double().numpy()) / (C * H * W)
        for i in range(N):
            check_ssim_grad(grad.reshape(shape)[i].cpu().numpy(), want[i], "gradient from poisoned surroundings, image %d" % i)


# ---- what the new path must not have captured, and what it refuses on a GPU -----------------------------------------------------
def test_single_image_path_is_still_the_old_one(dev):
    from igs_amd.losses import ssim
    c = batch_case(1, 3, 45, 37)
    E = _ext()
    for x, y in ((c["pred"][0], c["gt"]), (c["pred"], c["gt"])):                     # [3,H,W] against [1,3,H,W]; [1,3,H,W] on both sides
        a, gt = x.to(dev).requires_grad_(True), y.to(dev)
        v = ssim(a, gt, size_average=False)
        assert v.shape == (1,)
        old_mean, old_grad = E.ssim_mean(a.detach(), gt)
        assert same_bits(v[0], old_mean)
        torch.testing.assert_close(v.detach().cpu().double(), torch.from_numpy(c["means"]), rtol=1e-5, atol=1e-6)
        (1.0 - v).sum().backward()
        assert same_bits(a.grad, -old_grad.reshape(a.shape))
        check_ssim_grad(a.grad.reshape(3, 45, 37).cpu().numpy(), -c["grad"][0], "single-image gradient")


def test_refusals_on_gpu_tensors(dev):
    from igs_amd.losses import l1_ssim, ssim
    x = torch.rand(2, 3, 20, 27, device=dev)
    calls = [lambda: ssim(x[0], x[0], size_average=True), lambda: ssim(x.double(), x.double()), lambda: ssim(x.half(), x.half()),
             lambda: ssim(x.bfloat16(), x.bfloat16()), lambda: ssim(x, x.clone().requires_grad_(True)), lambda: ssim(x, x, window_size=7),
             lambda: ssim(x, x[:, :, :, :26]), lambda: ssim(x, x[:1]), lambda: ssim(x[:0], x[:0]), lambda: ssim(x, x.cpu()),
             lambda: l1_ssim(x.double(), x.double()), lambda: l1_ssim(x, x.clone().requires_grad_(True)), lambda: l1_ssim(x[0, 0], x[0, 0])]
    for f in calls:
        with pytest.raises(NotImplementedError):
            f()
